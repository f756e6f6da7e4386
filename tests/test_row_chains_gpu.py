"""The row-staged fp64 scorer both entries share (yams_amd/csrc/row_chains.h) at the shapes where a shared, pipelined stage
can go wrong, through yams_scan_doc_topk_device and yams_scan_entity_topk_device against the oracles of
tests/test_doc_topk_gpu.py and tests/test_entity_gpu.py: score bits, rows, documents, counts and matching counts identical.

The lattice: a chunk is 32 elements, so dim 1 and 4 end in the prologue fetch (one element, one float4), 31 / 32 are one chunk
short of and exactly full, 33 and 36 have a last chunk of one element and of one float4, 64 is exactly two chunks (no fetch past
the end), 65 is three.  A row base one float past a 16-byte boundary forces the scalar loads at every dim.  257 rows: the second
workgroup has one live thread.

Queries: both entries hand a whole slice of queries to the launcher, which takes QG = 1 for one slot, 4 up to four, else 8.
One query is <1>; three are <4> with one dead slot (only half the workgroup fills the query tile); five are ONE group of <8>
with five live slots and three dead ones.  Nine differ by entry: the document entry launches two groups of <8>, the second
(slot0 = 8) with one live slot and seven dead ones; the entity entry cuts its slices to whole groups of 8, so nine are a full
<8> and then <1> at q0 = 8, and its group with slot0 = 8 comes from sixteen (two full groups of <8>).  A ragged group with
slot0 > 0 cannot be reached through the entity entry at these sizes."""
import numpy as np
import pytest

from test_doc_topk_gpu import check as doc_check, corpus as doc_corpus, layout
from test_entity_cpu import special_rows
from test_entity_gpu import check as entity_check
from _doc_oracle import NO_DOC

pytestmark = pytest.mark.gpu

DIMS = (1, 4, 31, 32, 33, 36, 64, 65)
NQS = {"doc": (1, 3, 5, 9), "entity": (1, 3, 5, 9, 16)}     # the forms each count selects: the docstring above
N = 257


def lattice(entry):
    for d in DIMS:
        for offset in (0, 1):
            for nq in NQS[entry]:
                yield d, offset, nq


def queries_for(rng, rows, nq):
    q = rng.standard_normal((nq, rows.shape[1])).astype(np.float32)
    q[nq - 1] = rows[12] * np.float32(1.5)             # a duplicated row (doc_corpus) / a plain one: ties and a score of 1
    return q


@pytest.mark.parametrize("entry", ["doc", "entity"])
def test_the_lattice_is_bit_exact(acc, oracle, entry):
    for d, offset, nq in lattice(entry):
        rng = np.random.default_rng(7000 + 100 * d + 10 * offset + nq)
        if entry == "doc":
            rows = doc_corpus(rng, N, d, special=d >= 6)
            row_doc = layout(rng, N, 40, "random")
            doc_check(acc, oracle, rows, queries_for(rng, rows, nq), 20, -1.0, row_doc, 40, tie=rng.permutation(N).astype(np.uint32),
                      doc_rank=rng.permutation(40).astype(np.uint32), rows_offset=offset)
        else:
            rows = special_rows(rng, N, d) if d >= 3 else rng.standard_normal((N, d)).astype(np.float32)
            rows[N - 1] = rows[0] * np.float32(2.0)        # the one live thread of the second workgroup holds a best row
            entity_check(acc, rows, queries_for(rng, rows, nq), 20, -1.0, rows_offset=offset)


@pytest.mark.parametrize("offset", [0, 1])
def test_a_gathered_list_that_ends_inside_a_workgroup_with_rows_of_no_document(acc, oracle, offset):
    """dim 33, 300 allowed rows of 2600 (fewer than one in 8: gathered first; the list ends 44 items into the second
    workgroup), every eighth row without a document: counted, never returned."""
    rng = np.random.default_rng(7100 + offset)
    n, d, n_docs = 2600, 33, 60
    rows = doc_corpus(rng, n, d)
    row_doc = layout(rng, n, n_docs, "contiguous")
    row_doc[::8] = NO_DOC
    mask = np.sort(rng.choice(n, 300, replace=False))
    for nq in NQS["doc"]:
        doc_check(acc, oracle, rows, queries_for(rng, rows, nq), 20, -1.0, row_doc, n_docs, tie=rng.permutation(n).astype(np.uint32),
                  doc_rank=rng.permutation(n_docs).astype(np.uint32), mask_rows=mask, rows_offset=offset)
