"""Row and slot reachability of every filter form of the exact scan, held deterministically: the planted cases of
tests/_positions.py (every row a winner exactly once, from a query slot chosen so that every row position x slot pair, every
tile and unit edge, every boundary mask word occurs) through yams_scan_topk_device, one test per (form, case).  For EVERY query:
count, row ids, score bits, distance bits under L2, the padding of the unused slots; diag.path / filter_tier say that the
intended form ran and exact_fallback_queries == 0 that no exhaustive pass stood in for a list that lost its row.

Write contract of the entry, on the way: out_scores, out_rows, out_counts and out_dist are carved out of larger allocations with
256 guard bytes of 0xA5 on either side, at bases no better aligned than their element type (the header documents no more for
them; every store site — rescore_select_kernel, the scatter kernels, write_empty_slot, the fused scan — stores single elements);
after the call every guard byte is intact and the corpus, its shadows, the mask, the rank tables and the queries equal clones
taken before.

tests/test_scan_positions_cpu.py asserts the design's conditions (no other row near a planted one, coverage, what each shape
reaches in the tile geometry) and rehearses these bodies against the CPU oracle; nothing of that is recomputed here."""
import json

import numpy as np
import pytest

import _positions as P
from yams_amd import _lib

pytestmark = pytest.mark.gpu

GUARD = 256


class Guarded:
    """`nbytes` of output inside a larger device allocation: 256 guard bytes on either side, the payload `misalign` bytes past
    a 16-byte boundary."""
    def __init__(self, torch, nbytes, misalign):
        self.buf = torch.empty(GUARD + misalign + nbytes + GUARD, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.off, self.nbytes = GUARD + misalign, nbytes
        self.ptr = self.buf.data_ptr() + self.off
        assert self.ptr % 16 == misalign

    def arm(self):
        self.buf.fill_(0xA5)

    def read(self, dtype, shape, what):
        host = self.buf.cpu().numpy()
        lo, hi = host[:self.off], host[self.off + self.nbytes:]
        assert (lo == 0xA5).all() and (hi == 0xA5).all(), (what, "guard bytes written", np.flatnonzero(lo != 0xA5)[:4] - self.off, np.flatnonzero(hi != 0xA5)[:4])
        return host[self.off:self.off + self.nbytes].copy().view(dtype).reshape(shape)


def device_result(acc, case, f):
    """The case through yams_scan_topk_device as the form is driven; checks the write contract of every call."""
    import torch
    n, dim = case.corpus.shape
    nq, k = case.exp_rows.shape
    inputs = {}
    tc = inputs["rows"] = torch.from_numpy(np.array(case.corpus)).cuda()
    tq = inputs["queries"] = torch.from_numpy(np.ascontiguousarray(case.queries)).cuda()
    torch.cuda.synchronize()
    kw = {}
    shadow = f.get("shadow")
    i8_flags = getattr(_lib, f["i8_flags"]) if f.get("i8_flags") else 0
    if shadow in ("bf16", "both"):
        tb = inputs["rows_bf16"] = torch.empty((n, dim), dtype=torch.bfloat16, device="cuda")
        tn = inputs["rows_nsq"] = torch.empty(n, dtype=torch.float32, device="cuda")
        acc.build_shadow_device(tc.data_ptr(), n, dim, tb.data_ptr(), tn.data_ptr())
        kw.update(rows_bf16_ptr=tb.data_ptr(), rows_nsq_ptr=tn.data_ptr())
    if shadow in ("i8", "both"):
        t8 = inputs["rows_i8"] = torch.empty((_lib.i8_shadow_rows(n), dim), dtype=torch.int8, device="cuda")
        tm = inputs["rows_i8_meta"] = torch.empty(((n + 63) // 64, 2), dtype=torch.float32, device="cuda")
        acc.build_shadow_i8_device(tc.data_ptr(), n, dim, t8.data_ptr(), tm.data_ptr(), i8_flags=i8_flags)
        kw.update(rows_i8_ptr=t8.data_ptr(), rows_i8_meta_ptr=tm.data_ptr(), i8_flags=i8_flags)
    if case.tie_rank is not None:
        inv = np.empty(n, np.uint32); inv[case.tie_rank] = np.arange(n, dtype=np.uint32)
        tr = inputs["tie_rank"] = torch.from_numpy(case.tie_rank.view(np.int32).copy()).cuda()
        ti = inputs["rank_row"] = torch.from_numpy(inv.view(np.int32)).cuda()
        kw.update(tie_rank_ptr=tr.data_ptr(), rank_row_ptr=ti.data_ptr())
    if case.mask is not None:
        bits = np.zeros((n + 31) // 32 * 32, bool); bits[:n] = case.mask
        words = np.packbits(bits, bitorder="little").view(np.uint32)                 # bit (r & 31) of word (r >> 5)
        tmask = inputs["row_mask"] = torch.from_numpy(words.view(np.int32).copy()).cuda()
        kw.update(row_mask_ptr=tmask.data_ptr(), row_mask_count=int(case.mask.sum()))
    acc.synchronize(); torch.cuda.synchronize()
    clones = {name: t.clone() for name, t in inputs.items()}
    view = acc.corpus_view(tc.data_ptr(), n, dim, row_base=case.row_base, **kw)
    flags = 0
    for name in f.get("flags", ()):
        flags |= getattr(_lib, name)
    metric = _lib.SCAN_L2 if case.metric == "l2" else _lib.SCAN_COSINE
    per = max(c for _, c in P.call_ranges(nq, f.get("per_call")))
    g_s, g_r = Guarded(torch, per * k * 4, 4), Guarded(torch, per * k * 8, 8)
    g_n, g_d = Guarded(torch, per * 4, 4), Guarded(torch, per * k * 4, 4)

    def call(q0, cnt):
        for g in (g_s, g_r, g_n, g_d):
            g.arm()
        torch.cuda.synchronize()
        diag = acc.scan_topk_device(view, tq.data_ptr() + q0 * dim * 4, cnt, k, case.thr, metric, g_s.ptr, g_r.ptr, g_n.ptr, g_d.ptr, None, flags=flags)
        acc.synchronize()
        assert cnt == per
        return P.Result(g_n.read(np.uint32, (cnt,), "out_counts"), g_r.read(np.int64, (cnt, k), "out_rows"),
                        g_s.read(np.float32, (cnt, k), "out_scores"), g_d.read(np.float32, (cnt, k), "out_dist"), diag)

    res = P.drive(case, f, call)
    torch.cuda.synchronize()
    for name, t in inputs.items():
        assert torch.equal(t.view(torch.uint8), clones[name].view(torch.uint8)), ("input changed by the call", name)
    return res


@pytest.mark.parametrize("form,case", P.PARAMS)
def test_every_row_and_slot_of_the_form_returns_its_planted_winner(acc, oracle, form, case):
    f = P.FORMS[form]
    c = P.make_case(oracle, f, case)
    res = device_result(acc, c, f)
    print("POSITIONS " + json.dumps({"form": form, "case": case, "n": f["n"], "dim": f["dim"], "diag": {x: int(v) for x, v in res.diag.items()}}))
    P.verify(c, res, f)
