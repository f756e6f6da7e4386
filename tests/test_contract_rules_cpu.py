"""The result contract's rules (yams_amd/csrc/contract_rules.h: the functions every kernel inlines) on the CPU: compiled
with plain g++ into tests/cpp/contract_rules_test and held there, bit for bit, to the oracle's restatement of the reference —
query validity, computeCosineSimilarity, the fast path's cosine at its edges, the row id map, the allow-mask bit, an unused
slot.  The entity predicate is held here to tests/_entity_oracle.py's `admitted`."""
import subprocess

import numpy as np

import _cpp_build
import _entity_oracle as eo
from yams_amd import _lib


def test_the_rules_equal_the_oracle_bit_for_bit():
    exe = _cpp_build.build_contract_rules_test()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout[-3000:] + r.stderr[-1000:]


def test_entity_admits_equals_the_entity_oracle():
    """Each field alone, all three together, an unset column value against a filter value equal to the unset constant, a
    filter with no fields: one row per case, the expectation from `admitted`."""
    T, U = eo.TYPE_UNSET, eo.UNSET
    row_values = [(1, 10, 100), (2, 10, 100), (1, 11, 100), (1, 10, 101), (T, U, U), (T, 10, 100), (1, U, 100), (1, 10, U)]
    filters = [None, (None, None, None),
               (1, None, None), (2, None, None), (None, 10, None), (None, 11, None), (None, None, 100), (None, None, 101),
               (1, 10, 100), (1, 10, 101), (2, 10, 100), (1, 11, 100),
               (T, None, None), (None, U, None), (None, None, U), (T, U, U),      # a filter value equal to "unset" matches nothing
               (0, None, None), (None, 0, None), (None, None, 0)]
    cases, want = [], []
    for filt in filters:
        for rt, rn, rd in row_values:
            got = eo.admitted(1, np.array([rt], np.uint8), np.array([rn], np.uint32), np.array([rd], np.uint32), filt, None)
            want.append(len(got))
            t, nt, dc = filt if filt is not None else (None, None, None)
            fields = (_lib.ENTITY_FILTER_TYPE if t is not None else 0) | (_lib.ENTITY_FILTER_NODE_TYPE if nt is not None else 0) | \
                (_lib.ENTITY_FILTER_DOC if dc is not None else 0)
            cases.append("%d %d %d %d %d %d %d" % (fields, t or 0, nt or 0, dc or 0, rt, rn, rd))
    assert 0 in want and 1 in want
    exe = _cpp_build.build_contract_rules_test()
    r = subprocess.run([exe, "admits"], input="\n".join(cases) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in r.stdout.split()]
    assert len(got) == len(want)
    wrong = [(c, g, w) for c, g, w in zip(cases, got, want) if g != w]
    assert not wrong, wrong[:5]
