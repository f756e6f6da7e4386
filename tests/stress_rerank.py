"""Stress of the late-interaction rerank on the device (yams_rerank_maxsim) against the C++ restatement
(tests/cpp/rerank_oracle.cpp): seeded windows on ONE context, each drawn by tests/_rerank_oracle.py stress_case — dims, query
lengths and document lengths around the kernel's tiles, empty documents, in either form, through the device or the host entry,
aligned or not — and each PROVEN discriminating from the oracle alone before it counts: its score bits change under a reversed i
order, a dropped last document token and a dropped last query token, and for at least half of the cases under the other form.
Scores, row maxima and winning tokens are compared on bits.

    python tests/stress_rerank.py [--cases 60] [--seed 1]
    python tests/stress_rerank.py --dry-run      draws the cases and computes their oracle, no device
    python tests/stress_rerank.py --self-test    the comparison tells a flipped bit, no device
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import _rerank_oracle as ro  # noqa: E402


def oracle(c):
    return ro.maxsim_cpp(c["query"], c["rows"], c["off"], c["form"])


def device(acc, c):
    sc, mx, arg, _ = acc.rerank_maxsim(c["query"], c["rows"], c["off"], form=c["form"], want_rowmax=True, host_entry=c["host"],
                                       misalign=c["misalign"])
    return sc, mx, arg


def differs(got, want):
    """The outputs whose bits differ (a NaN matches any NaN)."""
    return [i for i, (g, w) in enumerate(zip(got, want)) if not ro.equal(g, w)]


def draw_all(seed, count):
    cases = [ro.stress_case(seed * 1000 + i) for i in range(count)]
    share = sum(c["other_form"] for c in cases)
    # the first three conditions hold for every case (stress_case redraws until they do); the form decides at least half
    assert 2 * share >= count, "only %d of %d cases tell the forms apart" % (share, count)
    return cases, share


def self_test():
    for seed in (1000, 1001, 1002):
        c = ro.stress_case(seed)
        assert all(ro.discriminates(c)[:3])
        want = oracle(c)
        assert differs([np.array(v, copy=True) for v in want], want) == []
        for i in range(len(want)):
            got = [np.array(v, copy=True) for v in want]
            flat = got[i].reshape(-1)
            at = int(np.flatnonzero(~np.isnan(flat.astype(np.float64)))[0])
            flat.view(np.uint32)[at] ^= 1
            assert differs(got, want) == [i], (seed, i)
    print("self-test OK")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=60)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--dry-run", action="store_true")
    ap.add_argument("--self-test", action="store_true")
    a = ap.parse_args()
    if a.self_test:
        return self_test()
    cases, share = draw_all(a.seed, a.cases)
    if a.dry_run:
        for c in cases[:9]:
            oracle(c)
        assert {c["form"] for c in cases} == {0, 1} and {c["host"] for c in cases} == {False, True}
        assert any((np.diff(c["off"].astype(np.int64)) == 0).any() for c in cases), "no empty document drawn"
        print(f"dry run OK: {len(cases)} cases drawn, {share} tell the forms apart, dims {sorted({c['query'].shape[1] for c in cases})}, "
              f"query tokens {sorted({c['query'].shape[0] for c in cases})}")
        return
    import torch
    from yams_amd.accel import Accel
    acc = Accel(0, torch.cuda.current_stream().cuda_stream)
    failed = 0
    for c in cases:
        bad = differs(device(acc, c), oracle(c))
        if bad:
            failed += 1
            print("FAIL seed", c["seed"], c["query"].shape, "docs", len(c["off"]) - 1, "form", c["form"], "host", c["host"], "misalign",
                  c["misalign"], "outputs", bad)
    acc.close()
    print(f"{len(cases)} cases, {failed} failures" + (" OK" if not failed else ""))
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
