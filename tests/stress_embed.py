"""Stress of the embedding model's pooling head on the device (yams_embed_pool) against the C++ restatement
(tests/cpp/embed_oracle.cpp): seeded batches on ONE context in sequence, each drawn by tests/_embed_oracle.py stress_case — dims
around the slab and vector widths, sequence lengths around the mask window, batches up to 257, mask_len one below, at and one
above the sequence, masks with scattered zeros, tail padding and zero runs across a window edge, MEAN or MAX (CLS reads no mask:
the lattice of tests/test_embed_gpu.py holds it), normalised or not, through the device or the host entry, aligned or not —
and each PROVEN discriminating from the oracle alone before it counts: every MEAN case changes bits when its tokens are summed in
reverse, every case with a masked token changes bits when the masked tokens are admitted; a draw that proves neither is redrawn,
at most 20 times per case.  Outputs are compared on bits, the diag's counts with the oracle's.

    python tests/stress_embed.py [--cases 120] [--seed 1]
    python tests/stress_embed.py --dry-run      draws the cases and proves them, no device
    python tests/stress_embed.py --self-test    the comparison tells a flipped bit, no device
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import _embed_oracle as eo  # noqa: E402


def oracle(c):
    out, counts = eo.pool_cpp(c["hidden"], c["mask"], c["mode"], c["normalize"], want_counts=True)
    return [out, np.array(counts, np.uint64)]


def device(acc, c):
    out, diag = acc.embed_pool(c["hidden"], c["mask"], mode=c["mode"], normalize=c["normalize"], host_entry=c["host"], misalign=c["misalign"])
    return [out, np.array([diag["tokens_considered"], diag["active_tokens"]], np.uint64)]


def draw_all(seed, count):
    cases = [eo.stress_case(seed * 1000 + i) for i in range(count)]
    assert max(c["redraws"] for c in cases) <= eo.MAX_REDRAWS
    assert all(c["proves_order"] for c in cases if c["mode"] == eo.MEAN), "a MEAN case that does not tell the token order"
    assert all(c["proves_mask"] for c in cases if c["has_masked"]), "a masked token whose admission changes nothing"
    assert all(c["proves_order"] or c["proves_mask"] for c in cases)
    return cases


def self_test():
    for seed in (1000, 1001, 1002):
        c = eo.stress_case(seed)
        want = oracle(c)
        assert eo.differs([np.array(v, copy=True) for v in want], want) == []
        got = [np.array(v, copy=True) for v in want]
        flat = got[0].reshape(-1)
        at = int(np.flatnonzero(~np.isnan(flat))[0])
        flat.view(np.uint32)[at] ^= 1
        assert eo.differs(got, want) == [0], seed
        got = [np.array(v, copy=True) for v in want]
        got[1][1] += 1
        assert eo.differs(got, want) == [1], seed
    print("self-test OK")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=120)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--dry-run", action="store_true")
    ap.add_argument("--self-test", action="store_true")
    a = ap.parse_args()
    if a.self_test:
        return self_test()
    cases = draw_all(a.seed, a.cases)
    if a.dry_run:
        assert {c["mode"] for c in cases} == {eo.MAX, eo.MEAN} and {c["host"] for c in cases} == {False, True}
        assert {c["normalize"] for c in cases} == {False, True} and {c["misalign"] for c in cases} == {0, 4}
        assert any(c["mask"].shape[1] != c["hidden"].shape[1] for c in cases)
        print(f"dry run OK: {len(cases)} cases drawn, {sum(c['proves_order'] for c in cases)} tell the token order, "
              f"{sum(c['proves_mask'] for c in cases)} tell a masked token, at most {max(c['redraws'] for c in cases)} redraws, "
              f"dims {sorted({c['hidden'].shape[2] for c in cases})}, seqs {sorted({c['hidden'].shape[1] for c in cases})}, "
              f"batches {sorted({c['hidden'].shape[0] for c in cases})}")
        return
    import torch
    from yams_amd.accel import Accel
    acc = Accel(0, torch.cuda.current_stream().cuda_stream)
    failed = 0
    for c in cases:
        bad = eo.differs(device(acc, c), oracle(c))
        if bad:
            failed += 1
            print("FAIL seed", c["seed"], c["hidden"].shape, "mask_len", c["mask"].shape[1], "mode", c["mode"], "normalize", c["normalize"],
                  "host", c["host"], "misalign", c["misalign"], "outputs", bad)
    acc.close()
    print(f"{len(cases)} cases, {failed} failures" + (" OK" if not failed else ""))
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
