"""Run by tests/test_rerank_gpu.py in its own process with YAMS_ACCEL_MEASURE_LIB=1 and YAMS_ACCEL_RERANK_FUSED_PATH=valu: the
measurement build then serves the fused form on the VALU register tile instead of the matrix cores.  The golden cases, the zero
ties and two lattice windows must give the oracle's bits on that path too, and the diag must name it."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import _rerank_oracle as ro  # noqa: E402


def main():
    import torch
    from yams_amd import _lib
    from yams_amd.accel import Accel
    assert os.environ.get("YAMS_ACCEL_MEASURE_LIB") and os.environ.get("YAMS_ACCEL_RERANK_FUSED_PATH") == "valu"
    acc = Accel(0, torch.cuda.current_stream().cuda_stream)
    cases = json.load(open(os.path.join(ROOT, "tests", "golden", "colbert_maxsim.json")))["cases"]
    got = ro.restated(ro.FUSED, lambda q, x, off, f: acc.rerank_maxsim(q, x, off, form=f)[0], lambda x, off: acc.rerank_maxpool(x, off))
    assert ro.nan_blind(got) == ro.nan_blind([c["fused"] for c in cases])
    windows = [(q, rows, off) for q, rows, off, _ in ro.zero_tie_cases()]
    rng = np.random.default_rng(11)
    for dim, tq, lengths in ((49, 65, [0, 1, 255, 256, 257, 513]), (128, 33, [513, 31])):
        off = ro.csr(lengths)
        windows.append((ro.mixed(rng, (tq, dim), -3, 3), ro.mixed(rng, (int(off[-1]), dim), -3, 3), off))
    for q, x, off in windows:
        want = ro.maxsim_cpp(q, x, off, ro.FUSED)
        sc, mx, arg, diag = acc.rerank_maxsim(q, x, off, form=ro.FUSED, want_rowmax=True)
        assert diag["path"] == _lib.RERANK_PATH_VALU, diag
        assert ro.equal(sc, want[0]) and ro.equal(mx, want[1]) and ro.equal(arg, want[2]), q.shape
    acc.close()
    print("fused on the VALU: OK")


if __name__ == "__main__":
    main()
