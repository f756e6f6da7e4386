"""bench.py's plain run (set-up, warm-up, the timed steps, the line: nothing of --full) and what `--dump-outputs` writes:
the merged top-k of the last timed step, identical from run to run under the same arguments, and equal to the oracle's
answer for that step's query batch over the resident rows."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N, D, NQ, K, STEPS, WARMUP, SEED = 300_000, 256, 300, 50, 3, 1, 42


def _plain_run(tmp_path, tag):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--rows-per-gpu", str(N), "--dim", str(D),
           "--queries", str(NQ), "--k", str(K), "--steps", str(STEPS), "--warmup", str(WARMUP), "--seed", str(SEED),
           "--extra-json", str(tmp_path / f"{tag}.json"), "--dump-outputs", str(tmp_path / tag)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=280, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and r.stdout.rstrip().endswith(lines[0])
    return json.loads(lines[0]), {n: np.load(tmp_path / tag / f"{n}.npy") for n in ("scores", "rows", "counts")}


def test_plain_run_dumps_the_last_timed_step(tmp_path, oracle):
    out, got = _plain_run(tmp_path, "a")
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in out, key
    assert out["steps"] == STEPS and out["warmup"] == WARMUP and out["ms_per_step"] > 0 and out["value"] > 0
    for key in ("bit_exact_vs_oracle", "cpu_baseline", "ingest", "config2", "pq", "non_uniform", "roofline_hbm_leg", "config3_l2"):
        assert key not in out, key                  # --full only
    assert got["scores"].dtype == np.float32 and got["scores"].shape == (NQ, K)
    assert got["rows"].dtype == np.float64 and got["rows"].shape == (NQ, K)
    assert got["counts"].dtype == np.float64 and got["counts"].shape == (NQ,) and (got["counts"] == K).all()
    # the same arguments: the same inputs, the same outputs
    _, again = _plain_run(tmp_path, "b")
    for n in got:
        assert np.array_equal(got[n], again[n]), n
    # the last timed step is batch WARMUP + STEPS - 1, which ran query batch (WARMUP + STEPS - 1) % 4 (--query-batches 4)
    corpus = oracle.synth_rows(SEED, 0, N, D)
    queries = oracle.synth_rows(SEED, (1 << 40) + ((WARMUP + STEPS - 1) % 4) * NQ, NQ, D)
    for qi in (0, 151, NQ - 1):
        rows, sims, _, _ = oracle.scan_cosine(corpus, queries[qi], K, -1.0)
        assert np.array_equal(got["rows"][qi], rows.astype(np.float64)), qi
        assert np.array_equal(got["scores"][qi].view(np.uint32), sims.view(np.uint32)), qi
