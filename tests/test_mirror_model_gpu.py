"""Model-based CRUD stress of the vector-store mirror on the device: tests/cpp/mirror_model_test.cpp replays one seeded stream of
inserts / replacements / deletes / compactions into the host model (tests/cpp/mirror_model.hpp) and into AccelVectorTable /
AccelVectorIndex, and compares every search — size, chunk ids in order, score bits, diagnostics counters.  One child process
at a time, each under its own timeout; nothing is retried."""
import signal
import subprocess

import pytest

from test_mirror_model_cpu import SEEDS, build_mirror_model_test, check_coverage, coverage_line

pytestmark = pytest.mark.gpu

CONFIGS = ['{"device":0}', '{"devices":[0,0],"stripe_rows":64}', '{"devices":[0,0,0],"stripe_rows":4096,"search_slots":2}']


def run(args, timeout=280):
    from yams_amd import build as b
    b.build()
    r = subprocess.run([build_mirror_model_test(), b.LIB] + args, capture_output=True, text=True, timeout=timeout)
    if r.returncode < 0:
        pytest.fail("mirror_model_test was ended by signal %s\n%s" % (signal.Signals(-r.returncode).name, r.stdout[-3000:] + r.stderr[-2000:]))
    return r


@pytest.mark.parametrize("config", CONFIGS)
def test_scripted_cases(config):
    """The 4000 / -1500 / +1500 PQ sequence, [a, b, a'] under the vec0 engine, [a(dim 8), a(dim 4)] through the table."""
    r = run(["--config", config, "--seed", "1", "--only-scripted"], timeout=120)
    assert r.returncode == 0 and "OK (0 failures" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    res = coverage_line(r.stdout)
    assert res["compared"] == 6 and res["not_implemented"] == (0 if config == CONFIGS[0] else 3), res


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("config", CONFIGS)
def test_random_stream_against_the_host_model(config, seed):
    r = run(["--config", config, "--seed", str(seed)])
    assert r.returncode == 0 and "OK (0 failures" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
    res = coverage_line(r.stdout)
    assert res["mode"] == "device" and res["seed"] == seed
    check_coverage(res)
    if config == CONFIGS[0]:
        assert res["not_implemented"] == 0, res
    else:
        assert res["not_implemented"] == res["pq"] + res["search_documents"], res
