"""The model-based CRUD stress of the vector-store mirror (tests/cpp/mirror_model_test.cpp) without a GPU: the generator and
the host model alone meet the coverage conditions for every committed seed (--dry-run), the model agrees bit for bit with the
reference-compiled table where oracle/_ref travelled (--model-only), its best-row-per-document reduction agrees with the
Python restatement of tests/_doc_select.py, and without a device the plugin refuses and the driver says so."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (1, 2, 3)                      # the seeds the GPU suite replays (tests/test_mirror_model_gpu.py)
SCAN_REF = os.path.join(ROOT, "oracle", "_ref", "libyams_scan_ref.so")


def build_mirror_model_test():
    """Compiles tests/cpp/mirror_model_test.cpp (plain g++; it dlopens the plugin or the reference-compiled table at run time)
    and links it with the oracle's C restatement, as tests/_cpp_build.py links l2_calibration_test.  Returns the executable."""
    import _oracle
    _oracle.build()
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "mirror_model_test")
    so = os.path.join(ROOT, "oracle", "_build", "libyams_oracle.so")
    deps = [os.path.join(ROOT, "tests", "cpp", f) for f in ("mirror_model_test.cpp", "mirror_model.hpp")] + [so, os.path.join(ROOT, "include", "yams_mi355x_accel.h")] + \
        [os.path.join(ROOT, "include", "yams_accel", f) for f in os.listdir(os.path.join(ROOT, "include", "yams_accel"))]
    if os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in deps):
        return exe
    r = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++20", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe, deps[0], so,
                        "-Wl,-rpath," + os.path.dirname(so), "-Wl,-rpath,$ORIGIN/../../../oracle/_build", "-ldl", "-pthread"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        raise RuntimeError("mirror_model_test failed to compile:\n" + r.stdout.decode())
    return exe


def coverage_line(stdout):
    lines = [ln for ln in stdout.splitlines() if ln.startswith("{")]
    assert lines, stdout[-3000:]
    return json.loads(lines[-1])


def check_coverage(res):
    """The conditions of the issue, on the counters the driver prints (it asserts them itself: coverage_missing)."""
    assert res["coverage_missing"] == 0 and res["failures"] == 0 and res["skipped"] == 0 and res["unpinned"] == 0, res
    assert res["compared"] >= 300 and res["compactions_b"] >= 2 and res["compactions_c"] >= 1 and res["big_batch_b"] >= 1, res
    assert res["replacements"] >= 20 and res["repeated_batches"] >= 5 and res["cross_dim_repeats"] >= 1 and res["tie_searches"] >= 10, res
    for kind in ("doc_restriction", "meta_path", "all_matching", "big_k", "search_documents", "pq"):
        assert res[kind] >= 10, (kind, res)
    assert res["empty_index"] >= 1 and res["max_live"] > 20_000 and res["layout_remeasures"] >= 2, res


@pytest.mark.parametrize("seed", SEEDS)
def test_dry_run_meets_the_coverage_conditions(seed):
    r = subprocess.run([build_mirror_model_test(), "--dry-run", "--seed", str(seed)], capture_output=True, text=True, timeout=280)
    assert r.returncode == 0 and "OK (0 failures" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    res = coverage_line(r.stdout)
    assert res["mode"] == "dry-run" and res["seed"] == seed
    check_coverage(res)


@pytest.mark.parametrize("seed", SEEDS)
def test_model_equals_the_reference_compiled_table(seed):
    if not os.path.exists(SCAN_REF):
        pytest.skip("oracle/_ref/libyams_scan_ref.so not present (built only where the reference checkout exists)")
    r = subprocess.run([build_mirror_model_test(), "--model-only", SCAN_REF, "--seed", str(seed)], capture_output=True, text=True, timeout=280)
    assert r.returncode == 0 and "OK (0 failures" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    res = coverage_line(r.stdout)
    print("searches compared with the reference-compiled table:", res["compared"])
    assert res["mode"] == "model-only" and res["failures"] == 0 and res["compared"] >= 100, res
    for kind in ("l2", "doc_restriction", "meta_path", "all_matching", "big_k", "tie_searches", "batches"):
        assert res[kind] >= 10, (kind, res)
    assert res["unpinned"] == res["search_documents"], res     # only the document reduction has no compiled counterpart there


def test_scripted_cases_agree_with_the_reference_compiled_table():
    """[a, b, a'] under the vec0 engine and [a(dim 8), a(dim 4)] alone: small enough to read when they fail."""
    if not os.path.exists(SCAN_REF):
        pytest.skip("oracle/_ref/libyams_scan_ref.so not present (built only where the reference checkout exists)")
    r = subprocess.run([build_mirror_model_test(), "--model-only", SCAN_REF, "--seed", "1", "--only-scripted"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK (0 failures, 3 comparisons)" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_document_reduction_agrees_with_the_python_restatement(tmp_path):
    """The two restatements of retainBestRecordPerDocument (mirror_model.hpp in C++, _doc_select.py in Python) on the cases
    of tests/test_doc_topk_cpu.py's kind: equal scores inside a document and across documents, rows without a document."""
    import _doc_select
    src = tmp_path / "reduce.cpp"
    src.write_text(r'''
#include "mirror_model.hpp"
int main() {
    namespace mm = mirror_model;
    mm::HostModel m;
    const char* docs[] = {"d2", "d1", "", "d1", "d3", "d2", "d3", "d4", "d1", "d4"};
    const char* ids[] = {"c9", "c3", "c5", "c1", "c7", "c2", "c8", "c4", "c0", "c6"};
    const float x[] = {3, 4, 1, 4, 3, 1, 3, 0, 4, 0}, y[] = {4, 3, 0, 3, 4, 0, 4, 1, 3, 1};
    std::vector<mm::Rec> recs;
    for (int i = 0; i < 10; ++i) { mm::Rec r; r.chunk_id = ids[i]; r.document_hash = docs[i]; r.embedding = {x[i], y[i], 0, 0}; recs.push_back(r); }
    m.insertBatch(recs);
    for (size_t k : {1, 2, 3, 10}) for (float thr : {-1.0f, 0.7f}) {
        const auto a = m.documents({1, 0, 0, 0}, k, thr, {});
        std::printf("%zu %g %llu", k, thr, (unsigned long long)a.returned);
        for (const auto& h : a.hits) std::printf(" %s:%08x", h.chunk_id.c_str(), h.bits);
        std::printf("\n");
    }
}''')
    exe = tmp_path / "reduce"
    so = os.path.join(ROOT, "oracle", "_build", "libyams_oracle.so")
    build_mirror_model_test()
    subprocess.run(["g++", "-std=c++20", "-O1", "-I" + os.path.join(ROOT, "tests", "cpp"), "-o", str(exe), str(src), so, "-Wl,-rpath," + os.path.dirname(so)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    docs = ["d2", "d1", "", "d1", "d3", "d2", "d3", "d4", "d1", "d4"]
    ids = ["c9", "c3", "c5", "c1", "c7", "c2", "c8", "c4", "c0", "c6"]
    x = np.array([3, 4, 1, 4, 3, 1, 3, 0, 4, 0], np.float64); y = np.array([4, 3, 0, 3, 4, 0, 4, 1, 3, 1], np.float64)
    scores = (x / np.sqrt(x * x + y * y)).astype(np.float32)
    line = iter(out)
    for k in (1, 2, 3, 10):
        for thr in (-1.0, 0.7):
            keep = [i for i in range(10) if scores[i] >= np.float32(thr)]
            want = _doc_select.best_per_document(keep, [scores[i] for i in keep], [ids[i] for i in keep], [docs[i] for i in keep], k)
            got = next(line).split()
            assert int(got[2]) == len(keep)
            assert got[3:] == ["%s:%08x" % (ids[r], int(np.float32(s).view(np.uint32))) for r, s, _ in want], (k, thr, got, want)


def test_driver_refuses_without_a_gpu(accel_lib):
    from yams_amd import build as b
    exe = build_mirror_model_test()
    if accel_lib.yams_accel_device_count() > 0:
        return                                                             # the GPU suite runs the whole binary
    r = subprocess.run([exe, b.LIB, "--expect-no-gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK (0 failures" in r.stdout, r.stdout + r.stderr
