"""The device k-means (yams_cluster_kmeans_device / _host, yams_cluster_assign_device, topology_cluster_v1) without a GPU: the
numpy restatement reproduces every partition the reference's own KMeansTopologyEngine produced (tests/golden/kmeans.json), the
new symbols and the interface table are there, the argument checks that need no device answer as documented, the stress
harness draws its cases, the adapter compiles; and kmeans_kernels.hip, compiled for gfx950, uses no scratch, runs its distance
chains on v_fma_f64 and divides the mean with the IEEE sequence."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import _kmeans_oracle as ko

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "kmeans.json")))
CASES = {c["name"]: c for c in GOLDEN["cases"]}


def build_kmeans_test():
    """Compiles tests/cpp/kmeans_test.cpp (plain g++; it dlopens the plugin at run time).  Returns the executable."""
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "kmeans_test")
    src = os.path.join(ROOT, "tests", "cpp", "kmeans_test.cpp")
    deps = [src, os.path.join(ROOT, "include", "yams_mi355x_accel.h")] + \
        [os.path.join(ROOT, "include", "yams_accel", f) for f in os.listdir(os.path.join(ROOT, "include", "yams_accel"))]
    if os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in deps):
        return exe
    r = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++20", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe, src, "-ldl"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        raise RuntimeError("kmeans_test failed to compile:\n" + r.stdout.decode())
    return exe


def test_the_golden_file_covers_the_cases_and_stays_small():
    assert set(CASES) == set(ko.CASES)
    biggest = max(os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) for f in os.listdir(os.path.join(ROOT, "tests", "golden"))
                  if f != "kmeans.json")
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "kmeans.json")) <= biggest
    for name, c in CASES.items():
        emb = ko.case_rows(name)
        assert (c["k"], c["max_iterations"]) == ko.CASES[name] and c["n"] == len(emb)
        assert ko.rows_digest(emb) == c["sha256"], name               # the recipe still gives the bits the reference saw
        if "rows_bits" in c:
            assert [np.asarray(e, np.float32).view(np.uint32).tolist() for e in emb] == c["rows_bits"], name
        assert sorted(i for g in c["partition"] for i in g) == list(range(len(emb)))


@pytest.mark.parametrize("name", sorted(ko.CASES))
def test_oracle_reproduces_the_reference_partition(name):
    c = CASES[name]
    assert ko.partition(ko.run_shell(ko.case_rows(name), c["k"], c["max_iterations"])) == c["partition"]


def test_the_cases_reach_the_paths_they_are_there_for():
    before = ko.REPAIRS[0]
    rows = np.array(ko.case_rows("duplicates"))
    _, cent, ke, _ = ko.kmeans(rows, 20, 0)
    assert ko.REPAIRS[0] > before and ke == 20                          # duplicate centroids: the repair path ran
    _, cent, _, _ = ko.kmeans(np.array(ko.case_rows("flt_max_quarter")), 4, 0)
    assert np.isnan(cent).any()                                         # the fp32 mean overflowed
    _, cent, _, _ = ko.kmeans(np.array(ko.case_rows("denormal_rows")), 3, 1)
    assert not np.isfinite(cent).all()                                  # 1 / sqrt(norm) overflowed fp32
    assert ko.effective_k(2000, 0) == 45 and ko.effective_k(2, 0) == 2 and ko.effective_k(10, 50) == 10 and ko.effective_k(6, 0) == 2
    assert ko.run_shell([], 0, 0).tolist() == [] and ko.run_shell(ko.case_rows("one_usable_row")).tolist() == [0, 1, 2]


def test_nearest_on_hand_computed_cases():
    rows = np.array([[1, 0], [0, 1], [1, 1], [0, 0]], np.float32)
    cents = np.array([[0, 2], [3, 0], [0, 5], [np.nan, 1]], np.float32)
    a, d = ko.nearest(rows, cents)
    assert a.tolist() == [1, 0, 0, 0]                                   # ties: the lowest index; the zero row: 2.0 from centroid 0
    assert d.tolist()[:2] == [0.0, 0.0] and d[3] == 2.0
    a, d = ko.nearest(rows, cents, np.array([1, 0, 0, 0], np.uint8))
    assert a.tolist() == [1, 2, 1, 1]                                   # centroid 0 skipped
    a, d = ko.nearest(rows[:3], cents[3:])
    assert a.tolist() == [0, 0, 0] and (d == ko.DBL_MAX).all()          # all NaN: 0, bestDist untouched
    a, d = ko.nearest(rows, cents, np.ones(4, np.uint8))
    assert a.tolist() == [0, 0, 0, 0] and (d == ko.DBL_MAX).all()


def test_kmeans_symbols_are_declared_and_exported(accel_lib):
    from yams_amd import _lib
    header = open(os.path.join(ROOT, "include", "yams_mi355x_accel.h")).read()
    for s in ("yams_cluster_kmeans_device", "yams_cluster_kmeans_host", "yams_cluster_assign_device"):
        assert hasattr(accel_lib, s) and s in _lib.EXPORTS and re.search(r"YAMS_ACCEL_API yams_status_t %s\(" % s, header), s
    assert "#define YAMS_CLUSTER_MAX_DIM %du" % _lib.CLUSTER_MAX_DIM in header and "#define YAMS_CLUSTER_MAX_K %du" % _lib.CLUSTER_MAX_K in header


def test_topology_cluster_interface_and_refusal_without_a_gpu(accel_lib):
    from yams_amd import _lib
    L = accel_lib
    p = C.c_void_p()
    assert L.yams_plugin_get_interface(b"topology_cluster_v1", 1, C.byref(p)) == 0
    vt = C.cast(p, C.POINTER(_lib.TopologyClusterV1)).contents
    assert vt.abi_version == 1
    for fname, _ in _lib.TopologyClusterV1._fields_[2:]:
        assert getattr(vt, fname), f"topology_cluster_v1.{fname} is NULL"
    for ver in (0, 2):
        q = C.c_void_p()
        assert L.yams_plugin_get_interface(b"topology_cluster_v1", ver, C.byref(q)) == -2      # NOT_FOUND
        assert q.value is None
    m = json.loads(L.yams_plugin_get_manifest_json())                      # the manifest is unchanged
    assert {(i["id"], i["version"]) for i in m["interfaces"]} == {("vector_scan_v1", 1), ("content_hash_v1", 1), ("chunker_v1", 3)}
    if L.yams_accel_device_count() > 0:
        return                                                             # the refusal below is what a CPU-only host sees
    L.yams_plugin_shutdown()
    assert L.yams_plugin_init(b"{}", None) == -3
    x = np.ones((4, 3), np.float32)
    mem = _lib.u32p(); ke = C.c_uint32(); it = C.c_uint32()
    st = vt.kmeans(None, x.ctypes.data_as(_lib.f32p), 4, 3, 0, 0, C.byref(mem), None, C.byref(ke), C.byref(it))
    assert st == _lib.YAMS_ERR_UNSUPPORTED                                  # it refuses, it does not fall back
    asg = _lib.u32p()
    assert vt.assign(None, x.ctypes.data_as(_lib.f32p), 4, 3, x.ctypes.data_as(_lib.f32p), 4, None, C.byref(asg), None) == _lib.YAMS_ERR_UNSUPPORTED


def test_argument_validation_that_needs_no_device(accel_lib):
    """The checks in front of the first device call, on a context-free call and on a context that was never used.  A context
    needs a device, so without one only the null-context refusals run."""
    from yams_amd import _lib
    L = accel_lib
    x = np.ones((4, 3), np.float32)
    out = np.zeros(4, np.uint32)
    ke = C.c_uint32(7); it = C.c_uint32(7)
    assert L.yams_cluster_kmeans_device(None, x.ctypes.data, 4, 3, 0, 0, out.ctypes.data, None, C.byref(ke), C.byref(it)) == _lib.YAMS_ERR_INVALID_ARG
    assert L.yams_cluster_kmeans_host(None, x.ctypes.data, 4, 3, 0, 0, out.ctypes.data, None, None, None) == _lib.YAMS_ERR_INVALID_ARG
    assert L.yams_cluster_assign_device(None, x.ctypes.data, 4, 3, x.ctypes.data, 4, None, out.ctypes.data, None) == _lib.YAMS_ERR_INVALID_ARG
    if L.yams_accel_device_count() <= 0:
        return
    ctx = C.c_void_p()
    assert L.yams_accel_ctx_create(0, None, C.byref(ctx)) == 0
    try:
        for fn in (L.yams_cluster_kmeans_device, L.yams_cluster_kmeans_host):
            call = lambda rows, n, dim, k, mem: fn(ctx, rows, n, dim, k, 0, mem, None, C.byref(ke), C.byref(it))
            assert call(None, 0, 3, 0, None) == _lib.YAMS_OK and ke.value == 0 and it.value == 0    # n == 0: an empty result
            assert call(x.ctypes.data, 4, 0, 0, out.ctypes.data) == _lib.YAMS_ERR_INVALID_ARG        # dim == 0
            assert call(None, 4, 3, 0, out.ctypes.data) == _lib.YAMS_ERR_INVALID_ARG                 # null rows
            assert call(x.ctypes.data, 1, 3, 0, out.ctypes.data) == _lib.YAMS_ERR_INVALID_ARG        # one row
            assert call(x.ctypes.data, 4, 3, 0, None) == _lib.YAMS_ERR_INVALID_ARG                   # null membership
            assert call(x.ctypes.data, 4, _lib.CLUSTER_MAX_DIM + 1, 0, out.ctypes.data) == _lib.YAMS_ERR_UNSUPPORTED
            assert call(x.ctypes.data, 1 << 31, 3, 0, out.ctypes.data) == _lib.YAMS_ERR_UNSUPPORTED
            assert call(x.ctypes.data, 1 << 20, 3, _lib.CLUSTER_MAX_K + 1, out.ctypes.data) == _lib.YAMS_ERR_UNSUPPORTED
        asg = lambda rows, n, dim, cents, nc, o: L.yams_cluster_assign_device(ctx, rows, n, dim, cents, nc, None, o, None)
        assert asg(None, 0, 3, None, 0, None) == _lib.YAMS_OK
        assert asg(x.ctypes.data, 4, 0, x.ctypes.data, 4, out.ctypes.data) == _lib.YAMS_ERR_INVALID_ARG
        assert asg(x.ctypes.data, 4, 3, None, 4, out.ctypes.data) == _lib.YAMS_ERR_INVALID_ARG
        assert asg(x.ctypes.data, 4, 3, x.ctypes.data, 4, None) == _lib.YAMS_ERR_INVALID_ARG
        assert asg(x.ctypes.data, 4, 3, x.ctypes.data, _lib.CLUSTER_MAX_K + 1, out.ctypes.data) == _lib.YAMS_ERR_UNSUPPORTED
    finally:
        L.yams_accel_ctx_destroy(ctx)


def test_stress_harness_dry_run():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "stress_kmeans.py"), "--dry-run", "--cases", "60", "--seed", "1"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["mode"] == "dry-run" and res["cases"] == 60
    assert all(v > 0 for v in res["paths"].values()), res["paths"]          # every path the harness names is drawn


def test_kmeans_adapter_compiles_and_refuses_without_a_gpu(accel_lib):
    from yams_amd import build as b
    exe = build_kmeans_test()
    if accel_lib.yams_accel_device_count() > 0:
        return                                                             # the GPU suite runs the whole binary
    r = subprocess.run([exe, b.LIB, "--expect-no-gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout + r.stderr


# ---- the kernels' ISA -------------------------------------------------------------------------------------------------------
def _kernels():
    """{mangled kernel name: [assembly lines]} of the product build of kmeans_kernels.hip."""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-x", "hip",
               "--cuda-device-only", "-S", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "yams_amd", "csrc"),
               os.path.join(ROOT, "yams_amd", "csrc", "kmeans_kernels.hip"), "-o", out]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-3000:]
        text = open(out).read().splitlines()
    kernels, cur = {}, None
    for line in text:
        m = re.match(r"^(_ZN10yams_accel\w+):", line)
        if m:
            cur = m.group(1); kernels[cur] = []
        elif cur is not None:
            kernels[cur].append(line.split(";")[0])
            if "s_endpgm" in line:
                cur = None
    return kernels, text


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="needs hipcc")
def test_kernel_resources_and_arithmetic_in_the_isa():
    kernels, text = _kernels()
    names = ["kmeans_norm_kernel", "kmeans_rowdist_kernelILb1", "kmeans_rowdist_kernelILb0", "kmeans_pick_kernel", "kmeans_assign_kernelILb1",
             "kmeans_assign_kernelILb0", "kmeans_hist_kernel", "kmeans_scan_kernel", "kmeans_group_kernel", "kmeans_centroid_kernel"]
    for frag in names:
        assert sum(frag in k for k in kernels) == 1, frag
    for name, body in kernels.items():
        assert not any("scratch_" in l for l in body), name                 # no scratch use in any kernel
    meta = "\n".join(text)
    assert re.findall(r"\.private_segment_fixed_size:\s*(\d+)", meta) and set(re.findall(r"\.private_segment_fixed_size:\s*(\d+)", meta)) == {"0"}
    for name, body in kernels.items():
        if "kmeans_assign_kernel" in name:
            fma = sum("v_fma_f64" in l for l in body)
            assert fma >= 64, (name, fma)                                   # 32 chains, the inner loop unrolled twice
            assert not any("v_mfma" in l for l in body), name               # no matrix-core summation order to argue about
            assert any("v_div_scale_f64" in l for l in body) and any("v_div_fixup_f64" in l for l in body), name
        if "kmeans_centroid_kernel" in name:
            ops = [l.split()[0] for l in body if l.strip() and not l.strip().startswith(".") and not l.strip().endswith(":")]
            # the IEEE divide of the mean: v_div_scale_f32 / v_div_fmas_f32 / v_div_fixup_f32, not a bare reciprocal multiply
            assert ops.count("v_div_scale_f32") >= 2 and "v_div_fmas_f32" in ops and "v_div_fixup_f32" in ops, name
            # the running sum of the mean is fp32 adds, never a fused multiply-add
            assert any(o.startswith("v_add_f32") for o in ops), name
            assert any(o.startswith("v_fma_f64") for o in ops), name         # normalized's fp64 chains
