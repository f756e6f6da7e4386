"""The device semantic-neighbour graph (yams_graph_semantic_neighbors_device / _host, semantic_graph_v1) without a GPU: the
numpy restatement equals, bit for bit, what the reference's own pair loop produced on every golden case
(tests/golden/semantic_neighbors.json); the golden cases reach the edges they are there for; header, exports and the index
agree; the argument checks that need no device answer as documented; the interface table is served and absent from the
manifest; the adapter, compiled with plain g++ over a stub of the entry, reproduces edges, weights, ranks and order; the stress
harness draws its cases and its comparison tells a flipped bit; and semgraph_kernels.hip, compiled for gfx950, runs its pair
chains on fp64 fused multiply-adds without scratch."""
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

import _semgraph_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
GOLDEN_PATH = os.path.join(ROOT, "tests", "golden", "semantic_neighbors.json")
GOLDEN = {c["name"]: c for c in json.load(open(GOLDEN_PATH))["cases"]}
CASES = so.golden_cases()


def build_semgraph_test():
    """Compiles tests/cpp/semgraph_test.cpp (plain g++; it dlopens the plugin at run time).  Returns the executable."""
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "semgraph_test")
    src = os.path.join(ROOT, "tests", "cpp", "semgraph_test.cpp")
    deps = [src, os.path.join(ROOT, "include", "yams_mi355x_accel.h")] + \
        [os.path.join(ROOT, "include", "yams_accel", f) for f in os.listdir(os.path.join(ROOT, "include", "yams_accel"))]
    if os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in deps):
        return exe
    r = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++20", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe, src, "-ldl"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        raise RuntimeError("semgraph_test failed to compile:\n" + r.stdout.decode())
    return exe


def write_adapter_cases():
    """The golden cases as the text tests/cpp/semgraph_test.cpp reads: the records in stream order — with a later record
    under the hash of row 0 (first hash wins), one without a hash and one without an embedding, all three to be ignored —
    and the edges the reference's loop leaves: sources in corpus order, similarity and effective threshold as recorded, weight
    = clamp(similarity, effective, 1), rank = position + 1."""
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "semgraph_cases.txt")
    with open(path, "w") as f:
        for name in sorted(CASES):
            c, v = GOLDEN[name], CASES[name]
            n, dim = v["rows"].shape
            src = None if v["sources"] is None else sorted(v["sources"])
            thr = v["threshold"]
            f.write(f"CASE {name} {n + 3} {dim} {v['k']} {0 if thr is None else 1} {c['threshold_bits'] or 0} {-1 if src is None else len(src)}\n")
            for h, r in zip(v["hashes"], c["rows_bits"]):
                f.write(f"{h} {dim} " + " ".join(map(str, r)) + "\n")
            f.write(f"{v['hashes'][0]} {dim} " + " ".join(map(str, so.bits(np.arange(1, dim + 1, dtype=np.float32)).tolist())) + "\n")
            f.write(f"- {dim} " + " ".join(map(str, so.bits(np.ones(dim, np.float32)).tolist())) + "\n")
            f.write("0" * 64 + " 0\n")
            if src is not None:
                f.write(" ".join(v["hashes"][s] for s in src) + "\n")
            edges = []
            for s in (range(n) if src is None else src):
                lst = c["neighbors"].get(str(s), [])
                if not lst:
                    continue
                eff = so.f32([c["effective_threshold_bits"][str(s)]])[0]
                for j, (r, b) in enumerate(lst):
                    sim = so.f32([b])[0]
                    w = eff if sim < eff else np.float32(1.0) if np.float32(1.0) < sim else sim       # std::clamp(sim, eff, 1.0f)
                    edges.append(f"{v['hashes'][s]} {v['hashes'][r]} {b} {int(so.bits(w)[0])} {j + 1}")
            f.write(f"EDGES {len(edges)}\n" + "".join(e + "\n" for e in edges))
            f.write(f"COUNTS {c['pairs_scored']} {c['pairs_admitted']}\n")
    return path


# ---- the restatement against the reference's own loop -------------------------------------------------------------------------
def test_the_golden_file_covers_the_cases_and_stays_small():
    assert set(GOLDEN) == set(CASES) and len(CASES) >= 12
    assert os.path.getsize(GOLDEN_PATH) < 64 * 1024
    for name, v in CASES.items():
        c = GOLDEN[name]
        assert c["rows_bits"] == so.bits(v["rows"]).tolist() and c["hashes"] == v["hashes"], name      # the recipe still gives the recorded bits
        assert (c["k"], c["sources"]) == (v["k"], v["sources"])
        assert c["threshold_bits"] == (None if v["threshold"] is None else int(so.bits(np.float32(v["threshold"]))[0]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_equals_the_reference_loop_bit_for_bit(name):
    c, v = GOLDEN[name], CASES[name]
    r = so.run_case(v)
    assert so.bits(r["inv"]).tolist() == c["inv_bits"]
    assert (r["pairs_scored"], r["pairs_admitted"]) == (c["pairs_scored"], c["pairs_admitted"])
    src = list(range(len(v["rows"]))) if v["sources"] is None else v["sources"]
    eff = so.effective_thresholds(r, v["threshold"])
    for i, s in enumerate(src):
        cnt = int(r["counts"][i])
        got = [[int(a), int(b)] for a, b in zip(r["rows"][i, :cnt], so.bits(r["sims"][i, :cnt]))]
        assert got == c["neighbors"].get(str(s), []), (name, s)
        assert (r["rows"][i, cnt:] == so.EMPTY_ROW).all() and np.isneginf(r["sims"][i, cnt:]).all()
        if cnt:
            assert int(so.bits(eff[i])[0]) == c["effective_threshold_bits"][str(s)], (name, s)
    assert set(c["neighbors"]) <= {str(s) for s in src}


def test_the_cases_reach_the_edges_they_are_there_for():
    sims = lambda name: np.array([b for lst in GOLDEN[name]["neighbors"].values() for _, b in lst], np.uint32).view(np.float32)
    tiny = np.float32(1.17549435e-38)
    d = sims("denormal_cosine")
    assert ((d > 0) & (d < tiny)).any()                                    # a positive denormal cosine is kept in adaptive mode
    p = sims("zero_plateau_explicit0")
    assert ((p == 0) & np.signbit(p)).any() and ((p == 0) & ~np.signbit(p)).any()      # both zeros stay at threshold 0, signs kept
    assert not (sims("zero_plateau_adaptive") <= 0).any()                   # ... and both go without a threshold
    row0 = GOLDEN["zero_plateau_explicit0"]["neighbors"]["0"]
    zeros = [r for r, b in row0 if so.f32([b])[0] == 0]
    rank = so.rank_of_hashes(CASES["zero_plateau_explicit0"]["hashes"])
    assert len(zeros) >= 3 and [int(rank[r]) for r in zeros] == sorted(int(rank[r]) for r in zeros)   # one score: the hash decides
    assert zeros != sorted(zeros)                                           # ... against row order
    inv = so.f32(GOLDEN["flt_max_quarter"]["inv_bits"])
    assert ((inv > 0) & (inv < tiny)).any()                                 # a denormal inverse norm is served
    assert 0 in GOLDEN["zero_rows"]["inv_bits"] and "2" not in GOLDEN["zero_rows"]["neighbors"]
    few = GOLDEN["fewer_than_k"]
    assert few["k"] == 8 and few["neighbors"] and all(1 <= len(l) <= 4 for l in few["neighbors"].values())
    assert all(len(l) == 1 for l in GOLDEN["k1"]["neighbors"].values())
    dup = GOLDEN["duplicates"]["neighbors"]["0"]
    assert dup[0][1] == dup[1][1] and {dup[0][0], dup[1][0]} == {5, 10}     # identical bits under other hashes are listed
    hr = so.run_case(CASES["hash_reverse"])["rows"]
    assert not np.array_equal(hr, so.neighbors(CASES["hash_reverse"]["rows"], 5)["rows"])          # the hash order matters there
    assert "2" not in GOLDEN["source_subset"]["neighbors"] and set(GOLDEN["source_subset"]["neighbors"]) == {"7", "0", "4"}


def test_refusals_of_the_restatement():
    x = so.uniform_rows(1, 6, 3)
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy(); y[4, 1] = bad
        with pytest.raises(so.InvalidArg):
            so.neighbors(y, 2)
    y = x.copy(); y[2] = np.float32(1e-40)
    with pytest.raises(so.InvalidArg):
        so.neighbors(y, 2)
    with pytest.raises(so.InvalidArg):
        so.neighbors(x, 2, source_rows=[0, 6])
    r = so.neighbors(x[:1], 4)
    assert r["counts"].tolist() == [0] and r["pairs_scored"] == 0


# ---- the surface ---------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_indexed(accel_lib):
    from yams_amd import _lib
    header = open(os.path.join(ROOT, "include", "yams_mi355x_accel.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    index = doc[doc.index("## 8. Index of the flat C ABI"):]
    for s in ("yams_graph_semantic_neighbors_device", "yams_graph_semantic_neighbors_host"):
        assert hasattr(accel_lib, s) and s in _lib.EXPORTS and re.search(r"YAMS_ACCEL_API yams_status_t %s\(" % s, header), s
    assert "yams_graph_semantic_neighbors_device / _host" in index
    assert "#define YAMS_GRAPH_MAX_DIM %du" % _lib.GRAPH_MAX_DIM in header and "#define YAMS_GRAPH_MAX_K %du" % _lib.GRAPH_MAX_K in header
    assert "#define YAMS_GRAPH_FLAG_EXPLICIT_THRESHOLD %du" % _lib.GRAPH_FLAG_EXPLICIT_THRESHOLD in header
    assert C.sizeof(_lib.GraphDiag) == 24
    for line in (":405-415", ":417-431", ":626-632", ":991-997", ":949-954", ":1001-1010"):     # the contract names its lines
        assert line in header, line


def test_semantic_graph_interface_and_refusal_without_a_gpu(accel_lib):
    from yams_amd import _lib
    L = accel_lib
    p = C.c_void_p()
    assert L.yams_plugin_get_interface(b"semantic_graph_v1", 1, C.byref(p)) == 0
    vt = C.cast(p, C.POINTER(_lib.SemanticGraphV1)).contents
    assert vt.abi_version == 1
    for fname, _ in _lib.SemanticGraphV1._fields_[2:]:
        assert getattr(vt, fname), f"semantic_graph_v1.{fname} is NULL"
    for ver in (0, 2):
        q = C.c_void_p()
        assert L.yams_plugin_get_interface(b"semantic_graph_v1", ver, C.byref(q)) == -2      # NOT_FOUND
        assert q.value is None
    m = json.loads(L.yams_plugin_get_manifest_json())                      # the manifest is unchanged
    assert {(i["id"], i["version"]) for i in m["interfaces"]} == {("vector_scan_v1", 1), ("content_hash_v1", 1), ("chunker_v1", 3)}
    if L.yams_accel_device_count() > 0:
        return                                                             # the refusal below is what a CPU-only host sees
    L.yams_plugin_shutdown()
    assert L.yams_plugin_init(b"{}", None) == -3
    x = np.ones((4, 3), np.float32)
    pr = _lib.u32p(); ps = _lib.f32p(); pc = _lib.u32p()
    st = vt.neighbors(None, x.ctypes.data_as(_lib.f32p), 4, 3, None, None, 4, 2, 0, 0.0, C.byref(pr), C.byref(ps), C.byref(pc), None, None)
    assert st == _lib.YAMS_ERR_UNSUPPORTED and not pr                       # it refuses, it does not fall back


def test_argument_validation_that_needs_no_device(accel_lib):
    """The checks in front of the first device call.  A context needs a device, so without one only the null-context refusals
    run."""
    from yams_amd import _lib
    L = accel_lib
    x = np.ones((4, 3), np.float32)
    o_r = np.zeros((4, 2), np.uint32); o_s = np.zeros((4, 2), np.float32); o_c = np.zeros(4, np.uint32)
    for fn in (L.yams_graph_semantic_neighbors_device, L.yams_graph_semantic_neighbors_host):
        assert fn(None, x.ctypes.data, 4, 3, None, None, 4, 2, 0, 0.0, o_r.ctypes.data, o_s.ctypes.data, o_c.ctypes.data, None, None) == _lib.YAMS_ERR_INVALID_ARG
    if L.yams_accel_device_count() <= 0:
        return
    ctx = C.c_void_p()
    assert L.yams_accel_ctx_create(0, None, C.byref(ctx)) == 0
    try:
        for fn in (L.yams_graph_semantic_neighbors_device, L.yams_graph_semantic_neighbors_host):
            diag = _lib.GraphDiag(9, 9, 9, 9)
            call = lambda rows, n, dim, k, flags=0, thr=0.0, out=o_r.ctypes.data, src=None, ns=0: \
                fn(ctx, rows, n, dim, None, src, ns, k, flags, thr, out, o_s.ctypes.data, o_c.ctypes.data, None, C.byref(diag))
            assert call(None, 0, 3, 2) == _lib.YAMS_OK and diag.as_dict() == dict(stripes=0, source_tiles=0, pairs_scored=0, pairs_admitted=0)
            assert call(None, 1, 3, 2) == _lib.YAMS_OK                        # fewer than two rows: empty
            assert call(None, 4, 3, 0) == _lib.YAMS_OK                        # k == 0: empty
            assert call(None, 4, 3, 2, src=o_c.ctypes.data, ns=0) == _lib.YAMS_OK                      # no sources: empty
            assert call(x.ctypes.data, 4, 0, 2) == _lib.YAMS_ERR_INVALID_ARG  # dim == 0
            assert call(None, 4, 3, 2) == _lib.YAMS_ERR_INVALID_ARG           # null rows
            assert call(x.ctypes.data, 4, 3, 2, out=None) == _lib.YAMS_ERR_INVALID_ARG
            assert call(x.ctypes.data, 4, 3, 2, flags=2) == _lib.YAMS_ERR_INVALID_ARG                  # an unknown flag
            assert call(x.ctypes.data, 4, 3, 2, flags=1, thr=float("inf")) == _lib.YAMS_ERR_INVALID_ARG
            assert call(x.ctypes.data, 4, 3, 2, flags=0, thr=float("nan")) == _lib.YAMS_OK             # ignored in adaptive mode
            assert call(x.ctypes.data, 4, _lib.GRAPH_MAX_DIM + 1, 2) == _lib.YAMS_ERR_UNSUPPORTED
            assert call(x.ctypes.data, 1 << 31, 3, 2) == _lib.YAMS_ERR_UNSUPPORTED
            assert call(x.ctypes.data, 4, 3, _lib.GRAPH_MAX_K + 1) == _lib.YAMS_ERR_UNSUPPORTED
    finally:
        L.yams_accel_ctx_destroy(ctx)


# ---- the adapter and the harness -----------------------------------------------------------------------------------------------
def test_adapter_over_a_stub_reproduces_edges_weights_ranks_and_order():
    r = subprocess.run([build_semgraph_test(), write_adapter_cases(), "--stub"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout and f"{len(CASES)} cases" in r.stdout, r.stdout + r.stderr


def test_stress_harness_dry_run_and_self_test():
    script = os.path.join(ROOT, "tests", "stress_semgraph.py")
    r = subprocess.run([sys.executable, script, "--dry-run", "--cases", "150", "--seed", "1"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["mode"] == "dry-run" and res["cases"] == 150 and res["skipped"] == 0
    assert all(v > 0 for v in res["paths"].values()), res["paths"]          # every path the harness names is drawn
    r = subprocess.run([sys.executable, script, "--self-test"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and json.loads(r.stdout.strip().splitlines()[-1]) == {"mode": "self-test", "ok": True}, r.stdout + r.stderr


# ---- the kernels' ISA ------------------------------------------------------------------------------------------------------------
def _kernels():
    """{mangled kernel name: [assembly lines]} of the product build of semgraph_kernels.hip, and the whole text."""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-x", "hip",
               "--cuda-device-only", "-S", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "yams_amd", "csrc"),
               os.path.join(ROOT, "yams_amd", "csrc", "semgraph_kernels.hip"), "-o", out]
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
    for frag in ("semgraph_norm_kernel", "semgraph_check_kernelILb0", "semgraph_check_kernelILb1", "semgraph_pairs_kernelILb1",
                 "semgraph_pairs_kernelILb0", "semgraph_merge_kernel"):
        assert sum(frag in k for k in kernels) == 1, frag
    for name, body in kernels.items():
        assert not any("scratch_" in l for l in body), name                 # no scratch use in any kernel
    meta = "\n".join(text)
    assert set(re.findall(r"\.private_segment_fixed_size:\s*(\d+)", meta)) == {"0"}
    vgprs = dict(zip(re.findall(r"\.name:\s+(_ZN10yams_accel\w+)", meta), map(int, re.findall(r"\.vgpr_count:\s*(\d+)", meta))))
    for name, body in kernels.items():
        if "semgraph_pairs_kernel" in name:
            # the chains: v_fma_f64, or its accumulate form v_fmac_f64 (dst = acc) — 32 chains, the inner loop unrolled twice
            fma = sum(bool(re.search(r"\bv_fmac?_f64", l)) for l in body)
            assert fma >= 64, (name, fma)
            assert not any("v_mfma" in l for l in body), name               # no matrix-core summation order to argue about
            assert vgprs[name] <= 256, (name, vgprs[name])                  # two workgroups per CU (launch bounds 256, 2)
