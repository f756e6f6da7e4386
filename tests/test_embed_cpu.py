"""The embedding model's pooling head on the device (yams_embed_*, embedding_pool_v1) without a GPU: the header, the exports and
the bindings agree; the restatements of tests/_embed_oracle.py (numpy, and our C++) equal each other and what the REFERENCE'S
OWN rank-3 batch block and rank-2 block leave in `result` (tests/golden/embed_pool.json, made by
tests/golden/make_embed_golden.py); the stress harness draws only cases it can prove discriminating; the shell
include/yams_accel/embedding_pool.hpp over a stand-in table equals the same file and keeps its own rules, also as a stand-alone
program under AddressSanitizer and UBSan."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import _embed_oracle as eo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_PATH = os.path.join(ROOT, "tests", "golden", "embed_pool.json")
GOLDEN_FILE = json.load(open(GOLDEN_PATH))
GOLDEN = {c["name"]: c for c in GOLDEN_FILE["cases"]}
ENTRIES = ["yams_embed_%s_%s" % (e, t) for e in ("pool", "normalize") for t in ("device", "host")]


def test_header_exports_and_bindings_agree(accel_lib):
    from yams_amd import _lib
    from yams_amd import build as b
    header = open(os.path.join(ROOT, "include", "yams_mi355x_accel.h")).read()
    launch = open(os.path.join(ROOT, "yams_amd", "csrc", "embed_launch.h")).read()
    for name in ENTRIES:
        assert re.search(r"YAMS_ACCEL_API yams_status_t " + name + r"\(", header), name
        assert name in _lib.EXPORTS and hasattr(accel_lib, name), name
    for macro, text, value in (("MAX_DIM", "8192u", _lib.EMBED_MAX_DIM), ("MAX_SEQ", "(1u << 16)", _lib.EMBED_MAX_SEQ),
                               ("MAX_ROWS", "(1ull << 22)", _lib.EMBED_MAX_ROWS), ("POOL_CLS", "0u", _lib.EMBED_POOL_CLS),
                               ("POOL_MAX", "1u", _lib.EMBED_POOL_MAX), ("POOL_MEAN", "2u", _lib.EMBED_POOL_MEAN),
                               ("NORMALIZE", "1u", _lib.EMBED_NORMALIZE)):
        assert re.search(r"#define YAMS_EMBED_%s %s(?=\s)" % (macro, re.escape(text)), header), macro
        assert eval(text.replace("ull", "").replace("u", "")) == value, macro      # the C literal without its suffix
    # 4096-wide models, 512-token texts in batches of 256, 8192-token texts in batches of 64
    assert _lib.EMBED_MAX_DIM >= 4096 and _lib.EMBED_MAX_SEQ >= 8192 and _lib.EMBED_MAX_ROWS >= 256 * 512 and _lib.EMBED_MAX_ROWS >= 64 * 8192
    assert _lib.EMBED_MAX_SEQ < 1 << 24      # the token count of a text is exact in fp32
    for const, value in (("kEmbedSlabDims", _lib.EMBED_SLAB_DIMS), ("kEmbedMinSlabDims", _lib.EMBED_MIN_SLAB_DIMS), ("kEmbedWindow", _lib.EMBED_WINDOW)):
        assert re.search(r"constexpr int %s = %d;" % (const, value), launch), const
    assert (eo.SLAB, eo.MIN_SLAB, eo.WINDOW) == (_lib.EMBED_SLAB_DIMS, _lib.EMBED_MIN_SLAB_DIMS, _lib.EMBED_WINDOW)
    assert (eo.CLS, eo.MAX, eo.MEAN) == (_lib.EMBED_POOL_CLS, _lib.EMBED_POOL_MAX, _lib.EMBED_POOL_MEAN)
    assert '#define YAMS_IFACE_EMBEDDING_POOL_V1 "embedding_pool_v1"' in header and _lib.IFACE_EMBEDDING_POOL_V1 == "embedding_pool_v1"
    assert C.sizeof(_lib.EmbeddingPoolV1) == 16 + 4 * C.sizeof(C.c_void_p)
    assert C.sizeof(_lib.EmbedDiag) == 48
    assert re.search(r"uint32_t mode;.*\n\s*uint32_t flags;.*\n\s*uint64_t batch;.*\n\s*uint32_t seq;.*\n\s*uint32_t dim;.*\n\s*uint64_t tokens_considered;"
                     r".*\n\s*uint64_t active_tokens;.*\n\s*uint32_t slab_dims;", header)
    for name in ("embed_kernels.hip", "embed_api.cpp"):
        assert name in b.SOURCES


def test_interface_table_is_served_at_version_1_only(accel_lib):
    from yams_amd import _lib
    p = C.c_void_p()
    assert accel_lib.yams_plugin_get_interface(b"embedding_pool_v1", 1, C.byref(p)) == 0 and p.value
    vt = C.cast(p, C.POINTER(_lib.EmbeddingPoolV1)).contents
    assert vt.abi_version == 1 and vt.pool and vt.normalize and vt.pool_device and vt.normalize_device
    for version in (0, 2):
        q = C.c_void_p()
        assert accel_lib.yams_plugin_get_interface(b"embedding_pool_v1", version, C.byref(q)) != 0 and not q.value
    assert b"embedding_pool_v1" not in accel_lib.yams_plugin_get_manifest_json()
    if accel_lib.yams_accel_device_count() == 0:      # without a device the door refuses
        assert vt.normalize(None, None, 0, 4, None) == _lib.YAMS_ERR_UNSUPPORTED
        assert vt.pool_device(None, None, 0, 1, 4, None, 0, 0, 0, None, None) == _lib.YAMS_ERR_UNSUPPORTED


def test_a_null_context_is_refused(accel_lib):
    from yams_amd import _lib
    for t in ("device", "host"):
        assert getattr(accel_lib, "yams_embed_pool_" + t)(None, None, 0, 1, 4, None, 0, 0, 0, None, None) == _lib.YAMS_ERR_INVALID_ARG
        assert getattr(accel_lib, "yams_embed_normalize_" + t)(None, None, 0, 4, None) == _lib.YAMS_ERR_INVALID_ARG


def test_the_golden_file_covers_the_cases_and_what_the_tests_rely_on():
    assert os.path.getsize(GOLDEN_PATH) < 256 << 10
    assert [c["name"] for c in GOLDEN_FILE["cases"]] == eo.case_names() and GOLDEN_FILE["builds_agree"] is True
    assert all(GOLDEN[n]["sha256"] == eo.case_digest(n) for n in GOLDEN)
    v = {n: eo.from_hex(GOLDEN[n]["out"]) for n in GOLDEN}
    pool = eo.pool_cases()
    assert {c["mode"] for c in pool.values()} == {eo.CLS, eo.MAX, eo.MEAN}
    assert {3, 7, 511} <= {int((c["mask"][0] > 0).sum()) for c in pool.values() if c["mode"] == eo.MEAN}
    assert np.isfinite(v["nan_masked_mean"]).all() and np.isfinite(v["nan_masked_max"]).all()      # the NaN sat in a masked row
    assert not v["nan_active_mean"][:5].any() and v["nan_active_mean"][5:].any()
    assert not eo.bits(v["all_masked_mean"][:6]).any() and not eo.bits(v["no_mask_mean"]).any()
    assert eo.bits(v["cls_masked_first"][:1])[0] == 0x80000000 and v["cls_masked_first"][1] == np.float32(0.6)
    assert not eo.bits(v["max_all_negative"]).any()
    assert not v["norm_tiny"][:3].any() and v["norm_just_above"][0] > 0.9
    assert v["subnormal_mean"].all() and (np.abs(v["subnormal_mean"]) < 1.2e-38).all()
    assert np.isfinite(v["flt_max_quarter"]).all() and v["flt_max_quarter"][0] > 0.4


def test_both_restatements_equal_the_reference():
    want = eo.nan_blind([c["out"] for c in GOLDEN_FILE["cases"]])
    assert eo.nan_blind(eo.restated()) == want                                          # numpy
    assert eo.nan_blind(eo.restated(eo.pool_cpp, eo.normalize_cpp)) == want             # C++


def test_the_wrong_forms_are_told_apart_by_the_golden_file():
    """Reversed tokens, a pairwise sum and v * (1 / total) each change the bits of several MEAN cases: a kernel that took one of
    these shortcuts could not equal the file."""
    pool = eo.pool_cases()
    means = [n for n, c in pool.items() if c["mode"] == eo.MEAN and c["mask"].shape[1] == c["hidden"].shape[1] and c["hidden"].shape[1] > 2]
    seq = lambda n: pool[n]["hidden"].shape[1]      # noqa: E731
    wrong = {"reversed": lambda n: eo.pool_cpp(pool[n]["hidden"], pool[n]["mask"], eo.MEAN, pool[n]["normalize"], order=np.arange(seq(n) - 1, -1, -1)),
             "pairwise": lambda n: eo.pool_py(pool[n]["hidden"], pool[n]["mask"], eo.MEAN, pool[n]["normalize"], pairwise=True),
             "reciprocal": lambda n: eo.pool_py(pool[n]["hidden"], pool[n]["mask"], eo.MEAN, pool[n]["normalize"], reciprocal=True)}
    told = {k: sum(eo.hexbits(fn(n)) != GOLDEN[n]["out"] for n in means) for k, fn in wrong.items()}
    assert told["reversed"] >= 4 and told["pairwise"] >= 4 and told["reciprocal"] >= 2, told
    for n in ("mean_count_3", "mean_count_7", "mean_count_511"):
        assert eo.hexbits(wrong["reciprocal"](n)) != GOLDEN[n]["out"], n


def test_the_restatements_agree_on_counts_and_orders():
    rng = np.random.default_rng(5)
    x = eo.mixed(rng, (3, 9, 5))
    m = rng.integers(-1, 3, (3, 11)).astype(np.int32)
    for mode in (eo.CLS, eo.MAX, eo.MEAN):
        out, counts = eo.pool_cpp(x, m, mode, True, want_counts=True)
        assert eo.equal(out, eo.pool_py(x, m, mode, True)) and counts == eo.counts_py(x, m, mode), mode      # (weights of 2: fp32 steps, both)
        order = rng.permutation(9)
        assert eo.equal(eo.pool_cpp(x, m, mode, False, order=order), eo.pool_py(x, m, mode, False, order=order.tolist()))
    assert eo.pool_cpp(x, None, eo.MEAN, False, want_counts=True)[1] == (0, 0) and not eo.pool_cpp(x, None, eo.MAX, True).any()


def test_every_stress_case_discriminates():
    """From the oracle alone: every MEAN case changes bits under reversed tokens, every case with a masked token changes bits
    when the masked tokens are admitted, and no case proves neither; the committed seeds need at most 20 redraws."""
    import stress_embed
    cases = stress_embed.draw_all(1, 120)
    for c in cases[::7]:
        rev, adm = eo.discriminates(c)
        assert rev == c["proves_order"] and (adm and c["has_masked"]) == c["proves_mask"]
    assert sum(c["mode"] == eo.MEAN for c in cases) >= 40 and sum(c["has_masked"] for c in cases) >= 60


def test_stress_harness_dry_run_and_self_test():
    script = os.path.join(ROOT, "tests", "stress_embed.py")
    r = subprocess.run([sys.executable, script, "--dry-run"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "dry run OK: 120 cases" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([sys.executable, script, "--self-test"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "self-test OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("sanitize", [False, True])
def test_shell_over_the_stand_in_equals_the_reference(sanitize):
    """AccelEmbeddingPooler over a table backed by the restatement: every golden case reaches the table and equals the file;
    --selftest: ragged masks and a MEAN weight above 1 reach the host loop, everything else the table, the result's shape, the
    error mapping.  sanitize: the same stand-alone program under AddressSanitizer and UBSan."""
    from _embed_build import build_shell_test
    exe = build_shell_test(sanitize=sanitize)
    r = subprocess.run([exe, "--selftest"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "selftest OK" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "cases.bin")
        eo.write_cases(path)
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
        own = subprocess.run([exe, "--host-loop", path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    info, got = eo.parse_driver_output(r.stdout)
    assert info == {"device_calls": len(GOLDEN), "host_calls": 0}, info
    assert eo.nan_blind(got) == eo.nan_blind([c["out"] for c in GOLDEN_FILE["cases"]])
    # the loop the shell carries for what the device refuses equals the reference's loops too
    assert own.returncode == 0, (own.stdout[-1000:], own.stderr[-3000:])
    assert eo.nan_blind(eo.parse_driver_output(own.stdout)[1]) == eo.nan_blind([c["out"] for c in GOLDEN_FILE["cases"]])
