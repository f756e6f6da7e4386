"""The batched CRC-32 without a GPU: yams_crc32_combine against zlib.crc32 and, for lengths no buffer has, against the
pure-Python model (itself held to zlib by concatenation); known answers; the reference's three implementations recorded in
tests/golden/crc32.json equal zlib (which is what pins "the reference's CRC is the standard one"); the ABI surface and the
content_checksum_v1 door; yams_amd/csrc/crc32_host.h under ASan and UBSan; the kernels' resources from the gfx950
metadata; the stress harness's generator and comparison."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys
import zlib

import numpy as np
import pytest

import _crc32_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = cm.S
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HARNESS = os.path.join(ROOT, "tests", "stress_crc32.py")


def z(b):
    return zlib.crc32(b) & 0xFFFFFFFF


def test_the_model_is_held_to_zlib_by_concatenation():
    rng = np.random.default_rng(1)
    for _ in range(40):
        a = rng.integers(0, 256, int(rng.integers(0, 3 * S)), dtype=np.uint8).tobytes()
        b = rng.integers(0, 256, int(rng.integers(0, 3 * S)), dtype=np.uint8).tobytes()
        assert cm.combine(z(a), z(b), len(b)) == z(a + b)
    for n in (0, 1, 2, 100, S, 1 << 20):
        assert cm.crc_of_zeros(n) == z(bytes(n))


def test_combine_against_zlib_and_the_model(accel_lib):
    L = accel_lib
    rng = np.random.default_rng(2)
    for len_b in (0, 1, 2, S - 1, S, S + 1):
        for _ in range(6):
            a = rng.integers(0, 256, int(rng.integers(0, 2 * S)), dtype=np.uint8).tobytes()
            b = rng.integers(0, 256, len_b, dtype=np.uint8).tobytes()
            assert L.yams_crc32_combine(z(a), z(b), len_b) == z(a + b), (len(a), len_b)
    for _ in range(30):
        buf = rng.integers(0, 256, int(rng.integers(1, 200_000)), dtype=np.uint8).tobytes()
        cut = int(rng.integers(0, len(buf) + 1))
        assert L.yams_crc32_combine(z(buf[:cut]), z(buf[cut:]), len(buf) - cut) == z(buf)
    # lengths no buffer has: against the model
    for len_b in (1 << 31, (1 << 32) + 5, (1 << 40) - 1, 1 << 40):
        for _ in range(3):
            ca, cb = int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32))
            assert L.yams_crc32_combine(ca, cb, len_b) == cm.combine(ca, cb, len_b), len_b
    assert L.yams_crc32_combine(z(b"12345"), cm.crc_of_zeros(1 << 33), 1 << 33) == cm.combine(z(b"12345"), cm.crc_of_zeros(1 << 33), 1 << 33)


KNOWN = [(b"", 0), (b"123456789", 0xCBF43926), (b"a", 0xE8B7BE43), (bytes(32), 0x190A55AD), (b"\xff" * 32, 0xFF6CAB0B)]


def test_known_answers(accel_lib):
    for data, want in KNOWN:
        assert z(data) == want
        # through combine: the message split in two at every position
        for cut in range(len(data) + 1):
            assert accel_lib.yams_crc32_combine(z(data[:cut]), z(data[cut:]), len(data) - cut) == want
    assert cm.crc_of_zeros(4096) == 0xC71C0011 and z(bytes(4096)) == 0xC71C0011
    assert cm.crc_of_zeros(1 << 20) == 0xA738EA1C and z(bytes(1 << 20)) == 0xA738EA1C
    assert accel_lib.yams_crc32_combine(cm.crc_of_zeros(4096), cm.crc_of_zeros((1 << 20) - 4096), (1 << 20) - 4096) == 0xA738EA1C


def test_the_reference_s_three_implementations_are_the_standard_crc32():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_crc32_golden as g
    doc = json.load(open(os.path.join(ROOT, "tests", "golden", "crc32.json")))
    assert len(doc["cases"]) >= 15
    names = set()
    for c in doc["cases"]:
        data = g.case_bytes(c)
        names.add(c["name"])
        want = z(data)
        assert c["stored_object"] == want and c["compression_utils"] == want and c["integrity_validator"] == want, c["name"]
        assert c["update_over_split"] == want and zlib.crc32(data[c["split"]:], z(data[:c["split"]])) & 0xFFFFFFFF == want, c["name"]
    assert {"empty", "check", "zeros_1MiB", "random_4097"} <= names
    # the file holds inputs and results only
    text = open(os.path.join(ROOT, "tests", "golden", "crc32.json")).read()
    assert "#include" not in text and "uint32_t" not in text and "crc >>" not in text


def declared_functions():
    src = open(os.path.join(ROOT, "include", "yams_mi355x_accel.h")).read()
    return set(re.findall(r"YAMS_ACCEL_API\s+[\w\s\*]+?\b(yams_\w+)\s*\(", src))


def test_header_exports_and_binding_agree(accel_lib):
    from yams_amd import _lib
    want = {"yams_crc32_combine", "yams_crc32_batch_device", "yams_crc32_chunks_device", "yams_crc32_verify_device", "yams_crc32_many_host",
            "yams_ingest_host_crc32"}
    assert want <= declared_functions() and want <= set(_lib.EXPORTS)
    for name in want:
        assert hasattr(accel_lib, name), name
    assert _lib.CRC32_SEGMENT_BYTES == S
    launch = open(os.path.join(ROOT, "yams_amd", "csrc", "crc32_launch.h")).read()
    assert "kCrcSegment = YAMS_CRC32_SEGMENT_BYTES" in launch
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = doc[doc.index("## 8. Index of the flat C ABI"):]
    for name in ("yams_crc32_combine", "yams_crc32_batch_device", "content_checksum_v1"):
        assert name in sec, name
    n = int(re.search(r"(\d+) exported symbols", sec).group(1))
    assert n == len(_lib.EXPORTS)


def test_content_checksum_v1_door(accel_lib):
    from yams_amd import _lib
    L = accel_lib
    p = C.c_void_p()
    assert L.yams_plugin_get_interface(b"content_checksum_v1", 2, C.byref(p)) == -2 and p.value is None      # NOT_FOUND
    assert L.yams_plugin_get_interface(b"content_checksum_v1", 0, C.byref(p)) == -2
    assert L.yams_plugin_get_interface(b"content_checksum_v1", 1, C.byref(p)) == 0
    vt = C.cast(p, C.POINTER(_lib.ContentChecksumV1)).contents
    assert vt.abi_version == 1
    for fname, _ in _lib.ContentChecksumV1._fields_[2:]:
        assert getattr(vt, fname), fname
    # the manifest keeps its three entries and their versions
    m = json.loads(L.yams_plugin_get_manifest_json())
    assert {(i["id"], i["version"]) for i in m["interfaces"]} == {("vector_scan_v1", 1), ("content_hash_v1", 1), ("chunker_v1", 3)}
    for name, ver in ((b"content_hash_v1", 1), (b"chunker_v1", 3)):
        assert L.yams_plugin_get_interface(name, ver, C.byref(p)) == 0 and L.yams_plugin_get_interface(name, ver + 1, C.byref(p)) == -2


def test_without_a_gpu_the_door_refuses(accel_lib):
    from yams_amd import _lib
    L = accel_lib
    if L.yams_accel_device_count() > 0:
        pytest.skip("a GPU is visible here; the refusal path is exercised on CPU-only hosts")
    p = C.c_void_p()
    assert L.yams_plugin_get_interface(b"content_checksum_v1", 1, C.byref(p)) == 0
    vt = C.cast(p, C.POINTER(_lib.ContentChecksumV1)).contents
    out = C.c_uint32(7)
    data = (C.c_uint8 * 4)(1, 2, 3, 4)
    assert vt.crc32(None, data, 4, C.byref(out)) == _lib.YAMS_ERR_UNSUPPORTED and out.value == 7
    ptrs = (C.c_void_p * 1)(C.addressof(data))
    lens = (C.c_size_t * 1)(4)
    assert vt.crc32_many(None, ptrs, lens, 1, C.byref(out)) == _lib.YAMS_ERR_UNSUPPORTED and out.value == 7
    valid = (C.c_uint8 * 1)(9)
    assert vt.verify_many(None, ptrs, lens, C.byref(out), 1, valid) == _lib.YAMS_ERR_UNSUPPORTED and valid[0] == 9
    # the flat entries refuse a NULL context whatever else they are given
    assert L.yams_crc32_batch_device(None, None, None, None, 1, None) == _lib.YAMS_ERR_INVALID_ARG
    assert L.yams_crc32_many_host(None, ptrs, lens, 1, C.byref(out)) == _lib.YAMS_ERR_INVALID_ARG
    assert L.yams_crc32_verify_device(None, None, None, None, 1, None, None, None) == _lib.YAMS_ERR_INVALID_ARG
    assert L.yams_crc32_chunks_device(None, None, None, 0, None, None, None) == _lib.YAMS_ERR_INVALID_ARG


def test_crc32_host_logic_under_asan_and_ubsan():
    import _crc32_build
    exe = _crc32_build.build_crc32_host_test()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# static LDS per kernel as DESIGN 3.12 states it
LDS = {"crc32_segments_kernel": 49152, "crc32_fold_kernel": 4096, "crc32_plan_count_kernel": 2048, "crc32_plan_blocks_kernel": 2048,
       "crc32_plan_add_kernel": 0, "crc32_chunk_table_kernel": 0, "crc32_compare_kernel": 0}


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="needs hipcc")
def test_kernel_resources():
    """Every CRC kernel: no scratch (private segment 0, no spill) and the static LDS DESIGN 3.12 states."""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-x", "hip", "--cuda-device-only", "-S",
               os.path.join(ROOT, "yams_amd", "csrc", "crc32_kernels.hip"), "-o", out]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-3000:]
        text = open(out).read().splitlines()
    meta, cur = {}, None
    for line in text:
        if line.startswith("  - ."):
            cur = {}
        m = re.match(r"^(?:  - |    )\.(\w+):\s+(\S+)$", line)
        if cur is None or not m:
            continue
        if m.group(1) == "name":
            meta[m.group(2)] = cur
        elif m.group(2).isdigit():
            cur[m.group(1)] = int(m.group(2))
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("### 3.12"):]
    seen = set()
    for name, m in meta.items():
        kernel = next((k for k in LDS if k in name), None)
        assert kernel, name
        seen.add(kernel)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["group_segment_fixed_size"] == LDS[kernel], (name, m)
        if LDS[kernel]:
            assert re.search(r"%s[^\n]*\b%d\b" % (kernel, LDS[kernel]), sec), (kernel, "DESIGN 3.12 does not state its LDS")
    assert seen == set(LDS)
    assert not [l for l in text if re.match(r"^\s+scratch_", l)]       # no scratch instruction anywhere in the unit


def _run(*args, timeout=600):
    r = subprocess.run([sys.executable, HARNESS, *args], capture_output=True, text=True, timeout=timeout)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert line, r.stdout[-2000:] + r.stderr[-2000:]
    return r.returncode, json.loads(line[-1])


def test_stress_harness_dry_run_reaches_every_path():
    rc, res = _run("--dry-run")
    assert rc == 0 and res["mode"] == "dry-run" and res["cases_run"] == cm.PINNED_CASES == 200 and res["mismatches"] == 0, res
    assert not res["paths_below_floor"] and set(res["paths"]) == set(cm.PATHS), res


def test_stress_harness_self_test_names_every_fault():
    rc, res = _run("--self-test")
    assert rc == 0 and res["ok"] and not res["clean"] and set(res["faults"]) == set(cm.FAULTS), res
