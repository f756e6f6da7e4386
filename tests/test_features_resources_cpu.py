"""features_kernels.hip compiled for gfx950 with the product flags: every kernel keeps f32 and f64 denormals, rounds to nearest,
uses no scratch and spills nothing; the static LDS is what the staging declares (row_chains.h for the ungathered norm, 256 x 33
floats for the gathered one, 4096 bucket counters for the sketch) and nothing where none is declared; no kernel needs so many
registers that fewer than four waves fit a SIMD; THE FORM IS REAL — the separate variance kernel squares with v_mul_f64 and
holds no squaring fma, the fused one squares with an fma and holds no squaring multiply; and no float atomics anywhere (the
sketch counts with integer LDS atomics only)."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ROW_LDS = 256 * 33 * 4            # RowLdsRows / the gather tile: 256 rows x (32 + 1) floats
KERNELS = ["features_aggregate_kernel", "features_variance_kernelILb0E", "features_variance_kernelILb1E", "features_row_nsq_kernel",
           "features_row_nsq_gather_kernel", "features_compose_store_kernel", "features_compose_sketch_kernel"]


@pytest.fixture(scope="module")
def assembly():
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.fail("hipcc is needed to compile features_kernels.hip")
    from yams_amd import build as b
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        cmd = [HIPCC, *[f for f in b.FLAGS if f not in ("-x", "hip")], "-x", "hip", "--cuda-device-only", "-S",
               os.path.join(ROOT, "yams_amd", "csrc", "features_kernels.hip"), "-o", out]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-3000:]
        text = open(out).read()
    kernels, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^(_ZN10yams_accel\w+):", line)
        if m:
            cur = m.group(1); kernels[cur] = []
        elif cur is not None:
            if line.startswith(".Lfunc_end"):
                cur = None
            else:
                kernels[cur].append(line.split(";")[0])
    meta = {}
    for block in text.split("  - .")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            meta[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, re.M)}
    return kernels, meta, text


def named(table, part):
    hits = [n for n in table if part in n]
    assert len(hits) == 1, (part, hits)
    return hits[0]


def test_the_kernels_keep_denormals_and_use_no_scratch(assembly):
    kernels, meta, text = assembly
    assert len(kernels) == len(KERNELS) and all(named(kernels, k) for k in KERNELS), sorted(kernels)
    for name in kernels:
        desc = text.split(".amdhsa_kernel " + name)[1].split(".end_amdhsa_kernel")[0]
        assert re.findall(r"\.amdhsa_float_denorm_mode_16_64\s+(\d+)", desc) == ["3"], name
        assert re.findall(r"\.amdhsa_float_denorm_mode_32\s+(\d+)", desc) == ["3"], name
        assert re.findall(r"\.amdhsa_float_round_mode_32\s+(\d+)", desc) == ["0"], name         # round to nearest even
        assert re.findall(r"\.amdhsa_float_round_mode_16_64\s+(\d+)", desc) == ["0"], name
        assert re.findall(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", desc) == ["0"], name
        m = meta[name]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert not any("scratch_" in l for l in kernels[name]), name
        assert not any(re.search(r"atomic_(add|pk_add|fadd|max|fmax|min|fmin)_f(32|64)|atomic_f(add|max|min)|ds_(add|max|min)_(rtn_)?f", l)
                       for l in kernels[name]), name
        assert not any("v_mfma" in l for l in kernels[name]), name
        # 512 registers per lane and SIMD: four waves per SIMD need at most 128 (these kernels wait on memory or on a chain)
        assert m["vgpr_count"] <= 128 and m.get("agpr_count", 0) == 0, (name, m)


def test_static_lds_is_what_the_staging_declares(assembly):
    _, meta, _ = assembly
    lds = {k: meta[named(meta, k)]["group_segment_fixed_size"] for k in KERNELS}
    for k in ("features_aggregate_kernel", "features_variance_kernelILb0E", "features_variance_kernelILb1E", "features_compose_store_kernel"):
        assert lds[k] == 0, (k, lds[k])
    # row_chains.h: the row tile, the ordinals, and at most the one query tile (no query is read: the compiler may drop it)
    assert ROW_LDS + 256 * 4 <= lds["features_row_nsq_kernel"] <= ROW_LDS + 256 * 4 + 32 * 4, lds
    assert lds["features_row_nsq_gather_kernel"] == ROW_LDS + 32 * 4 + 32 * 4, lds      # the tile, 32 kept columns, 32 weights
    assert lds["features_compose_sketch_kernel"] == 4096 * 4 + 8, lds                   # the bucket counters and the sum of squares
    assert all(v <= 64 << 10 for v in lds.values())


def test_the_sketch_counts_with_integer_lds_atomics(assembly):
    kernels, _, _ = assembly
    body = kernels[named(kernels, "features_compose_sketch_kernel")]
    assert any(re.search(r"\bds_add_(rtn_)?u32", l) for l in body)
    for k in KERNELS:
        if k != "features_compose_sketch_kernel":
            assert not any(re.search(r"\bds_add_|atomic", l) for l in kernels[named(kernels, k)]), k


def test_the_variance_form_is_real(assembly):
    """The variance pass squares a register pair (d * d), which nothing else in the kernel does: the divides' refinement steps
    take different operands.  Separate: one squaring v_mul_f64 per sample row of the unrolled batch and NO squaring fma:
    nothing was contracted.  Fused: as many squaring fmas and no squaring multiply."""
    kernels, _, _ = assembly
    square_fma = re.compile(r"\bv_fmac?_f64(?:_e32|_e64)?\s+v\[\d+:\d+\],\s*(v\[\d+:\d+\]),\s*\1\s*(?:,|$)")
    square_mul = re.compile(r"\bv_mul_f64(?:_e32|_e64)?\s+v\[\d+:\d+\],\s*(v\[\d+:\d+\]),\s*\1\s*(?:,|$)")
    for fused in (False, True):
        body = kernels[named(kernels, "features_variance_kernelILb%dE" % fused)]
        n_fma = sum(bool(square_fma.search(l)) for l in body)
        n_mul = sum(bool(square_mul.search(l)) for l in body)
        if fused:
            assert n_fma >= 8 and n_mul == 0, (n_fma, n_mul)
        else:
            assert n_mul >= 8 and n_fma == 0, (n_fma, n_mul)
