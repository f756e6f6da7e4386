"""rerank_kernels.hip compiled for gfx950 with the product flags: every kernel keeps f32 and f64 denormals, rounds to nearest,
uses no scratch and spills nothing; the static LDS is the fixed tile the staging declares (32 dimensions x (32 query tokens + 288
document-token slots) floats = 40 KiB, whatever the document's length) and the pooled row of the pooling kernel; no kernel needs
so many registers that fewer than four waves fit a SIMD; THE FORM IS REAL — the separate kernel multiplies and adds and holds no
f32 fma, the fused VALU kernel holds f32 fmas and no f32 multiply or add, the MFMA kernel holds v_mfma_f32_32x32x2_f32 and no
other f32 arithmetic; no float atomics anywhere."""
import os
import re
import shutil

import pytest

from _kernel_asm import kernel_asm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
TILE_LDS = 32 * (32 + 288) * 4
SEPARATE, FUSED_VALU, FUSED_MFMA = "rerank_rowmax_kernelILb0ELb0E", "rerank_rowmax_kernelILb1ELb0E", "rerank_rowmax_kernelILb1ELb1E"
KERNELS = [SEPARATE, FUSED_VALU, FUSED_MFMA, "rerank_score_kernel", "rerank_maxpool_kernel", "rerank_check_kernel"]
MUL = re.compile(r"\bv_(pk_)?mul_f32")
ADD = re.compile(r"\bv_(pk_)?add_f32")
FMA = re.compile(r"\bv_(pk_)?(fma|fmac|mad|mac)_f32")
MFMA = re.compile(r"\bv_mfma_f32_32x32x2_f32")


@pytest.fixture(scope="module")
def assembly():
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.fail("hipcc is needed to compile rerank_kernels.hip")
    return kernel_asm("rerank_kernels.hip")


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
        # 512 registers per lane and SIMD: four waves per SIMD need at most 128 (the unified count: the MFMA kernel's 32
        # accumulation registers are inside it)
        assert m["vgpr_count"] <= 128, (name, m)


def test_static_lds_is_one_fixed_tile(assembly):
    _, meta, _ = assembly
    lds = {k: meta[named(meta, k)]["group_segment_fixed_size"] for k in KERNELS}
    for k in (SEPARATE, FUSED_VALU, FUSED_MFMA):
        assert lds[k] == TILE_LDS == 40960, (k, lds[k])      # three workgroups (twelve waves) per CU of 160 KiB
    assert lds["rerank_maxpool_kernel"] == 1024 * 4 + 8, lds      # the pooled row and the norm
    assert lds["rerank_score_kernel"] == 0 and lds["rerank_check_kernel"] == 0, lds


def test_the_form_is_real(assembly):
    """Each i step of a lane's 4 x 8 register tile is 32 chains: the separate kernel holds at least 32 f32 multiplies and 32 f32
    adds (packed ones count for two) and NO f32 fma — nothing was contracted; the fused VALU kernel at least 32 fmas and no f32
    multiply or add at all; the MFMA kernel the two accumulators' v_mfma_f32_32x32x2_f32 and no VALU f32 arithmetic."""
    kernels, _, _ = assembly

    def count(body, rx):
        return sum(2 if m.group(1) else 1 for l in body for m in [rx.search(l)] if m)
    sep, fv, fm = (kernels[named(kernels, k)] for k in (SEPARATE, FUSED_VALU, FUSED_MFMA))
    assert count(sep, MUL) >= 32 and count(sep, ADD) >= 32 and count(sep, FMA) == 0 and count(sep, MFMA) == 0
    assert count(fv, FMA) >= 32 and count(fv, MUL) == 0 and count(fv, ADD) == 0 and count(fv, MFMA) == 0
    assert sum(bool(MFMA.search(l)) for l in fm) >= 2 and count(fm, FMA) == 0 and count(fm, MUL) == 0 and count(fm, ADD) == 0
    for k in ("rerank_score_kernel", "rerank_maxpool_kernel", "rerank_check_kernel"):
        body = kernels[named(kernels, k)]
        assert count(body, FMA) == 0 and not any("v_mfma" in l for l in body), k      # the score chain adds; the norm multiplies and adds in f64
    assert any(ADD.search(l) for l in kernels[named(kernels, "rerank_score_kernel")])


def test_the_mfma_accumulators_start_from_zero_and_are_two(assembly):
    """Two independent accumulators per wave: the unrolled k loop alternates two destination register blocks."""
    kernels, _, _ = assembly
    dests = {m.group(1) for l in kernels[named(kernels, FUSED_MFMA)] for m in [re.search(r"v_mfma_f32_32x32x2_f32\s+([av]\[\d+:\d+\])", l)] if m}
    assert len(dests) >= 2, dests
