"""persistence_kernels.hip compiled for gfx950 with the product flags: every kernel keeps f64 (and f32) denormals, uses no
scratch and spills nothing; THE FORM IS REAL — the separate-form pair kernels advance their chains with v_mul_f64 and v_add_f64
and hold no fma that squares a register, the fused-form kernels advance them with such fmas and hold no squaring multiply —;
and the tile kernels keep the two workgroups per CU their shape (fp64_tile.h) is meant for."""
import os
import re
import shutil

import pytest

from _kernel_asm import kernel_asm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def assembly():
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.fail("hipcc is needed to compile persistence_kernels.hip")
    return kernel_asm("persistence_kernels.hip")


def pair_kernels(names):
    """{(vector loads, fused): name}"""
    out = {}
    for n in names:
        m = re.search(r"persist_pairs_kernelILb([01])ELb([01])E", n)
        if m:
            out[(m.group(1) == "1", m.group(2) == "1")] = n
    return out


def test_the_kernels_keep_denormals_and_use_no_scratch(assembly):
    kernels, meta, text = assembly
    # check, pairs <vector / scalar loads> x <fused / separate>, select hist, select pick, boruvka init / vertex / edge / hook / jump
    assert len(kernels) == 12, sorted(kernels)
    for name in kernels:
        desc = text.split(".amdhsa_kernel " + name)[1].split(".end_amdhsa_kernel")[0]
        assert re.findall(r"\.amdhsa_float_denorm_mode_16_64\s+(\d+)", desc) == ["3"], name
        assert re.findall(r"\.amdhsa_float_denorm_mode_32\s+(\d+)", desc) == ["3"], name
        assert re.findall(r"\.amdhsa_float_round_mode_16_64\s+(\d+)", desc) == ["0"], name      # round to nearest even
        assert re.findall(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", desc) == ["0"], name
        m = meta[name]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert not any("scratch_" in l for l in kernels[name]), name
        assert not any(re.search(r"atomic_(add|pk_add|fadd|max|fmax|min|fmin)_f(32|64)|atomic_f(add|max|min)", l) for l in kernels[name]), name
        assert not any("v_mfma" in l for l in kernels[name]), name


def test_the_form_is_real(assembly):
    """The accumulate squares a register pair (d * d), which nothing else in the kernel does: the correctly rounded square
    root of the epilogue is v_rsq_f64 with refinement steps whose fmas and multiplies take different operands.  So the loop's
    step is told apart by its operands.  Separate: at least 32 squaring v_mul_f64 (one per chain of a lane), as many
    v_add_f64 beside the subtractions, and NO squaring fma anywhere: nothing was contracted.  Fused: at least 32 squaring
    v_fma_f64 / v_fmac_f64 and no squaring multiply."""
    kernels, _, _ = assembly
    pairs = pair_kernels(kernels)
    assert sorted(pairs) == [(False, False), (False, True), (True, False), (True, True)], sorted(kernels)
    square_fma = re.compile(r"\bv_fmac?_f64(?:_e32|_e64)?\s+v\[\d+:\d+\],\s*(v\[\d+:\d+\]),\s*\1\s*(?:,|$)")
    square_mul = re.compile(r"\bv_mul_f64(?:_e32|_e64)?\s+v\[\d+:\d+\],\s*(v\[\d+:\d+\]),\s*\1\s*(?:,|$)")
    for (vec, fused), name in pairs.items():
        body = kernels[name]
        n_square_fma = sum(bool(square_fma.search(l)) for l in body)
        n_square_mul = sum(bool(square_mul.search(l)) for l in body)
        n_add = sum(bool(re.search(r"\bv_add_f64", l)) for l in body)
        n_sub = sum(bool(re.search(r"\bv_add_f64(?:_e32|_e64)?\s+v\[\d+:\d+\],\s*v\[\d+:\d+\],\s*-v\[", l)) for l in body)
        assert n_sub >= 32, (name, n_sub)                      # d = a - b (an add with a negated operand)
        if fused:
            assert n_square_fma >= 32 and n_square_mul == 0, (name, n_square_fma, n_square_mul)
        else:
            assert n_square_mul >= 32 and n_add - n_sub >= 32 and n_square_fma == 0, (name, n_square_mul, n_add, n_sub, n_square_fma)


def test_the_tile_kernels_keep_the_occupancy_of_their_shape(assembly):
    """512 registers per lane and SIMD, handed out in granules of 8: 256 threads are one wave per SIMD, so two workgroups per
    CU need at most 256 registers per lane, and no more LDS than the staging of fp64_tile.h (2 x 8 x (130 + 66) doubles)."""
    _, meta, _ = assembly
    pairs = pair_kernels(meta)
    assert len(pairs) == 4
    for name in pairs.values():
        m = meta[name]
        assert m["group_segment_fixed_size"] == 25088 and m.get("agpr_count", 0) == 0 and m["vgpr_count"] <= 168, (name, m)
    trees = [k for k in meta if "persist_boruvka_" in k]
    assert len(trees) == 5, trees
    for name in trees:      # latency- and bandwidth-bound: nothing here may crowd out waves
        assert meta[name]["vgpr_count"] <= 64 and meta[name]["group_segment_fixed_size"] <= 256, (name, meta[name])
