"""embed_kernels.hip compiled for gfx950 with the product flags: every kernel keeps f32 and f64 denormals, rounds to nearest,
uses no scratch and spills nothing; the static LDS is what the source declares — the window's list of active token indices
(kEmbedWindow words, whatever the sequence length) for the pooling kernels, one chunk of a row and the norm for the normalise
kernel; no kernel needs more than 128 registers; THE CHAINS ARE REAL — the MEAN kernels add and hold no f32 fma or mac (nothing
was contracted; the divide is the finish kernel's), the MAX and CLS kernels hold no f32 arithmetic at all; the vector kernels load 16 bytes; no float
atomics anywhere."""
import os
import re
import shutil

import pytest

from _kernel_asm import kernel_asm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
POOL = {(mode, vec): "embed_pool_kernelILj%dELi%dEE" % (mode, vec) for mode in (0, 1, 2) for vec in (4, 1)}
KERNELS = list(POOL.values()) + ["embed_check_kernel", "embed_finish_kernel"]
ADD = re.compile(r"\bv_(pk_)?add_f32")
MUL = re.compile(r"\bv_(pk_)?mul_f32")
FMA = re.compile(r"\bv_(pk_)?(fma|fmac|mad|mac|madak|madmk|fmaak|fmamk)_f32")


@pytest.fixture(scope="module")
def assembly():
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.fail("hipcc is needed to compile embed_kernels.hip")
    return kernel_asm("embed_kernels.hip")


def named(table, part):
    hits = [n for n in table if part in n]
    assert len(hits) == 1, (part, hits)
    return hits[0]


def constant(name):
    launch = open(os.path.join(ROOT, "yams_amd", "csrc", "embed_launch.h")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, launch).group(1))


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
        assert m["vgpr_count"] <= 128, (name, m)


def test_static_lds_is_the_fixed_sizes_the_source_declares(assembly):
    _, meta, _ = assembly
    lds = {k: meta[named(meta, k)]["group_segment_fixed_size"] for k in KERNELS}
    window, chunk = constant("kEmbedWindow"), constant("kEmbedNormChunk")
    for (mode, vec), k in POOL.items():
        assert lds[k] == (0 if mode == 0 else window * 4), (k, lds[k])      # CLS reads no mask: no list
    assert lds["embed_finish_kernel"] == chunk * 4 + 8, lds              # one chunk of the row and the norm
    assert lds["embed_check_kernel"] == 0, lds


def test_the_chains_are_real(assembly):
    """A MEAN lane adds kEmbedAhead rows of its 4 (or 1) dimensions per step of the unrolled loop: f32 adds and NO f32 fma or mac
    of any kind — nothing was contracted, and the divide (whose refinement fuses) is the finish kernel's.  MAX compares and
    selects, CLS copies: no f32 arithmetic.  The finish kernel holds the IEEE divide and the fp64 chain: an f64 multiply and
    an f64 add."""
    kernels, _, _ = assembly

    def count(body, rx):
        return sum(2 if m.group(1) else 1 for l in body for m in [rx.search(l)] if m)
    ahead = constant("kEmbedAhead")
    for (mode, vec), k in POOL.items():
        body = kernels[named(kernels, k)]
        assert count(body, FMA) == 0 and count(body, MUL) == 0 and not any("v_div_" in l or "v_rcp_" in l for l in body), k
        assert (count(body, ADD) >= ahead * vec) if mode == 2 else (count(body, ADD) == 0), (k, count(body, ADD))
        if mode != 0:
            assert any("ds_read" in l or "ds_load" in l for l in body), k      # the list of active tokens
    for vec in (4, 1):
        for mode in (1, 2):
            wide = sum("global_load_dwordx4" in l for l in kernels[named(kernels, POOL[(mode, vec)])])
            assert (wide >= ahead) if vec == 4 else (wide == 0), (mode, vec, wide)
    finish = kernels[named(kernels, "embed_finish_kernel")]
    assert any("v_div_scale_f32" in l for l in finish) and any("v_div_fixup_f32" in l for l in finish)      # v / total
    assert any("v_div_scale_f64" in l for l in finish) and any("v_sqrt_f64" in l or "v_rsq_f64" in l for l in finish)
    assert any("v_add_f64" in l for l in finish) and any("v_mul_f64" in l for l in finish)                    # the chain of squares
