"""sgc_kernels.hip compiled for gfx950 with the product flags: the hop kernel's code-object metadata shows no private segment
(no scratch) in the vector-load form, the element-load form and the hub form; the adds of a chain are plain (or two-wide packed) fp32 adds, nothing
fused into them, and the products are fp64 multiplies; no kernel of the file uses an atomic on a float."""
import os
import re
import shutil

import pytest

from _kernel_asm import kernel_asm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FORMS = {"vector loads": "sgc_hop_kernelILi4ELb1ELb0E", "element loads": "sgc_hop_kernelILi4ELb0ELb0E", "hub rows": "sgc_hop_kernelILi1ELb0ELb1E"}


@pytest.fixture(scope="module")
def assembly():
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.fail("hipcc is needed to compile sgc_kernels.hip")
    kernels, _, text = kernel_asm("sgc_kernels.hip")
    meta = {}
    for block in text.split("- .agpr_count:")[1:] if "- .agpr_count:" in text else []:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            meta[name.group(1)] = block
    return kernels, meta, text


@pytest.mark.parametrize("form", sorted(FORMS))
def test_hop_kernel_has_no_private_segment(assembly, form):
    kernels, meta, text = assembly
    names = [k for k in kernels if FORMS[form] in k]
    assert len(names) == 1, (form, sorted(kernels))
    body = kernels[names[0]]
    assert not any("scratch_" in l for l in body), form
    sizes = re.findall(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", text.split(".amdhsa_kernel " + names[0])[1].split(".end_amdhsa_kernel")[0])
    assert sizes == ["0"], (form, sizes)
    if names[0] in meta:
        assert re.search(r"\.private_segment_fixed_size:\s*0\b", meta[names[0]]), form
    # the arithmetic of a chain: fp64 products, fp32 adds, nothing fused, no matrix core
    assert any(re.search(r"\bv_mul_f64", l) for l in body) and any(re.search(r"\bv_(pk_)?add_f32", l) for l in body), form
    # (v_fma_f32 may appear: the 24-bit integer division that deals threads to rows is computed in floats)
    assert not any(re.search(r"\bv_fmac?_f64|v_mfma|v_pk_fma|\bv_(fmac|mac)_f32", l) for l in body), form
    chain = [l for l in body if re.search(r"\bv_(pk_)?add_f32|\bv_fma_f32", l)]
    assert sum("add_f32" in l for l in chain) >= 5 and sum("v_fma_f32" in l for l in chain) <= 2, (form, chain)
    assert not any("atomic" in l for l in body), form
    if form == "vector loads":
        assert any("global_load_dwordx4" in l for l in body) and any("global_store_dwordx4" in l for l in body)


def test_every_kernel_of_the_file_is_scratch_free_and_sums_without_float_atomics(assembly):
    kernels, _, text = assembly
    assert len(kernels) == 7, sorted(kernels)
    assert set(re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)) == {"0"}
    for name, body in kernels.items():
        assert not any(re.search(r"atomic_(add|pk_add|fadd)_f(32|64)|atomic_fadd", l) for l in body), name
