"""The filter kernels track their LDS-DMA pieces with hand-counted `s_waitcnt vmcnt(N)`: a register spill inside
their k loops would put scratch loads / stores (VMEM operations the count does not know about) between the pieces
and the waits.  So "no scratch traffic between the first and the last MFMA" is a correctness property of these
kernels, checked here on the gfx950 assembly (hipcc cross-compiles without a GPU); the int8 kernels — the bench's
dominant kernel family — must not use scratch at all."""
import os
import re
import shutil

import pytest

from _kernel_asm import kernel_asm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="needs hipcc")
@pytest.mark.parametrize("src,kernel,lds,sgpr_spills", [("kmeans_kernels.hip", "kmeans_assign_kernel", 25088, (0, 0)),
                                                        ("semgraph_kernels.hip", "semgraph_pairs_kernel", 25152, (0, 6))])
def test_the_fp64_tile_kernels_keep_three_waves_their_lds_and_no_scratch(src, kernel, lds, sgpr_spills):
    """kmeans_assign_kernel and semgraph_pairs_kernel share their hot loop (fp64_tile.h) as an inlined function, and how that
    function is shaped moves the register allocation.  Both forms of both kernels (vector and scalar loads) must stay where they
    were measured: at most 168 registers — a SIMD has 512 registers per lane, handed out in granules of 8, so 168 is the most
    that leaves three waves per SIMD (3 x 168 = 504; 176 would leave two) — no scratch (private segment 0, no spill, no
    scratch_ instruction) and the static LDS of the two operand buffers (+ 64 bytes of counters in the pairs kernel).
    sgpr_spills = (vector form, scalar form): scalar registers parked in lanes of a vector register, never in memory; the
    scalar-load form of the pairs kernel has had six since it was written, the other three forms none."""
    meta = {k: v for k, v in kernel_asm(src).meta.items() if kernel in k}
    bodies = {k: v for k, v in kernel_asm(src).kernels.items() if kernel in k}
    assert len(meta) == 2 and set(meta) == set(bodies), (list(meta), list(bodies))
    assert {("ILb1E" in k) for k in meta} == {True, False}, list(meta)       # <VEC = true> and <VEC = false>
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] <= sgpr_spills["ILb0E" in name], (name, m)
        assert not any("scratch_" in l for l in bodies[name]), name
        assert m["group_segment_fixed_size"] == lds, (name, m)
        assert m.get("agpr_count", 0) == 0 and m["vgpr_count"] <= 168, (name, m)


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="needs hipcc")
@pytest.mark.parametrize("src,kernel,counters,waves", [
    # entity_score_kernel: two counters per query; <1> and <4> ship at four waves per SIMD, <8> (17 fp64 sums per lane beside
    # the eight float4 of the next chunk) at three
    ("entity_kernels.hip", "entity_score_kernel", 2, {1: 4, 4: 4, 8: 3}),
    # doc_score_kernel: one counter per query; the same core and the same classes — <8> gave up the fourth wave its 76
    # registers allowed before it prefetched (DESIGN 3.7 has the measurement that accepted it)
    ("doc_kernels.hip", "doc_score_kernel", 1, {1: 4, 4: 4, 8: 3})])
def test_the_row_chain_kernels_keep_their_waves_their_lds_and_no_scratch(src, kernel, counters, waves):
    """doc_score_kernel and entity_score_kernel share their staging and their chains (row_chains.h) as an inlined function.
    All three forms of each (QG = 1, 4, 8 queries per workgroup) must exist, use no scratch (private segment 0, no register
    spilled) and the static LDS the shared constants give: the padded rows, the query tile and the ordinals, plus the
    kernel's own counters.  Registers: by the arithmetic of the fp64-tile case above (512 per lane, granules of 8), at most
    128 leave four waves per SIMD — what the LDS of four workgroups per CU allows anyway — and at most 168 leave three."""
    header = open(os.path.join(ROOT, "yams_amd", "csrc", "row_chains.h")).read()
    c = {k: int(v) for k, v in re.findall(r"constexpr\s+int\s+(kRow\w+)\s*=\s*(\d+)\s*;", header)}
    assert {"kRowThreads", "kRowChunk"} <= set(c), c      # (the row stride is the chunk padded by one float: the LDS figure below)
    meta = {k: v for k, v in kernel_asm(src).meta.items() if kernel in k}
    assert len(meta) == 3, list(meta)
    for qg, w in waves.items():
        name = [k for k in meta if "%sILi%dEE" % (kernel, qg) in k]
        assert len(name) == 1, (qg, list(meta))
        m = meta[name[0]]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        lds = 4 * (c["kRowThreads"] * (c["kRowChunk"] + 1) + qg * c["kRowChunk"] + c["kRowThreads"] + counters * qg)
        assert m["group_segment_fixed_size"] == lds, (name, m, lds)
        assert m.get("agpr_count", 0) == 0 and m["vgpr_count"] <= {4: 128, 3: 168}[w], (name, m)


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="needs hipcc")
@pytest.mark.parametrize("src", ["scan_i8_kernel.hip", "scan_bf16_kernel.hip"])
def test_no_scratch_traffic_inside_the_mfma_loops(src):
    tiles = {k: v for k, v in kernel_asm(src).kernels.items() if "scan_tiles" in k}
    assert tiles
    for name, body in tiles.items():
        mf = [i for i, l in enumerate(body) if "v_mfma" in l]
        assert mf, name
        inside = [l.strip() for l in body[mf[0]:mf[-1] + 1] if "scratch_" in l]
        assert not inside, (name, inside[:3])
        if src == "scan_i8_kernel.hip":
            assert not any("scratch_" in l for l in body), name
    if src == "scan_i8_kernel.hip":     # both metrics of both kernel forms are there
        for frag in ("scan_tiles_i8r_kernelILi0ELb0ELb0", "scan_tiles_i8r_kernelILi0ELb1ELb0", "scan_tiles_i8r_kernelILi0ELb0ELb1",
                     "scan_tiles_i8r_kernelILi0ELb1ELb1", "scan_tiles_i8h_kernelILi1ELi0ELi0",
                     "scan_tiles_i8h_kernelILi1ELi0ELi1", "scan_tiles_i8h_kernelILi0ELi0ELi1"):
            assert any(frag in k for k in tiles), frag


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="needs hipcc")
def test_direct_row_loads_are_not_touched_while_in_flight():
    """The direct form of the resident-query filter (scan_tiles_i8r_kernel<..., DIRECT>) loads the next slab's row
    fragments from inline asm into registers the compiler owns, and only an s_waitcnt vmcnt(0) at the head of the next
    slab makes them valid.  Nothing the compiler puts in between — a copy at a loop edge, a spill, a reuse — may read or
    write those registers: checked on the assembly in program order (a linear walk; the kernel's loops are the unrolled
    slab pairs, so program order is what matters between a load and its wait)."""
    kernels = {k: v for k, v in kernel_asm("scan_i8_kernel.hip").kernels.items() if "scan_tiles_i8r_kernel" in k and "ELb1ELi" in k}   # <ABL, L2, DIRECT = true, ZSM>
    assert len(kernels) == 3, list(kernels)      # the cosine filter, the L2 filter, the cosine SAMPLE pass

    def regs(tok):
        tok = tok.strip().split()[0] if tok.strip() else ""
        m = re.match(r"v\[(\d+):(\d+)\]$", tok)
        if m:
            return list(range(int(m.group(1)), int(m.group(2)) + 1))
        m = re.match(r"v(\d+)$", tok)
        return [int(m.group(1))] if m else []
    for name, body in kernels.items():
        inflight, loads = {}, 0
        for line in body:
            t = line.split(";")[0].strip()
            if not t or t.startswith(".") or t.endswith(":"):
                continue
            ops = t.split(None, 1)
            if ops[0] == "global_load_dwordx4":
                for r in regs(ops[1].split(",")[0]):
                    inflight[r] = t
                loads += 1
                continue
            if ops[0] == "s_waitcnt" and "vmcnt(0)" in t:
                inflight.clear()
                continue
            if len(ops) < 2:
                continue
            toks = [x for x in ops[1].split(",")]
            stores = ops[0].startswith(("global_store", "ds_write", "scratch_store", "global_atomic"))
            for tok in (toks if stores else toks[1:]):
                for r in regs(tok):
                    assert r not in inflight, (name, "reads in-flight v%d" % r, t, inflight[r])
            if not stores and not ops[0].startswith("s_"):
                for r in regs(toks[0]):
                    assert r not in inflight, (name, "writes in-flight v%d" % r, t, inflight[r])
        assert loads >= 12, (name, loads)       # prologue + two slabs of the loop body, four fragments each


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="needs hipcc")
def test_deep_form_row_loads_are_not_touched_while_in_flight():
    """scan_tiles_i8d_kernel keeps TWO slabs of row fragments in flight per wave and waits for them with COUNTED waits
    (`s_waitcnt vmcnt(4)`: the four loads of the slab one ahead may stay out).  Its vector-memory operations retire in
    order, so a walk over the assembly with a FIFO of outstanding operations knows, at every instruction, which registers
    still have a load due: nothing may read or write them — not a copy, not a spill, not a temporary the allocator parks
    there (round 6: the flush after the last strip did exactly that and stored through an overwritten address; a bus error
    on shards of 4M rows and more).  The kernel must not use scratch at all."""
    kernels = {k: v for k, v in kernel_asm("scan_i8_kernel.hip").kernels.items() if "scan_tiles_i8d_kernel" in k}
    assert len(kernels) == 1, list(kernels)

    def regs(tok):
        tok = tok.strip().split()[0] if tok.strip() else ""
        m = re.match(r"v\[(\d+):(\d+)\]$", tok)
        if m:
            return list(range(int(m.group(1)), int(m.group(2)) + 1))
        m = re.match(r"v(\d+)$", tok)
        return [int(m.group(1))] if m else []
    for name, body in kernels.items():
        assert not any("scratch_" in l for l in body), name
        fifo, loads, counted = [], 0, 0
        for line in body:
            t = line.split(";")[0].strip()
            if not t or t.startswith(".") or t.endswith(":"):
                continue
            ops = t.split(None, 1)
            op = ops[0]
            toks = ops[1].split(",") if len(ops) > 1 else []
            busy = {r: txt for rs, txt in fifo for r in rs}
            vm_load = op.startswith(("global_load", "global_atomic")) and not op.startswith("global_load_lds")
            vm_other = op.startswith(("global_store", "global_load_lds", "buffer_", "flat_"))
            if op == "s_waitcnt":
                m = re.search(r"vmcnt\((\d+)\)", t)
                if m:
                    keep = int(m.group(1))
                    counted += keep == 4
                    while len(fifo) > keep:
                        fifo.pop(0)
                continue
            sources = toks if (vm_other or op.startswith(("ds_write", "global_atomic"))) else toks[1:]
            for tok in sources:
                for r in regs(tok):
                    assert r not in busy, (name, "reads in-flight v%d" % r, t, busy[r])
            if vm_load:
                dst = regs(toks[0]) if not op.startswith("global_atomic") or len(toks) >= 4 else []
                for r in dst:
                    assert r not in busy, (name, "loads into in-flight v%d" % r, t, busy[r])
                fifo.append((dst, t)); loads += op == "global_load_dwordx4"
                continue
            if vm_other:
                fifo.append(([], t))
                continue
            if toks and not op.startswith("s_"):
                for r in regs(toks[0]):
                    assert r not in busy, (name, "writes in-flight v%d" % r, t, busy[r])
        assert loads >= 8 + 12 and counted >= 4, (name, loads, counted)    # pipeline fill + three unrolled slabs; the counted waits are there
