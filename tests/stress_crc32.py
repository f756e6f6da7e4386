"""Randomised stress of the batched CRC-32 entry points (yams_crc32_batch_device, yams_crc32_verify_device,
yams_crc32_many_host, yams_crc32_chunks_device after yams_ingest_device) against zlib.crc32 alone.  Test infrastructure;
the generator, the expectation and the comparison live in tests/_crc32_model.py.

    python tests/stress_crc32.py [--cases 200] [--seed 23] [--dry-run] [--keep-going] [--self-test]

All cases run on ONE context in one process, one after the other, so the workspace grows and is reused between entry
points.  Each case draws an entry point, a message count (1, a few, hundreds), a base alignment 0..15, a length class
(tiny, around the segment size, multi-segment, one long message among tiny ones), the content (zeros, FF, random, a
period of 256) and how the messages lie in the buffer (packed, with gaps, overlapping); verify cases plant mismatches at
the first, a middle and the last index, or none, or all; chunk cases run yams_ingest_device over a few blobs first (an empty
one and one below the minimum chunk size among them), hold its chunk table to the CPU chunker, and draw a select mask for
half of them.  Every output sits between sentinel words that must not change.

The harness stops at the first failing case (--keep-going counts them all), never retries a case, and starts nothing more
after a status that is neither OK nor INVALID_ARG.  --dry-run draws the cases, computes the expectation and classifies
them without touching the device.  --self-test (CPU) injects one fault at a time into a correct result and demands that
the comparison names it.  One JSON summary line; exit 1 on a mismatch."""
import argparse, ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import _crc32_model as cm

ap = argparse.ArgumentParser()
ap.add_argument("--cases", type=int, default=cm.PINNED_CASES)
ap.add_argument("--seed", type=int, default=cm.PINNED_SEED)
ap.add_argument("--dry-run", action="store_true")
ap.add_argument("--keep-going", action="store_true", help="count the mismatching cases instead of stopping at the first")
ap.add_argument("--self-test", action="store_true")
a = ap.parse_args()

CHUNK_CFG = dict(min_size=2048, max_size=16384)


def self_test():
    plain, verify, chunks = cm.self_test_cases()
    exp = [0x11111111, 0x22222222, 0x33333333, 0x44444444]
    reported = {}
    clean = []
    for fault in cm.FAULTS:
        case = verify if fault in ("valid_flag", "invalid_count") else chunks if fault == "unselected_nonzero" else plain
        select = [1, 0, 1, 1] if case is chunks else None
        clean += cm.compare(case, exp, cm.perfect_outputs(case, exp, select), select)
        got = cm.perfect_outputs(case, exp, select)
        want = cm.inject(fault, got)
        said = cm.compare(case, exp, got, select)
        reported[fault] = {"want": want, "got": said}
    ok = not clean and all(r["got"] and r["got"][0].startswith(r["want"]) for r in reported.values())
    print(json.dumps({"mode": "self-test", "clean": clean, "faults": reported, "ok": ok}))
    sys.exit(0 if ok else 1)


if a.self_test:
    self_test()

acc = torch = oracle = None
import _oracle
oracle = _oracle.oracle()
if not a.dry_run:
    import torch
    from yams_amd.accel import Accel, cdc_config
    acc = Accel(0, torch.cuda.current_stream().cuda_stream)


def dev(arr):
    return torch.from_numpy(np.ascontiguousarray(arr)).cuda()


def run_case(case, data, offs, lens, exp, select):
    """The device's answer in the shape of perfect_outputs()."""
    n = len(lens)
    entry = case["entry"]
    if entry == "many_host":
        msgs = [data[o:o + m].copy() if m else None for o, m in zip(offs, lens)]     # separate arrays; an empty one is NULL
        ptrs = (C.c_void_p * n)(*[m.ctypes.data if m is not None else None for m in msgs])
        ln = (C.c_size_t * n)(*lens)
        out = np.full(n + 2, cm.SENTINEL, np.uint32)
        st = acc.L.yams_crc32_many_host(acc.ctx, ptrs, ln, n, C.cast(out.ctypes.data + 4, cm_u32p))
        return {"status": st, "crc": out}
    d_data = dev(data)
    n_out = len(exp)            # (for the chunk entry the messages are the chunks, not the blobs handed in)
    out = dev(np.full(n_out + 2, cm.SENTINEL, np.uint32).view(np.int32))      # [sentinel, results, sentinel]
    if entry == "chunks_device":
        res = acc.ingest_device(d_data.data_ptr(), offs, lens, cdc_config("streaming", **CHUNK_CFG), flags=1)
        if int(res.n_chunks) != n_out:       # (the output array is sized by the CPU chunker's count: nothing is launched into it)
            return {"status": cm.OK, "crc": None, "table": None}
        d_sel = dev(np.array(select, np.uint8)) if select is not None else None
        st = acc.L.yams_crc32_chunks_device(acc.ctx, d_data.data_ptr(), np.array(offs, np.uint64).ctypes.data_as(cm_u64p), len(offs),
                                            C.byref(res), d_sel.data_ptr() if d_sel is not None else None, out.data_ptr() + 4)
        got = {"status": st, "crc": out.cpu().numpy().view(np.uint32)}
        tab = acc.fetch_ingest(res, len(offs))
        got["table"] = (tab["chunk_blob"].tolist(), tab["chunk_offset"].tolist(), tab["chunk_size"].tolist())
        return got
    d_off, d_len = dev(np.array(offs, np.uint64).view(np.int64)), dev(np.array(lens, np.uint64).view(np.int64))
    if entry == "batch_device":
        st = acc.L.yams_crc32_batch_device(acc.ctx, d_data.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n, out.data_ptr() + 4)
        return {"status": st, "crc": out.cpu().numpy().view(np.uint32)}
    expected = np.array(exp, np.uint32)
    for i in case["bad"]:
        expected[i] ^= np.uint32(1 << (i % 32))
    d_exp = dev(np.concatenate([[0], expected]).astype(np.uint32).view(np.int32))       # (+ 4 bytes: only 4-byte aligned)
    valid = dev(np.full(n + 2, 0xA5, np.uint8))
    bad = C.c_uint64(0)
    st = acc.L.yams_crc32_verify_device(acc.ctx, d_data.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n, d_exp.data_ptr() + 4,
                                        valid.data_ptr() + 1, C.byref(bad))
    return {"status": st, "crc": None, "valid": valid.cpu().numpy(), "n_invalid": int(bad.value)}


cm_u32p = C.POINTER(C.c_uint32)
cm_u64p = C.POINTER(C.c_uint64)
rng = np.random.default_rng(a.seed)
ledger = {p: 0 for p in cm.PATHS}
bad, fatal = [], None
msgs_total = bytes_total = 0
t_device = 0.0
t0 = time.perf_counter()
case_no = -1
for case_no in range(a.cases):
    case = cm.draw_case(rng, case_no)
    data, offs, lens = cm.materialise(case, rng)
    select = None
    table = None
    if case["entry"] == "chunks_device":
        # the messages are the chunks: the CPU chunker's table is the expectation (and the device's table is held to it)
        blob_offs, blob_lens = offs, lens
        cb, co, cs = [], [], []
        for b, (o, n) in enumerate(zip(blob_offs, blob_lens)):
            if n:
                po, ps = oracle.chunks(data[o:o + n], "streaming", **CHUNK_CFG)
                cb += [b] * len(po); co += po.tolist(); cs += ps.tolist()
        table = (cb, co, cs)
        m_offs, m_lens = [blob_offs[b] + o for b, o in zip(cb, co)], cs
        if case["mask"]:
            select = np.random.default_rng(case["mask_seed"]).integers(0, 2, len(cs)).tolist()
    else:
        m_offs, m_lens = offs, lens
    exp = cm.expect(data, m_offs, m_lens)
    for p in cm.classify(case, m_offs, m_lens):
        ledger[p] += 1
    msgs_total += len(m_lens); bytes_total += sum(m_lens)
    if a.dry_run:
        wrong = cm.compare(case, exp, cm.perfect_outputs(case, exp, select), select)
    else:
        t1 = time.perf_counter()
        got = run_case(case, data, offs, lens, exp, select)
        t_device += time.perf_counter() - t1
        if got["status"] not in (cm.OK, cm.INVALID_ARG):
            fatal = {"case": case_no, "status": got["status"], "error": acc.L.yams_accel_last_error(acc.ctx).decode()}
            break
        wrong = []
        if table is not None and got.get("table") != table:
            wrong.append("the device's chunk table differs from the CPU chunker's")
        else:
            wrong = cm.compare(case, exp, got, select)
    if wrong:
        bad.append({"case": case_no, "wrong": wrong[:5], "entry": case["entry"], "content": case["content"], "class": case["class"],
                    "n": len(m_lens), "layout": case.get("layout"), "base": case["base"]})
        if not a.keep_going:
            break
summary = {"mode": "dry-run" if a.dry_run else "device", "seed": a.seed, "cases": a.cases, "cases_run": case_no + 1,
           "mismatches": len(bad), "fatal": fatal, "messages": msgs_total, "bytes": bytes_total, "paths": ledger,
           "paths_below_floor": [p for p in cm.PATHS if ledger[p] < cm.FLOOR], "device_s": round(t_device, 2),
           "wall_s": round(time.perf_counter() - t0, 2), "first_bad": bad[:3]}
print(json.dumps(summary))
sys.exit(1 if bad or fatal else 0)
