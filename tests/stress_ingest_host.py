"""Randomised stress of the HOST-memory ingest entry point (yams_ingest_host) against the CPU alone: oracle.chunks for the
boundaries, hashlib for every chunk digest and every blob digest, the reference's own chunker (oracle/_ref, where present)
for every eighth blob.  No device entry point is ever the check of another.  Test infrastructure; the generator, the
batch-partition model, the expectation and the comparison live in tests/_ingest_model.py.

    python tests/stress_ingest_host.py [--cases 96] [--seed 11] [--dry-run] [--keep-going] [--self-test]

All cases run on ONE context in one process, one after the other; a third of them are preceded by a yams_ingest_device call
and a third by a window call (yams_cdc_chunk_window_host) on the same context, so workspace growth and the pool of slot
buffers are crossed between calls.  Each case draws a blob set (1..200 blobs; the special lengths of stress_ingest.py,
log-uniform sizes and multiples of 16; random, constant, short-period, text-like and repeated-segment content), where the
blobs lie in host memory (separate arrays; slices of one buffer back to back, with gaps or at an odd alignment; a pinned
buffer), the chunker (both modes, the configurations of stress_ingest.py on both sides of the narrow kernel's limits, the
generic-kernel flag on a share), flags (0, 1, 2, 3, 3 | DEFER, 2 | DEFER), batch_bytes (one batch, fewer batches than
slots, exactly four, many more than four, 1, smaller than a blob, 0) and the output arrays (ample, exactly the required
size, one slot short, chunk_cap 0 with NULL arrays, NULL out_chunk_digest with the flag set).

Every output array is filled with a sentinel and carries guard words behind its capacity: nothing behind chunk_cap and
nothing behind n_chunks may change.  On the too-small status out_n_chunks must be the required size, out_blob_first
complete and every blob digest correct.  Entries of blobs above yams_ingest_defer_threshold_host are 32 zero bytes.  Where
batch_bytes is given, `batches` and `slots` of device_info()["last_host_ingest"] must equal the model's.

The harness stops at the first failing case (--keep-going counts them all), never retries a case, and starts nothing more
after a HIP error status.  --dry-run draws the cases, computes the CPU expectation and classifies them without touching
the device (mode "dry-run"): the path counts of the summary depend on the generator alone.  --self-test (CPU) injects one
fault at a time into a correct result and demands that the comparison names it.  One JSON summary line; exit 1 on a mismatch.
"""
import argparse, ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import _oracle
import _ingest_model as im

ap = argparse.ArgumentParser()
ap.add_argument("--cases", type=int, default=im.PINNED_CASES)
ap.add_argument("--seed", type=int, default=im.PINNED_SEED)
ap.add_argument("--dry-run", action="store_true")
ap.add_argument("--keep-going", action="store_true", help="count the mismatching cases instead of stopping at the first")
ap.add_argument("--self-test", action="store_true")
a = ap.parse_args()
o = _oracle.oracle()
THREADS = _oracle.host_threads(16)


def self_test():
    case = im.self_test_case()
    rng = np.random.default_rng(1)
    blobs, addrs, keep = im.materialise(case, rng)
    exp = im.expect(case, blobs, o, None, THREADS)
    plan = im.out_plan(case, exp["n_chunks"])
    clean = im.compare(case, exp, plan, im.perfect_outputs(case, exp, plan))
    reported = {}
    for fault in im.FAULTS:
        got = im.perfect_outputs(case, exp, plan)
        want = im.inject(fault, case, exp, got)
        reported[fault] = {"want": want, "got": im.compare(case, exp, plan, got)}
    ok = not clean and all(r["got"] == [r["want"]] for r in reported.values())
    print(json.dumps({"mode": "self-test", "clean": clean, "faults": reported, "ok": ok}))
    sys.exit(0 if ok else 1)


if a.self_test:
    self_test()

acc = torch = None
if not a.dry_run:
    import torch
    from yams_amd.accel import Accel, cdc_config
    acc = Accel(0, torch.cuda.current_stream().cuda_stream)


def pinned_alloc(n):
    return torch.empty(n, dtype=torch.uint8).pin_memory().numpy()


def predecessor(case, rng):
    """Another entry point on the same context in front of the case: its workspace buffers grow and shrink in between."""
    if case["previous"] == "ingest_device":
        lens = [int(rng.integers(0, 200_000)) for _ in range(int(rng.integers(1, 12)))]
        buf = rng.integers(0, 256, sum(lens) + 64, dtype=np.uint8)
        tb = torch.from_numpy(buf).cuda()
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
        acc.ingest_device(tb.data_ptr(), offs, lens, cdc_config("rabin", min_size=2048, max_size=16384), flags=3)
        acc.synchronize()
    elif case["previous"] == "window":
        buf = rng.integers(0, 256, int(rng.integers(1000, 600_000)), dtype=np.uint8)
        off, sz, _ = acc.chunk(buf, cdc_config("streaming", min_size=2048, max_size=16384), with_hashes=True, context_len=64)
        assert int(sz.sum()) == buf.size - 64 and int(off[0]) == 64


rng = np.random.default_rng(a.seed)
ref = _oracle.ref()
ledger = {p: 0 for p in im.PATHS}
bad, fatal = [], None
chunks_total = bytes_total = ref_blobs = model_checked = 0
t_device = 0.0
t0 = time.perf_counter()
for case_no in range(a.cases):
    case = im.draw_case(rng, case_no)
    blobs, addrs, keep = im.materialise(case, rng, None if a.dry_run else pinned_alloc)
    exp = im.expect(case, blobs, o, ref, THREADS)
    plan = im.out_plan(case, exp["n_chunks"])
    for p in im.classify(case, addrs, exp, plan):
        ledger[p] += 1
    chunks_total += exp["n_chunks"]; bytes_total += sum(case["lens"]); ref_blobs += exp["ref_blobs"]
    if a.dry_run:
        got = im.perfect_outputs(case, exp, plan)
        wrong = im.compare(case, exp, plan, got)
    else:
        predecessor(case, np.random.default_rng([a.seed, case_no]))     # (its own stream: the dry run draws the same cases)
        t1 = time.perf_counter()
        got = im.call_ingest_host(acc, case, addrs, plan)
        t_device += time.perf_counter() - t1
        if got["status"] not in (im.OK, im.INVALID_ARG):
            fatal = {"case": case_no, "status": got["status"], "error": acc.L.yams_accel_last_error(acc.ctx).decode()}
            break                                     # a HIP error status: nothing more is started
        wrong = im.compare(case, exp, plan, got)
        if case["batch_bytes"]:
            batches, slots = im.partition(case["lens"], case["batch_bytes"], case["flags"])
            info = acc.device_info().get("last_host_ingest") or {}
            model_checked += 1
            if (info.get("batches"), info.get("slots")) != (len(batches), slots):
                wrong.append("partition: device %s/%s, model %d/%d" % (info.get("batches"), info.get("slots"), len(batches), slots))
    if wrong:
        bad.append({"case": case_no, "wrong": wrong, "template": case["template"], "flags": case["flags"], "form": plan["form"],
                    "placement": case["placement"], "previous": case["previous"], "mode": case["mode"], "generic": case["generic"],
                    "cfg": case["cfg"], "batch_bytes": case["batch_bytes"], "n_blobs": len(case["lens"]),
                    "required": exp["n_chunks"], "got_n_chunks": got["n_chunks"], "status": got["status"]})
        if not a.keep_going:
            break
summary = {"mode": "dry-run" if a.dry_run else "device", "seed": a.seed, "cases": a.cases, "cases_run": case_no + 1 if a.cases else 0,
           "mismatches": len(bad), "fatal": fatal, "chunks": chunks_total, "bytes": bytes_total, "ref_blobs": ref_blobs,
           "partition_checked": model_checked, "paths": ledger, "paths_below_floor": [p for p in im.PATHS if ledger[p] < im.FLOOR],
           "device_s": round(t_device, 2), "wall_s": round(time.perf_counter() - t0, 2), "first_bad": bad[:3]}
print(json.dumps(summary))
sys.exit(1 if bad or fatal else 0)
