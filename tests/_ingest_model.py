"""The plain model behind tests/stress_ingest_host.py: the case generator, the batch-partition model of yams_ingest_host,
the CPU expectation (oracle.chunks for boundaries, hashlib for every digest) and the comparison.  No GPU, no torch: the
device run and the dry run share everything here, and tests/test_ingest_host_cpu.py imports it.  Test infrastructure.

The partition model restates the contract written in include/yams_mi355x_accel.h above yams_ingest_host: blobs are
consecutive, a blob is never split, each blob starts on a 16-byte boundary of its batch, a batch always takes at least one
blob, a batch closes when the next padded blob would pass batch_bytes, two slot buffers serve without whole-blob digests
and up to four with them, never more than there are batches.
"""
from __future__ import annotations

import hashlib
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAG_CHUNK, FLAG_BLOB, FLAG_DEFER = 1, 2, 4          # YAMS_INGEST_CHUNK_DIGESTS / _BLOB_DIGESTS / _DEFER_LONG_BLOB_DIGESTS
FLAGS = [0, 1, 2, 3, 3 | FLAG_DEFER, 2 | FLAG_DEFER]
OUT_FORMS = ["ample", "exact", "one_short", "cap0_null", "null_chunk_digest"]
PLACEMENTS = ["separate", "back_to_back", "gaps", "odd_align", "pinned"]
PREVIOUS = ["host", "ingest_device", "window"]
OK, INVALID_ARG = 0, 1
GUARD = 8                                             # guard entries behind every output array
SENT = 0xA5                                           # every output byte before the call
SPECIAL_LENS = [0, 1, 47, 48, 49, 4095, 4096, 16384, 16385, 70_001, 300_000, 1 << 20, 2_500_000]   # stress_ingest.py
CONFIGS = [dict(), dict(min_size=4096, max_size=65536), dict(min_size=64, max_size=256, mask=0xF),        # stress_ingest.py
           dict(min_size=1, max_size=100, mask=3, window=16), dict(min_size=2048, max_size=8192, mask=0xFFFFF),
           dict(min_size=512, max_size=4096, mask=(1 << 40) - 1), dict(min_size=100, max_size=100),
           dict(min_size=300, max_size=200, mask=0xFF), dict(min_size=37, max_size=4001, mask=0x155, window=1),
           dict(min_size=5000, max_size=9000, mask=0x3FF, window=7, polynomial=0xBFE6B8A5BF378D83),
           dict(min_size=8, max_size=5000, mask=0x7FFFFFFF), dict(min_size=8, max_size=5000, mask=0x80000000),
           dict(min_size=40, max_size=90, mask=0), dict(min_size=1000, max_size=1 << 20, mask=0x1FFF, window=47)]
WINDOW_CONFIGS = [dict(min_size=2048, max_size=65536), dict(), dict(min_size=64, max_size=256, mask=0xF),
                  dict(min_size=1, max_size=5000, mask=0x3FF, window=16), dict(min_size=512, max_size=4096, mask=(1 << 40) - 1),
                  dict(min_size=8, max_size=5000, mask=0x7FFFFFFF)]
PATHS = (["batches_1", "batches_2_3_with_digests", "batches_4", "batches_many", "one_blob_per_batch", "own_batch_blob",
          "batch_bytes_0", "slots_1", "slots_2", "slots_3", "slots_4", "merged_run", "neighbours_not_merged",
          "empty_first_in_batch", "empty_last_in_batch", "empty_between_merged", "all_empty", "defer_one_of_batch",
          "defer_whole_batch", "generic_kernel", "mode_rabin", "mode_streaming", "narrow_kernel_config", "wide_kernel_config"]
         + ["flags_%d" % f for f in FLAGS] + ["out_" + f for f in OUT_FORMS] + ["place_" + p for p in PLACEMENTS]
         + ["prev_" + p for p in PREVIOUS])
FLOOR = 5                                             # every path of PATHS, by the pinned seed and case count
PINNED_SEED, PINNED_CASES = 11, 96
TEMPLATES = 12


def header_constant(name: str) -> int:
    """An integer #define of include/yams_mi355x_accel.h, by name."""
    text = open(os.path.join(ROOT, "include", "yams_mi355x_accel.h")).read()
    m = re.search(r"^#define\s+%s\s+(.+?)\s*(/\*.*)?$" % re.escape(name), text, re.M)
    if not m:
        raise KeyError(name)
    expr = re.sub(r"(\d)(?:u|ull|ul)\b", r"\1", m.group(1), flags=re.I)
    if not re.fullmatch(r"[\s\d()<>+*xXa-fA-F-]+", expr):
        raise ValueError(expr)
    return int(eval(expr, {"__builtins__": {}}))


def defer_threshold_host(total: int) -> int:
    """yams_ingest_defer_threshold_host as the header documents it: 1/512 of the call's bytes, never below 1 MiB."""
    return max(1 << 20, total >> 9)


def pad16(n: int) -> int:
    return (n + 15) & ~15


def partition(lens, batch_bytes: int, flags: int):
    """-> ([(first, count, padded bytes)], slots) of a yams_ingest_host call with an explicit batch_bytes."""
    batches, b = [], 0
    while b < len(lens):
        first, count, size = b, 0, 0
        while b < len(lens):
            p = pad16(int(lens[b]))
            if count and size + p > batch_bytes:
                break
            size += p; count += 1; b += 1
        batches.append((first, count, size))
    return batches, min(4 if flags & FLAG_BLOB else 2, len(batches))


# ---- the generator ------------------------------------------------------------------------------------------------------
def log_uniform(rng, lo, hi):
    return int(min(hi, np.exp(rng.uniform(np.log(lo), np.log(hi + 1)))))


def content(rng, n):
    """The content kinds of stress_ingest.py: random, constant, short period, text-like, repeated segment."""
    kind = int(rng.integers(0, 5))
    if kind == 0 or n < 8:
        return rng.integers(0, 256, n, dtype=np.uint8)
    if kind == 1:
        return np.full(n, int(rng.integers(0, 256)), np.uint8)
    if kind == 2:
        p = rng.integers(0, 256, int(rng.integers(1, 200)), dtype=np.uint8)
        return np.tile(p, n // p.size + 1)[:n]
    if kind == 3:
        words = [bytes(rng.integers(97, 123, int(rng.integers(2, 9)), dtype=np.uint8)) for _ in range(50)]
        m = min(n, 1 << 16)
        s = b" ".join(words[int(i)] for i in rng.integers(0, 50, m // 4 + 8))
        t = np.frombuffer(s[:m].ljust(m, b"."), dtype=np.uint8)
        return np.tile(t, n // m + 1)[:n].copy()
    d = rng.integers(0, 256, n, dtype=np.uint8)
    seg = int(rng.integers(1, max(2, n // 3)))
    d[n - seg:] = d[:seg]
    return d


def _draw_len(rng, mult16_share):
    r = rng.random()
    if r < mult16_share:
        return 16 * log_uniform(rng, 1, 1 << 14)
    if r < mult16_share + (1 - mult16_share) * 0.4:
        n = SPECIAL_LENS[int(rng.integers(0, len(SPECIAL_LENS)))]
        return int(n * rng.uniform(0.5, 1.0)) if n > 100 and rng.random() < 0.5 else n
    return log_uniform(rng, 1, 1_500_000)


def _batch_bytes_for(lens, flags, want_lo, want_hi):
    """The smallest batch_bytes under which the model counts want_lo..want_hi batches, or None (the count falls as
    batch_bytes grows, so a bisection finds it)."""
    padded = [pad16(n) for n in lens]
    lo, hi = 1, max(16, sum(padded))
    while lo < hi:                                    # smallest batch_bytes with at most want_hi batches
        mid = (lo + hi) // 2
        if len(partition(lens, mid, flags)[0]) <= want_hi:
            hi = mid
        else:
            lo = mid + 1
    return lo if want_lo <= len(partition(lens, lo, flags)[0]) <= want_hi else None


def draw_case(rng, case: int) -> dict:
    """One yams_ingest_host case.  Every case that is drawn is run: nothing is filtered afterwards.  `case` picks the
    template (the batch shape the case aims at) and rotates flags, output form, placement and predecessor; everything else
    comes from rng.  The ledger classifies what was actually drawn, not what the template aimed at."""
    t, rnd = case % TEMPLATES, case // TEMPLATES
    flags = FLAGS[(case + rnd) % len(FLAGS)]
    out_form = OUT_FORMS[(case + 2 * rnd) % len(OUT_FORMS)]
    placement = PLACEMENTS[(3 * case + rnd) % len(PLACEMENTS)]
    previous = PREVIOUS[(case + rnd // 2) % len(PREVIOUS)]
    mode = "streaming" if rng.random() < 0.5 else "rabin"
    cfg = dict(CONFIGS[int(rng.integers(0, len(CONFIGS)))])
    generic = bool(rng.random() < 0.3)
    tiny = min(cfg.get("min_size", 16384), cfg.get("max_size", 1 << 20)) <= 100        # bound the per-chunk digest loop of the check
    n_blobs = log_uniform(rng, 1, 40 if tiny else 200)
    mult16 = 0.6 if placement in ("back_to_back", "pinned", "odd_align") else 0.2
    lens = [_draw_len(rng, mult16) for _ in range(n_blobs)]
    if t == 7:                                        # a call whose blobs are all empty
        lens = [0] * min(n_blobs, 20)
    if t in (8, 9):                                   # blobs above the deferral threshold (1 MiB for calls below 512 MiB)
        flags = FLAGS[4 + rnd % 2]
        for _ in range(int(rng.integers(1, 4))):
            lens.insert(int(rng.integers(0, len(lens) + 1)), int(rng.integers((1 << 20) + 1, 1_900_000)))
    if t == 10:                                       # empty blobs at the head, at the tail and between neighbours
        lens = [0] + lens + [0]
        for _ in range(1 + len(lens) // 6):
            lens.insert(int(rng.integers(0, len(lens) + 1)), 0)
    if t in (0, 10) and len(lens) >= 2:               # an empty blob between two blobs that travel as one copy
        i = int(rng.integers(0, len(lens) - 1))
        lens[i:i + 2] = [16 * int(rng.integers(1, 5000)), 0, 16 * int(rng.integers(1, 5000)), int(lens[i + 1])]
    if tiny and t not in (8, 9):
        lens = [min(n, 60_000) for n in lens]
    budget, tot = 24 << 20, 0
    for i, n in enumerate(lens):                      # the rare long ones stay few: past the budget blobs are short
        if tot + n > budget and n > 70_001:
            lens[i] = n = 70_001 + n % 4096
        tot += n
    total_padded = sum(pad16(n) for n in lens)
    if t == 0:   batch_bytes = total_padded + int(rng.integers(0, 1 << 20))                       # one batch
    elif t == 1: batch_bytes = _batch_bytes_for(lens, flags, 2, 3)                                # fewer batches than slots
    elif t == 2: batch_bytes = _batch_bytes_for(lens, flags, 4, 4)                                # exactly four
    elif t == 3: batch_bytes = _batch_bytes_for(lens, flags, 9, 40)                               # slots reused, chains joined late
    elif t == 4: batch_bytes = 1                                                                 # one blob per batch
    elif t == 5: batch_bytes = max(16, int(np.median([pad16(n) for n in lens])) // 2 * 2)        # blobs longer than a batch
    elif t == 6: batch_bytes = 0                                                                 # the library's own choice
    elif t == 7: batch_bytes = [0, 1, 64][rnd % 3]
    elif t == 8: batch_bytes = 4 << 20                                                           # one deferred blob among others
    elif t == 9: batch_bytes = 1 << 20                                                           # deferred blobs alone in a batch
    elif t == 10: batch_bytes = _batch_bytes_for(lens, flags, 3, 6)
    else:        batch_bytes = log_uniform(rng, 16, max(16, total_padded))
    if batch_bytes is None:                           # (too few blobs for the aimed count: any size will do)
        batch_bytes = log_uniform(rng, 16, max(16, total_padded))
    return {"case": case, "template": t, "flags": flags, "out_form": out_form, "placement": placement, "previous": previous,
            "mode": mode, "cfg": cfg, "generic": generic, "lens": [int(n) for n in lens], "batch_bytes": int(batch_bytes),
            "null_empty_ptrs": bool(rng.random() < 0.5), "null_blob_digest": bool(rng.random() < 0.5)}


def materialise(case: dict, rng, pinned_alloc=None):
    """The blobs where they lie in host memory -> (blobs [numpy views], addresses, keep-alive).  pinned_alloc(nbytes) gives
    a page-locked uint8 array; the dry run passes None and lays the same bytes out in pageable memory."""
    lens, place = case["lens"], case["placement"]
    if place == "separate":
        blobs = [content(rng, n) for n in lens]
        keep = blobs
    else:
        lead = int(rng.integers(1, 16)) | 1 if place == "odd_align" else 0
        gaps = [int(rng.integers(1, 41)) if place == "gaps" else 0 for _ in lens]
        size = lead + sum(lens) + sum(gaps) + 64
        buf = pinned_alloc(size) if (place == "pinned" and pinned_alloc) else np.empty(size, np.uint8)
        buf[:] = 0xAB
        blobs, pos = [], lead
        for n, g in zip(lens, gaps):
            buf[pos:pos + n] = content(rng, n)
            blobs.append(buf[pos:pos + n]); pos += n + g
        keep = buf
    addrs = [None if (b.size == 0 and case["null_empty_ptrs"]) else int(b.ctypes.data) for b in blobs]
    return blobs, addrs, keep


def upload_runs(case: dict, addrs, batches):
    """How the blobs of each batch travel, from addresses and lengths alone: (merged pairs, neighbouring pairs that do not
    merge, empty blobs that sit between the two halves of a merged pair).  Two non-empty blobs merge when the second starts
    where the first ends in host memory AND in the batch (every length of the run so far is a multiple of 16)."""
    lens = case["lens"]
    merged = not_merged = empty_between = 0
    for first, count, _ in batches:
        at = run_dst = run_len = empties = 0          # `at`: where the blob starts in the batch
        run_src = prev = None
        for j in range(first, first + count):
            n = lens[j]
            if n == 0:
                empties += 1
                continue
            if run_len and addrs[j] == run_src + run_len and at == run_dst + run_len:
                merged += 1; empty_between += empties; run_len += n
            else:
                if prev is not None and addrs[j] == addrs[prev] + lens[prev]:
                    not_merged += 1
                run_src, run_dst, run_len = addrs[j], at, n
            prev, empties = j, 0
            at += pad16(n)
    return merged, not_merged, empty_between


# ---- the CPU expectation -------------------------------------------------------------------------------------------------
def expect(case: dict, blobs, oracle, ref=None, threads=1) -> dict:
    """What the call must return, from the CPU alone: oracle.chunks (or the reference's own chunker for every eighth blob
    where it is present) for the boundaries, hashlib for every chunk digest and every blob digest."""
    mode, cfg, flags = case["mode"], case["cfg"], case["flags"]

    def one(bi):
        b = blobs[bi]
        ref_hashes = None
        if ref is not None and bi % 8 == 0 and b.size <= 400_000:
            off, sz, ref_hashes = ref.chunks(b, mode, with_hashes=True, **cfg)
        else:
            off, sz = oracle.chunks(b, mode, **cfg)
        mv = memoryview(np.ascontiguousarray(b))
        dg = b"".join(hashlib.sha256(mv[int(o):int(o) + int(s)]).digest() for o, s in zip(off, sz))
        if ref_hashes is not None and dg.hex() != "".join(ref_hashes):
            raise AssertionError("hashlib and the reference's Chunk::hash disagree on blob %d" % bi)
        return off, sz, dg, hashlib.sha256(mv).digest(), ref_hashes is not None

    with ThreadPoolExecutor(max_workers=max(1, threads)) as ex:
        parts = list(ex.map(one, range(len(blobs))))
    counts = [len(p[0]) for p in parts]
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    total = sum(case["lens"])
    thr = defer_threshold_host(total)
    deferred = [bool(flags & FLAG_DEFER and flags & FLAG_BLOB and n > thr) for n in case["lens"]]
    cat = lambda i, dt: np.concatenate([np.asarray(p[i], dt) for p in parts]) if parts else np.zeros(0, dt)
    return {"n_chunks": int(first[-1]), "blob_first": first, "chunk_offset": cat(0, np.uint64), "chunk_size": cat(1, np.uint64),
            "chunk_digest": np.frombuffer(b"".join(p[2] for p in parts), np.uint8).reshape(-1, 32),
            "blob_digest": np.frombuffer(b"".join(p[3] for p in parts), np.uint8).reshape(-1, 32),
            "deferred": deferred, "ref_blobs": sum(1 for p in parts if p[4])}


def out_plan(case: dict, required: int) -> dict:
    """The output arrays of the case: capacity, which pointers are NULL, the status the header promises."""
    form, flags = case["out_form"], case["flags"]
    if form == "one_short" and required == 0:
        form = "exact"                                # (nothing to be short of)
    if form == "null_chunk_digest" and not flags & FLAG_CHUNK:
        form = "ample"                                # (the flag is not set: an absent array is nothing special)
    cap = {"ample": required + 1 + case["case"] % 97, "exact": required, "one_short": required - 1, "cap0_null": 0,
           "null_chunk_digest": required + 3}[form]
    return {"form": form, "cap": cap, "null_chunk_arrays": form == "cap0_null", "null_chunk_digest": form in ("cap0_null", "null_chunk_digest"),
            "null_blob_digest": case["null_blob_digest"] and not flags & FLAG_BLOB,
            "status": INVALID_ARG if required > cap else OK}


def make_outputs(n_blobs: int, plan: dict) -> dict:
    """Sentinel-filled arrays with GUARD entries behind their capacity (None where the case passes NULL)."""
    cap = plan["cap"]
    u64 = lambda n: np.full(n + GUARD, SENT * 0x0101010101010101, np.uint64)
    return {"status": None, "n_chunks": None, "cap": cap, "blob_first": u64(n_blobs + 1),
            "chunk_offset": None if plan["null_chunk_arrays"] else u64(cap), "chunk_size": None if plan["null_chunk_arrays"] else u64(cap),
            "chunk_digest": None if plan["null_chunk_digest"] else np.full((cap + GUARD, 32), SENT, np.uint8),
            "blob_digest": None if plan["null_blob_digest"] else np.full((n_blobs + GUARD, 32), SENT, np.uint8)}


def perfect_outputs(case: dict, exp: dict, plan: dict) -> dict:
    """What a correct library leaves in make_outputs' arrays (the dry run's stand-in for the device, and the self-test's
    starting point).  On the too-small status the chunk arrays are left as they were: the header promises nothing about
    them there, and the comparison does not look."""
    n, flags = len(case["lens"]), case["flags"]
    got = make_outputs(n, plan)
    got["status"], got["n_chunks"] = plan["status"], exp["n_chunks"]
    got["blob_first"][:n + 1] = exp["blob_first"]
    if plan["status"] == OK:
        m = exp["n_chunks"]
        if got["chunk_offset"] is not None:
            got["chunk_offset"][:m] = exp["chunk_offset"]; got["chunk_size"][:m] = exp["chunk_size"]
        if got["chunk_digest"] is not None and flags & FLAG_CHUNK:
            got["chunk_digest"][:m] = exp["chunk_digest"]
    if flags & FLAG_BLOB:
        got["blob_digest"][:n] = exp["blob_digest"]
        for i, d in enumerate(exp["deferred"]):
            if d:
                got["blob_digest"][i] = 0
    return got


def call_ingest_host(acc, case: dict, addrs, plan: dict) -> dict:
    """yams_ingest_host on the context of `acc` (yams_amd.accel.Accel) with the case's arguments and make_outputs' arrays."""
    import ctypes as C
    from yams_amd import _lib
    from yams_amd.accel import cdc_config
    n = len(case["lens"])
    got = make_outputs(n, plan)
    cfg = cdc_config(case["mode"], generic_kernel=case["generic"], **case["cfg"])
    ptrs = (C.c_void_p * max(n, 1))(*addrs)
    bl = np.asarray(case["lens"], np.uint64)
    cnt = C.c_uint64(0xA5A5)
    u64 = lambda x: x.ctypes.data_as(_lib.u64p) if x is not None else None
    ptr = lambda x: x.ctypes.data if x is not None else None
    got["status"] = int(acc.L.yams_ingest_host(acc.ctx, ptrs, u64(bl), n, C.byref(cfg), case["flags"], case["batch_bytes"],
                                               u64(got["blob_first"]), u64(got["chunk_offset"]), u64(got["chunk_size"]),
                                               ptr(got["chunk_digest"]), plan["cap"], ptr(got["blob_digest"]), C.byref(cnt)))
    got["n_chunks"] = int(cnt.value)
    return got


def _sentinel(a):
    return bool((a.view(np.uint8) == SENT).all())


def compare(case: dict, exp: dict, plan: dict, got: dict) -> list:
    """The names of everything that is wrong with `got` (empty: the case passes).  Bit-exact throughout."""
    n, flags, bad = len(case["lens"]), case["flags"], []
    if got["status"] != plan["status"]:
        bad.append("status")
        if got["status"] not in (OK, INVALID_ARG):
            return bad
    if got["n_chunks"] != exp["n_chunks"]:
        bad.append("n_chunks")
    if not np.array_equal(got["blob_first"][:n + 1], exp["blob_first"]):
        bad.append("blob_first")
    if not _sentinel(got["blob_first"][n + 1:]):
        bad.append("guard:blob_first")
    fits = got["status"] == OK and plan["status"] == OK
    m = exp["n_chunks"] if fits else 0
    for name in ("chunk_offset", "chunk_size"):
        a = got[name]
        if a is None:
            continue
        if fits and not np.array_equal(a[:m], exp[name]):
            bad.append("boundary")
        # OK: nothing behind n_chunks changes; too small: nothing behind chunk_cap
        if not _sentinel(a[m:] if fits else a[got["cap"]:]):
            bad.append("guard:" + name)
    dg = got["chunk_digest"]
    if dg is not None:
        if not flags & FLAG_CHUNK:
            if not _sentinel(dg):
                bad.append("guard:chunk_digest")
        else:
            if fits and not np.array_equal(dg[:m], exp["chunk_digest"]):
                bad.append("chunk_digest")
            if not _sentinel(dg[m:] if fits else dg[got["cap"]:]):
                bad.append("guard:chunk_digest")
    bd = got["blob_digest"]
    if bd is not None:
        if not flags & FLAG_BLOB:
            if not _sentinel(bd):
                bad.append("guard:blob_digest")
        else:
            for i in range(n):
                if exp["deferred"][i]:
                    if bd[i].any():
                        bad.append("deferred_not_zero")
                        break
            if any(not exp["deferred"][i] and not np.array_equal(bd[i], exp["blob_digest"][i]) for i in range(n)):
                bad.append("blob_digest")
            if not _sentinel(bd[n:]):
                bad.append("guard:blob_digest")
    return sorted(set(bad))


# ---- the path ledger -----------------------------------------------------------------------------------------------------
def classify(case: dict, addrs, exp: dict, plan: dict) -> list:
    """The PATHS this case reaches, from the case as drawn, the addresses of its blobs and the model."""
    lens, flags, bb = case["lens"], case["flags"], case["batch_bytes"]
    p = ["flags_%d" % flags, "out_" + plan["form"], "place_" + case["placement"], "prev_" + case["previous"], "mode_" + case["mode"]]
    narrow = case["cfg"].get("window", 48) == 48 and case["cfg"].get("mask", 0x1FFF) < (1 << 31)
    p.append("narrow_kernel_config" if narrow else "wide_kernel_config")
    if case["generic"]:
        p.append("generic_kernel")
    if not any(lens):
        p.append("all_empty")
    # batch_bytes 0 on these small calls: the library's choice is never below 256 MiB, so everything is one batch
    batches, slots = partition(lens, bb if bb else 1 << 62, flags)
    if bb == 0:
        p.append("batch_bytes_0")
    nb = len(batches)
    if nb == 1: p.append("batches_1")
    if 2 <= nb <= 3 and flags & FLAG_BLOB: p.append("batches_2_3_with_digests")
    if nb == 4: p.append("batches_4")
    if nb > 8: p.append("batches_many")
    p.append("slots_%d" % slots)
    if nb == len(lens) and nb > 1: p.append("one_blob_per_batch")
    if bb and any(pad16(n) > bb for n in lens): p.append("own_batch_blob")
    merged, not_merged, empty_between = upload_runs(case, addrs, batches)
    if merged: p.append("merged_run")
    if not_merged: p.append("neighbours_not_merged")
    if empty_between: p.append("empty_between_merged")
    for first, count, _ in batches:
        if count > 1 and lens[first] == 0: p.append("empty_first_in_batch")
        if count > 1 and lens[first + count - 1] == 0: p.append("empty_last_in_batch")
        d = sum(exp["deferred"][first:first + count])
        if d == count: p.append("defer_whole_batch")
        if d == 1 and count > 1: p.append("defer_one_of_batch")
    return sorted(set(p))


# ---- faults for the self-test --------------------------------------------------------------------------------------------
def inject(fault: str, case: dict, exp: dict, got: dict):
    """One fault at a time into a correct result; returns the name compare() must report."""
    n = len(case["lens"])
    if fault == "boundary_shifted":
        got["chunk_offset"][exp["n_chunks"] // 2] += 1; return "boundary"
    if fault == "chunk_digest_bit":
        got["chunk_digest"][exp["n_chunks"] // 3, 7] ^= 0x10; return "chunk_digest"
    if fault == "blob_digest_swapped":
        i = next(i for i in range(n - 1) if not exp["deferred"][i] and not exp["deferred"][i + 1] and case["lens"][i] != case["lens"][i + 1])
        got["blob_digest"][[i, i + 1]] = got["blob_digest"][[i + 1, i]]; return "blob_digest"
    if fault == "blob_first_off_by_one":
        got["blob_first"][n // 2] += 1; return "blob_first"
    if fault == "guard_overwritten":
        got["chunk_size"][got["cap"] + 1] = 0; return "guard:chunk_size"
    if fault == "deferred_not_zero":
        got["blob_digest"][exp["deferred"].index(True), 31] = 1; return "deferred_not_zero"
    raise KeyError(fault)


FAULTS = ["boundary_shifted", "chunk_digest_bit", "blob_digest_swapped", "blob_first_off_by_one", "guard_overwritten",
          "deferred_not_zero"]


def self_test_case() -> dict:
    """A hand-written case for the self-test: a deferred blob among short ones, ample arrays, every flag."""
    return {"case": 0, "template": -1, "flags": 7, "out_form": "ample", "placement": "separate", "previous": "host",
            "mode": "streaming", "cfg": dict(min_size=2048, max_size=16384), "generic": False,
            "lens": [70_001, 0, (1 << 20) + 5, 4096, 300_000], "batch_bytes": 1 << 20, "null_empty_ptrs": False,
            "null_blob_digest": False}


# ---- windowed chunking ---------------------------------------------------------------------------------------------------
def window_stream(chunk_fn, data, rng, min_size: int, counts: dict):
    """A stream consumed through chunk_fn(buffer, context_len) -> (offsets, sizes, hexes), the way a bounded-memory reader
    would: at every step a freshly drawn window length (from below min_size, so short that no chunk closes, up to 1 MiB)
    and a freshly drawn history (56..300 bytes, or everything from the true start of the stream).  The last chunk of a
    window is open and is carried into the next.  -> the reassembled (offsets, sizes, hexes)."""
    offs, sizes, hexes = [], [], []
    start = end = 0                                   # stream offset of the open chunk; stream bytes read so far
    while True:
        r = rng.random()
        win = int(rng.integers(1, max(2, min_size))) if r < 0.15 else log_uniform(rng, max(1, min_size), 1 << 20)
        end = min(len(data), end + win)
        eof = end == len(data)
        h = start if (rng.random() < 0.1 and start <= (1 << 20)) else min(int(rng.integers(56, 301)), start)
        counts["true_start" if h == start else "history_56_300"] = counts.get("true_start" if h == start else "history_56_300", 0) + 1
        off, sz, hx = chunk_fn(data[start - h:end], h)
        keep = len(off) if eof else len(off) - 1
        counts["steps"] = counts.get("steps", 0) + 1
        if keep == 0 and not eof:
            counts["no_chunk_closed"] = counts.get("no_chunk_closed", 0) + 1
        for i in range(keep):
            offs.append(start + int(off[i]) - h); sizes.append(int(sz[i])); hexes.append(hx[i])
        if eof:
            return offs, sizes, hexes
        start = start + int(off[-1]) - h


def stream_with_dead_runs(rng, n: int):
    """Random bytes with runs that hold no boundary candidate (constant bytes: forced max-size chunks)."""
    data = rng.integers(0, 256, n, dtype=np.uint8)
    for _ in range(int(rng.integers(1, 4))):
        a = int(rng.integers(0, n)); data[a:a + int(rng.integers(1000, 400_000))] = int(rng.integers(0, 256))
    return data
