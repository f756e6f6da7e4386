"""The host-memory ingest and hash entry points on the GPU against the CPU alone (oracle.chunks, hashlib, the reference's
own chunker where oracle/_ref is present): yams_ingest_host through the randomised harness tests/stress_ingest_host.py,
and scripted cases for yams_cdc_chunk_window_host, the content_hash_v1 streaming handle, chunker_v1.chunk_many and
hash_many / verify_many.  Nothing here has a tolerance: digests, boundaries, counts and blob_first are bit-exact."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _ingest_model as im
from yams_amd import _lib
from yams_amd.accel import cdc_config

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM_FLUSH = 64 << 20          # kStreamFlush, plugin.cpp: the streaming handle pushes its whole blocks through the device
LONE_MAX = im.header_constant("YAMS_HASH_LONE_CHAIN_MAX")
RATIO = im.header_constant("YAMS_HASH_CHAIN_RATIO")
CHUNK_MANY_BUFFER_HASHES = im.header_constant("YAMS_CHUNK_MANY_BUFFER_HASHES")
CHUNK_MANY_DEFER = im.header_constant("YAMS_CHUNK_MANY_DEFER_LONG_BUFFER_HASHES")


def test_randomised_host_ingest_stress_against_cpu():
    """tests/stress_ingest_host.py with the pinned seed and case count: zero mismatches, every case run, every ledger path
    reached at least FLOOR times by the DEVICE run's own summary, and `batches` / `slots` of last_host_ingest equal to the
    partition model in every case that names batch_bytes.  Measured on an MI355X: 5.2 s for the whole harness
    (2.4 s inside yams_ingest_host), against the wrapper's limit of 280 s."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "stress_ingest_host.py"), "--cases", str(im.PINNED_CASES),
                        "--seed", str(im.PINNED_SEED)], capture_output=True, text=True, timeout=280)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert line, r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads(line[-1])
    print(line[-1])
    assert r.returncode == 0 and res["mode"] == "device" and res["fatal"] is None, res
    assert res["mismatches"] == 0 and res["cases"] == res["cases_run"] == im.PINNED_CASES, res
    short = {p: res["paths"].get(p, 0) for p in im.PATHS if res["paths"].get(p, 0) < im.FLOOR}
    assert not short, short
    assert res["partition_checked"] >= im.PINNED_CASES * 3 // 4 and res["chunks"] > 1_000_000, res


# ---- windowed chunking -----------------------------------------------------------------------------------------------------
def _plugin(L, name, vt_type):
    assert L.yams_plugin_init(b"{}", None) == 0
    p = C.c_void_p()
    assert L.yams_plugin_get_interface(name, 1, C.byref(p)) == 0
    return C.cast(p, C.POINTER(vt_type)).contents


def _health(L):
    hp = C.c_void_p()
    assert L.yams_plugin_get_health_json(C.byref(hp)) == 0
    h = json.loads(C.string_at(hp))
    C.CDLL(None).free(hp)
    return h


def test_windowed_stream_with_redrawn_windows_equals_one_oracle_pass(acc, accel_lib, oracle):
    """yams_cdc_chunk_window_host (acc.chunk(..., context_len=h), and chunker_v1.chunk_window for every other stream): streams
    of 1 to 8 MiB with runs without candidates, the window length redrawn at every step from below min_size (no chunk closes:
    the open chunk carries over and the loop still advances) up to 1 MiB, the history redrawn per step from 56 to 300 bytes
    or the true start of the stream.  The reassembled chunks and their hex digests equal ONE oracle pass over the whole
    stream."""
    vt = _plugin(accel_lib, b"chunker_v1", _lib.ChunkerV1)
    rng = np.random.default_rng(1201)
    counts = {}
    try:
        for si, cfg in enumerate(im.WINDOW_CONFIGS):
            data = im.stream_with_dead_runs(rng, int(rng.integers(1 << 20, (8 << 20) + 1)))
            want_off, want_sz = oracle.chunks(data, "streaming", **cfg)
            c = cdc_config("streaming", **cfg)

            def via_acc(buf, h):
                return acc.chunk(buf, c, with_hashes=True, context_len=h)

            def via_vtable(buf, h):
                buf = np.ascontiguousarray(buf)
                chunks = C.POINTER(_lib.ChunkRef)(); n = C.c_size_t()
                assert vt.chunk_window(None, buf.ctypes.data_as(_lib.u8p), buf.size, h, C.byref(c), C.byref(chunks), C.byref(n)) == 0
                out = ([chunks[i].offset for i in range(n.value)], [chunks[i].size for i in range(n.value)],
                       [chunks[i].hash_hex.decode() for i in range(n.value)])
                vt.free_chunks(None, chunks, n)
                return out

            off, sz, hx = im.window_stream(via_vtable if si % 2 else via_acc, data, rng, cfg.get("min_size", 16384), counts)
            assert off == [int(x) for x in want_off] and sz == [int(x) for x in want_sz], (cfg, len(off), len(want_off))
            mv = memoryview(data)
            wrong = [i for i in range(len(off)) if hx[i] != hashlib.sha256(mv[off[i]:off[i] + sz[i]]).hexdigest()]
            assert not wrong, (cfg, wrong[:5])
    finally:
        accel_lib.yams_plugin_shutdown()
    print(json.dumps(counts))
    assert counts.get("no_chunk_closed", 0) >= 5 and counts.get("true_start", 0) >= 5 and counts.get("history_56_300", 0) >= 50, counts


# ---- the streaming hash handle ---------------------------------------------------------------------------------------------
def _feed(vt, st, data, cuts):
    prev = 0
    for c in list(cuts) + [len(data)]:
        piece = data[prev:c]
        assert vt.stream_update(None, st, piece.ctypes.data_as(_lib.u8p) if piece.size else None, piece.size) == 0
        prev = c
    out = C.create_string_buffer(65)
    assert vt.stream_finalize(None, st, out) == 0
    return out.value.decode()


def test_streaming_hash_handle_every_short_length_random_splits(accel_lib):
    """Every length 0..200 under random update splits with empty updates in between, and the splits 63 / 64 / 65; one handle
    throughout, reused after every finalize."""
    vt = _plugin(accel_lib, b"content_hash_v1", _lib.ContentHashV1)
    rng = np.random.default_rng(1202)
    st = C.c_void_p()
    try:
        assert vt.stream_create(None, C.byref(st)) == 0
        for n in range(201):
            data = rng.integers(0, 256, n, dtype=np.uint8)
            want = hashlib.sha256(data.tobytes()).hexdigest()
            cuts = sorted(int(x) for x in rng.integers(0, n + 1, int(rng.integers(0, 6))))
            cuts = sorted(cuts + [c for c in cuts if rng.random() < 0.4])          # a repeated cut is an empty update
            assert _feed(vt, st, data, cuts) == want, (n, cuts)
            for cut in (63, 64, 65):
                if cut <= n:
                    assert _feed(vt, st, data, [cut]) == want, (n, cut)
            if n >= 65:
                assert _feed(vt, st, data, [63, 64, 64, 65]) == want, n
        vt.stream_destroy(None, st)
    finally:
        accel_lib.yams_plugin_shutdown()


@pytest.mark.parametrize("length", [STREAM_FLUSH + 5, 130 * (1 << 20) + 13], ids=["one_flush", "two_flushes"])
def test_streaming_hash_handle_across_the_flush_size(accel_lib, length):
    """Streams that cross the handle's flush size once (64 MiB + 5) and twice (~130 MiB): the second and third device calls
    start from a midstate that is not the initial one.  Each stream is fed as one update, as many odd-sized updates and as
    updates that end exactly on the flush size; the handle is reused after every finalize.  hashlib is the authority."""
    vt = _plugin(accel_lib, b"content_hash_v1", _lib.ContentHashV1)
    rng = np.random.default_rng(1203)
    data = np.frombuffer(rng.bytes(length), np.uint8)
    want = hashlib.sha256(data).hexdigest()
    st = C.c_void_p()
    try:
        assert vt.stream_create(None, C.byref(st)) == 0
        assert _feed(vt, st, data, []) == want, "one update"
        assert _feed(vt, st, data[:3], [1]) == hashlib.sha256(data[:3]).hexdigest()          # the handle after a long stream
        odd, pos = [], 0
        while True:
            pos += int(rng.integers(1, 3 << 20)) | 1
            if pos >= length:
                break
            odd.append(pos)
        assert _feed(vt, st, data, odd) == want, "odd-sized updates"
        quarter = STREAM_FLUSH // 4
        on_flush = list(range(quarter, length, quarter))                                      # every fourth update ends on it
        assert all(c % quarter == 0 for c in on_flush) and STREAM_FLUSH in on_flush
        assert _feed(vt, st, data, on_flush) == want, "updates that end on the flush size"
        assert _feed(vt, st, data[:0], []) == hashlib.sha256(b"").hexdigest()
        vt.stream_destroy(None, st)
    finally:
        accel_lib.yams_plugin_shutdown()


# ---- chunk_many ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["streaming", "rabin"])
def test_chunk_many_retries_when_its_first_capacity_guess_is_too_low(accel_lib, oracle, mode):
    """chunk_many guesses one chunk per max(min(min, max), 256) bytes and runs once more with the required size when that is
    too low.  Tiny-chunk configurations on buffers of 100 KiB and more make the guess too low (asserted from the count), so
    the retry runs: boundaries, every chunk digest and the buffer hashes against the CPU; without buffer hashes, with them,
    and with YAMS_CHUNK_MANY_DEFER_LONG_BUFFER_HASHES (entries above yams_ingest_defer_threshold_host are empty strings).
    Zero-length buffers pass NULL pointers."""
    vt = _plugin(accel_lib, b"chunker_v1", _lib.ChunkerV1)
    rng = np.random.default_rng(1204)
    bufs = [im.content(rng, n) for n in (150_000, 0, 100_000, 1, 0, 200_001, (1 << 20) + 7, 120_016)]
    ptrs = (C.c_void_p * len(bufs))(*[b.ctypes.data if b.size else None for b in bufs])
    lens = (C.c_size_t * len(bufs))(*[b.size for b in bufs])
    total = sum(b.size for b in bufs)
    try:
        for ci, kw in enumerate([dict(min_size=1, max_size=100, mask=3, window=16), dict(min_size=64, max_size=256, mask=0xF),
                                 dict(min_size=40, max_size=90, mask=0), dict(min_size=100, max_size=100)]):
            cfg = cdc_config(mode, **kw)
            want = [oracle.chunks(b, mode, **kw) for b in bufs]
            guess = sum(b.size // max(min(kw["min_size"], kw["max_size"]), 256) + 2 for b in bufs)
            for flags in (0, CHUNK_MANY_BUFFER_HASHES, CHUNK_MANY_BUFFER_HASHES | CHUNK_MANY_DEFER)[ci % 2:]:
                batch = C.POINTER(_lib.ChunkBatch)()
                assert vt.chunk_many(None, ptrs, lens, len(bufs), C.byref(cfg), flags, C.byref(batch)) == 0, (kw, flags)
                bt = batch.contents
                assert bt.n_buffers == len(bufs) and bt.n_chunks == sum(len(w[0]) for w in want) and bt.n_chunks > guess
                assert bool(bt.buffer_hash_hex) == bool(flags & CHUNK_MANY_BUFFER_HASHES)
                at = 0
                for b, data in enumerate(bufs):
                    ooff, osz = want[b]
                    assert bt.first_chunk[b] == at, (kw, flags, b)
                    mv = memoryview(data)
                    for i in range(len(ooff)):
                        ch = bt.chunks[at + i]
                        o, s = int(ooff[i]), int(osz[i])
                        assert (ch.offset, ch.size) == (o, s), (kw, flags, b, i)
                        assert ch.hash_hex.decode() == hashlib.sha256(mv[o:o + s]).hexdigest(), (kw, flags, b, i)
                    at += len(ooff)
                    if flags & CHUNK_MANY_BUFFER_HASHES:
                        got = C.string_at(C.addressof(bt.buffer_hash_hex.contents) + 65 * b).decode()
                        deferred = bool(flags & CHUNK_MANY_DEFER) and data.size > im.defer_threshold_host(total)
                        assert got == ("" if deferred else hashlib.sha256(mv).hexdigest()), (kw, flags, b)
                assert bt.first_chunk[len(bufs)] == at == bt.n_chunks
                vt.free_chunk_batch(None, batch)
        assert (1 << 20) + 7 > im.defer_threshold_host(total)          # the deferral above was not vacuous
    finally:
        accel_lib.yams_plugin_shutdown()


# ---- hash_many / verify_many -----------------------------------------------------------------------------------------------
def _suits_the_device(sizes):
    """The refusal rule as the header states it: the longest message against max(LONE_MAX, total / RATIO)."""
    return max(sizes) <= max(LONE_MAX, sum(sizes) // RATIO)


def test_hash_many_and_verify_many_on_both_sides_of_the_refusal_rule(accel_lib):
    """hash_many / verify_many refuse (YAMS_ERR_UNSUPPORTED, counted in refused_lone_chains) exactly when the longest message
    exceeds max(YAMS_HASH_LONE_CHAIN_MAX, total / YAMS_HASH_CHAIN_RATIO): the exact boundary and one byte past it on both
    arms of the max, and random batches on both sides; what is served equals hashlib.  verify_many accepts correct digests
    in lower and upper case, and reports a flipped nibble and a non-hex character as invalid entries of a call that succeeds."""
    vt = _plugin(accel_lib, b"content_hash_v1", _lib.ContentHashV1)
    rng = np.random.default_rng(1205)
    big = rng.integers(0, 256, (3 << 20) + 5000, dtype=np.uint8)

    def table(sizes):
        offs = [(i * 4099) % 1000 for i in range(len(sizes))]
        ptrs = (_lib.u8p * len(sizes))(*[C.cast(big.ctypes.data + o, _lib.u8p) if n else None for o, n in zip(offs, sizes)])
        return offs, ptrs, (C.c_size_t * len(sizes))(*sizes)

    def hash_many(sizes):
        offs, ptrs, lens = table(sizes)
        hexes = C.create_string_buffer(65 * len(sizes))
        st = vt.hash_many(None, ptrs, lens, len(sizes), hexes)
        want = [hashlib.sha256(big[o:o + n].tobytes()).hexdigest() for o, n in zip(offs, sizes)]
        return st, [hexes.raw[65 * i:65 * i + 64].decode() for i in range(len(sizes))], want

    k = LONE_MAX + 4096
    batches = [[LONE_MAX] + [100] * 5, [LONE_MAX + 1] + [100] * 5,                     # the lone-chain arm: at it, one past it
               [k] * RATIO, [k + 1] + [k] * (RATIO - 2) + [k - 1],                     # the ratio arm: total = RATIO * k both times
               [LONE_MAX + 1], [0, 0, 5], [1]]
    for _ in range(14):
        sizes = [im.log_uniform(rng, 1, 200_000) for _ in range(int(rng.integers(1, 60)))]
        sizes.insert(int(rng.integers(0, len(sizes) + 1)), im.log_uniform(rng, LONE_MAX // 2, 3 << 20))
        batches.append(sizes)
    try:
        served = refused = 0
        for sizes in batches:
            before = _health(accel_lib)["refused_lone_chains"]
            st, got, want = hash_many(sizes)
            if _suits_the_device(sizes):
                assert st == 0 and got == want, (sizes[:4], len(sizes))
                assert _health(accel_lib)["refused_lone_chains"] == before
                served += 1
            else:
                assert st == _lib.YAMS_ERR_UNSUPPORTED, (sizes[:4], len(sizes))
                assert _health(accel_lib)["refused_lone_chains"] == before + 1
                refused += 1
        assert served >= 6 and refused >= 6, (served, refused)
        assert _suits_the_device([k] * RATIO) and not _suits_the_device([k + 1] + [k] * (RATIO - 2) + [k - 1])

        # verify_many: the same rule, then the hex comparison
        sizes = [1, 0, 64, 70_001, LONE_MAX, 55, 4096, 300_000, 63, 65, 1000, 119]
        offs, ptrs, lens = table(sizes)
        want = [hashlib.sha256(big[o:o + n].tobytes()).hexdigest() for o, n in zip(offs, sizes)]
        forms, expect_valid = [], []
        for i, hx in enumerate(want):
            kind = i % 4
            if kind == 0:   forms.append(hx); expect_valid.append(1)
            elif kind == 1: forms.append(hx.upper()); expect_valid.append(1)
            elif kind == 2:
                p = int(rng.integers(0, 64))
                forms.append(hx[:p] + "%x" % (int(hx[p], 16) ^ 1) + hx[p + 1:]); expect_valid.append(0)        # one flipped nibble
            else:
                p = int(rng.integers(0, 64))
                forms.append(hx[:p] + "gG/:@` "[i % 7] + hx[p + 1:]); expect_valid.append(0)                     # not a hex digit
        blob = b"".join(f.encode() + b"\0" for f in forms)
        valid = (C.c_uint8 * len(sizes))(*([7] * len(sizes)))
        assert vt.verify_many(None, ptrs, lens, blob, len(sizes), valid) == 0
        assert list(valid) == expect_valid
        mixed = "".join(c.upper() if j % 3 else c for j, c in enumerate(want[3]))                                # mixed case
        blob = b"".join((mixed if i == 3 else h).encode() + b"\0" for i, h in enumerate(want))
        assert vt.verify_many(None, ptrs, lens, blob, len(sizes), valid) == 0 and list(valid) == [1] * len(sizes)
        before = _health(accel_lib)["refused_lone_chains"]
        offs, ptrs, lens = table([LONE_MAX + 1, 10])
        assert vt.verify_many(None, ptrs, lens, b"0" * 130, 2, valid) == _lib.YAMS_ERR_UNSUPPORTED
        assert _health(accel_lib)["refused_lone_chains"] == before + 1
    finally:
        accel_lib.yams_plugin_shutdown()
