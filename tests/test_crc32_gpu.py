"""The batched CRC-32 on the GPU against zlib.crc32, bit for bit: every alignment, the segment edges, length
alone, overlapping prefixes, every byte read once, segment order, skewed batches, workspace reuse, the verify and chunk
entries, host memory, the plugin door from four threads, the C++ shell, and the randomised harness.  Every device output
sits between sentinel words that must not change."""
import ctypes as C
import json
import os
import subprocess
import sys
import threading
import zlib

import numpy as np
import pytest

import _crc32_model as cm
from yams_amd import _lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = cm.S
SENT = cm.SENTINEL


def _dev(arr):
    import torch
    a = np.ascontiguousarray(arr)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def _batch(acc, d_data, offs, lens):
    """yams_crc32_batch_device over (offs, lens) -> uint32[n]; the words around the output must survive."""
    n = len(lens)
    out = _dev(np.full(n + 2, SENT, np.uint32))
    d_off, d_len = _dev(np.array(offs, np.uint64)), _dev(np.array(lens, np.uint64))
    acc.crc32_batch_device(d_data.data_ptr(), d_off.data_ptr() if n else None, d_len.data_ptr() if n else None, n, out.data_ptr() + 4)
    got = out.cpu().numpy().view(np.uint32)
    assert got[0] == SENT and got[n + 1] == SENT
    return got[1:n + 1]


def _zl(b, offs, lens):
    return np.array([zlib.crc32(b[o:o + n]) & 0xFFFFFFFF for o, n in zip(offs, lens)], np.uint32)


def _mismatch(got, want):
    bad = np.nonzero(got != want)[0]
    return [(int(i), hex(int(got[i])), hex(int(want[i]))) for i in bad[:5]]


def test_every_alignment_and_every_short_length(acc):
    rng = np.random.default_rng(1)
    offs, lens, at = [], [], 0
    for a in range(16):
        for n in range(81):
            at = (at + 15) // 16 * 16 + a
            offs.append(at); lens.append(n); at += n
    data = rng.integers(0, 256, at + 16, dtype=np.uint8)
    got = _batch(acc, _dev(data), offs, lens)
    assert not _mismatch(got, _zl(data.tobytes(), offs, lens))


def test_segment_edges_at_three_bases(acc):
    rng = np.random.default_rng(2)
    edge = [S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1, 3 * S + 5, 255 * S, 256 * S, 256 * S + 1, 257 * S]
    offs, lens, at = [], [], 0
    for base in (0, 1, 15):
        for n in edge:
            at = (at + 15) // 16 * 16 + base
            offs.append(at); lens.append(n); at += n
    data = rng.integers(0, 256, at + 16, dtype=np.uint8)
    got = _batch(acc, _dev(data), offs, lens)
    assert not _mismatch(got, _zl(data.tobytes(), offs, lens))


def test_length_alone_all_zero_messages(acc):
    """All-zero messages of every length 0..2S+3 differ in nothing but their length: a wrong shift length shows."""
    top = 2 * S + 3
    data = np.zeros(top + 16, np.uint8)
    lens = list(range(top + 1))
    got = _batch(acc, _dev(data), [0] * len(lens), lens)
    z = bytes(top)
    want = np.array([zlib.crc32(z[:n]) & 0xFFFFFFFF for n in lens], np.uint32)
    assert not _mismatch(got, want)
    assert len(set(want.tolist())) == len(lens)


def test_overlapping_prefixes_in_one_call(acc):
    rng = np.random.default_rng(3)
    data = rng.integers(0, 256, 4 * S + 16, dtype=np.uint8)
    lens = list(range(0, 4 * S + 1, 97))
    got = _batch(acc, _dev(data), [0] * len(lens), lens)
    assert not _mismatch(got, _zl(data.tobytes(), [0] * len(lens), lens))


def test_every_byte_is_read(acc):
    """One message of 3S + 37 bytes at offset 3; one bit flipped at the first four bytes, either side of every 16-byte and
    every segment boundary of the message and of memory, and the last byte: each result is zlib's of the flipped bytes, and
    differs from the unflipped value (CRC-32 detects every single-bit error, so the oracle alone discriminates)."""
    rng = np.random.default_rng(4)
    n, off = 3 * S + 37, 3
    base = rng.integers(0, 256, off + n + 16, dtype=np.uint8)
    pos = {0, 1, 2, 3, n - 1}
    for k in range(16, n, 16):            # message-relative and memory-relative granule boundaries
        pos |= {k - 1, k, k - off - 1, k - off}
    for k in range(S, n, S):
        pos |= {k - 1, k}
    pos = sorted(p for p in pos if 0 <= p < n)
    clean = zlib.crc32(base[off:off + n].tobytes()) & 0xFFFFFFFF
    stride = (off + n + 16 + 15) // 16 * 16
    data = np.tile(np.concatenate([base, np.zeros(stride - base.size, np.uint8)]), len(pos))
    for j, p in enumerate(pos):
        data[j * stride + off + p] ^= np.uint8(1 << (p % 8))
    offs = [j * stride + off for j in range(len(pos))]
    got = _batch(acc, _dev(data), offs, [n] * len(pos))
    want = _zl(data.tobytes(), offs, [n] * len(pos))
    assert not _mismatch(got, want)
    assert not np.any(want == clean)


def test_segment_order_matters(acc):
    rng = np.random.default_rng(5)
    segs = [rng.integers(0, 256, S, dtype=np.uint8) for _ in range(6)]
    a = np.concatenate(segs)
    swapped = list(segs); swapped[1], swapped[4] = swapped[4], swapped[1]
    b = np.concatenate(swapped)
    data = np.concatenate([a, b, np.zeros(16, np.uint8)])
    got = _batch(acc, _dev(data), [0, a.size], [a.size, b.size])
    want = _zl(data.tobytes(), [0, a.size], [a.size, b.size])
    assert want[0] != want[1]
    assert not _mismatch(got, want)


@pytest.fixture(scope="module")
def skewed():
    """One 64 MiB and one 1 MiB message, 20 000 messages of at most 100 bytes and zero-length ones, interleaved."""
    rng = np.random.default_rng(6)
    big, mid = 64 << 20, 1 << 20
    data = rng.integers(0, 256, big + mid + 2_100_000, dtype=np.uint8)
    small_at = big + mid + 7
    offs, lens = [], []
    for i in range(20_000):
        if i == 3_000:
            offs.append(5); lens.append(big)
        if i == 11_111:
            offs.append(big + 6); lens.append(mid)
        n = 0 if i % 17 == 0 else int(rng.integers(1, 101))
        offs.append(small_at); lens.append(n); small_at += n + int(rng.integers(0, 3))
    b = data.tobytes()
    return data, offs, lens, _zl(b, offs, lens)


def test_skewed_batch_in_input_order(acc, skewed):
    data, offs, lens, want = skewed
    got = _batch(acc, _dev(data), offs, lens)
    assert not _mismatch(got, want)


def test_workspace_small_large_small(acc, skewed):
    data, offs, lens, want = skewed
    d = _dev(data)
    small = slice(100, 140)
    assert not _mismatch(_batch(acc, d, offs[small], lens[small]), want[small])
    assert not _mismatch(_batch(acc, d, offs, lens), want)
    assert not _mismatch(_batch(acc, d, offs[small], lens[small]), want[small])


def test_n_zero_writes_nothing(acc):
    d = _dev(np.zeros(64, np.uint8))
    assert _batch(acc, d, [], []).size == 0
    bad = C.c_uint64(77)
    assert acc.L.yams_crc32_verify_device(acc.ctx, d.data_ptr(), None, None, 0, None, None, C.byref(bad)) == 0 and bad.value == 0
    assert acc.L.yams_crc32_many_host(acc.ctx, None, None, 0, None) == 0
    assert acc.L.yams_crc32_batch_device(None, d.data_ptr(), None, None, 0, None) == _lib.YAMS_ERR_INVALID_ARG
    assert acc.L.yams_crc32_batch_device(acc.ctx, d.data_ptr(), None, None, 3, None) == _lib.YAMS_ERR_INVALID_ARG
    assert acc.L.yams_crc32_batch_device(acc.ctx, d.data_ptr(), d.data_ptr(), d.data_ptr(), 1 << 31, d.data_ptr()) == _lib.YAMS_ERR_UNSUPPORTED


@pytest.mark.parametrize("kind", ["planted", "all_valid", "all_invalid"])
def test_verify_device(acc, kind):
    rng = np.random.default_rng(7)
    n = 301
    lens = [int(x) for x in rng.integers(0, 3 * S, n)]
    offs = np.concatenate([[3], 3 + np.cumsum(lens)[:-1]]).tolist()
    data = rng.integers(0, 256, sum(lens) + 32, dtype=np.uint8)
    want = _zl(data.tobytes(), offs, lens)
    bad = {"planted": [0, n // 2, n - 1], "all_valid": [], "all_invalid": list(range(n))}[kind]
    expected = want.copy()
    for i in bad:
        expected[i] ^= np.uint32(1 << (i % 32))
    d_exp = _dev(np.concatenate([[0], expected]).astype(np.uint32))       # handed in at + 4 bytes: only 4-byte aligned
    assert (d_exp.data_ptr() + 4) % 16 == 4
    valid = _dev(np.full(n + 2, 0xA5, np.uint8))
    d_data, d_off, d_len = _dev(data), _dev(np.array(offs, np.uint64)), _dev(np.array(lens, np.uint64))
    n_bad = acc.crc32_verify_device(d_data.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n, d_exp.data_ptr() + 4, valid.data_ptr() + 1)
    v = valid.cpu().numpy()
    assert v[0] == 0xA5 and v[n + 1] == 0xA5
    assert n_bad == len(bad)
    assert np.nonzero(v[1:n + 1] == 0)[0].tolist() == bad and set(v[1:n + 1].tolist()) <= {0, 1}


def test_chunks_of_an_ingest_result(acc):
    """yams_crc32_chunks_device after yams_ingest_device: an empty blob, one byte, below the minimum chunk size, 2 MiB of
    zeros (forced cuts at the maximum size), 3 MiB random; every chunk against zlib; with a select mask unselected entries
    are 0 and selected ones unchanged; the result's digest arrays are intact afterwards."""
    from yams_amd.accel import cdc_config
    rng = np.random.default_rng(8)
    blobs = [np.zeros(0, np.uint8), rng.integers(0, 256, 1, dtype=np.uint8), rng.integers(0, 256, 5000, dtype=np.uint8),
             np.zeros(2 << 20, np.uint8), rng.integers(0, 256, 3 << 20, dtype=np.uint8)]
    offs, at = [], 9
    for b in blobs:
        offs.append(at); at += b.size + 5
    data = np.zeros(at + 16, np.uint8)
    for o, b in zip(offs, blobs):
        data[o:o + b.size] = b
    d_data = _dev(data)
    res = acc.ingest_device(d_data.data_ptr(), offs, [b.size for b in blobs], cdc_config("streaming"), flags=3)
    tab = acc.fetch_ingest(res, len(blobs))
    n = int(tab["n_chunks"])
    assert n >= 1 + 1 + 2 + 3 and tab["blob_first"].tolist()[:2] == [0, 0]
    raw = data.tobytes()
    m_off = [offs[int(b)] + int(o) for b, o in zip(tab["chunk_blob"], tab["chunk_offset"])]
    want = _zl(raw, m_off, [int(s) for s in tab["chunk_size"]])
    out = _dev(np.full(n + 2, SENT, np.uint32))
    acc.crc32_chunks_device(d_data.data_ptr(), offs, res, out.data_ptr() + 4)
    got = out.cpu().numpy().view(np.uint32)
    assert got[0] == SENT and got[n + 1] == SENT and not _mismatch(got[1:n + 1], want)
    select = (np.arange(n) % 3 != 1).astype(np.uint8)
    d_sel = _dev(select)
    out2 = _dev(np.full(n + 2, SENT, np.uint32))
    acc.crc32_chunks_device(d_data.data_ptr(), offs, res, out2.data_ptr() + 4, d_sel.data_ptr())
    got2 = out2.cpu().numpy().view(np.uint32)
    assert got2[0] == SENT and got2[n + 1] == SENT and not _mismatch(got2[1:n + 1], np.where(select == 1, want, 0).astype(np.uint32))
    after = acc.fetch_ingest(res, len(blobs))
    for key in ("chunk_offset", "chunk_size", "chunk_blob", "blob_first", "chunk_digest", "blob_digest"):
        assert np.array_equal(after[key], tab[key]), key


def test_many_host(acc):
    rng = np.random.default_rng(9)
    assert acc.crc32(b"123456789") == 0xCBF43926 and acc.crc32(b"") == 0
    msgs = [rng.integers(0, 256, int(n), dtype=np.uint8) for n in rng.integers(0, 3 * S, 297)] + [None, b"", b"a"]
    got = acc.crc32_many(msgs)
    want = np.array([zlib.crc32(bytes(m) if m is not None else b"") & 0xFFFFFFFF for m in msgs], np.uint32)
    assert not _mismatch(got, want)
    big = [rng.integers(0, 256, 3_000_001, dtype=np.uint8) for _ in range(3)]        # a total above 8 MiB
    assert not _mismatch(acc.crc32_many(big), np.array([zlib.crc32(m.tobytes()) & 0xFFFFFFFF for m in big], np.uint32))
    # a NULL pointer with length 0 is an empty message; with a length it is refused; so are NULL tables
    L = acc.L
    ptrs = (C.c_void_p * 2)(None, None)
    out = (C.c_uint32 * 4)(SENT, SENT, SENT, SENT)
    assert L.yams_crc32_many_host(acc.ctx, ptrs, (C.c_size_t * 2)(0, 0), 2, C.cast(C.addressof(out) + 4, _lib.u32p)) == 0
    assert list(out) == [SENT, 0, 0, SENT]
    assert L.yams_crc32_many_host(acc.ctx, ptrs, (C.c_size_t * 2)(0, 5), 2, out) == _lib.YAMS_ERR_INVALID_ARG
    assert L.yams_crc32_many_host(acc.ctx, None, (C.c_size_t * 2)(0, 0), 2, out) == _lib.YAMS_ERR_INVALID_ARG
    assert L.yams_crc32_many_host(acc.ctx, ptrs, None, 2, out) == _lib.YAMS_ERR_INVALID_ARG
    assert L.yams_crc32_many_host(acc.ctx, ptrs, (C.c_size_t * 2)(0, 0), 2, None) == _lib.YAMS_ERR_INVALID_ARG
    assert L.yams_crc32_many_host(None, ptrs, (C.c_size_t * 2)(0, 0), 2, out) == _lib.YAMS_ERR_INVALID_ARG


def test_ingest_host_crc32_is_ingest_host_plus_one_array(acc):
    """yams_ingest_host_crc32 over blobs that take at least three batches: every other output identical to yams_ingest_host
    on the same blobs, every chunk's CRC zlib's, nothing written behind n_chunks."""
    from yams_amd.accel import cdc_config
    rng = np.random.default_rng(10)
    blobs = [rng.integers(0, 256, int(n), dtype=np.uint8) for n in (0, 1, 3000, 700_001, 1 << 20, 40_000, 900_000, 123_457)]
    blobs[4][:] = 0                              # forced cuts at the maximum size
    ptrs = [b.ctypes.data if b.size else None for b in blobs]
    lens = [b.size for b in blobs]
    cfg = cdc_config("streaming", min_size=4096, max_size=65536)
    kw = dict(cfg=cfg, flags=3, batch_bytes=1 << 20)
    plain = acc.ingest_host(ptrs, lens, **kw)
    assert acc.device_info()["last_host_ingest"]["batches"] >= 3
    both = acc.ingest_host(ptrs, lens, with_crc32=True, **kw)
    assert acc.device_info()["last_host_ingest"]["batches"] >= 3
    assert both["n_chunks"] == plain["n_chunks"] > len(blobs)
    for key in ("blob_first", "chunk_offset", "chunk_size", "chunk_digest", "blob_digest"):
        assert np.array_equal(both[key], plain[key]), key
    first = plain["blob_first"]
    want = []
    for b, blob in enumerate(blobs):
        raw = blob.tobytes()
        for c in range(int(first[b]), int(first[b + 1])):
            o, s = int(plain["chunk_offset"][c]), int(plain["chunk_size"][c])
            want.append(zlib.crc32(raw[o:o + s]) & 0xFFFFFFFF)
    assert not _mismatch(both["chunk_crc32"], np.array(want, np.uint32))
    # exactly the required capacity, guard words behind it
    n = plain["n_chunks"]
    crc = np.full(n + 2, SENT, np.uint32)
    off = np.zeros(n, np.uint64); sz = np.zeros(n, np.uint64); fb = np.zeros(len(blobs) + 1, np.uint64)
    cnt = C.c_uint64(0)
    pa = (C.c_void_p * len(blobs))(*ptrs)
    la = np.array(lens, np.uint64)
    st = acc.L.yams_ingest_host_crc32(acc.ctx, pa, la.ctypes.data_as(_lib.u64p), len(blobs), C.byref(cfg), 0, 1 << 20, fb.ctypes.data_as(_lib.u64p),
                                      off.ctypes.data_as(_lib.u64p), sz.ctypes.data_as(_lib.u64p), None, n, None, C.byref(cnt), crc.ctypes.data)
    assert st == 0 and cnt.value == n and crc[n] == SENT and crc[n + 1] == SENT and not _mismatch(crc[:n], np.array(want, np.uint32))
    assert acc.L.yams_ingest_host_crc32(acc.ctx, pa, la.ctypes.data_as(_lib.u64p), len(blobs), C.byref(cfg), 0, 1 << 20, fb.ctypes.data_as(_lib.u64p),
                                        off.ctypes.data_as(_lib.u64p), sz.ctypes.data_as(_lib.u64p), None, n, None, C.byref(cnt), None) == _lib.YAMS_ERR_INVALID_ARG


def test_the_plugin_door_from_four_threads(acc):
    L = acc.L
    assert L.yams_plugin_init(b'{"device": 0}', None) == 0
    try:
        p = C.c_void_p()
        assert L.yams_plugin_get_interface(b"content_checksum_v1", 1, C.byref(p)) == 0
        vt = C.cast(p, C.POINTER(_lib.ContentChecksumV1)).contents
        errors = []

        def work(seed):
            try:
                rng = np.random.default_rng(seed)
                for _ in range(4):
                    msgs = [rng.integers(0, 256, int(n), dtype=np.uint8) for n in rng.integers(0, 5 * S, 50)]
                    n = len(msgs)
                    want = [zlib.crc32(m.tobytes()) & 0xFFFFFFFF for m in msgs]
                    ptrs = (C.c_void_p * n)(*[m.ctypes.data if m.size else None for m in msgs])
                    lens = (C.c_size_t * n)(*[m.size for m in msgs])
                    out = (C.c_uint32 * n)()
                    assert vt.crc32_many(None, ptrs, lens, n, out) == 0 and list(out) == want
                    one = C.c_uint32(SENT)
                    assert vt.crc32(None, C.cast(ptrs[7], _lib.u8p), lens[7], C.byref(one)) == 0 and one.value == want[7]
                    expected = (C.c_uint32 * n)(*[w ^ (1 if i % 5 == 0 else 0) for i, w in enumerate(want)])
                    valid = (C.c_uint8 * n)(*([9] * n))
                    assert vt.verify_many(None, ptrs, lens, expected, n, valid) == 0
                    assert list(valid) == [0 if i % 5 == 0 else 1 for i in range(n)]
            except BaseException as e:       # noqa: BLE001 (reported by the main thread)
                errors.append(repr(e))
        ts = [threading.Thread(target=work, args=(s,)) for s in range(4)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errors, errors
    finally:
        L.yams_plugin_shutdown()


def test_the_cpp_shell_driver():
    import _crc32_build
    exe = _crc32_build.build_checksum_shell_test()
    r = subprocess.run([exe, _lib.LIB_PATH], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_randomised_crc32_stress_against_zlib():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "stress_crc32.py"), "--cases", str(cm.PINNED_CASES), "--seed",
                        str(cm.PINNED_SEED)], capture_output=True, text=True, timeout=280)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert line, r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads(line[-1])
    print(line[-1])
    assert r.returncode == 0 and res["mode"] == "device" and res["fatal"] is None, res
    assert res["mismatches"] == 0 and res["cases_run"] == cm.PINNED_CASES and not res["paths_below_floor"], res
