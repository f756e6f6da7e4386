"""GPU parity suite for the chunk dedup lookup and the batched integrity check.

Oracle for the set semantics: a Python set walked in order, which is what ContentStore::store does
with storage_->exists() (src/api/content_store_impl.cpp:246-287): chunk i is new iff its hash is
neither in the store nor carried by an earlier chunk of the same walk (walk() in tests/_dedup.py).

The collision tests place digests on chosen slots (digest() in tests/_dedup.py): same-tag families at one home, at
adjacent homes, across the wrap from the last slot to slot 0, and tag words 0 and 1 (which share tag 1).  Every call
of those is checked by Checked: is_new against walk(), then probe true for every digest ever inserted, false for the
near misses of all of them, and len() equal to the oracle's size."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from _dedup import (Checked, adjacent_homes, capacity_after, digest, digests, near_misses, same_home, tag01, walk,
                    wrap)
from yams_amd import _lib
from yams_amd.accel import cdc_config

pytestmark = pytest.mark.gpu

TAG = 0x1F2E3D4C5B6A7988          # an arbitrary tag word for the collision families


def test_dedup_matches_sequential_exists_walk(acc):
    rng = np.random.default_rng(1)
    s = acc.dedup_set(0)
    store = set()
    pool = rng.integers(0, 256, (5000, 32), dtype=np.uint8)
    for n in (1, 7, 1000, 20000, 3):
        idx = rng.integers(0, len(pool), n)                 # heavy duplication inside and across calls
        d = pool[idx]
        got = s.insert(d)
        assert np.array_equal(got, walk(store, d)), n
        assert len(s) == len(store)
    probe = np.concatenate([pool[:100], rng.integers(0, 256, (100, 32), dtype=np.uint8)])
    exp = np.array([p.tobytes() in store for p in probe])
    assert np.array_equal(s.probe(probe), exp)
    assert not s.insert(np.zeros((0, 32), np.uint8)).any()


def test_dedup_growth_and_scale(acc):
    rng = np.random.default_rng(2)
    s = acc.dedup_set(16)                                    # forces several rehashes
    store = set()
    total = 0
    for n in (3000, 50000, 400000):
        d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        d[n // 2:] = d[: n - n // 2]                          # second half repeats the first
        got = s.insert(d)
        assert np.array_equal(got, walk(store, d))
        total += n
    assert len(s) == len(store)
    old = rng.integers(0, 256, (10, 32), dtype=np.uint8)
    assert not s.probe(old).any()


def test_dedup_tag_collisions_and_zero_tags(acc):
    """Digests that share their first 8 bytes (the slot tag) but differ later, all-zero prefixes
    (tag 0 is the empty marker), and first-8-bytes == 1 (what a zero tag maps to)."""
    rng = np.random.default_rng(3)
    base = rng.integers(0, 256, (64, 32), dtype=np.uint8)
    fam = np.repeat(base, 8, axis=0)
    fam[:, 8:] = rng.integers(0, 256, (fam.shape[0], 24), dtype=np.uint8)    # 8 digests per shared tag
    zero = rng.integers(0, 256, (16, 32), dtype=np.uint8); zero[:, :8] = 0
    one = zero.copy(); one[:, 0] = 1; one[:, 8:] = rng.integers(0, 256, (16, 24), dtype=np.uint8)
    d = np.concatenate([fam, zero, one, fam[::3], zero[::2]])
    rng.shuffle(d, axis=0)
    s = acc.dedup_set(0)
    store = set()
    assert np.array_equal(s.insert(d), walk(store, d))
    assert np.array_equal(s.insert(d), np.zeros(len(d), bool))               # everything is known now
    assert s.probe(d).all() and len(s) == len(store)
    near = fam.copy(); near[:, 31] ^= 1                                        # same tag, never inserted
    assert not s.probe(near).any()


def test_ingest_dedup_verify_pipeline(acc):
    """Ingest (CDC + digests) -> dedup lookup -> integrity check, all on device-resident arrays:
    the second ingest of the same blobs is 100 % deduplicated; a corrupted byte is pinned to its chunk."""
    import torch
    rng = np.random.default_rng(4)
    blob = rng.integers(0, 256, 3 << 20, dtype=np.uint8)
    data = np.concatenate([blob, blob, rng.integers(0, 256, 1 << 20, dtype=np.uint8)])   # blob twice + a new one
    offs, lens = [0, len(blob), 2 * len(blob)], [len(blob), len(blob), 1 << 20]
    td = torch.from_numpy(data).cuda()
    res = acc.ingest_device(td.data_ptr(), offs, lens, cdc_config("streaming"), flags=3)
    got = acc.fetch_ingest(res, 3)
    n = int(res.n_chunks)
    s = acc.dedup_set(0)
    flags = torch.zeros(n, dtype=torch.uint8, device="cuda")
    n_new, b_new, b_dup = s.insert_device(res.chunk_digest, n, res.chunk_size, flags.data_ptr())
    first = int(got["blob_first"][1])
    is_new = flags.cpu().numpy().astype(bool)
    assert is_new[:first].all() and not is_new[first:2 * first].any()        # the repeated blob dedups completely
    assert n_new == int(is_new.sum()) == len(s)
    sizes = got["chunk_size"]
    assert b_new == int(sizes[is_new].sum()) and b_dup == int(sizes[~is_new].sum())
    assert b_new + b_dup == len(data)
    # oracle for the digests the set saw
    store = set()
    dg = got["chunk_digest"].reshape(n, 32)
    assert np.array_equal(is_new, walk(store, dg))
    # --- integrity check against the manifest (offset within blob + blob base)
    base = np.asarray(offs, np.uint64)[got["chunk_blob"]]
    abs_off = torch.from_numpy((got["chunk_offset"] + base).astype(np.uint64).view(np.int64)).cuda()
    szs = torch.from_numpy(sizes.astype(np.uint64).view(np.int64)).cuda()
    valid = torch.zeros(n, dtype=torch.uint8, device="cuda")
    assert acc.verify_chunks_device(td.data_ptr(), abs_off.data_ptr(), szs.data_ptr(), n, res.chunk_digest,
                                    valid.data_ptr()) == 0 and bool(valid.all())
    expected = torch.from_numpy(dg.copy()).cuda()                              # survives the next ingest call
    victim = n // 3
    pos = int(got["chunk_offset"][victim] + base[victim]) + 5
    td[pos] ^= 0x40
    bad = acc.verify_chunks_device(td.data_ptr(), abs_off.data_ptr(), szs.data_ptr(), n, expected.data_ptr(),
                                   valid.data_ptr())
    v = valid.cpu().numpy().astype(bool)
    assert bad == 1 and not v[victim] and v.sum() == n - 1
    # and the reference rule itself: SHA-256 of the slice vs the expected hex
    sl = td[int(abs_off[victim]):int(abs_off[victim]) + int(sizes[victim])].cpu().numpy().tobytes()
    assert hashlib.sha256(sl).digest() != dg[victim].tobytes()


# ---- tag collisions on chosen slots ----------------------------------------------------------------------------------
def test_lost_key_when_a_lower_index_arrives_in_a_later_round(acc):
    """Z (index 0) and A (1) share tag and home h, B (2) has the tag and home h + 1.  Round 1: Z owns h, A moves on;
    B claims h + 1.  Round 2: A reaches h + 1 — B's key is written there and must not be replaced by A's."""
    c = Checked(acc.dedup_set(0))
    h = 100
    z, a, b = digest(TAG, h, 1), digest(TAG, h, 2), digest(TAG, h + 1, 3)
    assert c.insert([z, a, b], "first").all()
    assert not c.insert([z, a, b], "again").any()
    assert not c.insert([b, a, z], "reversed").any()


@pytest.mark.parametrize("k", [1, 2, 3])
def test_lost_key_when_the_late_arrival_comes_in_round_k_plus_1(acc, k):
    """k same-tag entries at homes h .. h+k-1 (one call each), then [A, B] in one call with A at home h and B at home
    h + k: A passes the k settled entries one round each and reaches B's slot in round k + 1."""
    c = Checked(acc.dedup_set(0))
    h = 300
    for j in range(k):
        assert c.insert([digest(TAG, h + j, 100 + j)], f"settled {j}").all()
    a, b = digest(TAG, h, 1), digest(TAG, h + k, 2)
    assert c.insert([a, b], "a, b").all()
    assert not c.insert([a, b], "a, b again").any()
    assert c.insert([digest(TAG, h + k, 3)], "behind b").all()


def test_first_occurrence_under_every_order(acc):
    """One multiset of same-tag digests at adjacent homes, with duplicates, in several index orders: is_new is true
    exactly at each digest's first index (walk() on an empty store), on a fresh set per order."""
    rng = np.random.default_rng(11)
    base = np.concatenate([same_home(TAG, 500, 3, 0), same_home(TAG, 501, 2, 10), same_home(TAG, 502, 2, 20),
                           same_home(TAG + 1, 501, 2, 30)])
    ms = np.concatenate([base, base[[0, 0, 2, 3, 5, 7, 8]]])
    orders = [np.arange(len(ms)), np.arange(len(ms))[::-1]] + [rng.permutation(len(ms)) for _ in range(6)]
    for o, perm in enumerate(orders):
        c = Checked(acc.dedup_set(0))
        d = ms[perm]
        got = c.insert(d, f"order {o}")
        first = {}
        for i, row in enumerate(d):
            first.setdefault(row.tobytes(), i)
        assert np.array_equal(np.flatnonzero(got), np.array(sorted(first.values()))), o
        assert not c.insert(d, f"order {o} again").any()


def test_deep_same_tag_chains(acc):
    """Chains far longer than 66 slots: 200 same-tag same-home digests in one call; 60 then 70 more at one home in two
    calls; a chain that runs through settled entries of three earlier calls.  Every call returns OK."""
    c = Checked(acc.dedup_set(0))
    assert c.insert(same_home(TAG, 10, 200, 0), "200 in one call").all()
    c = Checked(acc.dedup_set(0))
    assert c.insert(same_home(TAG, 20, 60, 0), "60").all()
    assert c.insert(same_home(TAG, 20, 70, 1000), "70 more").all()
    known = np.concatenate([same_home(TAG, 20, 60, 0), same_home(TAG, 20, 70, 1000)])
    assert not c.insert(known[::-1], "all 130 known").any()
    c = Checked(acc.dedup_set(0))
    for j in range(3):
        c.insert(adjacent_homes(TAG, 700, 4, 25, 100 * j), f"settled call {j}")
    d = np.concatenate([adjacent_homes(TAG, 700, 4, 40, 5000), adjacent_homes(TAG, 700, 4, 10, 150)])
    c.insert(d[np.random.default_rng(12).permutation(len(d))], "through settled")


def test_wrap_around_chain_and_tag_0_1_aliasing(acc):
    """A same-tag chain at the last slot that wraps to slots 0, 1, ... (with entries of another tag already sitting
    there), and digests whose first words are 0 and 1 — both carry tag 1 — at one home."""
    c = Checked(acc.dedup_set(0))
    c.insert(digests(TAG + 5, [0, 1, 2], [1, 2, 3]), "other tag at slots 0..2")
    w = wrap(TAG, 12, 0, spill=3)
    assert c.insert(w[::2], "wrap, even rows").all()
    c.insert(np.concatenate([w, w[:4]])[::-1], "wrap, all rows reversed, repeats")
    c.insert(wrap(TAG, 5, 100), "more at LAST")
    t = tag01(40, 12, 0)
    assert c.insert(t[:6], "tag 0/1, first six").all()
    c.insert(np.concatenate([t, t[::3], digests([0, 1], 40, [500, 500])]), "tag 0/1, all + repeats")
    c.insert(np.concatenate([tag01(41, 4, 50), same_home(1, 40, 3, 900)]), "tag word 1 at home 40 and 41")


def test_growth_with_same_tag_clusters_in_flight(acc):
    """Start from dedup_set(0) (1024 slots); settle adjacent-home families, then one call that forces a rehash while it
    carries more members of those families and new ones.  Homes below 1024 keep their slots at every capacity."""
    rng = np.random.default_rng(13)
    c = Checked(acc.dedup_set(0))
    fams = [adjacent_homes(TAG + f, 64 * f, 3, 8, 0) for f in range(8)]
    c.insert(np.concatenate([f[:5] for f in fams] + [wrap(TAG, 6, 0)]), "families, before growth")
    big = np.concatenate([rng.integers(0, 256, (2600, 32), dtype=np.uint8)] + fams +
                         [adjacent_homes(TAG + 99, 1000, 4, 12, 0), wrap(TAG, 10, 0, spill=4)])
    assert capacity_after(1024, len(c.store), len(big)) > 1024
    c.insert(big[rng.permutation(len(big))], "growth call")
    allk = c.keys()
    assert not c.insert(allk[rng.permutation(len(allk))], "everything again").any()


def _dev_copy(torch, a, offset=0):
    """a's bytes at `offset` bytes into a zero-padded device buffer: (buffer, pointer)."""
    raw = np.ascontiguousarray(a).view(np.uint8).ravel()
    buf = torch.zeros(raw.size + offset + 64, dtype=torch.uint8, device="cuda")
    if raw.size:
        buf[offset:offset + raw.size] = torch.from_numpy(raw.copy()).cuda()
    torch.cuda.synchronize()
    return buf, buf.data_ptr() + offset


def _probe_device(torch, s, ptr, n):
    out = torch.full((n,), 0xAA, dtype=torch.uint8, device="cuda")
    s.acc._check(s.acc.L.yams_dedup_probe_device(s.h, ptr, n, out.data_ptr()))
    return out.cpu().numpy()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 4097])
def test_device_entry_points_byte_counters_and_alignment(acc, n):
    """yams_dedup_insert_device / probe_device against walk() and numpy sums: n_new, bytes_new, bytes_deduped with
    chunk sizes above 2^32 (64-bit sums); chunk_sizes = NULL; digests 8 bytes into a larger buffer; a pointer 4 bytes
    in is refused with INVALID_ARG and leaves the set unchanged and usable; the host forms answer the same."""
    import torch
    rng = np.random.default_rng(100 + n)
    pool = np.concatenate([rng.integers(0, 256, (max(1, n // 2), 32), dtype=np.uint8),
                           adjacent_homes(TAG + n, 40, 3, 6, 0), wrap(TAG + n, 3, 0)])
    d = pool[rng.integers(0, len(pool), n)]                                    # repeats inside the call
    sizes = rng.integers(0, 1 << 36, n, dtype=np.uint64) + np.uint64(1 << 32)    # every size above 2^32
    ds, hs, store = acc.dedup_set(0), acc.dedup_set(0), set()
    dbuf, dptr = _dev_copy(torch, d, 8)
    sbuf, sptr = _dev_copy(torch, sizes)
    flags = torch.full((n,), 0xAA, dtype=torch.uint8, device="cuda")
    n_new, b_new, b_dup = ds.insert_device(dptr, n, sptr, flags.data_ptr())
    exp = walk(store, d)
    got = flags.cpu().numpy()
    assert np.array_equal(got, exp.astype(np.uint8)), np.flatnonzero(got != exp)[:20]
    assert n_new == int(exp.sum()) == len(ds)
    assert b_new == int(sizes[exp].sum()) and b_dup == int(sizes[~exp].sum()) and b_new + b_dup > (1 << 32)
    assert np.array_equal(hs.insert(d), exp) and len(hs) == len(store)
    keys = np.frombuffer(b"".join(store), np.uint8).reshape(-1, 32)
    near = near_misses(keys)
    q = np.concatenate([d, near, rng.integers(0, 256, (5, 32), dtype=np.uint8)])
    qexp = np.array([r.tobytes() in store for r in q], np.uint8)
    qbuf, qptr = _dev_copy(torch, q, 8)
    assert np.array_equal(_probe_device(torch, ds, qptr, len(q)), qexp)
    assert np.array_equal(hs.probe(q).astype(np.uint8), qexp)
    # a digest pointer that is not 8-byte aligned: refused, nothing changes
    new = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    nbuf, nptr = _dev_copy(torch, new, 8)
    for bad in (lambda: ds.insert_device(nptr - 4, n, sptr, flags.data_ptr()),
                lambda: ds.acc._check(ds.acc.L.yams_dedup_probe_device(ds.h, nptr - 4, n, flags.data_ptr()))):
        with pytest.raises(_lib.AccelError) as e:
            bad()
        assert e.value.status == _lib.YAMS_ERR_INVALID_ARG
    assert len(ds) == len(store)
    assert np.array_equal(_probe_device(torch, ds, qptr, len(q)), qexp)
    # chunk_sizes = NULL: no byte sums, the same answers
    d2 = np.concatenate([new, d])[rng.permutation(2 * n)][:n]
    d2buf, d2ptr = _dev_copy(torch, d2, 8)
    flags.fill_(0xAA); torch.cuda.synchronize()
    n_new, b_new, b_dup = ds.insert_device(d2ptr, n, None, flags.data_ptr())
    exp2 = walk(store, d2)
    assert np.array_equal(flags.cpu().numpy(), exp2.astype(np.uint8))
    assert n_new == int(exp2.sum()) and b_new == 0 and b_dup == 0 and len(ds) == len(store)
    assert np.array_equal(hs.insert(d2), exp2)
    # everything known: all bytes deduplicated
    n_new, b_new, b_dup = ds.insert_device(dptr, n, sptr, flags.data_ptr())
    assert n_new == 0 and b_new == 0 and b_dup == int(sizes.sum()) and not flags.cpu().numpy().any()
    allk = np.frombuffer(b"".join(store), np.uint8).reshape(-1, 32)
    abuf, aptr = _dev_copy(torch, allk, 8)
    assert _probe_device(torch, ds, aptr, len(allk)).all() and hs.probe(allk).all()
    assert len(ds) == len(hs) == len(store)


# ---- content_hash_v1.dedup_* -----------------------------------------------------------------------------------------
def _hexes(rows, upper=()):
    return b"".join((r.tobytes().hex().upper() if i in upper else r.tobytes().hex()).encode() + b"\0"
                    for i, r in enumerate(rows))


def test_plugin_dedup_hex_case_bad_hex_independence_and_destroy(accel_lib):
    """content_hash_v1.dedup_*: upper- and lower-case hex of one digest are one entry; one bad hex string anywhere in a
    call is INVALID_ARG and inserts nothing; two sets are independent; every use after dedup_destroy is NOT_FOUND."""
    L = accel_lib
    assert L.yams_plugin_init(b"{}", None) == 0
    p = C.c_void_p()
    assert L.yams_plugin_get_interface(b"content_hash_v1", 1, C.byref(p)) == 0
    vt = C.cast(p, C.POINTER(_lib.ContentHashV1)).contents
    rng = np.random.default_rng(14)

    def call(fn, sid, hx, n):
        out = np.full(n, 0xAA, np.uint8)
        return fn(None, sid, hx, n, out.ctypes.data_as(_lib.u8p)), out

    def size(sid):
        v = C.c_uint64(0)
        assert vt.dedup_size(None, sid, C.byref(v)) == 0
        return v.value

    a, b = C.c_uint64(0), C.c_uint64(0)
    assert vt.dedup_create(None, 0, C.byref(a)) == 0 and vt.dedup_create(None, 0, C.byref(b)) == 0
    a, b = a.value, b.value
    assert a != b
    d = np.concatenate([adjacent_homes(TAG, 90, 2, 6, 0), rng.integers(0, 256, (4, 32), dtype=np.uint8)])
    rows = np.concatenate([d, d])
    st, out = call(vt.dedup_insert, a, _hexes(rows, upper=set(range(1, 20, 2))), 20)  # each digest once lower, once upper
    assert st == 0 and np.array_equal(out, np.r_[np.ones(10), np.zeros(10)].astype(np.uint8)) and size(a) == 10
    st, out = call(vt.dedup_contains, a, _hexes(d, upper=set(range(10))), 10)
    assert st == 0 and out.all()
    # one bad string anywhere: INVALID_ARG, nothing inserted
    fresh = rng.integers(0, 256, (5, 32), dtype=np.uint8)
    good = _hexes(fresh)
    for pos in (0, 2, 4):
        for kind in ("g", "short", "no_nul"):
            hx = bytearray(good)
            if kind == "g":
                hx[65 * pos + 17] = ord("g")
            elif kind == "short":
                hx[65 * pos + 63] = 0
            else:
                hx[65 * pos + 64] = ord("0")
            for fn in (vt.dedup_insert, vt.dedup_contains):
                st, _ = call(fn, a, bytes(hx), 5)
                assert st == _lib.YAMS_ERR_INVALID_ARG, (pos, kind)
    assert size(a) == 10
    st, out = call(vt.dedup_contains, a, good, 5)
    assert st == 0 and not out.any()
    # independence
    st, out = call(vt.dedup_contains, b, _hexes(d), 10)
    assert st == 0 and not out.any() and size(b) == 0
    st, out = call(vt.dedup_insert, b, _hexes(fresh, upper={1}), 5)
    assert st == 0 and out.all() and size(b) == 5 and size(a) == 10
    st, out = call(vt.dedup_contains, a, good, 5)
    assert st == 0 and not out.any()
    # destroy
    assert vt.dedup_destroy(None, a) == 0
    assert call(vt.dedup_insert, a, _hexes(d), 10)[0] == _lib.YAMS_ERR_NOT_FOUND
    assert call(vt.dedup_contains, a, _hexes(d), 10)[0] == _lib.YAMS_ERR_NOT_FOUND
    assert call(vt.dedup_insert, a, None, 0)[0] == _lib.YAMS_ERR_NOT_FOUND
    v = C.c_uint64(0)
    assert vt.dedup_size(None, a, C.byref(v)) == _lib.YAMS_ERR_NOT_FOUND
    assert vt.dedup_destroy(None, a) == _lib.YAMS_ERR_NOT_FOUND
    st, out = call(vt.dedup_contains, b, good, 5)
    assert st == 0 and out.all() and size(b) == 5
    assert vt.dedup_destroy(None, b) == 0
    L.yams_plugin_shutdown()


# ---- yams_verify_chunks_device ----------------------------------------------------------------------------------------
VERIFY_LENGTHS = [0, 1, 55, 56, 63, 64, 65, 119, 120, 4095, 4096, 65537]


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_verify_chunks_device_edges(acc, n):
    """Message lengths around every SHA-256 padding edge, corruption of a chunk's first and last byte and of one byte in
    each of the 8 words of the expected digest, expected digests at an odd address; out_valid against hashlib and
    out_n_invalid equal to the number of zeros in out_valid."""
    import torch
    rng = np.random.default_rng(200 + n)
    lens = np.array([VERIFY_LENGTHS[(5 * i + n) % len(VERIFY_LENGTHS)] for i in range(n)], np.uint64)
    gaps = rng.integers(0, 9, n).astype(np.uint64)
    offs = np.uint64(3) + np.concatenate([np.zeros(1, np.uint64), np.cumsum(lens + gaps)[:-1]])
    data = rng.integers(0, 256, int(offs[-1] + lens[-1]) + 16, dtype=np.uint8)
    expected = np.stack([np.frombuffer(hashlib.sha256(data[int(o):int(o + l)].tobytes()).digest(), np.uint8)
                         for o, l in zip(offs, lens)])
    for i in range(n):                               # kind 0: intact; 1 / 2: data first / last byte; 3..10: digest word
        kind, o, l = (i + n) % 11, int(offs[i]), int(lens[i])
        if kind == 1 and l:
            data[o] ^= 0x01
        elif kind == 2 and l:
            data[o + l - 1] ^= 0x80
        elif kind >= 3:
            expected[i, 4 * (kind - 3) + i % 4] ^= 0x20
    exp_valid = np.array([hashlib.sha256(data[int(o):int(o + l)].tobytes()).digest() == expected[i].tobytes()
                          for i, (o, l) in enumerate(zip(offs, lens))])
    assert (~exp_valid).any()
    td, tptr = _dev_copy(torch, data)
    to, optr = _dev_copy(torch, offs)
    tl, lptr = _dev_copy(torch, lens)
    te, eptr = _dev_copy(torch, expected, 1)                                    # any alignment
    valid = torch.full((n,), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    bad = acc.verify_chunks_device(tptr, optr, lptr, n, eptr, valid.data_ptr())
    v = valid.cpu().numpy()
    assert np.array_equal(v, exp_valid.astype(np.uint8)), np.flatnonzero(v != exp_valid)[:20]
    assert bad == int((v == 0).sum()) == int((~exp_valid).sum())


STRESS_CASES, STRESS_TIMEOUT = 400, 60


def test_randomised_dedup_stress_against_the_oracle():
    """tests/stress_dedup.py: sequences of calls on one set mixing random digests, repeats, adjacent-home same-tag
    families, wrap-around and tag-0/1 families, chains deeper than 66, growth and the device entry point with chunk
    sizes; every call checked against walk(), probe of everything, near misses and len()."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "stress_dedup.py"), "--cases", str(STRESS_CASES),
                        "--seed", "7"], capture_output=True, text=True, timeout=STRESS_TIMEOUT)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and line, r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads(line[-1])
    assert res["cases"] == STRESS_CASES and res["calls"] >= 3 * STRESS_CASES and res["mismatches"] == 0, res
    assert all(v > 0 for v in res["counters"].values()), res["counters"]

