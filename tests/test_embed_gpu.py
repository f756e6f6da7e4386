"""The embedding model's pooling head on the GPU (yams_embed_pool / _normalize, _device and _host, embedding_pool_v1, the shell
over the real plugin) against the C++ restatement (tests/cpp/embed_oracle.cpp) and the golden file made from the reference's own
loops.  Every output is compared on bits (eo.equal: a NaN matches any NaN); every device output is followed by guard bytes that
the wrapper checks; every refusal is made behind guard words that must come back untouched.

The lattice sits at the kernel's own edges, the constants of embed_launch.h restated here: a slab of at most 256 dimensions per
workgroup (64 lanes x one 16-byte load; 64 dimensions with scalar loads and for small batches), a window of 128 tokens whose
active indices are compacted at a time, 8 row loads ahead of the chain, 1024 floats of a row per step of the finish kernel.  The
references are computed once per shape and left unchanged."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import _embed_oracle as eo

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "embed_pool.json")
SLAB, MIN_SLAB, WINDOW, CUS = 256, 64, 128, 256
MAX_DIM, MAX_SEQ, MAX_ROWS = 8192, 1 << 16, 1 << 22
DIMS = [1, 3, 4, 5, 63, 64, 65, SLAB - 1, SLAB, SLAB + 1, 384, 768, 1024, 1025, MAX_DIM]
SEQS = [1, 2, WINDOW - 1, WINDOW, WINDOW + 1, 2 * WINDOW + 1]
BATCHES = [1, 2, 3, 257]
MODES = [eo.CLS, eo.MAX, eo.MEAN]
_CACHE = {}


def golden():
    return json.load(open(GOLDEN))["cases"]


def slab_of(batch, dim, vec4=True):
    """embed_slab_dims restated: the widest of 256 / 128 / 64 that still gives every compute unit two workgroups."""
    if not vec4 or dim % 4:
        return MIN_SLAB
    for slab in (256, 128):
        if batch * -(-dim // slab) >= 2 * CUS:
            return slab
    return MIN_SLAB


def drawn(batch, seq, dim, mask_len, seed=0, keep=0.7):
    """(hidden, mask, {(mode, normalize): (out, counts)}) — drawn and restated once."""
    key = (batch, seq, dim, mask_len, seed, keep)
    if key not in _CACHE:
        rng = np.random.default_rng(7000 + 131 * dim + 17 * seq + 5 * batch + mask_len + seed)
        x = eo.mixed(rng, (batch, seq, dim), -3, 3)
        m = (rng.random((batch, mask_len)) < keep).astype(np.int32)
        _CACHE[key] = (x, m, {(mode, nz): eo.pool_cpp(x, m, mode, nz, want_counts=True) for mode in MODES for nz in (False, True)})
    return _CACHE[key]


def check(acc, x, m, mode, normalize, want, **kw):
    out, diag = acc.embed_pool(x, m, mode=mode, normalize=normalize, **kw)
    assert eo.equal(out, want[0]), (x.shape, None if m is None else m.shape, mode, normalize, kw)
    assert (diag["tokens_considered"], diag["active_tokens"]) == want[1], (diag, want[1])
    assert diag["mode"] == mode and diag["flags"] == int(normalize) and (diag["batch"], diag["seq"], diag["dim"]) == x.shape
    if not kw.get("host_entry"):
        assert diag["slab_dims"] == slab_of(x.shape[0], x.shape[2], not kw.get("misalign")), diag
    return diag


# ---- the golden file, through all four doors ---------------------------------------------------------------------------------
@pytest.mark.parametrize("host", [False, True])
def test_the_flat_entries_equal_the_golden_file(acc, host):
    cases = golden()
    got = eo.restated(lambda x, m, mode, nz: acc.embed_pool(x, m, mode=mode, normalize=nz, host_entry=host)[0],
                      lambda r: acc.embed_normalize(r, host_entry=host))
    want = [c["out"] for c in cases]
    assert eo.nan_blind(got) == eo.nan_blind(want), [c["name"] for c, g, w in zip(cases, eo.nan_blind(got), eo.nan_blind(want)) if g != w]


@pytest.fixture(scope="module")
def vtable():
    from yams_amd import _lib
    L = _lib.load()
    assert L.yams_plugin_init(b'{"device":0}', None) == 0
    p = C.c_void_p()
    assert L.yams_plugin_get_interface(b"embedding_pool_v1", 1, C.byref(p)) == 0
    yield C.cast(p, C.POINTER(_lib.EmbeddingPoolV1)).contents
    L.yams_plugin_shutdown()


def test_the_plugin_interface_equals_the_golden_file(vtable):
    """pool and normalize over host memory; pool_device and normalize_device over hidden states that live on the device, with
    the masks and the outputs in host memory."""
    import torch
    from yams_amd import _lib
    assert vtable.abi_version == 1
    p = lambda a: a.ctypes.data if a is not None and a.size else None      # noqa: E731

    def pool(device):
        def go(x, m, mode, nz):
            x = np.ascontiguousarray(x, np.float32)
            m = None if m is None else np.ascontiguousarray(m, np.int32)
            out, dg = np.full((x.shape[0], x.shape[2]), 7.0, np.float32), _lib.EmbedDiag()
            args = (x.shape[0], x.shape[1], x.shape[2], p(m), 0 if m is None else m.shape[1], mode, int(nz), p(out), C.byref(dg))
            if device:
                t = torch.from_numpy(x).cuda()
                assert vtable.pool_device(None, t.data_ptr(), *args) == 0
            else:
                assert vtable.pool(None, p(x), *args) == 0
            assert dg.mode == mode and dg.batch == x.shape[0] and (dg.tokens_considered, dg.active_tokens) == eo.counts_py(x, m, mode)
            return out
        return go

    def normalize(device):
        def go(r):
            r = np.ascontiguousarray(r, np.float32)
            out = np.full(r.shape, 7.0, np.float32)
            if device:
                t = torch.from_numpy(r).cuda()
                assert vtable.normalize_device(None, t.data_ptr(), r.shape[0], r.shape[1], p(out)) == 0
            else:
                assert vtable.normalize(None, p(r), r.shape[0], r.shape[1], p(out)) == 0
            return out
        return go

    want = eo.nan_blind([c["out"] for c in golden()])
    for device in (False, True):
        assert eo.nan_blind(eo.restated(pool(device), normalize(device))) == want, device
    # a refusal comes back as its status, the outputs untouched
    x, m, out = np.ones((1, 2, 4), np.float32), np.array([[1, 2]], np.int32), np.full(4, 7.0, np.float32)
    t = torch.from_numpy(x).cuda()
    for fn, hidden in ((vtable.pool, p(x)), (vtable.pool_device, t.data_ptr())):
        assert fn(None, hidden, 1, 2, 4, p(m), 2, eo.MEAN, 1, p(out), None) == _lib.YAMS_ERR_UNSUPPORTED and (out == 7.0).all()      # a weight of 2
        assert fn(None, hidden, 1, 2, 4, p(m), 2, 3, 1, p(out), None) == _lib.YAMS_ERR_INVALID_ARG and (out == 7.0).all()             # an unknown mode
        assert fn(None, hidden, 1, 2, MAX_DIM + 1, p(m), 2, eo.MAX, 1, p(out), None) == _lib.YAMS_ERR_UNSUPPORTED and (out == 7.0).all()
        assert fn(None, hidden, 1, 2, 4, p(m), 2, eo.MAX, 1, p(out), None) == 0 and (out != 7.0).all()                                  # MAX serves it
        out[:] = 7.0


def test_shell_through_the_real_plugin_equals_the_golden_file():
    """include/yams_accel/embedding_pool.hpp over the real embedding_pool_v1: every case reaches the device (the driver counts
    the calls its host loop served), the bits are the reference's."""
    from _embed_build import build_shell_test
    from yams_amd import _lib
    exe = build_shell_test()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "cases.bin")
        eo.write_cases(path)
        r = subprocess.run([exe, "--plugin", _lib.LIB_PATH, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    info, got = eo.parse_driver_output(r.stdout)
    assert info == {"device_calls": len(golden()), "host_calls": 0}, info
    assert eo.nan_blind(got) == eo.nan_blind([c["out"] for c in golden()])


# ---- the lattice -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
def test_every_dimension(acc, dim):
    """Three texts of a window plus one token, every mode, normalised or not; the scalar-load path behind a base pointer offset
    by one float; the host entry."""
    x, m, want = drawn(3, WINDOW + 1, dim, WINDOW + 1)
    for mode in MODES:
        for nz in (False, True):
            check(acc, x, m, mode, nz, want[(mode, nz)])
        check(acc, x, m, mode, True, want[(mode, True)], misalign=4)
    check(acc, x, m, eo.MEAN, True, want[(eo.MEAN, True)], host_entry=True)
    check(acc, x, m, eo.CLS, False, want[(eo.CLS, False)], host_entry=True)


@pytest.mark.parametrize("seq", SEQS)
def test_every_sequence_length(acc, seq):
    for dim in (5, 64):
        for mask_len in sorted({0, seq - 1, seq, seq + 1}):
            x, m, want = drawn(2, seq, dim, mask_len, keep=0.8)
            for mode in MODES:
                check(acc, x, m, mode, True, want[(mode, True)])
            check(acc, x, m, eo.MEAN, False, want[(eo.MEAN, False)], host_entry=True)
            check(acc, x, m, eo.MAX, False, want[(eo.MAX, False)], misalign=4)
            if mask_len == 0:
                assert not eo.bits(want[(eo.MEAN, True)][0]).any() and want[(eo.MEAN, True)][1] == (0, 0)
                out, diag = acc.embed_pool(x, None, mode=eo.MAX, normalize=False)      # a null mask
                assert not eo.bits(out).any() and diag["tokens_considered"] == 0


@pytest.mark.parametrize("batch", BATCHES)
def test_every_batch(acc, batch):
    """Small batches are cut into narrow slabs so that they still cover the device; 257 texts take the widest that keeps two
    workgroups per compute unit.  The diag names the choice."""
    slabs = set()
    for dim in (768, 256, 260, 128):
        x, m, want = drawn(batch, 9, dim, 9)
        for mode in (eo.MEAN, eo.MAX):
            slabs.add(check(acc, x, m, mode, True, want[(mode, True)])["slab_dims"])
        check(acc, x, m, eo.MEAN, True, want[(eo.MEAN, True)], host_entry=True)
    assert slabs == ({64, 128, 256} if batch == 257 else {64}), slabs


# ---- masks -------------------------------------------------------------------------------------------------------------------
def test_mask_shapes(acc):
    seq, dim, batch = 2 * WINDOW + 1, 20, 9
    rng = np.random.default_rng(11)
    x = eo.mixed(rng, (batch, seq, dim), -3, 3)
    m = np.ones((batch, seq), np.int32)
    m[0] = 0                                      # all zero
    m[2, :-1] = 0                                 # only the last token
    m[3, 0] = 0                                   # only the first masked
    m[4, ::2] = 0                                 # alternating
    m[5] = -np.arange(seq) % 3 - 1                # negative values and zeros among ones: -1, 1, 0, -1, ...
    m[6, WINDOW - 3:WINDOW + 5] = 0               # a zero run straddling a window edge
    m[7, :WINDOW] = 0                             # a whole window masked
    m[8, WINDOW:2 * WINDOW] = 0
    assert (m[5] == 1).any() and (m[5] < 0).any()
    for mode in MODES:
        for nz in (False, True):
            want = eo.pool_cpp(x, m, mode, nz, want_counts=True)
            assert mode == eo.CLS or want[1] == (batch * seq, int((m > 0).sum()))
            check(acc, x, m, mode, nz, want)
    assert not eo.bits(eo.pool_cpp(x, m, eo.MEAN, False)[0]).any()
    # MAX treats any positive value as active
    m7 = m * 7
    want = eo.pool_cpp(x, m7, eo.MAX, True, want_counts=True)
    assert eo.equal(want[0], eo.pool_cpp(x, (m > 0).astype(np.int32), eo.MAX, True))
    check(acc, x, m7, eo.MAX, True, want)
    check(acc, x, m7, eo.MAX, True, want, host_entry=True)


# ---- values ------------------------------------------------------------------------------------------------------------------
def test_cancellation_rows_at_every_position(acc):
    """1e8, 1 and -1e8 at every ordered choice of three positions of a five-token text: the sum is 1-ish or 0-ish depending on
    the order alone, so a lost, repeated or reordered token changes bits."""
    import itertools
    places = list(itertools.permutations(range(5), 3))
    x = np.full((len(places), 5, 4), 0.25, np.float32)
    for b, (i, j, k) in enumerate(places):
        x[b, i], x[b, j], x[b, k] = 1e8, 1.0, -1e8
    x *= np.array([1, 3, -1, 0.5], np.float32)
    m = np.ones((len(places), 5), np.int32)
    want = eo.pool_cpp(x, m, eo.MEAN, False, want_counts=True)
    assert len({eo.hexbits(r) for r in want[0]}) >= 3      # the orders give different sums
    assert not eo.equal(want[0], eo.pool_cpp(x, m, eo.MEAN, False, order=np.arange(4, -1, -1)))
    for kw in (dict(), dict(misalign=4), dict(host_entry=True)):
        check(acc, x, m, eo.MEAN, False, want, **kw)
    check(acc, x, m, eo.MEAN, True, eo.pool_cpp(x, m, eo.MEAN, True, want_counts=True))


def test_special_values_in_active_and_masked_rows(acc):
    rng = np.random.default_rng(77)
    batch, seq, dim = 6, WINDOW + 9, 65
    x = eo.mixed(rng, (batch, seq, dim), -3, 3)
    m = (rng.random((batch, seq)) < 0.6).astype(np.int32)
    specials = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-42, -1e-42, np.finfo(np.float32).max / 4], np.float32)
    flat = x.reshape(-1)
    k = flat.size // 50
    flat[rng.integers(0, flat.size, k)] = rng.choice(specials, k)
    clean = x[5].copy()
    x[5][m[5] <= 0] = rng.choice(specials[2:5], ((m[5] <= 0).sum(), dim))      # masked rows full of NaN and infinities
    x[5][m[5] > 0] = np.where(np.isfinite(clean[m[5] > 0]), clean[m[5] > 0], np.float32(1.0))
    for mode in MODES:
        for nz in (False, True):
            want = eo.pool_cpp(x, m, mode, nz, want_counts=True)
            if mode != eo.CLS:
                assert np.isfinite(want[0][5]).all()      # nothing of a masked row reached text 5
                assert not np.isfinite(want[0][:5]).all() or nz
            check(acc, x, m, mode, nz, want)
            check(acc, x, m, mode, nz, want, misalign=4)
    # subnormals are kept: sums and means below 2^-126; signed zeros; FLT_MAX / 4 through MAX and the normalisation
    x = eo.mixed(rng, (2, 7, 8), -140, -130)
    x[1, :, :4] = -0.0
    x[1, :, 4:] = np.float32(np.finfo(np.float32).max / 4) * np.array([1, -1, 0.5, 1], np.float32)
    m = np.ones((2, 7), np.int32)
    for mode in MODES:
        for nz in (False, True):
            want = eo.pool_cpp(x, m, mode, nz, want_counts=True)
            check(acc, x, m, mode, nz, want)
            check(acc, x, m, mode, nz, want, host_entry=True)
    sub = eo.pool_cpp(x, m, eo.MEAN, False)[0]
    assert sub.all() and (np.abs(sub) < 1.2e-38).all()
    assert np.isfinite(eo.pool_cpp(x, m, eo.MAX, True)[1]).all()


def test_the_norm_threshold(acc):
    rows = np.array([[3e-9, -4e-9, 0], [6e-9, 8e-9, 1e-12], [1e-8, 2e-9, 0], [0, 0, 0], [1e-30, 1e-25, -1], [1e-42, 1e-40, 0]], np.float32)
    want = eo.normalize_cpp(rows)
    assert not want[0].any() and want[2][0] > 0.9 and not want[3].any() and want[4][2] == -1.0 and not want[5].any()
    for kw in (dict(), dict(host_entry=True), dict(misalign=4)):
        assert eo.equal(acc.embed_normalize(rows, **kw), want), kw
    x = rows.reshape(6, 1, 3)
    for mode in MODES:
        check(acc, x, np.ones((6, 1), np.int32), mode, True, eo.pool_cpp(x, np.ones((6, 1), np.int32), mode, True, want_counts=True))


# ---- normalize alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
def test_normalize_at_every_dimension(acc, dim):
    rng = np.random.default_rng(dim)
    rows = eo.mixed(rng, (5, dim), -6, 6)
    rows[1] = 0.0
    rows[2, dim // 2] = np.nan
    rows[3] *= np.float32(1e-12)
    want = eo.normalize_cpp(rows)
    assert not want[1].any() and not want[2].any()
    for kw in (dict(), dict(misalign=4), dict(host_entry=True)):
        assert eo.equal(acc.embed_normalize(rows, **kw), want), (dim, kw)


def test_normalize_of_257_rows(acc):
    rng = np.random.default_rng(257)
    rows = eo.mixed(rng, (257, 1025), -6, 6)
    assert eo.equal(acc.embed_normalize(rows), eo.normalize_cpp(rows))


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def refused(acc, host, status, x, m, batch, seq, dim, mask_len, mode=eo.MEAN, flags=1, out=True, out_is=None):
    """The call with its output behind guard words (the wrapper's _artifact_call asserts that a refusal left them as they were);
    arrays may be None: a null pointer.  out_is: the input whose address is passed as the output."""
    from yams_amd import _lib
    dg = _lib.EmbedDiag(mode=77)
    with pytest.raises(_lib.AccelError) as e:
        acc._artifact_call(acc.L.yams_embed_pool_device, acc.L.yams_embed_pool_host, host, [x, m], [(np.float32, 64) if out or out_is is not None else None],
                           lambda i, o: (i[0], batch, seq, dim, i[1], mask_len, mode, flags, o[0] if out_is is None else i[out_is], C.byref(dg)))
    assert e.value.status == status, (e.value, status)
    assert dg.mode == 77      # the diag is an output too


@pytest.mark.parametrize("host", [False, True])
def test_refusals_leave_every_output_untouched(acc, host):
    from yams_amd import _lib
    inv, uns = _lib.YAMS_ERR_INVALID_ARG, _lib.YAMS_ERR_UNSUPPORTED
    x, m = np.ones((2, 3, 4), np.float32), np.ones((2, 3), np.int32)
    refused(acc, host, inv, x, m, 2, 3, 0, 3)                            # dim == 0
    refused(acc, host, inv, x, m, 2, 0, 4, 3)                            # seq == 0
    refused(acc, host, inv, x, m, 2, 3, 4, 3, mode=3)                    # an unknown mode
    refused(acc, host, inv, x, m, 2, 3, 4, 3, flags=2)                   # an unknown flag bit
    refused(acc, host, inv, x, m, 2, 3, 4, 3, flags=3)
    refused(acc, host, inv, None, m, 2, 3, 4, 3)                         # null hidden
    refused(acc, host, inv, x, m, 2, 3, 4, 3, out=False)                 # null out
    refused(acc, host, inv, x, None, 2, 3, 4, 3)                         # null mask, MEAN
    refused(acc, host, inv, x, None, 2, 3, 4, 3, mode=eo.MAX)            # null mask, MAX
    refused(acc, host, inv, x, m, 2, 3, 4, 3, out_is=0)                  # out overlaps hidden
    refused(acc, host, inv, x, m, 1, 1, 1, 3, mode=eo.MAX, out_is=1)     # out overlaps mask
    # the limits, each one past its boundary; nothing of that size is allocated: the refusal precedes every read
    refused(acc, host, uns, x, m, 2, 3, MAX_DIM + 1, 3)
    refused(acc, host, uns, x, m, 2, MAX_SEQ + 1, 4, 3)
    refused(acc, host, uns, x, m, MAX_ROWS + 1, 1, 4, 3)
    refused(acc, host, uns, x, m, MAX_ROWS // MAX_SEQ + 1, MAX_SEQ, 4, 3)
    refused(acc, host, uns, x, m, 2, MAX_ROWS // 2 + 1, 4, 3)            # (seq is past its own limit too)
    # MEAN with a weight of 2 at the last considered position: refused; one position past min(seq, mask_len): served
    for seq, mask_len in ((5, 7), (7, 5), (5, 5)):
        x = eo.mixed(np.random.default_rng(seq), (3, seq, 6))
        m = np.ones((3, mask_len), np.int32)
        m[2, min(seq, mask_len) - 1] = 2
        refused(acc, host, uns, x, m, 3, seq, 6, mask_len)
        check(acc, x, m, eo.MAX, True, eo.pool_cpp(x, m, eo.MAX, True, want_counts=True), host_entry=host)      # MAX serves the same mask
        check(acc, x, m, eo.CLS, True, eo.pool_cpp(x, m, eo.CLS, True, want_counts=True), host_entry=host)
        m[2, min(seq, mask_len) - 1] = 1
        if mask_len > seq:
            m[2, seq] = 2
        check(acc, x, m, eo.MEAN, True, eo.pool_cpp(x, m, eo.MEAN, True, want_counts=True), host_entry=host)
    # CLS needs no mask; a null mask with mask_len == 0 is served
    x = eo.mixed(np.random.default_rng(1), (2, 3, 4))
    check(acc, x, None, eo.CLS, True, eo.pool_cpp(x, None, eo.CLS, True, want_counts=True), host_entry=host)
    check(acc, x, None, eo.MEAN, True, eo.pool_cpp(x, None, eo.MEAN, True, want_counts=True), host_entry=host)
    # batch == 0 is YAMS_OK and writes nothing
    out, = acc._artifact_call(acc.L.yams_embed_pool_device, acc.L.yams_embed_pool_host, host, [x, np.ones((2, 3), np.int32)], [(np.uint8, 16)],
                              lambda i, o: (i[0], 0, 3, 4, i[1], 3, eo.MEAN, 1, o[0], None))
    assert (out == acc._GUARD).all()
    # normalize
    rows = np.ones((2, 4), np.float32)
    for args, status in (((2, 0), inv), ((2, MAX_DIM + 1), uns), ((MAX_ROWS + 1, 4), uns)):
        with pytest.raises(_lib.AccelError) as e:
            acc._artifact_call(acc.L.yams_embed_normalize_device, acc.L.yams_embed_normalize_host, host, [rows], [(np.float32, 64)],
                               lambda i, o: (i[0], args[0], args[1], o[0]))
        assert e.value.status == status
    for build in (lambda i, o: (None, 2, 4, o[0]), lambda i, o: (i[0], 2, 4, None), lambda i, o: (i[0], 2, 4, i[0])):      # nulls, an overlap
        with pytest.raises(_lib.AccelError) as e:
            acc._artifact_call(acc.L.yams_embed_normalize_device, acc.L.yams_embed_normalize_host, host, [rows], [(np.float32, 64)], build)
        assert e.value.status == inv
    out, = acc._artifact_call(acc.L.yams_embed_normalize_device, acc.L.yams_embed_normalize_host, host, [rows], [(np.uint8, 16)],
                              lambda i, o: (i[0], 0, 4, o[0]))
    assert (out == acc._GUARD).all()


def test_the_limits_themselves_are_served(acc):
    """dim, seq and batch * seq AT their limits (the lattice holds dim = YAMS_EMBED_MAX_DIM): one text of 65536 tokens, and 64 of
    them — 2^22 rows of one dimension."""
    for batch in (1, MAX_ROWS // MAX_SEQ):
        rng = np.random.default_rng(batch)
        x = eo.mixed(rng, (batch, MAX_SEQ, 1), -3, 3)
        m = (rng.random((batch, MAX_SEQ)) < 0.9).astype(np.int32)
        check(acc, x, m, eo.MEAN, False, eo.pool_cpp(x, m, eo.MEAN, False, want_counts=True))
    check(acc, x, m, eo.MAX, True, eo.pool_cpp(x, m, eo.MAX, True, want_counts=True), host_entry=True)


def test_normalize_at_its_row_limit(acc):
    """yams_embed_normalize of exactly YAMS_EMBED_MAX_ROWS rows (one dimension): the largest grid of the finish kernel."""
    rng = np.random.default_rng(22)
    rows = eo.mixed(rng, (MAX_ROWS, 1), -3, 3)
    rows[::1000] = np.float32(1e-9)      # below the threshold: zeros
    want = eo.normalize_cpp(rows)
    assert set(np.unique(want).tolist()) == {-1.0, 0.0, 1.0}
    assert eo.equal(acc.embed_normalize(rows), want)


@pytest.mark.parametrize("dim", [4, 768])
def test_an_output_that_is_float_aligned_only(acc, dim):
    """The 16-byte loads' predicate covers the OUTPUT base too: hidden states on a 16-byte boundary and an output one float past
    one take the scalar path (the diag's slab says so); the float in front of the output and the guard bytes behind it stay."""
    x, m, want = drawn(3, 9, dim, 9)
    n = 3 * dim
    for mode in MODES:
        for nz in (False, True):
            from yams_amd import _lib
            dg = _lib.EmbedDiag()
            out, = acc._artifact_call(acc.L.yams_embed_pool_device, acc.L.yams_embed_pool_host, False, [x, m], [(np.float32, n + 1)],
                                      lambda i, o: (i[0], 3, 9, dim, i[1], 9, mode, int(nz), o[0] + 4, C.byref(dg)))
            assert (out[:1].view(np.uint8) == acc._GUARD).all(), "the float in front of the output was written"
            assert eo.equal(out[1:].reshape(3, dim), want[(mode, nz)][0]), (dim, mode, nz)
            assert dg.slab_dims == MIN_SLAB
    rows = x[:, 0, :]
    out, = acc._artifact_call(acc.L.yams_embed_normalize_device, acc.L.yams_embed_normalize_host, False, [rows], [(np.float32, n + 1)],
                              lambda i, o: (i[0], 3, dim, o[0] + 4))
    assert (out[:1].view(np.uint8) == acc._GUARD).all() and eo.equal(out[1:].reshape(3, dim), eo.normalize_cpp(rows))


# ---- the stress --------------------------------------------------------------------------------------------------------------
def test_stress_harness():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "stress_embed.py"), "--cases", "120"], capture_output=True, text=True,
                       timeout=280)
    assert r.returncode == 0 and "120 cases, 0 failures OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
