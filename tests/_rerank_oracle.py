"""The late-interaction rerank restated in numpy (ColBERT MaxSim over a window of documents; max-pool + L2 normalisation),
from the contract in include/yams_mi355x_accel.h, plus the ctypes door to the C++ restatement (tests/cpp/rerank_oracle.cpp),
the golden cases and the stress-case generator.

Forms: SEPARATE rounds a[i] * b[i] to fp32 and then the sum; FUSED is fmaf.  numpy has no fmaf: the product of two floats is
exact in fp64, the fp64 sum is made ROUND-TO-ODD (TwoSum gives the error; an inexact even result moves to its odd neighbour),
and fp64 -> fp32 of a round-to-odd value with 29 spare bits is the correctly rounded fmaf."""
import ctypes as C
import hashlib
import struct

import numpy as np

SEPARATE, FUSED = 0, 1
FORMS = {"separate": SEPARATE, "fused": FUSED}
NONE = 0xFFFFFFFF
_LIB = None


# ---- helpers -------------------------------------------------------------------------------------------------------------------
def mixed(rng, shape, lo=-4, hi=4):
    """Floats of mixed exponents 2^lo .. 2^hi and both signs, full mantissas."""
    m = rng.uniform(1.0, 2.0, shape) * np.exp2(rng.integers(lo, hi + 1, shape)) * rng.choice([-1.0, 1.0], shape)
    return m.astype(np.float32)


def csr(lengths):
    off = np.zeros(len(lengths) + 1, np.uint64)
    off[1:] = np.cumsum(np.asarray(lengths, np.uint64))
    return off


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool((bits(a) == bits(b)).all())


def equal(a, b):
    """Bit for bit; a NaN matches any NaN (x86 and the device give the default NaN different signs)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    same = bits(a) == bits(b)
    if a.dtype.kind == "f":
        same = same | (np.isnan(a) & np.isnan(b))
    return bool(same.all())


def hexbits(a):
    return np.ascontiguousarray(a).tobytes().hex()


def from_hex(h, dtype=np.float32):
    return np.frombuffer(bytes.fromhex(h), dtype)


# ---- numpy restatement ---------------------------------------------------------------------------------------------------------
def fmaf(a, b, c):
    """round32(a * b + c), elementwise."""
    with np.errstate(all="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)      # exact
        c = np.broadcast_to(c.astype(np.float64), p.shape)
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)                      # TwoSum: s + err == p + c exactly
        inexact = np.isfinite(s) & (err != 0)
        even = (s.view(np.int64) & 1) == 0
        toward = np.where(err > 0, np.inf, -np.inf)
        s = np.where(inexact & even, np.nextafter(s, toward), s)
        return s.astype(np.float32)


def sims_py(query, rows, form, order=None):
    """[tq][n] chains, i in `order` (ascending by default)."""
    q, x = np.ascontiguousarray(query, np.float32), np.ascontiguousarray(rows, np.float32)
    dim = q.shape[1]
    s = np.zeros((q.shape[0], x.shape[0]), np.float32)
    with np.errstate(all="ignore"):
        for i in (range(dim) if order is None else order):
            a, b = q[:, i][:, None], x[:, i][None, :]
            s = fmaf(a, b, s) if form == FUSED else (s + (a * b).astype(np.float32)).astype(np.float32)
    return s


def maxsim_py(query, rows, off, form, order=None):
    """Returns (scores [n_docs], rowmax [n_docs][tq], rowarg [n_docs][tq])."""
    q = np.ascontiguousarray(query, np.float32)
    tq, n_docs = q.shape[0], len(off) - 1
    s = sims_py(q, rows, form, order)
    scores = np.zeros(n_docs, np.float32)
    rowmax = np.full((n_docs, tq), -np.inf, np.float32)
    rowarg = np.full((n_docs, tq), NONE, np.uint32)
    with np.errstate(all="ignore"):
        for d in range(n_docs):
            lo, hi = int(off[d]), int(off[d + 1])
            if hi > lo and tq:
                sd = s[:, lo:hi]
                cmp = np.where(np.isnan(sd), -np.inf, sd)
                m = cmp.max(axis=1)
                first = (cmp == m[:, None]).argmax(axis=1)      # equal values (zeros of both signs): the first stays
                won = m > -np.inf
                rowmax[d] = np.where(won, sd[np.arange(tq), first], np.float32(-np.inf))
                rowarg[d] = np.where(won, first, NONE).astype(np.uint32)
            acc = np.float32(0.0)
            for v in rowmax[d]:
                acc = np.float32(acc + v)
            scores[d] = acc
    return scores, rowmax, rowarg


def maxpool_py(rows, off):
    x = np.ascontiguousarray(rows, np.float32)
    n_docs, dim = len(off) - 1, x.shape[1]
    out = np.zeros((n_docs, dim), np.float32)
    with np.errstate(all="ignore"):
        for d in range(n_docs):
            p = np.full(dim, -np.inf, np.float32)
            for r in range(int(off[d]), int(off[d + 1])):
                p = np.where(p < x[r], x[r], p)
            p = np.where(np.isfinite(p), p, np.float32(0.0)).astype(np.float32)
            norm = 0.0
            for v in p.astype(np.float64):
                norm = norm + v * v
            norm = np.sqrt(norm)
            out[d] = (p.astype(np.float64) / norm).astype(np.float32) if norm > 1e-8 else 0.0
    return out


# ---- the C++ restatement -------------------------------------------------------------------------------------------------------
def lib():
    global _LIB
    if _LIB is None:
        import _rerank_build
        _LIB = C.CDLL(_rerank_build.build_oracle())
        vp = C.c_void_p
        _LIB.rerank_oracle_maxsim.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp, C.c_uint64, C.c_uint32, vp, vp, vp]
        _LIB.rerank_oracle_maxsim.restype = None
        _LIB.rerank_oracle_maxpool.argtypes = [vp, C.c_uint32, vp, C.c_uint64, vp]
        _LIB.rerank_oracle_maxpool.restype = None
    return _LIB


def maxsim_cpp(query, rows, off, form):
    q, x, off = np.ascontiguousarray(query, np.float32), np.ascontiguousarray(rows, np.float32), np.ascontiguousarray(off, np.uint64)
    tq, dim, d = q.shape[0], q.shape[1], len(off) - 1
    sc, mx, arg = np.zeros(d, np.float32), np.zeros((d, tq), np.float32), np.zeros((d, tq), np.uint32)
    lib().rerank_oracle_maxsim(q.ctypes.data, tq, dim, x.ctypes.data, off.ctypes.data, d, form, sc.ctypes.data, mx.ctypes.data, arg.ctypes.data)
    return sc, mx, arg


def maxpool_cpp(rows, off):
    x, off = np.ascontiguousarray(rows, np.float32), np.ascontiguousarray(off, np.uint64)
    d, dim = len(off) - 1, x.shape[1]
    out = np.zeros((d, dim), np.float32)
    lib().rerank_oracle_maxpool(x.ctypes.data, dim, off.ctypes.data, d, out.ctypes.data)
    return out


# ---- the golden cases ----------------------------------------------------------------------------------------------------------
def _f(*v):
    return np.array(v, np.float32)


def _flip_case(seed):
    """One query token against one document token at dim 48, exponents mixed: the forms differ in most draws."""
    rng = np.random.default_rng(seed)
    return mixed(rng, (1, 48)), mixed(rng, (1, 48)), csr([1])


def maxsim_cases():
    """name -> (query [tq][dq], rows [n][dd], off).  dq and dd may differ: the shell takes the smaller."""
    inf, nan, sub = np.float32(np.inf), np.float32(np.nan), np.float32(1e-42)
    rng = np.random.default_rng(20)
    cases = {}
    for k in range(6):
        cases["flip_%d" % k] = _flip_case(100 + k)
    cases["window_mixed_lengths"] = (mixed(rng, (5, 48)), mixed(rng, (40, 48)), csr([7, 0, 1, 20, 12]))
    cases["empty_document"] = (mixed(rng, (3, 4)), np.zeros((0, 4), np.float32), csr([0]))
    cases["empty_query"] = (np.zeros((0, 4), np.float32), mixed(rng, (3, 4)), csr([3]))
    cases["nan_document_token"] = (_f([1, 2], [3, -1]), _f([nan, 1], [1, 1], [2, nan]), csr([3]))
    cases["nan_query_token"] = (_f([1, 2], [nan, 1], [0.5, 0.5]), _f([1, 1], [2, 3]), csr([2]))
    cases["inf_pair"] = (_f([1, 0], [-1, 0]), _f([inf, 1]), csr([1]))
    cases["subnormal_only"] = (_f([sub, sub]), _f([1, 1], [0.5, 2]), csr([2]))
    cases["signed_zeros"] = (_f([0.0, -0.0], [1, -1]), _f([1, 1], [-1, 1], [2, 2]), csr([3]))
    cases["min_dim_query_shorter"] = (mixed(rng, (4, 5)), mixed(rng, (9, 8)), csr([4, 5]))
    cases["min_dim_document_shorter"] = (mixed(rng, (4, 8)), mixed(rng, (9, 5)), csr([9]))
    return cases


def pool_cases():
    """name -> (rows [n][dim], off)."""
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    rng = np.random.default_rng(21)
    return {
        "pool_mixed": (mixed(rng, (30, 48)), csr([7, 0, 1, 22])),
        "pool_all_nan_dimension": (_f([nan, 1, -2], [nan, 3, -1]), csr([2])),
        "pool_nonfinite": (_f([inf, 1, -inf], [2, -inf, -inf]), csr([2])),
        "pool_tiny_norm": (_f([1e-9, -1e-9, 3e-9], [2e-9, 0, 0]), csr([2])),
        "pool_just_above": (_f([1e-8, 2e-9], [0, 0]), csr([2])),
        "pool_subnormal": (_f([1e-42, 1e-40]), csr([1])),
    }


def zero_tie_cases():
    """[(query, rows, off, {form: the bits of each document's row maximum})]: two documents whose two sims are zeros of both
    signs in the fused form (a negative product that underflows is -0.0f there; separate chains give +0.0f twice), in either
    order.  The first in document order stays: its sign, and token 0."""
    tiny = np.float32(1e-30)
    neg, pos = 0x80000000, 0
    out = []
    for dim in (1, 3):      # dim 3: the later steps add +-0.0f products that keep the sign
        q = np.zeros((1, dim), np.float32)
        q[0, 0] = tiny
        a, b = np.zeros(dim, np.float32), np.zeros(dim, np.float32)
        a[0], b[0] = -tiny, tiny
        if dim == 3:
            q[0, 1:] = 1.0
            a[1:] = -0.0      # 1 * -0.0f = -0.0f: -0.0f + -0.0f stays -0.0f
        rows = np.stack([a, b, b, a])
        out.append((q, rows, csr([2, 2]), {SEPARATE: [pos, pos], FUSED: [neg, pos]}))
    return out


def case_names():
    return list(maxsim_cases()) + list(pool_cases())


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def case_digest(name):
    c = maxsim_cases().get(name) or pool_cases()[name]
    return digest(c)


def write_cases(path):
    """The cases as the drivers read them: u32 count; per case u32 kind (0 maxsim, 1 pool); maxsim: u32 dq, tq, dd, n_docs, the
    query, then per document u32 len and its rows; pool: u32 dim, n_docs, then per document u32 len and its rows."""
    ms, pl = maxsim_cases(), pool_cases()
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(ms) + len(pl)))
        for q, x, off in ms.values():
            f.write(struct.pack("<IIIII", 0, q.shape[1], q.shape[0], x.shape[1], len(off) - 1))
            f.write(np.ascontiguousarray(q, np.float32).tobytes())
            for d in range(len(off) - 1):
                f.write(struct.pack("<I", int(off[d + 1] - off[d])))
                f.write(np.ascontiguousarray(x[int(off[d]):int(off[d + 1])], np.float32).tobytes())
        for x, off in pl.values():
            f.write(struct.pack("<III", 1, x.shape[1], len(off) - 1))
            for d in range(len(off) - 1):
                f.write(struct.pack("<I", int(off[d + 1] - off[d])))
                f.write(np.ascontiguousarray(x[int(off[d]):int(off[d + 1])], np.float32).tobytes())


def parse_driver_output(text):
    """('separate' | 'fused' | 'neither' | None, [hex of the case's output floats])."""
    probe, out = None, []
    for line in text.splitlines():
        w = line.split()
        if w[:1] == ["probe"]:
            probe = w[1]
        elif w[:1] == ["case"]:
            out.append(w[2] if len(w) > 2 else "")
    return probe, out


def restated(form, maxsim=None, maxpool=None):
    """The hex outputs of every case: the scores of a maxsim case (dim = min of the two sides), the rows of a pool case."""
    maxsim = maxsim or (lambda q, x, off, f: maxsim_py(q, x, off, f)[0])
    maxpool = maxpool or maxpool_py
    out = []
    for q, x, off in maxsim_cases().values():
        dim = min(q.shape[1], x.shape[1])
        out.append(hexbits(np.asarray(maxsim(np.ascontiguousarray(q[:, :dim]), np.ascontiguousarray(x[:, :dim]), off, form), np.float32)))
    for x, off in pool_cases().values():
        out.append(hexbits(np.asarray(maxpool(x, off), np.float32)))
    return out


def nan_blind(hexes):
    """The hex outputs with every NaN made one NaN."""
    out = []
    for h in hexes:
        v = from_hex(h).copy()
        v[np.isnan(v)] = np.float32(np.nan)
        out.append(hexbits(v))
    return out


# ---- stress cases --------------------------------------------------------------------------------------------------------------
S_DIMS = [3, 4, 47, 48, 49, 64, 127, 128]
S_TQ = [1, 31, 32, 33, 65]
S_LENS = [0, 1, 2, 31, 255, 256, 257, 513]


def _draw(seed, attempt):
    rng = np.random.default_rng([seed, attempt])
    dim, tq = int(rng.choice(S_DIMS)), int(rng.choice(S_TQ))
    n_docs = int(rng.choice([1, 2, 7, 40]))
    lengths = rng.choice(S_LENS[1:] if n_docs == 1 else S_LENS, n_docs)
    if n_docs > 7:
        lengths = np.minimum(lengths, 31)
    if not lengths.any():
        lengths[0] = 2
    off = csr(lengths)
    q = mixed(rng, (tq, dim), -3, 3)
    x = mixed(rng, (int(off[-1]), dim), -3, 3)
    # the last token of every document is the last query token, scaled: its sim with that query token is a sum of squares,
    # in most draws the largest of its row, so that dropping it changes the score
    for d in range(n_docs):
        if lengths[d]:
            x[int(off[d + 1]) - 1] = q[-1] * np.float32(4.0)
    return {"seed": seed, "query": q, "rows": x, "off": off, "form": int(rng.integers(0, 2)), "host": bool(rng.random() < 0.3),
            "misalign": 4 if rng.random() < 0.3 else 0}


def stress_case(seed):
    """A window whose score bits PROVABLY depend on the i order, on every document's last token and on the last query token: the
    draw is repeated (seed, attempt) until the oracle shows all three; c["other_form"] says whether the other form changes the
    bits too.  Exponents are mixed so that the sums round at every step."""
    for attempt in range(64):
        c = _draw(seed, attempt)
        r = discriminates(c)
        if all(r[:3]):
            c["other_form"] = bool(r[3])
            return c
    raise AssertionError("no discriminating draw for seed %d" % seed)


def discriminates(c):
    """(reversed i order changes the score bits, a dropped last document token does, a dropped last query token does, the other
    form does) — from the oracle alone."""
    q, x, off, form = c["query"], c["rows"], c["off"], c["form"]
    base = maxsim_cpp(q, x, off, form)[0]
    rev = maxsim_cpp(q[:, ::-1], x[:, ::-1], off, form)[0]
    lengths = np.diff(off.astype(np.int64))
    keep = np.ones(len(x), bool)
    keep[(off[1:][lengths > 0] - 1).astype(np.int64)] = False
    dropped = maxsim_cpp(q, x[keep], csr(np.maximum(lengths - 1, 0)), form)[0]
    noq = maxsim_cpp(q[:-1], x, off, form)[0]
    other = maxsim_cpp(q, x, off, 1 - form)[0]
    return (not same_bits(base, rev), not same_bits(base, dropped), not same_bits(base, noq), not same_bits(base, other))
