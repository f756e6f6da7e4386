"""The embedding model's pooling head restated in numpy (CLS, max or mean over the tokens of each text, then the L2
normalisation), from the contract in include/yams_mi355x_accel.h, plus the ctypes door to the C++ restatement
(tests/cpp/embed_oracle.cpp), the golden cases and the stress-case generator.

Every fp32 step is rounded on its own: numpy's float32 multiply, add and divide are the correctly rounded ones; the norm is a
Python-float (fp64) chain in element order."""
import ctypes as C
import hashlib
import struct

import numpy as np

from _rerank_oracle import bits, equal, from_hex, hexbits, mixed, nan_blind, same_bits  # noqa: F401  (one set of bit helpers)

CLS, MAX, MEAN = 0, 1, 2
MODES = {"cls": CLS, "max": MAX, "mean": MEAN}
WINDOW, SLAB, MIN_SLAB = 128, 256, 64      # embed_launch.h, restated
_LIB = None


# ---- numpy restatement ---------------------------------------------------------------------------------------------------------
def normalize_row_py(v):
    norm = 0.0
    for x in v.astype(np.float64).tolist():
        norm = norm + x * x
    norm = float(np.sqrt(np.float64(norm)))
    if norm > 1e-8:
        with np.errstate(all="ignore"):
            return (v.astype(np.float64) / norm).astype(np.float32)
    return np.zeros_like(v)


def _pairwise(terms):
    while len(terms) > 1:
        terms = [(terms[i] + terms[i + 1]).astype(np.float32) if i + 1 < len(terms) else terms[i] for i in range(0, len(terms), 2)]
    return terms[0]


def pool_py(hidden, mask, mode, normalize, order=None, pairwise=False, reciprocal=False):
    """out [batch][dim].  order: the token visiting order (ascending by default); pairwise: the MEAN terms summed as a tree;
    reciprocal: v * (1 / total) in place of v / total — the wrong forms the golden generator holds the reference against."""
    x = np.ascontiguousarray(hidden, np.float32)
    batch, seq, dim = x.shape
    m = None if mask is None else np.ascontiguousarray(mask, np.int32).reshape(batch, -1)
    t_len = 0 if m is None else min(seq, m.shape[1])
    out = np.zeros((batch, dim), np.float32)
    with np.errstate(all="ignore"):
        for b in range(batch):
            emb = np.zeros(dim, np.float32)
            if mode == CLS:
                emb = x[b, 0].copy()
            else:
                idx = [i for i in (range(seq) if order is None else order) if i < t_len and m[b, i] > 0]
                if mode == MAX:
                    for i in idx:
                        emb = np.where(emb < x[b, i], x[b, i], emb)
                else:
                    total = np.float32(0.0)
                    for i in idx:
                        total = np.float32(total + np.float32(m[b, i]))
                    if pairwise and idx:
                        emb = (emb + _pairwise([(x[b, i] * np.float32(m[b, i])).astype(np.float32) for i in idx])).astype(np.float32)
                    else:
                        for i in idx:
                            emb = (emb + (x[b, i] * np.float32(m[b, i])).astype(np.float32)).astype(np.float32)
                    if total > 0:
                        emb = (emb * (np.float32(1.0) / total)).astype(np.float32) if reciprocal else (emb / total).astype(np.float32)
            out[b] = normalize_row_py(emb) if normalize else emb
    return out


def normalize_py(rows):
    x = np.ascontiguousarray(rows, np.float32)
    return np.stack([normalize_row_py(r) for r in x]) if len(x) else x.copy()


def counts_py(hidden, mask, mode):
    """(tokens considered, active tokens): both 0 for CLS or without a mask."""
    if mask is None or mode == CLS:
        return 0, 0
    m = np.ascontiguousarray(mask, np.int32).reshape(hidden.shape[0], -1)
    t_len = min(hidden.shape[1], m.shape[1])
    return hidden.shape[0] * t_len, int((m[:, :t_len] > 0).sum())


# ---- the C++ restatement -------------------------------------------------------------------------------------------------------
def lib():
    global _LIB
    if _LIB is None:
        import _embed_build
        _LIB = C.CDLL(_embed_build.build_oracle())
        vp = C.c_void_p
        _LIB.embed_oracle_pool.argtypes = [vp, C.c_uint64, C.c_uint32, C.c_uint32, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp]
        _LIB.embed_oracle_pool.restype = None
        _LIB.embed_oracle_normalize.argtypes = [vp, C.c_uint64, C.c_uint32, vp]
        _LIB.embed_oracle_normalize.restype = None
    return _LIB


def pool_cpp(hidden, mask, mode, normalize, order=None, want_counts=False):
    x = np.ascontiguousarray(hidden, np.float32)
    batch, seq, dim = x.shape
    m = None if mask is None else np.ascontiguousarray(mask, np.int32).reshape(batch, -1)
    o = None if order is None else np.ascontiguousarray(order, np.uint32)
    out, counts = np.zeros((batch, dim), np.float32), np.zeros(2, np.uint64)
    lib().embed_oracle_pool(x.ctypes.data, batch, seq, dim, None if m is None else m.ctypes.data, 0 if m is None else m.shape[1], mode,
                            int(bool(normalize)), None if o is None else o.ctypes.data, out.ctypes.data, counts.ctypes.data)
    return (out, (int(counts[0]), int(counts[1]))) if want_counts else out


def normalize_cpp(rows):
    x = np.ascontiguousarray(rows, np.float32)
    out = np.zeros_like(x)
    lib().embed_oracle_normalize(x.ctypes.data, x.shape[0], x.shape[1], out.ctypes.data)
    return out


# ---- the golden cases ----------------------------------------------------------------------------------------------------------
def _case(hidden, mask, mode, normalize):
    return {"hidden": np.ascontiguousarray(hidden, np.float32), "mask": None if mask is None else np.ascontiguousarray(mask, np.int32),
            "mode": mode, "normalize": bool(normalize)}


def _f(*v):
    return np.array(v, np.float32)


def pool_cases():
    """name -> {hidden [B][S][D], mask [B][L] or None, mode, normalize}."""
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    rng = np.random.default_rng(30)
    cases = {}
    for k, count in enumerate((3, 7, 511)):      # the counts at which v / total and v * (1 / total) part
        seq = count + 1
        m = np.ones((2, seq), np.int32)
        m[0, count // 2] = 0
        m[1, 0] = 0
        cases["mean_count_%d" % count] = _case(mixed(rng, (2, seq, 8)), m, MEAN, k % 2 == 0)
    for k in range(6):
        m = (rng.random((3, 40)) < 0.7).astype(np.int32)
        m[:, 0] = 1
        m[:, 1] = 1
        cases["mean_mixed_%d" % k] = _case(mixed(rng, (3, 40, 48)), m, MEAN, k % 2 == 1)
    m = (rng.random((3, 40)) < 0.6).astype(np.int32)
    for name, mode in (("max_mixed", MAX), ("cls_mixed", CLS)):
        cases[name] = _case(mixed(rng, (3, 40, 48)), m, mode, True)
        cases[name + "_raw"] = _case(mixed(rng, (3, 40, 48)), m, mode, False)
    # a NaN and infinities planted in masked rows
    x = mixed(rng, (2, 6, 5))
    m = np.array([[1, 0, 1, 1, 0, 1], [0, 1, 1, 0, 1, 1]], np.int32)
    x[0, 1], x[0, 4, 2], x[1, 0, 1], x[1, 3] = nan, inf, -inf, nan
    for name, mode in (("nan_masked_mean", MEAN), ("nan_masked_max", MAX)):
        cases[name] = _case(x, m, mode, True)
    # a NaN in an active row: the norm is NaN, the row is zeros under normalisation; without it the NaN stays
    x = mixed(rng, (2, 4, 5))
    x[0, 2, 3] = nan
    cases["nan_active_mean"] = _case(x, np.ones((2, 4), np.int32), MEAN, True)
    cases["nan_active_mean_raw"] = _case(x, np.ones((2, 4), np.int32), MEAN, False)
    cases["inf_active_max"] = _case(np.where(np.isnan(x), inf, x), np.ones((2, 4), np.int32), MAX, True)
    # all masked: zeros; no mask at all: zeros
    x = mixed(rng, (2, 5, 6))
    m = np.zeros((2, 5), np.int32)
    m[1, 2] = 1
    cases["all_masked_mean"] = _case(x, m, MEAN, True)
    cases["all_masked_max"] = _case(x, m, MAX, False)
    cases["no_mask_mean"] = _case(x, np.zeros((2, 0), np.int32), MEAN, False)
    # CLS copies a masked first token; -0.0f keeps its sign through the normalisation
    x = mixed(rng, (2, 3, 4))
    x[0, 0] = _f(-0.0, 3.0, 0.0, -4.0)
    cases["cls_masked_first"] = _case(x, np.array([[0, 1, 1], [0, 0, 0]], np.int32), CLS, True)
    # MAX of all-negative tokens is the initial +0.0f; negative zero never replaces it
    x = -np.abs(mixed(rng, (2, 5, 6)))
    x[1, :, 0] = -0.0
    cases["max_all_negative"] = _case(x, np.ones((2, 5), np.int32), MAX, False)
    # any positive mask value is active for MAX; negative values are masked
    m = np.array([[7, -1, 2, 0, 1, -5], [0, 3, -2, 1, 1, 9]], np.int32)
    cases["max_mask_7"] = _case(mixed(rng, (2, 6, 9)), m, MAX, True)
    cases["mean_negative_mask"] = _case(mixed(rng, (2, 6, 9)), np.minimum(m, 1), MEAN, True)
    # the mask shorter and longer than the sequence: min(seq, mask_len) tokens are considered; a weight of 2 past them is not seen
    x = mixed(rng, (2, 6, 7))
    cases["mask_shorter"] = _case(x, np.ones((2, 4), np.int32), MEAN, False)
    m = np.ones((2, 8), np.int32)
    m[:, 6] = 2
    m[1, 2] = 0
    cases["mask_longer"] = _case(x, m, MEAN, True)
    # the norm threshold: at or below 1e-8 zeros, just above served
    cases["norm_tiny"] = _case(_f([3e-9, -4e-9, 0], [6e-9, -8e-9, 0]).reshape(2, 1, 3), np.ones((2, 1), np.int32), MEAN, True)
    cases["norm_just_above"] = _case(_f([1e-8, 2e-9, 0], [1.0000001e-8, 0, 0]).reshape(2, 1, 3), np.ones((2, 1), np.int32), CLS, True)
    # subnormal means are kept
    cases["subnormal_mean"] = _case(_f([1e-40, 3e-41, -2e-42], [2e-40, 1e-41, -7e-42], [4e-41, 5e-41, 1e-45]).reshape(1, 3, 3), np.ones((1, 3), np.int32),
                                    MEAN, False)
    # FLT_MAX / 4: the squares overflow fp32, not fp64
    big = np.float32(np.finfo(np.float32).max / 4)
    cases["flt_max_quarter"] = _case(np.full((1, 2, 5), big, np.float32) * _f(1, -1, 1, 0.5, 1), np.ones((1, 2), np.int32), MAX, True)
    return cases


def rank2_cases():
    """name -> rows [B][D], normalised."""
    rng = np.random.default_rng(31)
    big = np.float32(np.finfo(np.float32).max / 4)
    return {
        "rank2_mixed": mixed(rng, (4, 48)),
        "rank2_specials": _f([np.nan, 1, 2], [np.inf, 1, 2], [-0.0, 0.0, -2], [3e-9, -4e-9, 0], [1e-8, 2e-9, 0], [big, -big, big]),
    }


def case_names():
    return list(pool_cases()) + list(rank2_cases())


def case_arrays(c):
    if isinstance(c, dict):
        return [c["hidden"], np.zeros((0,), np.int32) if c["mask"] is None else c["mask"], np.array([c["mode"], int(c["normalize"])], np.uint32)]
    return [c]


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def case_digest(name):
    c = pool_cases().get(name)
    return digest(case_arrays(c if c is not None else rank2_cases()[name]))


def write_case_list(path, cases):
    """The cases as the drivers read them: u32 count; per case u32 kind; kind 0 (rank 3): u32 B, S, D, mode, normalize, mask_len,
    the masks [B][mask_len] int32, the hidden states [B][S][D]; kind 1 (rank 2): u32 B, D, normalize (1), the rows."""
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for c in cases:
            if isinstance(c, dict):
                x = c["hidden"]
                m = np.zeros((x.shape[0], 0), np.int32) if c["mask"] is None else c["mask"]
                f.write(struct.pack("<IIIIIII", 0, x.shape[0], x.shape[1], x.shape[2], c["mode"], int(c["normalize"]), m.shape[1]))
                f.write(np.ascontiguousarray(m, np.int32).tobytes())
                f.write(np.ascontiguousarray(x, np.float32).tobytes())
            else:
                f.write(struct.pack("<IIII", 1, c.shape[0], c.shape[1], 1))
                f.write(np.ascontiguousarray(c, np.float32).tobytes())


def write_cases(path):
    write_case_list(path, list(pool_cases().values()) + list(rank2_cases().values()))


def parse_driver_output(text):
    """({counter name: value}, [hex of the case's output floats])."""
    info, out = {}, []
    for line in text.splitlines():
        w = line.split()
        if w[:1] == ["case"]:
            out.append(w[2] if len(w) > 2 else "")
        elif len(w) == 2 and w[1].lstrip("-").isdigit():
            info[w[0]] = int(w[1])
    return info, out


def restated(pool=None, normalize=None):
    """The hex outputs of every case."""
    pool = pool or pool_py
    normalize = normalize or normalize_py
    out = [hexbits(np.asarray(pool(c["hidden"], c["mask"], c["mode"], c["normalize"]), np.float32)) for c in pool_cases().values()]
    return out + [hexbits(np.asarray(normalize(r), np.float32)) for r in rank2_cases().values()]


def reversed_case(c):
    """The same texts with their tokens in reverse order (mask_len == seq): an in-order loop then sums in reverse."""
    assert c["mask"].shape[1] == c["hidden"].shape[1]
    return _case(c["hidden"][:, ::-1], c["mask"][:, ::-1], c["mode"], c["normalize"])


# ---- stress cases --------------------------------------------------------------------------------------------------------------
S_DIMS = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 384, 768, 1024, 1025]
S_SEQS = [1, 2, 3, WINDOW - 1, WINDOW, WINDOW + 1, 2 * WINDOW + 1]
S_BATCHES = [1, 2, 3, 9, 257]
MAX_REDRAWS = 20


def _draw(seed, attempt):
    rng = np.random.default_rng([seed, attempt])
    dim, seq, batch = int(rng.choice(S_DIMS)), int(rng.choice(S_SEQS)), int(rng.choice(S_BATCHES))
    while batch * seq * dim > 1 << 21:      # a few MiB at the most
        batch = max(1, batch // 3)
    mode = MEAN if rng.random() < 0.6 else MAX      # CLS reads no mask and no second token: nothing to prove; the lattice holds it
    mask_len = seq + int(rng.choice([-1, 0, 0, 0, 1])) if seq > 1 else seq + int(rng.choice([0, 1]))
    kind = int(rng.integers(0, 4))
    m = np.ones((batch, mask_len), np.int32)
    if kind == 1:
        m = (rng.random((batch, mask_len)) < 0.7).astype(np.int32)
    elif kind == 2:      # padding at the tail, of a different length per text
        for b in range(batch):
            m[b, int(rng.integers(1, mask_len + 1)):] = 0
    elif kind == 3:      # a zero run that straddles a window edge
        lo = max(0, min(mask_len, WINDOW) - int(rng.integers(1, 9)))
        m[:, lo:lo + int(rng.integers(2, 17))] = 0
    if mode == MAX:
        m = m * rng.choice(np.array([1, 1, 7], np.int32), m.shape) - (rng.random(m.shape) < 0.05) * (m == 0)
    x = mixed(rng, (batch, seq, dim), -3, 3)
    # masked rows are LARGER than active ones, so that admitting one moves a maximum as surely as a mean
    t_len = min(seq, mask_len)
    off = np.ones((batch, seq), bool)
    off[:, :t_len] = m[:, :t_len] <= 0
    x[off] *= np.float32(16.0)
    return {"seed": seed, "hidden": x, "mask": m.astype(np.int32), "mode": mode, "normalize": bool(rng.random() < 0.5),
            "host": bool(rng.random() < 0.3), "misalign": 4 if rng.random() < 0.3 else 0, "has_masked": bool(off.any())}


def discriminates(c):
    """(reversing the tokens changes the output bits, admitting every masked token does) — from the oracle alone."""
    x, m = c["hidden"], c["mask"]
    base = pool_cpp(x, m, c["mode"], c["normalize"])
    rev = pool_cpp(x, m, c["mode"], c["normalize"], order=np.arange(x.shape[1] - 1, -1, -1))
    admitted = pool_cpp(x, np.ones(x.shape[:2], np.int32), c["mode"], c["normalize"])
    return (not equal(base, rev), not equal(base, admitted))


def stress_case(seed):
    """A batch whose output bits PROVABLY depend on the token order (every MEAN case) and on every masked token staying out
    (every case that has one): the draw is repeated (seed, attempt) until the oracle shows it.  c["redraws"]: how often."""
    for attempt in range(MAX_REDRAWS + 1):
        c = _draw(seed, attempt)
        rev, adm = discriminates(c)
        if (rev or c["mode"] != MEAN) and (adm or not c["has_masked"]) and (rev or (adm and c["has_masked"])):
            c["redraws"], c["proves_order"], c["proves_mask"] = attempt, bool(rev), bool(adm and c["has_masked"])
            return c
    raise AssertionError("no discriminating draw for seed %d within %d redraws" % (seed, MAX_REDRAWS))


def differs(got, want):
    """The outputs whose bits differ (a NaN matches any NaN)."""
    return [i for i, (g, w) in enumerate(zip(got, want)) if not equal(g, w)]
