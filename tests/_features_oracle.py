"""Test infrastructure: the restatement of the topology build's input features (aggregateEmbedding, computeVarianceWeights,
composeFeatureVector of TopologyInputExtractor::extract) in numpy, written from the contract in include/yams_mi355x_accel.h
with every fp32 / fp64 step explicit and the fma emulated exactly, plus the ctypes door to tests/cpp/features_oracle.cpp (the
same contract in C++, fast enough for the large shapes) and the inputs of the golden cases."""
import ctypes as C
import hashlib

import numpy as np

from _artifacts_oracle import fma

SEPARATE, FUSED = 0, 1
FORMS = {"separate": SEPARATE, "fused": FUSED}
MAX_DIM = 4096
MAX_SIG_LEN = 65536
SAMPLE_CAP = 4096
f32, f64 = np.float32, np.float64


def hexbits(a):
    """The bits of an array as one hex string (little-endian bytes, as stored)."""
    return np.ascontiguousarray(a).tobytes().hex()


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        if a is None:
            h.update(b"none")
            continue
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- aggregate ---------------------------------------------------------------------------------------------------------------
def aggregate_py(rows, off, records):
    """(out [n_docs][dim] float32, counts [n_docs] uint32): the first record assigned, the later ones added, / float(count)."""
    rows = np.ascontiguousarray(rows, f32)
    off = np.asarray(off, np.int64)
    n_docs, dim = len(off) - 1, rows.shape[1]
    out = np.zeros((n_docs, dim), f32)
    cnt = np.zeros(n_docs, np.uint32)
    with np.errstate(all="ignore"):
        for d in range(n_docs):
            lst = records[off[d]:off[d + 1]]
            cnt[d] = len(lst)
            if len(lst) == 0:
                continue
            s = rows[lst[0]].copy()      # assigned: the bits are kept
            for r in lst[1:]:
                s = (s + rows[r]).astype(f32)
            if len(lst) > 1:
                s = (s / f32(len(lst))).astype(f32)
            out[d] = s
    return out, cnt


# ---- variance ----------------------------------------------------------------------------------------------------------------
def variance_py(rows, select, form):
    """(mean [dim], var [dim]) float64 over rows[select] in order (all rows without select)."""
    rows = np.ascontiguousarray(rows, f32)
    sample = rows if select is None else rows[np.asarray(select, np.int64)]
    m, dim = sample.shape
    with np.errstate(all="ignore"):
        mean = np.zeros(dim, f64)
        for e in sample:
            mean = mean + e.astype(f64)
        mean = mean / f64(m)
        var = np.zeros(dim, f64)
        for e in sample:
            d = e.astype(f64) - mean
            if form == FUSED:
                var = np.array([fma(d[i], d[i], var[i]) for i in range(dim)], f64)
            else:
                p = d * d
                var = var + p
        var = var / f64(m)
    return mean, var


def _adjust_heap(a, hole, length, value, comp):
    top, child = hole, hole
    while child < (length - 1) // 2:
        child = 2 * (child + 1)
        if comp(a[child], a[child - 1]):
            child -= 1
        a[hole] = a[child]
        hole = child
    if (length & 1) == 0 and child == (length - 2) // 2:
        child = 2 * (child + 1)
        a[hole] = a[child - 1]
        hole = child - 1
    parent = (hole - 1) // 2
    while hole > top and comp(a[parent], value):
        a[hole] = a[parent]
        hole = parent
        parent = (hole - 1) // 2
    a[hole] = value


def heap_select(var, target):
    """The indices std::partial_sort(idx, idx + target, idx + dim, var[a] > var[b]) of the GNU library leaves in front (as a
    set: the heap select keeps them, the sort that follows only orders them)."""
    idx = list(range(len(var)))
    comp = lambda x, y: var[x] > var[y]      # noqa: E731
    if target >= 2:
        parent = (target - 2) // 2
        while True:
            _adjust_heap(idx, parent, target, idx[parent], comp)
            if parent == 0:
                break
            parent -= 1
    for i in range(target, len(idx)):
        if target and comp(idx[i], idx[0]):
            value = idx[i]
            idx[i] = idx[0]
            _adjust_heap(idx, 0, target, value, comp)
    return sorted(idx[:target])


def weights_py(var, target):
    """float(sqrt(var)) at the kept dimensions, 0 elsewhere; None when a variance is a NaN."""
    var = np.asarray(var, f64)
    if np.isnan(var).any():
        return None
    w = np.zeros(len(var), f32)
    with np.errstate(all="ignore"):
        for i in heap_select(var, target):
            w[i] = f32(np.sqrt(var[i]))
    return w


def variance_weights_py(sample, target, form):
    """computeVarianceWeights over equal-sized rows (the early returns are the shell's)."""
    _, var = variance_py(sample, None, form)
    return weights_py(var, target)


# ---- compose -----------------------------------------------------------------------------------------------------------------
def _normalize_rows(v):
    """l2NormalizeInPlace of every row of v [n][len] float32: one fp64 chain per row in element order."""
    n, ln = v.shape
    s = np.zeros(n, f64)
    for j in range(ln):
        x = v[:, j].astype(f64)
        s = s + x * x      # exact product, one rounded add
    norm = np.sqrt(s).astype(f32)
    leave = s <= 0.0       # False for a NaN
    out = (v / norm[:, None]).astype(f32)
    out[leave] = v[leave]
    return out


def longest_row(dim, weights, entity, k, sig, sig_len, sketch_dim):
    kc = dim if weights is None else int((np.asarray(weights, f32) > 0).sum())
    return kc + (k if entity is not None and k else 0) + (sketch_dim if sig is not None and sig_len and sketch_dim else 0)


def compose_py(dense, weights, entity, entity_on, sig, sketch_on, sketch_dim, alpha_e, alpha_m, out_stride=None):
    """(out [n][out_stride] float32, dims [n] uint32).  entity [n][K] or None, sig [n][sig_len] uint32 or None."""
    dense = np.ascontiguousarray(dense, f32)
    n, dim = dense.shape
    k = 0 if entity is None else entity.shape[1]
    sig_len = 0 if sig is None else sig.shape[1]
    longest = longest_row(dim, weights, entity, k, sig, sig_len, sketch_dim)
    stride = longest if out_stride is None else out_stride
    assert stride >= longest
    with np.errstate(all="ignore"):
        if weights is not None:
            w = np.asarray(weights, f32)
            kept = np.nonzero(w > 0)[0]
            view = (dense[:, kept] * w[kept][None, :]).astype(f32)
        else:
            view = dense.copy()
        kc = view.shape[1]
        view = _normalize_rows(view) if kc else view
        has_e, has_m = entity is not None and k > 0, sig is not None and sig_len > 0 and sketch_dim > 0
        e_on = np.asarray(entity_on, bool) if has_e else np.zeros(n, bool)
        m_on = np.asarray(sketch_on, bool) if has_m else np.zeros(n, bool)
        a_e = np.where(e_on, f32(alpha_e), f32(0)).astype(f32)
        a_m = np.where(m_on, f32(alpha_m), f32(0)).astype(f32)
        t = ((f32(1) - a_e).astype(f32) - a_m).astype(f32)
        a_d = np.where(f32(0) < t, t, f32(0)).astype(f32)
        out = np.zeros((n, stride), f32)
        dims = np.zeros(n, np.uint32)
        if has_m:
            counts = np.zeros((n, sketch_dim), f32)
            for r in np.nonzero(m_on)[0]:
                counts[r] = np.bincount(sig[r].astype(np.int64) % sketch_dim, minlength=sketch_dim).astype(f32)
            sketch = _normalize_rows(counts)
        for r in range(n):
            on = e_on[r] or m_on[r]
            out[r, :kc] = (view[r] * a_d[r]).astype(f32) if on else view[r]
            ln = kc
            if e_on[r]:
                out[r, ln:ln + k] = (np.asarray(entity[r], f32) * a_e[r]).astype(f32)
                ln += k
            if m_on[r]:
                out[r, ln:ln + sketch_dim] = (sketch[r] * a_m[r]).astype(f32)
                ln += sketch_dim
            dims[r] = ln
    return out, dims


# ---- the C++ restatement -----------------------------------------------------------------------------------------------------
_LIB = None
vp = C.c_void_p


def _lib():
    global _LIB
    if _LIB is None:
        import _features_build
        L = C.CDLL(_features_build.build_oracle())
        L.features_aggregate_oracle.argtypes = [vp, C.c_uint32, vp, vp, C.c_uint64, vp, vp]
        L.features_aggregate_oracle.restype = None
        L.features_variance_oracle.argtypes = [vp, C.c_uint32, vp, C.c_uint64, C.c_int, vp, vp]
        L.features_variance_oracle.restype = None
        L.features_weights_oracle.argtypes = [vp, C.c_uint32, C.c_uint32, vp]
        L.features_weights_oracle.restype = C.c_int
        L.features_compose_oracle.argtypes = [vp, C.c_uint64, C.c_uint32, vp, vp, C.c_uint32, vp, vp, C.c_uint32, vp, C.c_uint32, C.c_float,
                                              C.c_float, vp, C.c_uint32, vp]
        L.features_compose_oracle.restype = C.c_uint32
        _LIB = L
    return _LIB


def _p(a):
    return None if a is None else a.ctypes.data


def aggregate_cpp(rows, off, records):
    rows = np.ascontiguousarray(rows, f32)
    off = np.ascontiguousarray(off, np.uint64)
    rec = np.ascontiguousarray(records, np.uint32)
    n_docs, dim = len(off) - 1, rows.shape[1]
    out = np.empty((n_docs, dim), f32)
    cnt = np.empty(n_docs, np.uint32)
    _lib().features_aggregate_oracle(_p(rows), dim, _p(off), _p(rec), n_docs, _p(out), _p(cnt))
    return out, cnt


def variance_cpp(rows, select, form):
    rows = np.ascontiguousarray(rows, f32)
    sel = None if select is None else np.ascontiguousarray(select, np.uint32)
    m = rows.shape[0] if sel is None else len(sel)
    dim = rows.shape[1]
    mean, var = np.empty(dim, f64), np.empty(dim, f64)
    _lib().features_variance_oracle(_p(rows), dim, _p(sel), m, int(form == FUSED), _p(mean), _p(var))
    return mean, var


def weights_cpp(var, target):
    var = np.ascontiguousarray(var, f64)
    w = np.empty(len(var), f32)
    return None if _lib().features_weights_oracle(_p(var), len(var), target, _p(w)) else w


def compose_cpp(dense, weights, entity, entity_on, sig, sketch_on, sketch_dim, alpha_e, alpha_m, out_stride=None):
    dense = np.ascontiguousarray(dense, f32)
    n, dim = dense.shape
    w = None if weights is None else np.ascontiguousarray(weights, f32)
    ent = None if entity is None else np.ascontiguousarray(entity, f32)
    eon = None if entity_on is None else np.ascontiguousarray(entity_on, np.uint8)
    sg = None if sig is None else np.ascontiguousarray(sig, np.uint32)
    son = None if sketch_on is None else np.ascontiguousarray(sketch_on, np.uint8)
    k = 0 if ent is None else ent.shape[1]
    sig_len = 0 if sg is None else sg.shape[1]
    stride = longest_row(dim, w, ent, k, sg, sig_len, sketch_dim) if out_stride is None else out_stride
    out = np.empty((n, stride), f32)
    dims = np.empty(n, np.uint32)
    longest = _lib().features_compose_oracle(_p(dense), n, dim, _p(w), _p(ent), k, _p(eon), _p(sg), sig_len, _p(son), sketch_dim,
                                             alpha_e, alpha_m, _p(out), stride, _p(dims))
    assert longest <= stride
    return out, dims


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def mixed(rng, shape, lo=-12, hi=12):
    """Floats of mixed exponents: full mantissas, binary exponents in [lo, hi)."""
    return (rng.standard_normal(shape) * np.exp2(rng.integers(lo, hi, shape))).astype(f32)


def csr(lengths):
    off = np.zeros(len(lengths) + 1, np.uint64)
    off[1:] = np.cumsum(lengths)
    return off


def flip_sample(seed, m=4):
    """A sample of m rows x 2 dimensions whose second column is the first reversed: the same values, so the same mean and
    the same residuals in another order; which of the two variances is the larger is decided in the last place, where the
    two forms round differently."""
    rng = np.random.default_rng(seed)
    col = (rng.integers(1, 1 << 12, m) * np.exp2(rng.integers(-3, 4, m))).astype(f32)      # few bits: the sum is exact
    return np.stack([col, col[::-1]], axis=1).astype(f32)


def find_flip_samples(count, m=4, start=0, limit=200000):
    """Seeds of flip_sample whose kept dimension (target 1 of 2) differs between the forms, strictly in both (no tie)."""
    found = []
    for seed in range(start, start + limit):
        x = flip_sample(seed, m)
        _, vs = variance_cpp(x, None, SEPARATE)
        _, vf = variance_cpp(x, None, FUSED)
        if (vs[0] > vs[1] and vf[0] < vf[1]) or (vs[0] < vs[1] and vf[0] > vf[1]):
            found.append(seed)
            if len(found) == count:
                break
    return found


# ---- the shell's rules, restated (what include/yams_accel/topology_features.hpp keeps on the host) -----------------------------
CHUNK, DOCUMENT = 0, 1


def shell_aggregate(docs, aggregate=aggregate_py):
    """aggregateEmbedding per document; docs: lists of (level, float32 array).  Returns a list of float32 arrays."""
    out = [None] * len(docs)
    groups = {}
    for d, recs in enumerate(docs):
        short = next((e for lv, e in recs if lv == DOCUMENT and len(e)), None)
        if short is not None:
            out[d] = np.asarray(short, f32).copy()
            continue
        contributing = [e for _, e in recs if len(e)]
        contributing = [e for e in contributing if len(e) == len(contributing[0])]
        if not contributing:
            out[d] = np.zeros(0, f32)
            continue
        groups.setdefault(len(contributing[0]), []).append((d, contributing))
    for dim, members in groups.items():
        rows = np.stack([e for _, c in members for e in c]).astype(f32)
        off = csr([len(c) for _, c in members])
        got, cnt = aggregate(rows, off, np.arange(len(rows), dtype=np.uint32))
        assert cnt.tolist() == [len(c) for _, c in members]
        for (d, _), row in zip(members, got):
            out[d] = row
    return out


def shell_variance_weights(sample, target, form, variance=variance_py, weights=weights_py):
    """computeVarianceWeights(sample, target): a float32 array (empty where the reference returns {})."""
    if len(sample) == 0 or target == 0:
        return np.zeros(0, f32)
    full = len(sample[0])
    if target >= full:
        return np.zeros(0, f32)
    rows = [e for e in sample if len(e) == full]
    if not rows or full == 0:
        return np.zeros(0, f32)
    _, var = variance(np.stack(rows).astype(f32), None, form)
    return weights(var, target)


def shell_compose(case, compose=compose_py):
    """composeFeatureVector per row of a compose case.  Returns a list of float32 arrays."""
    cfg, dense, w = case["cfg"], case["dense"], case["weights"]
    n, dim = dense.shape
    mat = cfg["matryoshka"] and len(w) > 0 and 0 < cfg["target"] < dim
    e_nonempty = np.array([len(e) > 0 for e in case["entity"]])
    s_nonempty = np.array([len(s) > 0 for s in case["sig"]])
    e_on = e_nonempty & bool(cfg["entity"])
    m_on = s_nonempty & bool(cfg["minhash"] and cfg["sketch_dim"] > 0)
    if mat and len(w) != dim:      # :169-171 — dense comes back un-normalised; the shell serves it only with both parts off
        assert not e_on.any() and not m_on.any()
        return [r.copy() for r in dense]
    k = max([len(e) for e in case["entity"]] + [0])
    sl = max([len(s) for s in case["sig"]] + [0])
    ent = np.stack([np.asarray(e, f32) if len(e) else np.zeros(k, f32) for e in case["entity"]]) if k and e_on.any() else None
    sig = np.stack([np.asarray(s, np.uint32) if len(s) else np.zeros(sl, np.uint32) for s in case["sig"]]) if sl and m_on.any() else None
    out, dims = compose(dense, w if mat else None, ent, e_on.astype(np.uint8), sig, m_on.astype(np.uint8),
                        cfg["sketch_dim"] if sig is not None else 0, cfg["alpha_e"], cfg["alpha_m"])
    return [out[r, :dims[r]].copy() for r in range(n)]


# ---- the golden cases ----------------------------------------------------------------------------------------------------------
FLIP_SEEDS = {3: [81, 93, 167], 5: [13, 39, 92]}      # find_flip_samples(…, m): the kept dimension differs between the forms
NZ = np.float32(-0.0)
TINY = np.float32(1.401298464324817e-45)               # 2^-149
HUGE = np.float32(3.0e38)


def _aggregate_case():
    rng = np.random.default_rng(101)
    d = 5
    r = lambda: mixed(rng, d)      # noqa: E731
    e = np.zeros(0, f32)
    negz = np.array([NZ, 1, NZ, -2, NZ], f32)
    negz2 = np.array([NZ, 3, 0.0, 5, NZ], f32)
    nan = np.array([np.nan, np.inf, -np.inf, 1, 2], f32)
    return [
        [],                                                            # no record: an empty vector
        [(CHUNK, negz)],                                               # one record: assigned, -0.0f stays
        [(CHUNK, negz), (CHUNK, negz2)],                               # -0.0f + -0.0f = -0.0f, / 2 = -0.0f; 0.0f + would give +0.0f
        [(CHUNK, r()) for _ in range(17)],
        [(CHUNK, r()), (DOCUMENT, r()), (CHUNK, r())],                 # the document-level record short-circuits
        [(CHUNK, r()), (DOCUMENT, e), (CHUNK, r())],                   # an empty document-level record does not
        [(CHUNK, e), (CHUNK, r()), (CHUNK, mixed(rng, 3)), (CHUNK, r()), (CHUNK, e)],      # empty and ragged records are skipped
        [(CHUNK, mixed(rng, 3)), (CHUNK, r()), (CHUNK, mixed(rng, 3))],                    # the first contributing record sets the size
        [(CHUNK, nan), (CHUNK, r())],
        [(CHUNK, np.full(d, HUGE, f32))] * 3 + [(CHUNK, -np.full(d, HUGE, f32))],          # the fp32 sum overflows
        [(CHUNK, np.full(d, TINY, f32))] * 3,                                              # denormals are kept
    ]


def _variance_cases():
    rng = np.random.default_rng(202)
    cases = {}
    for m, seeds in FLIP_SEEDS.items():
        for s in seeds:
            cases["var_flip_m%d_s%d" % (m, s)] = ([r for r in flip_sample(s, m)], 1)
    x = mixed(rng, (9, 7))
    cases["var_mixed_9x7_t3"] = ([r for r in x], 3)
    rag = [r for r in mixed(rng, (6, 5))]
    rag.insert(2, mixed(rng, 4))
    rag.append(np.zeros(0, f32))
    cases["var_ragged_rows_t2"] = (rag, 2)
    tie = mixed(rng, (7, 4), -2, 2)
    tie[:, 0] *= 64
    tie[:, 2] = tie[:, 1]                     # equal variances straddling the cut at target 2
    tie[:, 3] /= 64
    cases["var_tie_at_cut_t2"] = ([r for r in tie], 2)
    zer = mixed(rng, (6, 4), -2, 2)
    zer[:, 1] = 3.5
    zer[:, 3] = -0.25                         # two zero variances: target 3 keeps only 2
    cases["var_zero_inside_top_t3"] = ([r for r in zer], 3)
    cases["var_target_ge_dim"] = ([r for r in x], 7)
    cases["var_target_zero"] = ([r for r in x], 0)
    cases["var_one_row_t2"] = ([x[0]], 2)
    return cases


def _compose_cases():
    rng = np.random.default_rng(303)
    cases = {}
    n, dim, k, sl = 8, 9, 3, 11
    dense = mixed(rng, (n, dim))
    dense[1] = 0.0                                      # sumSq == 0: left as it is
    dense[2] = 0.0
    dense[2, 4] = TINY                                  # the smallest norm there is: 2^-149 (no norm can round to 0.0f)
    dense[3] = HUGE                                     # the norm rounds to inf: every element becomes 0.0f
    dense[4, 0] = np.nan
    dense[5, 3] = NZ
    ent_all = [mixed(rng, k, -2, 2) for _ in range(n)]
    sig_all = [rng.integers(0, 1 << 32, sl, dtype=np.uint64).astype(np.uint32) for _ in range(n)]
    none_f, none_u = np.zeros(0, f32), np.zeros(0, np.uint32)
    combos = [(i & 1, (i >> 1) & 1) for i in range(n)]      # every (entity, minhash) combination, twice
    ent = [ent_all[i] if e else none_f for i, (e, _) in enumerate(combos)]
    sig = [sig_all[i] if m else none_u for i, (_, m) in enumerate(combos)]
    cfg = dict(entity=1, matryoshka=0, target=0, minhash=1, sketch_dim=7, alpha_e=0.25, alpha_m=0.125)
    cases["compose_four_combinations"] = dict(dense=dense, weights=none_f, entity=ent, sig=sig, cfg=cfg)
    cases["compose_all_off"] = dict(dense=dense, weights=none_f, entity=ent, sig=sig, cfg=dict(cfg, entity=0, minhash=0))
    cases["compose_nan_alpha"] = dict(dense=dense, weights=none_f, entity=ent, sig=sig, cfg=dict(cfg, alpha_e=float("nan")))
    cases["compose_alphas_above_one"] = dict(dense=dense, weights=none_f, entity=ent, sig=sig, cfg=dict(cfg, alpha_e=0.75, alpha_m=0.5))
    cases["compose_sketch_dim_1"] = dict(dense=dense, weights=none_f, entity=ent, sig=sig, cfg=dict(cfg, sketch_dim=1))
    w = np.zeros(dim, f32)
    w[[1, 4, 7]] = [0.5, 2.0, 1e-3]
    w[2] = np.nan                                       # a NaN weight is not kept
    w[6] = -1.0
    cases["compose_matryoshka_kept3"] = dict(dense=dense, weights=w, entity=ent, sig=sig, cfg=dict(cfg, matryoshka=1, target=4))
    cases["compose_matryoshka_alone"] = dict(dense=dense, weights=w, entity=ent, sig=sig,
                                             cfg=dict(cfg, matryoshka=1, target=4, entity=0, minhash=0))
    cases["compose_target_ge_dim"] = dict(dense=dense, weights=w, entity=ent, sig=sig, cfg=dict(cfg, matryoshka=1, target=dim))
    cases["compose_weights_of_another_size"] = dict(dense=dense, weights=w[:5].copy(), entity=ent, sig=sig,
                                                    cfg=dict(cfg, matryoshka=1, target=4, entity=0, minhash=0))
    cases["compose_no_weight_kept"] = dict(dense=dense, weights=np.zeros(dim, f32), entity=ent, sig=sig, cfg=dict(cfg, matryoshka=1, target=4))
    return cases


AGGREGATE_CASE = _aggregate_case()
VARIANCE_CASES = _variance_cases()
COMPOSE_CASES = _compose_cases()


def aggregate_digest():
    return digest(*[np.concatenate([[lv], e]).astype(f32) for recs in AGGREGATE_CASE for lv, e in recs])


def variance_digest(name):
    sample, target = VARIANCE_CASES[name]
    return digest(np.array([target], np.uint32), *sample)


def compose_digest(name):
    c = COMPOSE_CASES[name]
    cfg = c["cfg"]
    return digest(c["dense"], c["weights"], *c["entity"], *c["sig"],
                  np.array([cfg[k] for k in ("entity", "matryoshka", "target", "minhash", "sketch_dim")], np.uint32),
                  np.array([cfg["alpha_e"], cfg["alpha_m"]], f32))


def write_cases(path):
    """The golden cases as one binary file for the drivers (uint32 / float32 words, little endian):
    'A' n_docs {n_records {level size floats}} | per variance case 'V' target m {size floats} | per compose case
    'C' entity matryoshka target minhash sketch_dim alpha_e alpha_m |weights| weights n {|dense| dense |entity| entity |sig| sig}."""
    words = []
    u = lambda *v: words.append(np.array(v, np.uint32).tobytes())      # noqa: E731
    arr = lambda a, t=f32: (u(len(a)), words.append(np.ascontiguousarray(a, t).tobytes()))      # noqa: E731
    u(ord("A"), len(AGGREGATE_CASE))
    for recs in AGGREGATE_CASE:
        u(len(recs))
        for lv, e in recs:
            u(lv)
            arr(e)
    for name in VARIANCE_CASES:
        sample, target = VARIANCE_CASES[name]
        u(ord("V"), target, len(sample))
        for e in sample:
            arr(e)
    for name in COMPOSE_CASES:
        c = COMPOSE_CASES[name]
        cfg = c["cfg"]
        u(ord("C"), cfg["entity"], cfg["matryoshka"], cfg["target"], cfg["minhash"], cfg["sketch_dim"])
        words.append(np.array([cfg["alpha_e"], cfg["alpha_m"]], f32).tobytes())
        arr(c["weights"])
        u(len(c["dense"]))
        for r in range(len(c["dense"])):
            arr(c["dense"][r])
            arr(c["entity"][r])
            arr(c["sig"][r], np.uint32)
    with open(path, "wb") as f:
        f.write(b"".join(words))


def case_names():
    return ["aggregate"] + list(VARIANCE_CASES) + list(COMPOSE_CASES)


def restated(form, aggregate=aggregate_py, variance=variance_py, weights=weights_py, compose=compose_py):
    """What the drivers print, from a restatement: per case the list of the output vectors' bits."""
    out = [[hexbits(v) for v in shell_aggregate(AGGREGATE_CASE, aggregate)]]
    for name in VARIANCE_CASES:
        sample, target = VARIANCE_CASES[name]
        out.append([hexbits(shell_variance_weights(sample, target, form, variance, weights))])
    for name in COMPOSE_CASES:
        out.append([hexbits(v) for v in shell_compose(COMPOSE_CASES[name], compose)])
    return out


def parse_driver_output(text):
    """(probe, per case the list of the vectors' bits) from a driver's output: `probe <form>`, then `case`, then one `vec <hex>`
    line per output vector (`vec -` for an empty one)."""
    lines = text.split("\n")
    assert lines[0].startswith("probe "), lines[0]
    cases = []
    for ln in lines[1:]:
        if ln == "case":
            cases.append([])
        elif ln.startswith("vec "):
            cases[-1].append("" if ln[4:] == "-" else ln[4:])
    return lines[0].split()[1], cases


def equal(got, want):
    """Bit for bit, element by element; where the restatement has a NaN the other side must have a NaN (a NaN that arithmetic
    made is some NaN: the payload and sign an invalid operation produces belong to the processor)."""
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if g.shape != w.shape or g.dtype != w.dtype:
        return False
    if g.dtype.kind != "f":
        return bool((g == w).all())
    u = {4: np.uint32, 8: np.uint64}[g.dtype.itemsize]
    return bool(((g.view(u) == w.view(u)) | (np.isnan(g) & np.isnan(w))).all())
