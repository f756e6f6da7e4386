"""The dimension lattice of the general scan, shared by tests/stress_dims.py, tests/test_dim_lattice_cpu.py and
tests/test_dim_lattice_gpu.py (numpy, the oracle and the constants of yams_amd/_lib.py; nothing here needs a device).

The host picks the tier, the kernel form, the slab width and the re-score walk from dim's divisibility by 4, 16, 32, 64 and
128 and a handful of thresholds.  CLASSES names every class of that lattice with the dims at its edges:

  A  dim % 4 != 0                       exhaustive fp64 path, scalar walk (scan_api.cpp prep: `aligned`)
  B  dim % 4 == 0, misaligned base      the row pointer 4, 8 or 12 bytes into an allocation: path 1 although n >= 4096
  C  dim % 4 == 0, dim % 16 != 0        f32 tier: scan_tiles_kernel, kSlabK = 32, a predicated partial last slab
  D  dim % 16 == 0, dim % 32 != 0       bf16 tier, 16-wide slabs (bf16_slab_k, scan_launch.h); single pass and SPLIT_FILTER
  E  dim % 32 == 0                      bf16 tier, 32-wide slabs, at the edges of the persistent / narrow / shared-slab forms
  F  dim % 64 == 0, dim >= 256          int8 tier: a view that carries only the int8 shadow (cosine), both shadows (L2)

Dims added to the issue's lists, and where the branch was read:
  A 129 and 8189          rescore row_sums over a scalar tail behind a multiple of 32, below the 8192 limit
  C 132                   the float4 walk's FIRST dim with a 32-element body AND a 4-element tail past 128 (scan_kernels.hip:903-931)
  E 96 and 288            96: three 32-slabs below the narrow form's second 64; 288: inside the persistent form, dim % 64 != 0
  F 512                   a power of two inside the rotated range: ONE transform (i8_rotation_window(dim) == dim)

Half the queries of every case are LOCALISED on a group G of at most 16 consecutive elements: q = sqrt(.95) u_G + sqrt(.05) u_R,
u_G a unit vector on G, u_R unit Gaussian noise off G.  For each of them rows of three families are planted, built EXACTLY
as a u_G + b u_R + g z with z a unit vector orthogonal to both, so that their scores are closed forms of (a, b, g):

  W  k rows that win because of G  (the scaled noisy copies of the query's elements on G),
  D  k / 4 + 2 rows that rely on G alone, just BEHIND every W row; counting G twice lifts them over the weakest W rows,
  Z  k / 4 + 2 rows that do not touch G, just AHEAD of what a W row keeps when G is zeroed.

So the oracle's top-k row set changes when the rows' elements on G are dropped and when they are counted twice: a kernel
that loses, repeats or mis-strides the slab that holds G answers with other rows.  discriminates() proves that from the oracle
alone for every localised query.  Dims below 8 have no group with two free directions beside it: their queries are dense.
Below dim 128 the best of ~4000 random rows (cosine ~ 3.9 / sqrt(dim)) would reach into the planted scores: there at most 9
queries are localised, all on ONE group with orthonormal u_G and u_R, and the random rows are redrawn until none comes within 0.3 of them.
"""
import math

import numpy as np

import _score_edges as se
from _score_edges import SCAN_COSINE, SCAN_L2, FLAG_FORCE_EXACT, FLAG_F32_FILTER, FLAG_SPLIT_FILTER, FLAG_WIDE_TILE, \
    FLAG_NO_I8_FILTER, FLAG_RESIDENT_QUERIES
from yams_amd._lib import TIER_NONE, TIER_I8, TIER_BF16, TIER_SPLIT, TIER_F32, I8_ROTATED, i8_shadow_rows

FLAG_L2_ACC_F32, FLAG_L2_ACC_F32X8, FLAG_L2_ACC_F32X16, FLAG_L2_ACC_FUSED = 256, 512, 768, 2048
ACC_LANES = {FLAG_L2_ACC_F32: 1, FLAG_L2_ACC_F32X8: 8, FLAG_L2_ACC_F32X16: 16}
L2_ACCS = [0, FLAG_L2_ACC_F32, FLAG_L2_ACC_F32X8, FLAG_L2_ACC_F32X16, FLAG_L2_ACC_F32 | FLAG_L2_ACC_FUSED,
           FLAG_L2_ACC_F32X8 | FLAG_L2_ACC_FUSED, FLAG_L2_ACC_F32X16 | FLAG_L2_ACC_FUSED]
K_RESCORE_MAX, K_MFMA_MIN_ROWS = 2048, 4096        # scan_launch.h kRescoreMax, kMfmaMinRows

CLASSES = {
    "A": [1, 3, 5, 30, 37, 129, 301, 1025, 8189, 8191],
    "B": [64, 100, 768],
    "C": [4, 20, 36, 100, 132, 300, 1028, 4100, 8188],
    "D": [16, 48, 112, 272, 528, 1040, 1552, 4112, 8176],
    "E": [32, 64, 96, 224, 256, 288, 512, 544, 1024, 1056, 2048, 3072, 8192],
    "F": [256, 320, 384, 448, 512, 768, 832, 896, 1088, 1536, 2048, 3072, 4032, 4096, 4160, 8192],
}
FORMS = {"A": ["default"], "B": ["default"], "C": ["default"], "D": ["default", "split"],
         "E": ["default", "wide", "split", "bare"], "F": ["plain", "rotated", "resident"]}
FORM_FLAGS = {"default": 0, "bare": 0, "plain": 0, "rotated": 0, "split": FLAG_SPLIT_FILTER, "wide": FLAG_WIDE_TILE,
              "resident": FLAG_RESIDENT_QUERIES}
NS = [4096, 4097, 4223, 4352, 5001]
NQS = [1, 17, 64, 65, 128, 129, 257]
KS = [1, 10, 100, 300]
THRESHOLDS = [-1.0, 0.0, 0.1]
B_OFFSETS = [4, 8, 12]
G_KINDS = ["first", "tail", "last32", "last64", "straddle_P", "middle"]
MAX_WORK = 6e8          # n * dim * nq of a case: what keeps the oracle's share of a case near a second
S95, S05 = math.sqrt(0.95), math.sqrt(0.05)


def i8_rotation_window(dim):
    """scan_i8_kernel.hip i8_rotation_window: P = 2^floor(log2 dim) for 256 <= dim <= 4096, else 0."""
    if dim < 256 or dim > 4096:
        return 0
    p = 256
    while p * 2 <= dim:
        p *= 2
    return p


def form_applies(cls, form, dim, metric):
    if cls == "F":
        if form == "rotated":
            return i8_rotation_window(dim) != 0
        if form == "resident":
            return dim % 128 == 0 and dim <= 768 and metric == SCAN_COSINE
    return True


def cells():
    """Every (class, form, metric) cell, in the order the harness cycles through."""
    out = []
    for cls in "ABCDEF":
        for form in FORMS[cls]:
            for metric in (SCAN_COSINE, SCAN_L2):
                if any(form_applies(cls, form, dim, metric) for dim in CLASSES[cls]):
                    out.append((cls, form, metric))
    return out


def walk(dim, aligned):
    """The walk rescore_select_kernel takes over a candidate row (scan_kernels.hip:801, 850)."""
    if dim % 32 == 0 and aligned:
        return "staged"
    if dim % 4 == 0 and aligned:
        return "vec4_tail"
    return "scalar"


def group(dim, kind):
    """(start, length) of the group of that kind, or None where the dim has none."""
    if dim < 8:
        return None
    gl = min(16, dim // 2)
    if kind == "first":
        return 0, gl
    if kind == "tail":
        t = min(dim % 32 or 16, gl)
        return dim - t, t
    if kind == "last32":
        return ((dim // 32 - 1) * 32, 16) if dim >= 64 else None
    if kind == "last64":
        return ((dim // 64 - 1) * 64 + 24, 16) if dim >= 128 else None
    if kind == "straddle_P":
        p = 1 << (dim.bit_length() - 1)
        if p == dim or dim < 24:
            return None
        return p - 8, min(16, dim - p + 8)
    if kind == "middle":
        return max(0, (dim // 2) - gl // 2), gl
    raise ValueError(kind)


def restated_route(dim, aligned, shadows, nq, k, metric, flags, n, n_allowed):
    """(path, filter_tier) of yams_scan_diag_t for a call, restated from scan_api.cpp (small_scan_applies, prep, choose_filter,
    i8_filter_possible).  shadows: a set out of {"bf16", "i8"}; n_allowed: None without a mask.  filter_tier is None — not
    asserted — where the library's choice depends on the device's CU count: batches of <= 128 queries on a view with both
    shadows at a dim the resident form takes (dim % 128 == 0, dim <= 768), L2 included; at every other dim such a batch
    is the bf16 tier's.  (L2 queries whose norm is outside
    [1e-15, 1e15) and rows whose norms spread over more than a factor of two are not modelled: no caller here draws them.)"""
    path = se.restated_diag_path(n, n_allowed, dim, nq, k, metric, flags, aligned)
    if path == 1:
        return 1, TIER_NONE
    if (flags & FLAG_F32_FILTER) or dim % 16 != 0:
        return 0, TIER_F32
    need1 = 6 * k + 128 if metric == SCAN_L2 else 3 * k + 64
    split = bool(flags & FLAG_SPLIT_FILTER) or need1 > K_RESCORE_MAX
    i8 = (not split and "i8" in shadows and dim % 64 == 0 and dim >= 256 and 3 * k + 64 <= K_RESCORE_MAX
          and not (flags & (FLAG_NO_I8_FILTER | FLAG_F32_FILTER | FLAG_SPLIT_FILTER))
          and (metric == SCAN_COSINE or "bf16" in shadows))
    if i8:
        if "bf16" in shadows and nq <= 128:
            # a small batch beside a bf16 shadow stays on the int8 tier only in the resident form (i8_resident_plan:
            # dim % 128 == 0, 256 <= dim <= 768 = R_MAX_SLABS slabs, then the CU count and the shard's length decide)
            if dim % 128 == 0 and dim <= 768 and not (flags & FLAG_WIDE_TILE):
                return 0, None
            return 0, TIER_BF16
        return 0, TIER_I8
    return 0, (TIER_SPLIT if split else TIER_BF16)


def form_fields(cls, form, metric, l2_acc=0):
    """flags, shadows and i8_flags of a cell: what the form means on the view and in the call."""
    out = {"flags": FORM_FLAGS[form] | (l2_acc if metric == SCAN_L2 else 0), "i8_flags": 0}
    if cls == "F":      # cosine: only the int8 shadow, so every batch size takes the tier; L2 on the tier needs the norms too
        out["shadows"] = ["bf16", "i8"] if metric == SCAN_L2 else ["i8"]
        out["i8_flags"] = I8_ROTATED if form == "rotated" else 0
    else:
        out["shadows"] = ["bf16"] if cls in "CDE" and form != "bare" else []
    return out


def fixed_draw(cls, form, metric, dim, n=4097, nq=17, k=10, seed=1, thr=-1.0, tie=True, mask=False, offset=None, l2_acc=0, g0=0,
               mask_keep=None):
    """A scripted draw (tests/test_dim_lattice_gpu.py): the same dict draw_case returns."""
    d = {"case": -1, "seed": seed, "cls": cls, "form": form, "metric": metric, "dim": dim, "n": n, "nq": nq, "k": k, "thr": thr,
         "mask": mask, "tie": tie, "offset": (4 if offset is None else offset) if cls == "B" else 0, "g0": g0}
    d.update(form_fields(cls, form, metric, l2_acc))
    if mask_keep is not None:
        d["mask_keep"] = mask_keep
    return d


def fits(n, dim, nq, k):
    nloc = (nq + 1) // 2
    planted = nloc * (k + 2 * (k // 4 + 2)) if dim >= 8 else 0
    return n * dim * nq <= MAX_WORK and planted <= 0.6 * n


def draw_case(rng, i, cell_list=None):
    """The draw of case i: plain numbers and strings (the JSON line of a failure is this dict).  The cell follows from i, the
    dim cycles through the cell's dims; everything else is drawn."""
    cell_list = cell_list or cells()
    cls, form, metric = cell_list[i % len(cell_list)]
    rnd = i // len(cell_list)
    dims = [d for d in CLASSES[cls] if form_applies(cls, form, d, metric)]
    if cls == "F" and form == "rotated":       # one transform (dim a power of two) and two overlapping ones, in turn
        dims = [x for x in dims if (x & (x - 1) == 0) == (rnd % 2 == 0)]
    dim = dims[int(rng.integers(0, len(dims)))]
    d = {"case": i, "seed": int(rng.integers(1, 1 << 30)), "cls": cls, "form": form, "metric": metric, "dim": int(dim)}
    ns = [n for n in NS if dim < 2048 or n <= 4223]
    for _ in range(64):
        n, nq, k = int(rng.choice(ns)), int(rng.choice(NQS)), int(rng.choice(KS))
        if fits(n, dim, nq, k):
            break
    else:
        n, nq, k = 4096, 1, 10
    d.update(n=n, nq=nq, k=k)
    d["thr"] = float(rng.choice(THRESHOLDS))
    d["mask"] = bool(rng.random() < 0.15)
    if rnd % 2 == 1 and cls == "E" and form in ("default", "bare") and metric == SCAN_COSINE:
        # the fused small scan answers (dim % 32 == 0, dim <= 1024, nq <= 16, ceil(n / 256) * k <= 1024): drawn on purpose here,
        # counted under `fused`, and never expected to show a filter
        small = [x for x in CLASSES[cls] if x <= 1024]
        d.update(dim=int(small[int(rng.integers(0, len(small)))]), nq=1, k=int(rng.choice([1, 10])), mask=False)
    d["tie"] = bool(rng.random() < 0.5)
    d["offset"] = int(B_OFFSETS[rnd % 3]) if cls == "B" else 0
    acc = L2_ACCS[(rnd + "ABCDE".index(cls)) % len(L2_ACCS)] if metric == SCAN_L2 and cls != "F" else 0
    d.update(form_fields(cls, form, metric, acc))
    if cls == "F" and form == "rotated":
        d["mask"] = False                      # (an allow-mask this small goes to the exhaustive path: the layout would not be scanned)
    d["g0"] = int(rng.integers(0, len(G_KINDS)))
    return d


class Case:
    pass


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


# (a, b, g) of the planted families.  Cosine is scale-free; under L2 the W and D rows are normalised and the Z rows have
# norm 0.55 (every squared norm stays within a factor of four: the int8 tier's L2 form takes such shards).
#   cosine  W (.975 a + .2236 b) / sqrt(a^2 + b^2 + g^2): .496 .. .567, G twice .700 .. .783, G dropped .212
#           D .4699, G twice .7215;  Z .2169
#   L2      W d^2 .254 .. .287, G twice .749 .. .776, G dropped 1.2 .. 1.22;  D .6956, G twice .7337;  Z 1.056
FAMILY = {
    SCAN_COSINE: {"W": ((1.0, 1.3), (3.0, 3.0), 1.0), "D": ((0.54, 0.56), (0.0, 0.0), 1.0), "Z": ((0.0, 0.0), (3.9, 4.1), 1.0)},
    SCAN_L2: {"W": ((0.97, 1.05), (S05, S05), 0.6), "D": ((0.44, 0.46), (0.0, 0.0), 0.5), "Z": ((0.0, 0.0), (0.9, 1.1), 0.1)},
}


def build_case(d):
    """The corpus, the queries and what was planted, from the draw's numbers alone."""
    n, dim, nq, k, metric = d["n"], d["dim"], d["nq"], d["k"], d["metric"]
    rng = np.random.default_rng([d["seed"], n, dim, nq, k])
    c = Case()
    c.d = d
    corpus = rng.standard_normal((n, dim), dtype=np.float32)
    corpus /= np.sqrt(np.einsum("ij,ij->i", corpus, corpus))[:, None]
    queries = _unit(rng.standard_normal((nq, dim)))
    c.localised, c.groups, c.kinds, c.planted = [], {}, {}, {}
    if dim >= 8:
        c.localised = list(range(0, nq, 2))                      # every second query, the first one included
        kinds = [kd for kd in G_KINDS if group(dim, kd) is not None]
        free = rng.permutation(n)
        edge = 64 * int(rng.integers(1, n // 64))
        special = [0, n - 1, edge - 1, edge]                       # the corpus's ends and both sides of a 64-row block edge
        free = [r for r in free.tolist() if r not in special]
        m = k // 4 + 2
        if dim < 128:                   # (one group for the whole case: another group's u_R would lie on this one's G)
            kinds = [kinds[d["g0"] % len(kinds)]]
            g0, gl = group(dim, kinds[0])
            c.localised = c.localised[:min(9, gl, dim - gl - 2)]     # (few: the random rows have to keep off them, see below)
            # ... and their u_G, u_R orthonormal sets: a row planted for one scores ~0 with the others
            ortho_g = np.linalg.qr(rng.standard_normal((gl, gl)))[0].T
            ortho_r = np.linalg.qr(rng.standard_normal((dim - gl, dim - gl)))[0].T
        plant, tiny = [], {}
        for t, qi in enumerate(c.localised):
            # a group of fewer than 8 elements (the tail of dim 129 is ONE element) takes at most as many queries as it has
            # directions, their u_G orthonormal: two parallel u_G would share their D rows
            for step in range(len(kinds)):
                kind = kinds[(d["g0"] + t + step) % len(kinds)]
                g0, gl = group(dim, kind)
                if dim < 128 or gl >= 8 or len(tiny.setdefault(kind, [])) < gl:
                    break
            on = np.zeros(dim, bool); on[g0:g0 + gl] = True
            if dim < 128:
                ug_on = ortho_g[t]
            elif gl >= 8:
                ug_on = _unit(rng.standard_normal(gl))
            else:
                if not tiny[kind]:
                    tiny[kind + "/basis"] = np.linalg.qr(rng.standard_normal((gl, gl)))[0].T
                ug_on = tiny[kind + "/basis"][len(tiny[kind])]
                tiny[kind].append(qi)
            ug = np.zeros(dim); ug[on] = ug_on
            ur = np.zeros(dim); ur[~on] = ortho_r[t] if dim < 128 else _unit(rng.standard_normal(dim - gl))
            queries[qi] = S95 * ug + S05 * ur
            cnt = k + 2 * m
            take = []
            if t == 0:
                take, special = special[:min(k, 4)], special[min(k, 4):]
            elif special:
                take, special = special[:1], special[1:]
            rows = np.array(take + [free.pop() for _ in range(cnt - len(take))], np.int64)
            z = rng.standard_normal((cnt, dim))
            z[:, on] = 0.0                                          # (off G: what G carries of a planted row is a u_G alone)
            z -= np.outer(z @ ur, ur)
            z = _unit(z)
            fam = FAMILY[metric]
            aw = rng.uniform(*fam["W"][0], k)
            aw[0] = fam["W"][0][0]                                  # the weakest W row sits at the family's lower end
            a = np.concatenate([aw, rng.uniform(*fam["D"][0], m), rng.uniform(*fam["Z"][0], m)])
            b = np.concatenate([rng.uniform(*fam["W"][1], k), rng.uniform(*fam["D"][1], m), rng.uniform(*fam["Z"][1], m)])
            g = np.concatenate([np.full(k, fam["W"][2]), np.full(m, fam["D"][2]), np.full(m, fam["Z"][2])])
            x = _unit(a[:, None] * ug + b[:, None] * ur + g[:, None] * z)
            if metric == SCAN_L2:
                x[k + m:] *= 0.55
            plant.append((rows, x))
            c.groups[qi], c.kinds[qi], c.planted[qi] = (g0, gl), kind, rows[:k]
        if dim < 128:
            # the best of ~4000 random rows of a small dim (cosine up to 3.9 / sqrt(dim)) reaches into the planted scores, and
            # a row that G carries survives G counted twice: the random rows are redrawn until none is within 0.3 of a
            # localised query — which takes FEW localised queries: at most 9 below dim 128 (fewer where the group or its complement
            # has fewer directions), the others are dense
            ql = _unit(queries[c.localised])
            for _ in range(64):
                near = np.flatnonzero((corpus @ ql.T).max(axis=1) > 0.3)
                if len(near) == 0:
                    break
                corpus[near] = _unit(rng.standard_normal((len(near), dim)))
            else:
                corpus[near] = -_unit(ql.sum(axis=0))[None, :]
        for rows, x in plant:
            corpus[rows] = x
    if metric == SCAN_COSINE:                                       # cosine is scale-free: rows and queries of any length
        corpus *= rng.uniform(0.5, 2.0, (n, 1)) * float(rng.choice([0.25, 1.0, 3.0]))
        queries *= rng.uniform(0.5, 2.0, (nq, 1))
    c.corpus = np.ascontiguousarray(corpus, np.float32)
    c.queries = np.ascontiguousarray(queries, np.float32)
    c.tie = rng.permutation(n).astype(np.uint32) if d["tie"] else None
    c.allowed = np.flatnonzero(rng.random(n) < d.get("mask_keep", rng.uniform(0.3, 0.95))) if d["mask"] else None
    if c.allowed is not None:                                       # a planted row stays a row of the search
        keep = np.zeros(n, bool); keep[c.allowed] = True
        for rows in c.planted.values():
            keep[rows] = True
        keep[[0, n - 1]] = True
        c.allowed = np.flatnonzero(keep)
    return c


def aligned(d):
    return d["offset"] == 0


def route(d, n_allowed):
    return restated_route(d["dim"], aligned(d), set(d["shadows"]), d["nq"], d["k"], d["metric"], d["flags"], d["n"], n_allowed)


def oracle_query(o, c, qi, flags=None):
    """(rows, sims, dist | None) of query qi in the corpus's own row ordinals, from the single-query oracle functions."""
    d = c.d
    flags = d["flags"] if flags is None else flags
    n = c.corpus.shape[0]
    sel = np.arange(n) if c.allowed is None else c.allowed
    sub = c.corpus if c.allowed is None else c.corpus[sel]
    if d["metric"] == SCAN_COSINE:
        rank = None if c.tie is None else c.tie.astype(np.uint64)[sel]
        r = o.scan_cosine(sub, c.queries[qi], d["k"], d["thr"], rank)
        assert r is not None, "the lattice draws valid queries only"
        return sel[r[0]], r[1], None
    lanes = ACC_LANES.get(flags & se.FLAG_L2_ACC_MASK)
    if lanes:
        r = o.scan_l2_f32acc(sub, c.queries[qi], d["k"], d["thr"], None, lanes=-lanes if (flags & FLAG_L2_ACC_FUSED) else lanes)
    else:
        r = o.scan_l2(sub, c.queries[qi], d["k"], d["thr"], None)     # (the chunk-id ranking belongs to the cosine comparator only)
    return sel[r[0]], r[2], r[1]


def _top_sets(o, corpus, queries, k, metric):
    """The top-k row SET of every query (no threshold, no tie rank: the planted scores are distinct)."""
    if len(queries) >= 8:
        many = o.scan_cosine_many(corpus, queries, k, -1.0) if metric == SCAN_COSINE else o.scan_l2_many(corpus, queries, k)
        cnt = many[2] if metric == SCAN_COSINE else many[3]
        return [frozenset(many[0][i, :cnt[i]].tolist()) for i in range(len(queries))]
    if metric == SCAN_COSINE:
        return [frozenset(o.scan_cosine(corpus, q, k, -1.0)[0].tolist()) for q in queries]
    return [frozenset(o.scan_l2(corpus, q, k, -1.0)[0].tolist()) for q in queries]


def discriminates(o, c):
    """None when, for EVERY localised query of the case, the oracle's top-k row set changes when the rows' elements on the
    query's group are zeroed AND when they are counted twice; else what does not.  The oracle alone decides.  (The
    planted W rows must also BE the oracle's top k of the untouched corpus: that is the design.)"""
    d = c.d
    k, metric = d["k"], d["metric"]
    by_group = {}
    for qi in c.localised:
        by_group.setdefault(c.groups[qi], []).append(qi)
    for (g0, gl), qis in by_group.items():
        q = c.queries[qis]
        base = _top_sets(o, c.corpus, q, k, metric)
        for j, qi in enumerate(qis):
            if base[j] != frozenset(c.planted[qi].tolist()):
                return "q%d (%s): the planted rows are not the oracle's top %d" % (qi, c.kinds[qi], k)
        saved = c.corpus[:, g0:g0 + gl].copy()
        try:
            for name, factor in (("zeroed", 0.0), ("counted twice", 2.0)):
                c.corpus[:, g0:g0 + gl] = saved * np.float32(factor)
                got = _top_sets(o, c.corpus, q, k, metric)
                for j, qi in enumerate(qis):
                    if got[j] == base[j]:
                        return "q%d (%s at %d+%d): the top-%d set survives its group %s" % (qi, c.kinds[qi], g0, gl, k, name)
        finally:
            c.corpus[:, g0:g0 + gl] = saved
    return None


def pick_queries(rng, nq, localised, limit=8):
    """The queries of a case that go through the CPU oracle: all of them up to `limit`; else the first, the last, one on each
    side of 64 and 128 where those exist, at least three localised ones, the rest drawn."""
    if nq <= limit:
        return list(range(nq))
    picks = [0, nq - 1] + [x for x in (63, 64, 127, 128) if x < nq - 1]
    picks = picks[:limit]
    loc = [q for q in localised if q in picks]
    others = [q for q in localised if q not in picks]
    while len(loc) < 3 and others:
        q = others.pop(int(rng.integers(0, len(others))))
        loc.append(q)
        if len(picks) < limit:
            picks.append(q)
        else:                                                       # replace a pick that is not localised (never the first or last)
            for j in range(len(picks) - 1, 1, -1):
                if picks[j] not in localised:
                    picks[j] = q
                    break
    while len(picks) < limit:
        q = int(rng.integers(0, nq))
        if q not in picks:
            picks.append(q)
    return sorted(set(picks))


def compare_query(qi, count, rows, scores, dist, expected, k, metric):
    """One query's device answer (count, rows [k], scores [k], dist [k] | None) against the oracle's (rows, sims, dist | None),
    as tests/test_scan_gpu.py check does and _score_edges.compare states it: the count, the row ids in order, the score bits,
    the distance bits under L2, -1 / -inf / +inf behind the count.  None, or the first difference."""
    msg = se.compare(np.array([count]), np.asarray(rows)[None, :k], np.asarray(scores)[None, :k],
                     None if dist is None else np.asarray(dist)[None, :k], 0, [expected], k, metric, 0)
    return None if msg is None else "q%d%s" % (qi, msg[2:])


def compare_calls(a, b, k, metric):
    """Two device answers of one batch (ScanResult-like: counts, rows, scores, dist) bit for bit, every query."""
    for qi in range(len(a.counts)):
        ca = int(a.counts[qi])
        if ca != int(b.counts[qi]):
            return "q%d: count %d != %d (the exhaustive path)" % (qi, ca, int(b.counts[qi]))
        if not np.array_equal(a.rows[qi], b.rows[qi]):
            j = int(np.flatnonzero(a.rows[qi] != b.rows[qi])[0])
            return "q%d: row[%d] %d != %d (the exhaustive path)" % (qi, j, a.rows[qi, j], b.rows[qi, j])
        if not np.array_equal(a.scores[qi].view(np.uint32), b.scores[qi].view(np.uint32)):
            return "q%d: score bits differ from the exhaustive path" % qi
        if metric == SCAN_L2 and not np.array_equal(a.dist[qi].view(np.uint32), b.dist[qi].view(np.uint32)):
            return "q%d: distance bits differ from the exhaustive path" % qi
    return None
