"""Planted winners at every row position and query slot of the exact scan's filter forms: the plain design.

The filter of the exact scan lists candidate rows per query; only listed rows are re-scored and the completeness proof reasons
about listed rows alone, so a row a filter kernel never scores (a dropped row position, a dropped query slot, a ragged tail, a
sample tile, a masked word boundary) cannot fail a proof: it is simply absent.  Random data puts a given row into a top k with
probability k / n.  Here EVERY row is a winner whose whole answer is known by construction:

  self     query j is row perm[j] bit for bit; k = 10, cosine threshold 0.9: one hit, that row, score oracle.cosine(row, row)
           (under L2: distance bits of 0.0, the same cosine, the threshold after the top k by distance: one hit again);
  twins    rows h .. 2h - 1 (h = n // 2) are copies of rows 0 .. h - 1 under a second permutation, a tie-rank permutation is
           attached: two hits, ascending tie rank, identical score bits (an odd n keeps one single row: one hit);
  masked   the twins corpus behind an allow-mask that clears one twin of every pair: one hit, the surviving twin;
  medium   query j = 0.5 r + sqrt(0.75) w, r the unit row, w a seeded unit vector orthogonalised against it in fp64; threshold
           -1, k = 10: rank 1 is the planted row at similarity 0.5 (a filter whose bound is 30 % low at some position loses a
           winner at 0.5 against a threshold near 0.15, it would not lose one at 1.0); ranks 2 .. k come from the full oracle for
           24 queries spread over the batch.

That no other row comes near (off-diagonal cosine below 0.8; medium: every other row below the planted one) is a condition
asserted on the CPU from the inputs (tests/test_scan_positions_cpu.py), not by an O(n^2) oracle.

The geometry below restates yams_amd/csrc/scan_api.cpp make_plan (:34-68) and yams_amd/csrc/scan_i8_kernel.hip
i8_resident_plan (:1886-1915) ONLY to choose shapes and to assert what they reach; the product never reads it.  The plan code
includes the HIP runtime (common.h:3; i8_resident_plan asks the device for its CU count), so it cannot be compiled into a plain
host program and is not pinned that way: the GPU test holds each shape to the diagnostics the entry returns instead (path,
filter_tier, candidate counts).  No GPU and no torch are needed here."""
import functools
from math import gcd

import numpy as np

TILE_ROWS = 256        # rows of a filter tile on the bf16 / int8 tiers (scan_api.cpp:37; common.h:38), 128 for the exact-f32 kernel
F32_TILE_ROWS = 128    # common.h:24 kTileRows
BLOCK_ROWS = 64        # rows sharing one int8 scale (yams_mi355x_accel.h: rows_i8_meta; scan_i8d_kernel.h:45)
GROUP_ROWS = 16        # rows under one sample group maximum (common.h:27)
QUERY_TILE = 128       # queries of one resident query tile / wave tile column (scan_i8_kernel.hip:1896 R_QUERIES)
SLICE_QUERIES = 1024   # the entry cuts batches that take the resident-query form into slices of 1024 (scan_api.cpp:917-929)
RESCORE_MAX = 2047     # scan_launch.h:90
MFMA_MIN_ROWS = 4096   # scan_api.cpp:23
MASK_MIN_ALLOWED = 16384   # an allow-mask that admits fewer rows takes the exhaustive path (yams_mi355x_accel.h, diag.path)
K, SELF_THR = 10, 0.9
MEDIUM_C = 0.5
NEG_INF_BITS, POS_INF_BITS = 0xFF800000, 0x7F800000


def _round_up(v, m):
    return (v + m - 1) // m * m


def plan(n, k=K, tile_rows=TILE_ROWS, single_pass=True, l2_band=False):
    """make_plan at depth 0 (scan_api.cpp:34-68): the tile geometry and the candidate budget."""
    n_tiles = -(-n // tile_rows)
    if single_pass:
        kprime = min(_round_up(6 * k + 128 if l2_band else 3 * k + 64, 32), RESCORE_MAX)     # :41-42
    else:
        kprime = min(_round_up(k + max(16, k // 4), 32), RESCORE_MAX)                       # :43
    s_target = min(n, max(n // 64, 8192))                                                   # :44
    want_tiles = max(1, -(-s_target // tile_rows))                                          # :45-46
    stride = max(1, n_tiles // want_tiles)                                                  # :47
    n_sample = -(-n_tiles // stride)                                                        # :48
    return dict(n=n, tile_rows=tile_rows, n_tiles=n_tiles, stride=stride, n_sample_tiles=n_sample,
                n_filter_tiles=n_tiles - n_sample, kprime=kprime, n_groups=n_sample * tile_rows // GROUP_ROWS)


def is_sample_tile(tile, stride):
    """Sample tile s is tile s * stride (scan_i8_kernel.hip:150)."""
    return tile % stride == 0


def filter_tile(sel, stride):
    """The renumbering of filter tiles around the sample tiles (scan_i8_kernel.hip:151, scan_i8d_kernel.h:56)."""
    return sel + sel // (stride - 1) + 1


def filter_tiles(p):
    return [t for t in range(p["n_tiles"]) if not is_sample_tile(t, p["stride"])]


def units(p):
    """The resident-query form's units: filter tiles 2u and 2u + 1 (scan_i8d_kernel.h:50-57).  [(first row, last row)] with
    the last row cut at the shard's end, and the number of tiles of the last unit."""
    ft = filter_tiles(p)
    out = []
    for u in range((len(ft) + 1) // 2):
        mine = ft[2 * u:2 * u + 2]
        out.append((mine[0] * p["tile_rows"], min(p["n"], (mine[-1] + 1) * p["tile_rows"]) - 1))
    return out, (2 - len(ft) % 2 if ft else 0)


def resident(p, nq, n_cu=256):
    """i8_resident_plan with the caller's RESIDENT_QUERIES flag (scan_i8_kernel.hip:1886-1915) on a 256-CU device."""
    per_xcd = n_cu // 8
    n_qt = -(-nq // QUERY_TILE)
    ok = 0 < n_qt <= per_xcd
    n_streams = per_xcd // n_qt * 8 if ok else 0
    return dict(use=ok and p["n_filter_tiles"] > 0, n_qt=n_qt, n_streams=n_streams, n_units=(p["n_filter_tiles"] + 1) // 2)


# ---- permutations -------------------------------------------------------------------------------------------------------
def tile_pins(n):
    """(row, slot) pairs the first permutation must hold: the first row of every 256-row tile is the winner of a query in slot
    0, its last row (cut at the shard's end) of a query in slot 127.  Unit boundaries are a subset of tile boundaries."""
    pins = []
    for t in range(-(-n // TILE_ROWS)):
        first, last = t * TILE_ROWS, min(n, (t + 1) * TILE_ROWS) - 1
        pins.append((first, 0))
        if last != first:
            pins.append((last, QUERY_TILE - 1))
    return pins


def wanted_class(j):
    """The row position mod 256 the structured permutation gives query j = 128 t + s: 64-row offset (s + t) mod 64 — for a
    fixed slot the offsets of 64 consecutive query tiles are all different — in quarter (s / 64 + 2 (t / 8 mod 2)) mod 4 of the
    tile, which does not depend on the slice-local tile t mod 8."""
    s, t = j & 127, j >> 7
    return 64 * (((s >> 6) + 2 * ((t >> 3) & 1)) & 3) + ((s + t) & 63)


def structured_perm(n, seed, pins=True):
    """A seeded bijection query -> row: every query gets a row of its wanted class mod 256 while that class has rows left
    (seeded choice), the remainder is matched at random; then the tile pins are set by swaps."""
    rng = np.random.default_rng(seed)
    cls = wanted_class(np.arange(n))
    perm = np.full(n, -1, np.int64)
    left_q, left_r = [], []
    for c in range(TILE_ROWS):
        qs = rng.permutation(np.flatnonzero(cls == c))
        rs = rng.permutation(np.arange(c, n, TILE_ROWS))
        m = min(len(qs), len(rs))
        perm[qs[:m]] = rs[:m]
        left_q.append(qs[m:]); left_r.append(rs[m:])
    left_q, left_r = np.concatenate(left_q), np.concatenate(left_r)
    perm[left_q] = rng.permutation(left_r)
    if pins:
        inv = np.empty(n, np.int64); inv[perm] = np.arange(n)
        pinned = np.zeros(n, bool)
        for row, slot in tile_pins(n):
            jq = int(inv[row])
            if jq % QUERY_TILE != slot:
                cand = np.arange(slot, n, QUERY_TILE)
                cand = cand[~pinned[cand]]
                j2 = int(cand[rng.integers(len(cand))])
                r2 = int(perm[j2])
                perm[j2], perm[jq] = row, r2
                inv[row], inv[r2] = j2, jq
                jq = j2
            pinned[jq] = True
        _fill_pairs(perm, inv, pinned, rng)
    assert np.array_equal(np.sort(perm), np.arange(n))
    return perm


def _fill_pairs(perm, inv, pinned, rng):
    """The classes do not divide evenly and the pins move a few rows: some (row mod 64, slot) pairs are left without a query.
    Each is filled by ONE swap between a query of that slot and the query that holds a row of that offset, both taken from pairs
    that occur at least twice and neither pinned (shards of fewer than 8192 rows cannot hold every pair: left as they are)."""
    n = len(perm)
    if n < BLOCK_ROWS * QUERY_TILE:
        return
    j = np.arange(n)
    count = np.zeros((BLOCK_ROWS, QUERY_TILE), np.int64)
    np.add.at(count, (perm % BLOCK_ROWS, j % QUERY_TILE), 1)
    for o, s in np.argwhere(count == 0):
        done = False
        for j1 in rng.permutation(np.arange(s, n, QUERY_TILE)):
            o1 = perm[j1] % BLOCK_ROWS
            if pinned[j1] or count[o1, s] < 2:
                continue
            for r in rng.permutation(np.arange(o, n, BLOCK_ROWS)):
                j2 = inv[r]; s2 = j2 % QUERY_TILE
                if pinned[j2] or s2 == s or count[o, s2] < 2:
                    continue
                r1 = perm[j1]
                perm[j1], perm[j2] = r, r1
                inv[r], inv[r1] = j1, j2
                count[o1, s] -= 1; count[o, s2] -= 1; count[o, s] += 1; count[o1, s2] += 1
                done = True
                break
            if done:
                break


def affine_perm(n, seed):
    """j -> (a j + b) mod n with a coprime to n (a near n / golden ratio: consecutive queries land far apart)."""
    a = int(n * 0.6180339887498949) | 1
    while gcd(a, n) != 1:
        a += 2
    b = int(np.random.default_rng(seed).integers(n))
    return (a * np.arange(n, dtype=np.int64) + b) % n


def coverage(perms, n):
    """What the permutations reach together, on the test's own indices: {all_rows, pairs64 (of 8192: row mod 64 x query mod
    128), pairs256 (of 2048: row mod 256 x slice-local query tile), pins (tile pins the FIRST permutation holds, of how many)}."""
    j = np.arange(n)
    p64 = np.zeros(BLOCK_ROWS * QUERY_TILE, bool)
    p256 = np.zeros(TILE_ROWS * (SLICE_QUERIES // QUERY_TILE), bool)
    for perm in perms:
        p64[(perm % BLOCK_ROWS) * QUERY_TILE + j % QUERY_TILE] = True
        p256[(perm % TILE_ROWS) * (SLICE_QUERIES // QUERY_TILE) + (j % SLICE_QUERIES) // QUERY_TILE] = True
    inv = np.empty(n, np.int64); inv[perms[0]] = j
    pins = tile_pins(n)
    held = sum(1 for row, slot in pins if inv[row] % QUERY_TILE == slot)
    return dict(all_rows=all(np.array_equal(np.sort(p), j) for p in perms), pairs64=int(p64.sum()), pairs256=int(p256.sum()),
                pins=held, n_pins=len(pins))


def assert_coverage(perms, n):
    c = coverage(perms, n)
    assert c["all_rows"], c
    assert c["pairs64"] == BLOCK_ROWS * QUERY_TILE, c
    assert c["pairs256"] == TILE_ROWS * (SLICE_QUERIES // QUERY_TILE), c
    assert c["pins"] == c["n_pins"], c
    return c


# ---- the shapes and forms ---------------------------------------------------------------------------------------------
N_A = 161 * 256 + 1    # 41 217: 162 tiles, stride 5, 129 filter tiles -> 65 units, the last of ONE tile; its last 64-row block holds one row
N_B = 160 * 256 + 70   # 41 030: 161 tiles, stride 5, the last tile (160) is a SAMPLE tile, ragged; 128 filter tiles
N_S = 65 * 256 + 1     # 16 641: 66 tiles of 256 (131 of 128), stride 2, a last tile of one row
N_X = 32 * 256 + 129   # 8 321: the exhaustive fp64 path (no tiles to reach)
N_M = 129 * 256 + 1    # 33 025: the smallest such shard whose masked half (16 513 rows) still takes the filter path
SEED = 7100

# flags / i8_flags by the names of yams_amd._lib; tier: diag.filter_tier; cases: which planted cases the form runs
FORMS = {f["name"]: f for f in [
    # resident-query int8 forms: scan_tiles_i8d_kernel at dims 384 / 768, scan_tiles_i8r_kernel at 512
    dict(name="i8d_384", n=N_A, dim=384, shadow="i8", flags=("FLAG_RESIDENT_QUERIES",), tier=1, cases=("self", "self2", "twins", "masked", "medium")),
    dict(name="i8r_512", n=N_A, dim=512, shadow="i8", flags=("FLAG_RESIDENT_QUERIES",), tier=1, cases=("self", "twins", "masked")),
    dict(name="i8d_768", n=N_B, dim=768, shadow="i8", flags=("FLAG_RESIDENT_QUERIES",), tier=1, cases=("self", "self2", "twins", "medium")),
    dict(name="i8d_768_rotated", n=N_B, dim=768, shadow="i8", i8_flags="I8_ROTATED", flags=("FLAG_RESIDENT_QUERIES",), tier=1, cases=("self", "masked")),
    # half tiles: the library's own choice on a small shard, dim % 64 == 0 and dim % 128 != 0
    dict(name="i8h_320", n=N_S, dim=320, shadow="i8", tier=1, cases=("self", "self2", "twins")),
    # bf16 tier, shadow in the view (launch_scan_bf16, scan_bf16_kernel.hip:1318-1372).  Dim 256, more than 128 queries: the
    # default is the persistent scan_tiles_bf16p_kernel (:1338-1351: 256 <= dim <= 512, cosine filter pass), WIDE_TILE the per-tile
    # scan_tiles_bf16s_kernel.  Dim 112 has 16-wide slabs: scan_tiles_bf16v2_kernel whatever the flag (:1398-), so it runs once.
    dict(name="bf16_wide_256", n=N_S, dim=256, shadow="bf16", flags=("FLAG_WIDE_TILE",), tier=2, cases=("self", "twins")),
    dict(name="bf16_112", n=N_S, dim=112, shadow="bf16", tier=2, cases=("self", "twins")),
    dict(name="bf16_256", n=N_S, dim=256, shadow="bf16", tier=2, cases=("self", "self2", "twins")),
    dict(name="bf16_256_masked", n=N_M, dim=256, shadow="bf16", tier=2, cases=("masked",)),
    # the narrow form scan_tiles_bf16n_kernel (:1357-1372): calls of <= 128 queries at a dim with 32-wide slabs OUTSIDE
    # [256, 512] (inside it the persistent kernel is chosen first).  128 queries per call: the 4-block filter form, the sample
    # pass on the 256-query form; 64 per call: the 2-block filter form and the narrow sample form; L2: narrow up to 64 queries.
    dict(name="bf16n_192_q128", n=N_S, dim=192, shadow="bf16", per_call=128, tier=2, cases=("self", "twins")),
    dict(name="bf16n_192_q64", n=N_S, dim=192, shadow="bf16", per_call=64, tier=2, cases=("self", "twins")),
    dict(name="l2_bf16n_192_q64", n=N_S, dim=192, shadow="bf16", metric="l2", per_call=64, tier=2, cases=("self",)),
    # dim 100 is no multiple of 16: choose_filter (scan_api.cpp:434) gives it the exact-f32 kernel whatever the shadow
    dict(name="f32_100_row_base", n=N_S, dim=100, shadow="bf16", tier=4, tile_rows=F32_TILE_ROWS, row_base=(1 << 33) + 5, cases=("self", "twins")),
    dict(name="f32_20", n=N_S, dim=20, shadow=None, flags=("FLAG_F32_FILTER",), tier=4, tile_rows=F32_TILE_ROWS, cases=("self", "twins")),
    dict(name="split_256", n=N_S, dim=256, shadow="bf16", flags=("FLAG_SPLIT_FILTER",), tier=3, single_pass=False, cases=("self", "twins")),
    dict(name="exact_100", n=N_X, dim=100, shadow=None, flags=("FLAG_FORCE_EXACT",), tier=0, path=1, cases=("self", "twins")),
    # L2 (vec0): int8 tier with both shadows (L2 batches take scan_tiles_i8r_kernel at every dim, scan_i8_kernel.hip:2084-2096),
    # bf16 tier; fp64 accumulation and the 8-lane fp32 form
    dict(name="l2_i8r_384", n=N_A, dim=384, shadow="both", metric="l2", flags=("FLAG_RESIDENT_QUERIES",), tier=1, cases=("self",)),
    dict(name="l2_bf16_256", n=N_S, dim=256, shadow="bf16", metric="l2", tier=2, cases=("self",)),
    dict(name="l2_bf16_256_f32x8", n=N_S, dim=256, shadow="bf16", metric="l2", flags=("FLAG_L2_ACC_F32X8",), l2_lanes=8, tier=2, cases=("self",)),
]}
RESIDENT_FORMS = ("i8d_384", "i8r_512", "i8d_768", "i8d_768_rotated", "l2_i8r_384")
PARAMS = [(name, case) for name, f in FORMS.items() for case in f["cases"]]


def form_plan(f, n=None):
    return plan(n or f["n"], K, f.get("tile_rows", TILE_ROWS), f.get("single_pass", True), f.get("metric") == "l2" and f["tier"] != 1)


# ---- the planted cases -------------------------------------------------------------------------------------------------
class Case:
    """One planted case: inputs, and for every query the expected count, rows, score bits (distance bits under L2); `known`
    marks the slots below the count whose row and bits are known by construction (all of them but ranks 2 .. k of most medium
    queries)."""
    def __init__(self, **kw):
        self.tie_rank = self.mask = self.exp_dist_bits = None
        self.row_base, self.metric, self.l2_lanes = 0, "cosine", 1
        self.__dict__.update(kw)


THIN_BELOW_DIM, THIN_COS = 64, 0.75


def thinned_rows(oracle, n, dim):
    """Random rows of a small dimension crowd: among 16 641 rows of dim 20 thousands of pairs lie above cosine 0.8.  The first n
    rows of the synthetic stream that stay below THIN_COS with every row kept before them (greedy, in stream order)."""
    kept = np.empty((n, dim), np.float32)
    unit = np.empty((n, dim), np.float32)
    m, row0, step = 0, 0, 512
    while m < n:
        cand = oracle.synth_rows(SEED, row0, step, dim); row0 += step
        cu = cand / np.linalg.norm(cand, axis=1, keepdims=True)
        ok = (cu @ unit[:m].T).max(1) < THIN_COS if m else np.ones(step, bool)
        inner = cu @ cu.T
        for i in np.flatnonzero(ok):
            if m < n and not (inner[i, :i][ok[:i]] >= THIN_COS).any():
                kept[m], unit[m] = cand[i], cu[i]; m += 1
            else:
                ok[i] = False
    return kept


@functools.lru_cache(maxsize=2)
def self_corpus(oracle, n, dim):
    """n distinct random rows and the bits of each row's similarity with itself."""
    corpus = oracle.synth_rows(SEED, 0, n, dim) if dim >= THIN_BELOW_DIM else thinned_rows(oracle, n, dim)
    bits = np.array([np.float32(oracle.cosine(r, r)) for r in corpus], np.float32).view(np.uint32)
    corpus.setflags(write=False); bits.setflags(write=False)
    return corpus, bits


@functools.lru_cache(maxsize=2)
def twins_corpus(oracle, n, dim):
    """Rows h .. 2h - 1 are rows 0 .. h - 1 under a seeded permutation (row 2h of an odd n stays single); (corpus, twin_of
    (-1 for the single row), tie_rank, self-similarity bits)."""
    base, bits = self_corpus(oracle, n, dim)
    h = n // 2
    rng = np.random.default_rng(SEED + 1)
    sigma = rng.permutation(h)
    corpus = base.copy()
    corpus[h:2 * h] = base[sigma]
    twin = np.full(n, -1, np.int64)
    twin[h:2 * h] = sigma; twin[sigma] = np.arange(h, 2 * h)
    b2 = bits.copy(); b2[h:2 * h] = bits[sigma]
    tie_rank = rng.permutation(n).astype(np.uint32)
    for a in (corpus, twin, tie_rank, b2):
        a.setflags(write=False)
    return corpus, twin, tie_rank, b2


def twin_mask(n, twin, seed=SEED + 2):
    """Allow-mask over the twins corpus: one twin of every pair cleared (seeded which), the single row kept.  Mask words 0, 1,
    the last whole word and the ragged last word (when there is one) are forced to hold cleared AND kept bits."""
    rng = np.random.default_rng(seed)
    h = n // 2
    keep = np.ones(n, bool)
    first_cleared = rng.random(h) < 0.5
    lo = np.flatnonzero(twin[:h] >= 0)
    keep[lo[first_cleared[lo]]] = False
    keep[twin[lo[~first_cleared[lo]]]] = False
    words = boundary_words(n)
    for w in words:
        rows = np.arange(32 * w, min(n, 32 * w + 32))
        rows = rows[twin[rows] >= 0]
        if keep[rows].all():
            keep[rows[0]] = False; keep[twin[rows[0]]] = True
        if not keep[rows].any():
            keep[rows[0]] = True; keep[twin[rows[0]]] = False
    for w in words:
        rows = np.arange(32 * w, min(n, 32 * w + 32))
        assert keep[rows].any() and not keep[rows].all(), w
    pairs = np.flatnonzero(twin >= 0)
    assert (keep[pairs] != keep[twin[pairs]]).all() and keep[twin < 0].all()
    return keep


def boundary_words(n):
    """Mask words 0 and 1, the last whole word, the ragged last word."""
    words = {0, 1, n // 32 - 1}
    if n % 32 > 1:                  # (a ragged word of one row cannot hold both kinds)
        words.add(n // 32)
    return sorted(words)


@functools.lru_cache(maxsize=2)
def medium_queries(oracle, n, dim):
    """Per ROW r: the query 0.5 r^ + sqrt(0.75) w^ (fp64, rounded to fp32), w^ seeded and orthogonal to r^."""
    corpus, _ = self_corpus(oracle, n, dim)
    out = np.empty((n, dim), np.float32)
    for i0 in range(0, n, 4096):
        r = corpus[i0:i0 + 4096].astype(np.float64)
        r /= np.linalg.norm(r, axis=1, keepdims=True)
        w = np.random.default_rng([SEED + 3, i0]).standard_normal(r.shape)
        w -= (w * r).sum(1, keepdims=True) * r
        w /= np.linalg.norm(w, axis=1, keepdims=True)
        out[i0:i0 + 4096] = (MEDIUM_C * r + np.sqrt(1.0 - MEDIUM_C * MEDIUM_C) * w).astype(np.float32)
    out.setflags(write=False)
    return out


def medium_full_queries(nq):
    """The 24 queries whose ranks 2 .. k are held to the full oracle: 0, 127, 128, 1023, the last, the rest spread evenly."""
    must = [q for q in (0, 127, 128, 1023, nq - 1) if 0 <= q < nq]
    spread = [int(x) for x in np.linspace(0, nq - 1, 24 + len(must)).round()]
    out = list(dict.fromkeys(must + spread))[:24]
    return sorted(out)


def perm_for(case, n):
    return affine_perm(n, SEED + 5) if case == "self2" else structured_perm(n, SEED + 4)


def make_case(oracle, f, case, n=None):
    n = n or f["n"]
    dim, metric = f["dim"], f.get("metric", "cosine")
    perm = perm_for(case, n)
    exp_rows = np.full((n, K), -1, np.int64)
    exp_bits = np.full((n, K), NEG_INF_BITS, np.uint32)
    known = np.zeros((n, K), bool)
    kw = dict(name=case, form=f["name"], perm=perm, k=K, metric=metric, row_base=f.get("row_base", 0), l2_lanes=f.get("l2_lanes", 1))
    if case in ("self", "self2"):
        corpus, bits = self_corpus(oracle, n, dim)
        exp_rows[:, 0] = perm; exp_bits[:, 0] = bits[perm]; known[:, 0] = True
        c = Case(corpus=corpus, queries=corpus[perm], thr=SELF_THR, exp_counts=np.ones(n, np.uint32), **kw)
        if metric == "l2":
            c.exp_dist_bits = np.full((n, K), POS_INF_BITS, np.uint32); c.exp_dist_bits[:, 0] = 0
    elif case in ("twins", "masked"):
        corpus, twin, tie_rank, bits = twins_corpus(oracle, n, dim)
        other = twin[perm]
        if case == "twins":
            pair = other >= 0
            first = np.where(pair & (tie_rank[np.maximum(other, 0)] < tie_rank[perm]), other, perm)
            exp_rows[:, 0] = first
            exp_rows[pair, 1] = (perm + other - first)[pair]
            exp_bits[:, 0] = bits[perm]; exp_bits[pair, 1] = bits[perm][pair]
            known[:, 0] = True; known[pair, 1] = True
            c = Case(corpus=corpus, queries=corpus[perm], thr=SELF_THR, tie_rank=tie_rank, exp_counts=(1 + pair).astype(np.uint32), **kw)
        else:
            keep = twin_mask(n, twin)
            exp_rows[:, 0] = np.where(keep[perm], perm, other)
            assert keep[exp_rows[:, 0]].all()
            exp_bits[:, 0] = bits[perm]; known[:, 0] = True
            c = Case(corpus=corpus, queries=corpus[perm], thr=SELF_THR, tie_rank=tie_rank, mask=keep, exp_counts=np.ones(n, np.uint32), **kw)
    elif case == "medium":
        corpus, _ = self_corpus(oracle, n, dim)
        queries = medium_queries(oracle, n, dim)[perm]
        exp_rows[:, 0] = perm; known[:, 0] = True
        exp_bits[:, 0] = np.array([np.float32(oracle.cosine(queries[j], corpus[perm[j]])) for j in range(n)], np.float32).view(np.uint32)
        full = medium_full_queries(n)
        rows, sims, counts = oracle.scan_cosine_many(corpus, queries[full], K, -1.0)
        assert (counts == K).all()
        exp_rows[full] = rows; exp_bits[full] = sims.view(np.uint32); known[full] = True
        c = Case(corpus=corpus, queries=queries, thr=-1.0, exp_counts=np.full(n, K, np.uint32), full=full, **kw)
    else:
        raise KeyError(case)
    c.exp_rows, c.exp_bits, c.known = exp_rows, exp_bits, known
    return c


# ---- the comparison ----------------------------------------------------------------------------------------------------
class Result:
    def __init__(self, counts, rows, scores, dist, diag):
        self.counts, self.rows, self.scores, self.dist, self.diag = counts, rows, scores, dist, diag


def where(case, q, tile_rows=TILE_ROWS):
    """The geometry a failing query names: its slot and slice-local tile, its planted row's position."""
    row = int(case.perm[q])
    return dict(query=int(q), slot=int(q % QUERY_TILE), slice_tile=int(q % SLICE_QUERIES // QUERY_TILE), planted_row=row,
                tile=row // tile_rows, row_in_tile=row % tile_rows, row_in_block=row % BLOCK_ROWS, mask_word=row // 32, mask_bit=row % 32)


def verify(case, res, f):
    """Every query of the result against the case: count, row ids, score bits, distance bits under L2, the padding of the
    unused slots (score -inf, row -1, distance +inf); then the diagnostics that say which form ran.  Returns the diagnostics
    worth recording."""
    nq, k = case.exp_rows.shape
    tr = f.get("tile_rows", TILE_ROWS)
    counts = np.asarray(res.counts).astype(np.int64)
    bad = np.flatnonzero(counts != case.exp_counts)
    assert bad.size == 0, ("count", len(bad), where(case, bad[0], tr), int(counts[bad[0]]), int(case.exp_counts[bad[0]]), res.rows[bad[0]].tolist(), res.diag)
    want_rows = np.where(case.exp_rows >= 0, case.exp_rows + case.row_base, -1)
    live = np.arange(k)[None, :] < counts[:, None]
    chk = case.known & live
    bad = np.flatnonzero(((res.rows != want_rows) & chk).any(1))
    assert bad.size == 0, ("rows", len(bad), where(case, bad[0], tr), res.rows[bad[0]].tolist(), want_rows[bad[0]].tolist(), res.diag)
    got_bits = np.ascontiguousarray(res.scores, np.float32).view(np.uint32)
    bad = np.flatnonzero(((got_bits != case.exp_bits) & chk).any(1))
    assert bad.size == 0, ("score bits", len(bad), where(case, bad[0], tr), got_bits[bad[0]].tolist(), case.exp_bits[bad[0]].tolist())
    dist_bits = np.ascontiguousarray(res.dist, np.float32).view(np.uint32)
    if case.exp_dist_bits is not None:
        bad = np.flatnonzero(((dist_bits != case.exp_dist_bits) & chk).any(1))
        assert bad.size == 0, ("distance bits", len(bad), where(case, bad[0], tr), dist_bits[bad[0]].tolist())
    pad = ~live
    assert (res.rows[pad] == -1).all(), ("row padding", np.argwhere(pad & (res.rows != -1))[0].tolist())
    assert (got_bits[pad] == NEG_INF_BITS).all(), ("score padding", np.argwhere(pad & (got_bits != NEG_INF_BITS))[0].tolist())
    assert (dist_bits[pad] == POS_INF_BITS).all(), ("distance padding", np.argwhere(pad & (dist_bits != POS_INF_BITS))[0].tolist())
    d = res.diag
    assert d["path"] == f.get("path", 0) and d["filter_tier"] == f["tier"], d
    assert d["exact_fallback_queries"] == 0, d          # (an exhaustive pass would hide a list that lost its row)
    return {x: d[x] for x in ("path", "filter_tier", "filter_candidates", "rescored_rows", "widened_queries", "escalated_queries",
                              "retried_queries", "exact_fallback_queries") if x in d}


def call_ranges(nq, per_call):
    """[(first query, count)] of the calls a form is driven by: one call, or calls of `per_call` queries starting at multiples
    of it — the last one moved back so that it is full too (a call of a few queries on a small shard takes the fused scan)."""
    if not per_call or nq <= per_call:
        return [(0, nq)]
    starts = list(range(0, nq - per_call + 1, per_call))
    if starts[-1] + per_call < nq:
        starts.append(nq - per_call)
    return [(s, per_call) for s in starts]


def drive(case, f, call):
    """Runs the case through `call(first query, count) -> Result` as the form is driven (one call, or calls of 128 queries)
    and assembles one Result; diagnostics: counters summed, path the largest, filter_tier of every call the same."""
    nq, k = case.exp_rows.shape
    out = Result(np.zeros(nq, np.uint32), np.zeros((nq, k), np.int64), np.zeros((nq, k), np.float32), np.zeros((nq, k), np.float32), {})
    for q0, c in call_ranges(nq, f.get("per_call")):
        r = call(q0, c)
        out.counts[q0:q0 + c], out.rows[q0:q0 + c], out.scores[q0:q0 + c], out.dist[q0:q0 + c] = r.counts, r.rows, r.scores, r.dist
        for key, v in r.diag.items():
            if key not in out.diag:
                out.diag[key] = v
            elif key == "filter_tier":
                assert out.diag[key] == v, (q0, r.diag)
            elif key == "path":
                out.diag[key] = max(out.diag[key], v)
            elif key not in ("used_exact_scan", "rows_visited_observed"):
                out.diag[key] += v
    return out


def stand_in(oracle, case, f, q0=0, count=None):
    """A device that answers from the CPU oracle, query by query: rehearses the expectations and the comparison code (at a
    reduced n); it proves nothing about the kernels."""
    k = case.k
    nq = case.exp_rows.shape[0] - q0 if count is None else count
    counts = np.zeros(nq, np.uint32)
    rows = np.full((nq, k), -1, np.int64)
    scores = np.full((nq, k), -np.inf, np.float32)
    dist = np.full((nq, k), np.inf, np.float32)
    corpus, ids, rank = case.corpus, None, None if case.tie_rank is None else case.tie_rank.astype(np.uint64)
    if case.mask is not None:
        ids = np.flatnonzero(case.mask)
        corpus = np.ascontiguousarray(corpus[ids]); rank = None if rank is None else rank[ids]
    for q in range(nq):
        query = case.queries[q0 + q]
        if case.metric == "cosine":
            r, s = oracle.scan_cosine(corpus, query, k, case.thr, rank)[:2]
            d = None
        elif case.l2_lanes == 1:
            r, d, s = oracle.scan_l2(corpus, query, k, case.thr)
        else:
            r, d, s = oracle.scan_l2_f32acc(corpus, query, k, case.thr, None, case.l2_lanes)
        c = len(r)
        counts[q] = c
        rows[q, :c] = (r if ids is None else ids[r]) + case.row_base
        scores[q, :c] = s
        if d is not None:
            dist[q, :c] = d
        elif c:
            dist[q, :c] = np.float32(1.0) - s
    diag = dict(path=f.get("path", 0), filter_tier=f["tier"], exact_fallback_queries=0)
    return Result(counts, rows, scores, dist, diag)
