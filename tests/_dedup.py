"""Shared pieces of the dedup-set tests (tests/test_dedup_gpu.py, tests/stress_dedup.py).

walk() is the oracle: a Python set walked in order, which is what ContentStore::store does with storage_->exists()
(src/api/content_store_impl.cpp:246-287): chunk i is new iff its hash is neither in the store nor carried by an earlier
chunk of the same walk.

digest() builds 32-byte values whose slot geometry is known: the table's home slot of a digest d (four little-endian
64-bit words) is (d[1] ^ (d[0] >> 17)) & (capacity - 1) (dedup_home in yams_amd/csrc/dedup_kernels.hip), and its tag is
d[0] (0 maps to 1).  digest(tag_word, home, salt) sets d[0] = tag_word and d[1] = (tag_word >> 17) ^ home, so for
home < 1024 the home slot is `home` at every capacity the set can have (1024 ... 2^31) and the geometry survives
rehashes; home = LAST lands on slot capacity - 1 at every capacity, so probing wraps to slot 0.  d[2], d[3] come from
the salt: equal (tag, home, salt) give equal digests, different salts different ones.
"""
import numpy as np

M64 = (1 << 64) - 1
LAST = -1                       # home of the last slot at every capacity
MIN_CAPACITY, MAX_CAPACITY = 1 << 10, 1 << 31


def walk(store: set, digests: np.ndarray) -> np.ndarray:
    out = np.zeros(len(digests), bool)
    for i, d in enumerate(digests):
        b = d.tobytes()
        if b not in store:
            store.add(b)
            out[i] = True
    return out


def _mix(x):
    """splitmix64 finaliser (a bijection of uint64), vectorised."""
    x = np.asarray(x, np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def digests(tag_words, homes, salts) -> np.ndarray:
    """[n][32] uint8: digest(tag_words[i], homes[i], salts[i]) for every i (arrays broadcast)."""
    t, h, s = np.broadcast_arrays(np.asarray(tag_words, np.uint64),
                                  np.asarray(homes, np.int64), np.asarray(salts, np.uint64))
    hv = np.where(h == LAST, np.int64(0xFFFFFFFF), h).astype(np.uint64)
    w = np.empty((t.size, 4), np.dtype("<u8"))
    w[:, 0] = t.ravel()
    w[:, 1] = (t.ravel() >> np.uint64(17)) ^ hv.ravel()
    w[:, 2] = _mix(s.ravel())
    w[:, 3] = _mix(s.ravel() ^ np.uint64(0x5DEECE66D))
    return w.view(np.uint8).reshape(-1, 32)


def digest(tag_word: int, home: int, salt: int) -> np.ndarray:
    """One 32-byte digest (uint8[32]) with tag tag_word (0 acts as 1) and home slot `home` (see the module doc)."""
    return digests([tag_word], [home], [salt])[0]


def home_of(d: np.ndarray, capacity: int) -> int:
    """The table's home slot of one digest at one capacity (the formula of dedup_home)."""
    w = np.asarray(d, np.uint8).view("<u8")
    return int((int(w[1]) ^ (int(w[0]) >> 17)) & (capacity - 1))


def tag_of(d: np.ndarray) -> int:
    t = int(np.asarray(d, np.uint8).view("<u8")[0])
    return t if t else 1


# ---- families (rows are distinct unless a salt repeats) ------------------------------------------------------------
def same_home(tag_word, home, k, salt0):
    """k digests with one tag and one home."""
    return digests(tag_word, home, np.arange(salt0, salt0 + k))


def adjacent_homes(tag_word, home0, homes, k, salt0, rng=None):
    """k digests with one tag; homes home0 .. home0 + homes - 1, in turn (or drawn from them with rng)."""
    off = np.arange(k) % homes if rng is None else rng.integers(0, homes, k)
    return digests(tag_word, home0 + off, np.arange(salt0, salt0 + k))


def tag01(home, k, salt0):
    """k digests at one home whose first words alternate 0 and 1: all carry tag 1."""
    return digests(np.arange(k) % 2, home, np.arange(salt0, salt0 + k))


def wrap(tag_word, k, salt0, spill=0):
    """k digests with one tag at home LAST, plus `spill` more of that tag at homes 0, 1, ... (the wrapped run)."""
    a = digests(tag_word, LAST, np.arange(salt0, salt0 + k))
    if not spill:
        return a
    return np.concatenate([a, digests(tag_word, np.arange(spill), np.arange(salt0 + k, salt0 + k + spill))])


def near_misses(d: np.ndarray) -> np.ndarray:
    """For every row, three digests with its tag and home that differ in one byte: the top byte of word 1 (outside the
    home mask at every capacity) and one byte each of words 2 and 3."""
    d = np.asarray(d, np.uint8).reshape(-1, 32)
    out = np.repeat(d, 3, axis=0)
    out[0::3, 15] ^= 0x80
    out[1::3, 19] ^= 0x01
    out[2::3, 30] ^= 0x10
    return out


# ---- capacity rule (dedup_api.cpp: capacity_for / ensure_room) ------------------------------------------------------
def capacity_for(entries: int) -> int:
    want, c = max(MIN_CAPACITY, entries * 2), MIN_CAPACITY
    while c < want:
        c <<= 1
    return min(c, MAX_CAPACITY)


def capacity_after(capacity: int, count: int, incoming: int) -> int:
    """The table's capacity once an insert of `incoming` digests into a set of `count` entries has made room."""
    need = count + incoming
    return capacity if need * 2 <= capacity else capacity_for(need * 2)


class Checked:
    """A DedupSet next to its oracle.  insert() compares is_new with walk() and then runs check(): probe is true for
    every digest ever inserted, false for the near misses of all of them, and len() equals the oracle's size."""

    def __init__(self, s):
        self.s, self.store = s, set()

    def keys(self) -> np.ndarray:
        if not self.store:
            return np.zeros((0, 32), np.uint8)
        return np.frombuffer(b"".join(self.store), np.uint8).reshape(-1, 32)

    def insert(self, d, what=""):
        d = np.ascontiguousarray(d, np.uint8).reshape(-1, 32)
        got = self.s.insert(d)
        exp = walk(self.store, d)
        assert np.array_equal(got, exp), (what, np.flatnonzero(got != exp)[:20], got.astype(int)[:20], exp.astype(int)[:20])
        self.check(what)
        return got

    def check(self, what=""):
        k = self.keys()
        assert self.s.probe(k).all(), (what, "stored digests not found", np.flatnonzero(~self.s.probe(k))[:20])
        near = near_misses(k)
        exp = np.array([b.tobytes() in self.store for b in near], bool)
        assert np.array_equal(self.s.probe(near), exp), (what, "near misses")
        assert len(self.s) == len(self.store), (what, len(self.s), len(self.store))
