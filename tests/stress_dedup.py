"""Randomised stress of the device digest set (yams_dedup_*) on the GPU against the oracle.  A case is a sequence of
calls on one set.  A call mixes random digests, repeats of earlier calls and repeats within the call, same-tag families
of 2-12 digests at homes inside a window a few slots wide (the tag sometimes shared with an earlier family, so chains
run through settled entries), wrap-around families at the last slot, tag-0/1 families, chains that grow past 66 slots,
and calls large enough to grow the table; it goes through the host or the device entry point (with chunk sizes).
Every call: is_new against walk() (tests/_dedup.py), then probe true for every digest ever inserted, false for the near
misses of all of them, len() equal to the oracle's size; device calls also n_new, bytes_new and bytes_deduped against
numpy sums.  Test infrastructure.

    python tests/stress_dedup.py [--cases 24] [--seed 1]

The summary counts what the drawn inputs contain (input-side: families of 3 or more, chains deeper than 66, wrap
families, calls predicted to grow the table by capacity_for, device calls with sizes) and the mismatches; exit 1 on any.
"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from _dedup import adjacent_homes, capacity_after, capacity_for, near_misses, same_home, tag01, walk, wrap
from yams_amd.accel import Accel

ap = argparse.ArgumentParser()
ap.add_argument("--cases", type=int, default=24)
ap.add_argument("--seed", type=int, default=1)
a = ap.parse_args()
rng = np.random.default_rng(a.seed)
acc = Accel(0, torch.cuda.current_stream().cuda_stream)
DEEP = 66                                     # the parent's round cap: chains longer than this used to fail
COUNTERS = ["families_3plus", "chains_deeper_than_66", "wrap_families", "growing_calls", "device_calls_with_sizes"]


def log_uniform(lo, hi):
    return lo - 1 + int(np.exp(rng.uniform(0.0, np.log(hi - lo + 2))))


def tag_word():
    return int(rng.integers(1, 1 << 63, dtype=np.int64)) * 2 + int(rng.integers(0, 2))


def to_device(arr, offset):
    raw = np.ascontiguousarray(arr).view(np.uint8).ravel()
    buf = torch.zeros(raw.size + offset + 64, dtype=torch.uint8, device="cuda")
    if raw.size:
        buf[offset:offset + raw.size] = torch.from_numpy(raw.copy()).cuda()
    return buf, buf.data_ptr() + offset


def after_call(s, store):
    keys = np.frombuffer(b"".join(store), np.uint8).reshape(-1, 32) if store else np.zeros((0, 32), np.uint8)
    if not s.probe(keys).all():
        return "a stored digest is not found"
    near = near_misses(keys)
    if not np.array_equal(s.probe(near), np.array([r.tobytes() in store for r in near], bool)):
        return "near miss"
    if len(s) != len(store):
        return f"len {len(s)} != {len(store)}"
    return None


hits, bad, calls, salt = {c: 0 for c in COUNTERS}, [], 0, 1
t0 = time.perf_counter()
for case in range(a.cases):
    expected = int(rng.choice([0, 0, 16, 3000]))
    s, store, cap = acc.dedup_set(expected), set(), capacity_for(expected)
    fam_tags, chains, history = [], {}, []
    for call in range(int(rng.integers(3, 8))):
        parts = [rng.integers(0, 256, (log_uniform(0, 600), 32), dtype=np.uint8)]
        for _ in range(int(rng.integers(0, 6))):                           # adjacent-home same-tag families
            k = int(rng.integers(2, 13))
            if fam_tags and rng.random() < 0.35:
                t, h0 = fam_tags[int(rng.integers(0, len(fam_tags)))]         # grows a family settled earlier
            else:
                t, h0 = tag_word(), int(rng.integers(0, 1000))
                fam_tags.append((t, h0))
            parts.append(adjacent_homes(t, h0, int(rng.integers(1, 5)), k, salt, rng)); salt += k
            hits["families_3plus"] += k >= 3
        if rng.random() < 0.3:                                             # wrap-around: last slot -> 0, 1, ...
            k, spill = int(rng.integers(2, 9)), int(rng.integers(0, 4))
            t = fam_tags[0][0] if fam_tags and rng.random() < 0.3 else tag_word()
            parts.append(wrap(t, k, salt, spill)); salt += k + spill
            hits["wrap_families"] += 1
        if rng.random() < 0.25:                                            # first words 0 and 1: one tag
            k = int(rng.integers(2, 10))
            parts.append(tag01(int(rng.integers(0, 1000)), k, salt)); salt += k
        if rng.random() < 0.15:                                            # a chain that grows past 66 slots
            key = list(chains)[0] if chains and rng.random() < 0.6 else (tag_word(), int(rng.integers(0, 1000)))
            k = int(rng.integers(30, 90))
            parts.append(same_home(key[0], key[1], k, salt)); salt += k
            chains[key] = chains.get(key, 0) + k
            hits["chains_deeper_than_66"] += chains[key] > DEEP
        old = np.concatenate(history) if history else np.zeros((0, 32), np.uint8)
        if len(old) and rng.random() < 0.7:                                # repeats of earlier calls
            parts.append(old[rng.integers(0, len(old), int(rng.integers(1, 200)))])
        if rng.random() < 0.15:                                            # enough to grow the table
            parts.append(rng.integers(0, 256, (max(1, cap // 2 - len(store) + int(rng.integers(1, 400))), 32),
                                      dtype=np.uint8))
        d = np.concatenate(parts)
        if len(d) and rng.random() < 0.7:                                  # repeats inside the call
            d = np.concatenate([d, d[rng.integers(0, len(d), int(rng.integers(1, 1 + len(d) // 3 + 1)))]])
        d = np.ascontiguousarray(d[rng.permutation(len(d))])
        n = len(d)
        new_cap = capacity_after(cap, len(store), n)
        hits["growing_calls"] += new_cap > cap
        cap = new_cap
        device = n > 0 and rng.random() < 0.35
        desc = {"case": case, "call": call, "n": n, "device": device, "entries": len(store), "capacity": cap}
        calls += 1
        try:
            if device:
                hits["device_calls_with_sizes"] += 1
                sizes = rng.integers(0, 1 << 40, n, dtype=np.uint64)
                dbuf, dptr = to_device(d, 8)
                sbuf, sptr = to_device(sizes, 0)
                flags = torch.full((n,), 0xAA, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                n_new, b_new, b_dup = s.insert_device(dptr, n, sptr, flags.data_ptr())
                got = flags.cpu().numpy()
                exp = walk(store, d)
                why = None if np.array_equal(got, exp.astype(np.uint8)) else "is_new (device)"
                if why is None and (n_new, b_new, b_dup) != (int(exp.sum()), int(sizes[exp].sum()), int(sizes[~exp].sum())):
                    why = "counters"
            else:
                got = s.insert(d)
                exp = walk(store, d)
                why = None if np.array_equal(got, exp) else "is_new (host)"
            why = why or after_call(s, store)
        except Exception as e:                                             # every drawn call is a valid one
            why = "error: " + str(e)[:160]
        history.append(d)
        if why:
            bad.append(dict(desc, why=why))
            break                                                          # the set no longer matches the oracle
    s.close()
print(json.dumps({"cases": a.cases, "calls": calls, "mismatches": len(bad), "counters": hits,
                  "seconds": round(time.perf_counter() - t0, 2), "first_bad": bad[:3]}))
sys.exit(1 if bad else 0)
