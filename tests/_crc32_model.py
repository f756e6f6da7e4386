"""The CRC-32 tests' model: a pure-Python restatement of the arithmetic (GF(2) multiply, x^(8 n), combine — held to
zlib.crc32 by concatenation in tests/test_crc32_cpu.py, and then trusted for lengths no buffer has), and the case
generator, expectation and comparison of the stress harness tests/stress_crc32.py.  The oracle of every device result is
zlib.crc32; nothing the device computes is the check of anything else it computes."""
import os
import re
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POLY = 0xEDB88320
ONE = 0x80000000            # x^0 in the reflected register


def header_constant(name):
    src = open(os.path.join(ROOT, "include", "yams_mi355x_accel.h")).read()
    return int(re.search(r"#define\s+%s\s+\(?\s*(\d+)" % name, src).group(1))


S = header_constant("YAMS_CRC32_SEGMENT_BYTES")


def mulmod(a, b):
    p = 0
    for _ in range(32):
        if a & ONE:
            p ^= b
        a = (a << 1) & 0xFFFFFFFF
        b = (b >> 1) ^ (POLY if b & 1 else 0)
    return p


def x_pow_8n(n):
    """x^(8 n) mod P by square-and-multiply."""
    power, out = ONE >> 1, ONE
    for _ in range(3):
        power = mulmod(power, power)
    while n:
        if n & 1:
            out = mulmod(out, power)
        power = mulmod(power, power)
        n >>= 1
    return out


def combine(crc_a, crc_b, len_b):
    """CRC-32 of A || B from the finalised crc(A), crc(B) and |B|."""
    return mulmod(crc_a, x_pow_8n(len_b)) ^ crc_b


def crc_of_zeros(n):
    """CRC-32 of n zero bytes without the bytes: ~(FFFFFFFF * x^(8 n))."""
    return mulmod(0xFFFFFFFF, x_pow_8n(n)) ^ 0xFFFFFFFF


def crc(data):
    return zlib.crc32(bytes(data)) & 0xFFFFFFFF


# ---- the stress harness ---------------------------------------------------------------------------------------------
PINNED_SEED, PINNED_CASES, FLOOR = 23, 200, 4
ENTRIES = ("batch_device", "verify_device", "many_host", "chunks_device")
CONTENTS = ("zeros", "ff", "random", "period256")
CLASSES = ("tiny", "around_s", "multi", "one_long")
PATHS = tuple("entry:" + e for e in ENTRIES) + tuple("content:" + c for c in CONTENTS) + tuple("class:" + c for c in CLASSES) + \
    ("empty_message", "unaligned_offset", "overlap", "select_mask", "no_mask", "planted_mismatch", "all_valid", "single_message")
FAULTS = ("wrong_value", "swapped_pair", "sentinel_front", "sentinel_back", "valid_flag", "invalid_count", "unselected_nonzero")
SENTINEL = 0xA5A5A5A5
OK, INVALID_ARG = 0, 1


def _length(rng, cls):
    if cls == "tiny":
        return int(rng.integers(0, 101))
    if cls == "around_s":
        return int(S + rng.integers(-3, 4)) * int(rng.integers(1, 3)) + int(rng.integers(-1, 2))
    if cls == "multi":
        return int(rng.integers(2 * S, 40 * S))
    return int(rng.integers(1, 5)) << 20 | int(rng.integers(0, 1 << 12))      # one_long: 1..4 MiB and an odd tail


def draw_case(rng, case_no):
    entry = ENTRIES[case_no % len(ENTRIES)] if case_no < 4 * len(ENTRIES) else ENTRIES[int(rng.integers(0, len(ENTRIES)))]
    content = CONTENTS[int(rng.integers(0, len(CONTENTS)))]
    cls = CLASSES[int(rng.integers(0, len(CLASSES)))]
    case = {"no": case_no, "entry": entry, "content": content, "class": cls}
    if entry == "chunks_device":
        # blobs chunked on the device with a small configuration: an empty one, one below the minimum, longer ones
        case["blob_lens"] = [0, int(rng.integers(1, 2048))] + [int(rng.integers(2048, 300_000)) for _ in range(int(rng.integers(1, 5)))]
        rng.shuffle(case["blob_lens"])
        case["base"] = int(rng.integers(0, 16))
        case["mask"] = bool(rng.integers(0, 2))
        case["mask_seed"] = int(rng.integers(0, 1 << 30))
        return case
    n = 1 if rng.integers(0, 8) == 0 else int(rng.integers(2, 40)) if cls in ("multi", "one_long") else int(rng.integers(2, 400))
    lens = []
    for i in range(n):
        if cls == "one_long":
            lens.append(_length(rng, "one_long") if i == n // 2 else _length(rng, "tiny"))
        else:
            lens.append(0 if rng.integers(0, 12) == 0 else max(0, _length(rng, cls)))
    case["lens"] = lens
    case["layout"] = ("packed", "gaps", "overlap")[int(rng.integers(0, 3))] if entry != "many_host" else "separate"
    case["base"] = int(rng.integers(0, 16))
    if entry == "verify_device":
        kind = ("planted", "all_valid", "all_invalid")[int(rng.integers(0, 3))]
        case["verify"] = kind
        case["bad"] = sorted({0, n // 2, n - 1}) if kind == "planted" else list(range(n)) if kind == "all_invalid" else []
    return case


def _fill(rng, content, n):
    if content == "zeros":
        return np.zeros(n, np.uint8)
    if content == "ff":
        return np.full(n, 0xFF, np.uint8)
    if content == "period256":
        return (np.arange(n, dtype=np.uint64) + int(rng.integers(0, 256))).astype(np.uint8)
    return rng.integers(0, 256, n, dtype=np.uint8)


def materialise(case, rng):
    """-> (data uint8[], offsets, lengths): the messages as ranges of one buffer (many_host copies them out)."""
    if case["entry"] == "chunks_device":
        offs, at = [], case["base"]
        for n in case["blob_lens"]:
            offs.append(at); at += n + int(rng.integers(0, 3))
        data = _fill(rng, case["content"], at + 16)
        if case["content"] != "random":      # constant content never cuts before max_size: mix some noise in for boundaries
            k = max(1, data.size // 3)
            data[:k] = rng.integers(0, 256, k, dtype=np.uint8)
        return data, offs, list(case["blob_lens"])
    lens = case["lens"]
    offs, at = [], case["base"]
    for i, n in enumerate(lens):
        if case["layout"] == "overlap" and i and offs:
            at = max(case["base"], offs[-1] + int(rng.integers(0, max(1, lens[i - 1] // 2 + 1))))
        offs.append(at)
        at += n + (int(rng.integers(0, 19)) if case["layout"] == "gaps" else 0)
    total = max([o + n for o, n in zip(offs, lens)] + [case["base"]]) + 16
    return _fill(rng, case["content"], total), offs, list(lens)


def expect(data, offs, lens):
    b = data.tobytes()
    return [zlib.crc32(b[o:o + n]) & 0xFFFFFFFF for o, n in zip(offs, lens)]


def classify(case, offs, lens):
    p = ["entry:" + case["entry"], "content:" + case["content"], "class:" + case["class"]]
    if any(n == 0 for n in lens):
        p.append("empty_message")
    if any(o % 16 for o in offs):
        p.append("unaligned_offset")
    if case.get("layout") == "overlap":
        p.append("overlap")
    if case["entry"] == "chunks_device":
        p.append("select_mask" if case["mask"] else "no_mask")
    if case.get("verify") == "planted":
        p.append("planted_mismatch")
    if case.get("verify") == "all_valid":
        p.append("all_valid")
    if len(lens) == 1:
        p.append("single_message")
    return p


def perfect_outputs(case, exp, select=None):
    """What a correct device hands back: `crc` between two sentinel words, and for verify the flags and the count."""
    vals = [0 if (select is not None and not select[i]) else e for i, e in enumerate(exp)]
    got = {"status": OK, "crc": np.array([SENTINEL] + vals + [SENTINEL], np.uint32)}
    if case["entry"] == "verify_device":
        bad = set(case["bad"])
        got["valid"] = np.array([0xA5] + [0 if i in bad else 1 for i in range(len(exp))] + [0xA5], np.uint8)
        got["n_invalid"] = len(bad)
        got["crc"] = None
    return got


def compare(case, exp, got, select=None):
    wrong = []
    if got["status"] != OK:
        return ["status %d" % got["status"]]
    n = len(exp)
    if got.get("crc") is not None:
        c = got["crc"]
        if int(c[0]) != SENTINEL:
            wrong.append("the word in front of the output changed")
        if int(c[n + 1]) != SENTINEL:
            wrong.append("the word behind the output changed")
        for i in range(n):
            want = 0 if (select is not None and not select[i]) else exp[i]
            if int(c[1 + i]) != want:
                wrong.append(("unselected entry %d is %08x" if (select is not None and not select[i]) else "crc %d is %08x") % (i, int(c[1 + i])) +
                             ", want %08x" % want)
                if len(wrong) > 4:
                    break
    if case["entry"] == "verify_device":
        v, bad = got["valid"], set(case["bad"])
        if int(v[0]) != 0xA5 or int(v[n + 1]) != 0xA5:
            wrong.append("a guard byte of out_valid changed")
        flags = [i for i in range(n) if int(v[1 + i]) != (0 if i in bad else 1)]
        if flags:
            wrong.append("valid flags differ at %s" % flags[:5])
        if got["n_invalid"] != len(bad):
            wrong.append("n_invalid %d, want %d" % (got["n_invalid"], len(bad)))
    return wrong


def self_test_cases():
    plain = {"no": 0, "entry": "batch_device", "content": "random", "class": "tiny", "lens": [5, 0, 70, 33], "layout": "packed", "base": 3}
    verify = dict(plain, entry="verify_device", verify="planted", bad=[0, 2])
    chunks = {"no": 0, "entry": "chunks_device", "content": "random", "class": "tiny", "mask": True}
    return plain, verify, chunks


def inject(fault, got):
    """Damages a perfect result in place; returns the text compare() must report first."""
    if fault == "wrong_value":
        got["crc"][2] ^= 1; return "crc 1 is"
    if fault == "swapped_pair":
        got["crc"][[1, 3]] = got["crc"][[3, 1]]; return "crc 0 is"
    if fault == "sentinel_front":
        got["crc"][0] = 0; return "the word in front"
    if fault == "sentinel_back":
        got["crc"][-1] = 0; return "the word behind"
    if fault == "valid_flag":
        got["valid"][2] ^= 1; return "valid flags differ"
    if fault == "invalid_count":
        got["n_invalid"] += 1; return "n_invalid"
    if fault == "unselected_nonzero":
        got["crc"][2] = 7; return "unselected entry 1"
    raise ValueError(fault)
