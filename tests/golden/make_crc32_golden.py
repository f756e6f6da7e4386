"""Regenerates tests/golden/crc32.json from the reference's OWN three CRC-32 implementations.

    python tests/golden/make_crc32_golden.py /path/to/reference

At generation time the reference's text is cut out by text anchors (a missing or ambiguous anchor is an error): the
bit-at-a-time loop of src/storage/compressed_storage_engine.cpp (what header.uncompressedCRC32 is computed with), the table
and calculateCRC32 / updateCRC32 of src/compression/compression_utils.cpp, and the CRC32Table class of
src/compression/integrity_validator.cpp with its global instance.  Each piece goes into a namespace of its own inside the
driver below, which is compiled with g++ into a temporary directory and run once over all cases; none of the cut text is
kept.  The JSON holds inputs (hex, or a seeded recipe: numpy default_rng(seed).integers(0, 256, n)) and the recorded results
only: per case the three values, and updateCRC32 continued over a split of the input."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# (name, file, first line, last line, inclusive) — lines matched after stripping; `begin` must occur exactly once in its file,
# `end` is its first occurrence at or after `begin`
PIECES = [
    ("stored", "src/storage/compressed_storage_engine.cpp", "uint32_t calculateCRC32(std::span<const std::byte> data) {", "return ~crc;", True),
    ("utils_table", "src/compression/compression_utils.cpp", "constexpr uint32_t CRC32_POLY = 0xEDB88320U;", "constexpr CRC32Table crc32Table;", True),
    ("utils_functions", "src/compression/compression_utils.cpp", "uint32_t calculateCRC32(std::span<const std::byte> data) {",
     "bool isLikelyCompressed(std::span<const std::byte> data) {", False),
    ("validator", "src/compression/integrity_validator.cpp", "class CRC32Table {", "static const CRC32Table g_crc32Table(0xEDB88320);", True),
]
CLOSERS = {"stored": "}"}       # the matched last line sits inside the function: its closing brace follows

DRIVER = r"""
#include <array>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <span>
#include <string>
#include <vector>

namespace stored {
//@stored@
}
namespace utils {
//@utils_table@
//@utils_functions@
}
namespace validator {
//@validator@
}

int main(int, char** argv) {
    std::ifstream in(argv[1]);
    std::size_t cases;
    in >> cases;
    for (std::size_t c = 0; c < cases; ++c) {
        std::size_t n, split;
        in >> n >> split;
        std::vector<std::byte> data(n);
        for (auto& b : data) { unsigned v; in >> v; b = static_cast<std::byte>(v); }
        const std::span<const std::byte> all(data);
        const uint32_t head = utils::calculateCRC32(all.first(split));
        std::printf("%u %u %u %u\n", stored::calculateCRC32(all), utils::calculateCRC32(all), validator::g_crc32Table.calculate(all),
                    utils::updateCRC32(head, all.subspan(split)));
    }
    return 0;
}
"""


def cut(reference, name, path, begin, end, inclusive):
    lines = open(os.path.join(reference, path)).read().splitlines()
    starts = [i for i, l in enumerate(lines) if l.strip() == begin]
    if len(starts) != 1:
        raise SystemExit(f"anchor for {name!r}: {len(starts)} matches of {begin!r} in {path}")
    for j in range(starts[0], len(lines)):
        if lines[j].strip() == end:
            break
    else:
        raise SystemExit(f"anchor for {name!r}: no {end!r} after its first line")
    piece = lines[starts[0]:j + 1 if inclusive else j]
    if name in CLOSERS:
        piece.append(CLOSERS[name])
    return "\n".join(piece)


def cases():
    """[{name, hex | (seed, n), split}]: short inputs spelled out, longer ones as seeded recipes."""
    out = [{"name": "empty", "hex": "", "split": 0}, {"name": "check", "hex": b"123456789".hex(), "split": 4},
           {"name": "a", "hex": b"a".hex(), "split": 1}, {"name": "zeros32", "hex": "00" * 32, "split": 7},
           {"name": "ff32", "hex": "ff" * 32, "split": 31}, {"name": "text", "hex": b"The quick brown fox jumps over the lazy dog".hex(), "split": 16}]
    for seed, n in [(1, 1), (2, 15), (3, 16), (4, 17), (5, 255), (6, 4095), (7, 4096), (8, 4097), (9, 12293), (10, 65536), (11, 300001)]:
        out.append({"name": f"random_{n}", "seed": seed, "n": n, "split": n // 3})
    out.append({"name": "zeros4096", "fill": 0, "n": 4096, "split": 1000})
    out.append({"name": "zeros_1MiB", "fill": 0, "n": 1 << 20, "split": 12345})
    return out


def case_bytes(c):
    if "hex" in c:
        return bytes.fromhex(c["hex"])
    if "fill" in c:
        return bytes([c["fill"]]) * c["n"]
    return np.random.default_rng(c["seed"]).integers(0, 256, c["n"], dtype=np.uint8).tobytes()


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    reference = sys.argv[1]
    src = DRIVER
    for name, path, begin, end, inclusive in PIECES:
        src = src.replace("//@%s@" % name, cut(reference, name, path, begin, end, inclusive))
    cs = cases()
    with tempfile.TemporaryDirectory() as tmp:
        cpp, exe, inp = (os.path.join(tmp, f) for f in ("driver.cpp", "driver", "cases.txt"))
        open(cpp, "w").write(src)
        subprocess.run([os.environ.get("CXX", "g++"), "-std=c++20", "-O2", "-o", exe, cpp], check=True)
        with open(inp, "w") as f:
            f.write("%d\n" % len(cs))
            for c in cs:
                b = case_bytes(c)
                f.write("%d %d\n%s\n" % (len(b), c["split"], " ".join(map(str, b))))
        lines = subprocess.run([exe, inp], check=True, capture_output=True, text=True).stdout.split("\n")
    for c, line in zip(cs, lines):
        c["stored_object"], c["compression_utils"], c["integrity_validator"], c["update_over_split"] = map(int, line.split())
    doc = {"note": "CRC-32 of each input by the reference's three implementations (compressed_storage_engine.cpp:49-59, "
                   "compression_utils.cpp:31-52, integrity_validator.cpp:36-65) and updateCRC32 continued over [split:) from "
                   "calculateCRC32([:split)).  Inputs: hex, fill x n, or numpy default_rng(seed).integers(0, 256, n, uint8).",
           "cases": cs}
    with open(os.path.join(HERE, "crc32.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", len(cs), "cases")


if __name__ == "__main__":
    main()
