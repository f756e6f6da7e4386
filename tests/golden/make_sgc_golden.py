"""Generates tests/golden/sgc.json from the REFERENCE'S OWN applySGCSmoothing.

    python tests/golden/make_sgc_golden.py [reference checkout]     (default /root/reference; dev container only)

The reference's topology_sgc.cpp is compiled as it is (-std=c++20 -I oracle/shim -I <ref>/include) and linked with the small
driver below — ours — which also includes include/yams_accel/topology_sgc.hpp over the reference's own types
(-DYAMS_ACCEL_USE_HOST_TYPES) and prints the lists AccelSGC::buildLists makes of the same documents.  Nothing of the reference,
text or binary, is written into the repository: the build lives in a temporary directory.

Per case the file holds the recipe's name (inputs: tests/_sgc_oracle.py GOLDEN_CASES), the configuration and hops, the SHA-256
of the input bits, the lists the shell's builder produced under this machine's standard library (their order is the order of
the reference's sums), the raw input and output bits where they are few, and the SHA-256 of the output bits.
"""
import json
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _sgc_oracle as sg  # noqa: E402

DRIVER = r'''
#include <yams/topology/topology_sgc.h>
#include <yams_accel/topology_sgc.hpp>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>
using namespace yams::topology;
static bool rd(FILE* f, void* p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }
static bool rd_str(FILE* f, std::string& s) { uint32_t n; if (!rd(f, &n, 4)) return false; s.resize(n); return rd(f, s.data(), n); }
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t n, hops; double min_edge; uint32_t reciprocal_only;
    if (!rd(f, &n, 8) || !rd(f, &hops, 8) || !rd(f, &min_edge, 8) || !rd(f, &reciprocal_only, 4)) return 2;
    std::vector<TopologyDocumentInput> docs(n);
    for (auto& d : docs) {
        uint32_t dim, nn;
        if (!rd_str(f, d.documentHash) || !rd(f, &dim, 4)) return 2;
        d.embedding.resize(dim);
        if (!rd(f, d.embedding.data(), dim * 4ull) || !rd(f, &nn, 4)) return 2;
        d.neighbors.resize(nn);
        for (auto& nb : d.neighbors) {
            uint8_t r;
            if (!rd_str(f, nb.documentHash) || !rd(f, &nb.score, 4) || !rd(f, &r, 1)) return 2;
            nb.reciprocal = r != 0;
        }
    }
    TopologyBuildConfig config;
    config.minEdgeScore = min_edge;
    config.reciprocalOnly = reciprocal_only != 0;
    const SGCLists lists = AccelSGC::buildLists(docs, config);
    std::printf("OFFSETS");
    for (auto v : lists.rowOffsets) std::printf(" %llu", static_cast<unsigned long long>(v));
    std::printf("\nCOLS");
    for (auto v : lists.cols) std::printf(" %u", v);
    std::printf("\nWEIGHTS");
    for (float v : lists.weights) { uint32_t b; std::memcpy(&b, &v, 4); std::printf(" %u", b); }
    std::printf("\n");
    applySGCSmoothing(docs, config, hops);
    for (const auto& d : docs) {
        std::printf("DOC");
        for (float v : d.embedding) { uint32_t b; std::memcpy(&b, &v, 4); std::printf(" %u", b); }
        std::printf("\n");
    }
    return 0;
}
'''


def build_driver(ref, tmp):
    src = os.path.join(tmp, "sgc_driver.cpp")
    with open(src, "w") as f:
        f.write(DRIVER)
    exe = os.path.join(tmp, "sgc_driver")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++20", "-O2", "-DYAMS_ACCEL_USE_HOST_TYPES", "-I" + os.path.join(ROOT, "oracle", "shim"),
           "-I" + os.path.join(ref, "include"), "-I" + os.path.join(ROOT, "include"), src,
           os.path.join(ref, "src", "topology", "topology_sgc.cpp"), "-ldl", "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def write_case(path, docs, min_edge, reciprocal_only, hops):
    with open(path, "wb") as f:
        f.write(struct.pack("<QQdI", len(docs), hops, min_edge, 1 if reciprocal_only else 0))
        for d in docs:
            h = d["hash"].encode()
            f.write(struct.pack("<I", len(h))); f.write(h)
            f.write(struct.pack("<I", len(d["emb"]))); f.write(np.asarray(d["emb"], np.float32).tobytes())
            f.write(struct.pack("<I", len(d["nbrs"])))
            for a, s, r in d["nbrs"]:
                a = a.encode()
                f.write(struct.pack("<I", len(a))); f.write(a)
                f.write(np.float32(s).tobytes()); f.write(b"\1" if r else b"\0")


def run_reference(exe, tmp, docs, min_edge, reciprocal_only, hops):
    path = os.path.join(tmp, "case.bin")
    write_case(path, docs, min_edge, reciprocal_only, hops)
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, ("the reference driver failed", r.returncode, r.stderr[-500:])
    lines = r.stdout.splitlines()
    nums = lambda line, tag: [int(v) for v in line.split()[1:]] if line.split()[0] == tag else None
    off, cols, w = nums(lines[0], "OFFSETS"), nums(lines[1], "COLS"), nums(lines[2], "WEIGHTS")
    embs = [np.array(nums(line, "DOC"), np.uint32) for line in lines[3:]]
    assert len(embs) == len(docs)
    return off, cols, w, embs


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    cases = []
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(ref, tmp)
        for name, (make, min_edge, reciprocal_only, hops) in sg.GOLDEN_CASES.items():
            docs = make()
            off, cols, w, embs = run_reference(exe, tmp, docs, min_edge, reciprocal_only, hops)
            case = {"name": name, "min_edge_score": min_edge, "reciprocal_only": reciprocal_only, "hops": hops, "n": len(docs),
                    "sha256": sg.docs_digest(docs), "row_offsets": off, "cols": cols, "weights_bits": w,
                    "out_sha256": sg.embeddings_digest([e.view(np.float32) for e in embs])}
            if sum(len(d["emb"]) for d in docs) <= sg.RAW_BITS_MAX:
                case["docs"] = [{"hash": d["hash"], "emb_bits": sg.bits(d["emb"]).tolist(),
                                 "nbrs": [[a, int(sg.bits([s])[0]), int(r)] for a, s, r in d["nbrs"]]} for d in docs]
                case["out_bits"] = [e.tolist() for e in embs]
            cases.append(case)
            print(name, len(docs), "documents,", len(cols), "list entries")
    out = os.path.join(HERE, "sgc.json")
    with open(out, "w") as f:
        f.write('{"source": "applySGCSmoothing (src/topology/topology_sgc.cpp); lists: AccelSGC::buildLists under the generating machine\'s standard library",\n "cases": [\n')
        f.write(",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in cases))
        f.write("\n]}\n")
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
