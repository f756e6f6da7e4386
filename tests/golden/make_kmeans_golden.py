"""Generates tests/golden/kmeans.json from the REFERENCE'S OWN KMeansTopologyEngine.

    python tests/golden/make_kmeans_golden.py [reference checkout]     (default /root/reference; dev container only)

The reference's topology_alternate_engines.cpp, topology_representatives.cpp and protected_relation_cover.cpp are compiled as
they are (-std=c++20 -I oracle/shim -I <ref>/include -I <ref>/src/topology) and linked with the small driver below — ours —
under -Wl,--unresolved-symbols=ignore-all: the only unresolved symbols are StaticCosineAnnIndex's, inside a boundary-spill
function that returns before it uses them under the default TopologyBuildConfig.  A case that did reach one would call address
zero; every case must exit with status 0.  Nothing of the reference, text or binary, is written into the repository: the build
lives in a temporary directory.

Per case the file holds the recipe's name (inputs: tests/_kmeans_oracle.py case_rows), k and max_iterations, the SHA-256 of the
input bits, the raw bits themselves where they are few (the size limit of a golden file rules them out for the large cases), and
the partition — sorted lists of row indices — read off the clusters' memberDocumentHashes.
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
import _kmeans_oracle as ko  # noqa: E402

DRIVER = r'''
#include <yams/topology/topology_alternate_engines.h>
#include <cstdio>
#include <cstdint>
#include <string>
#include <vector>
using namespace yams::topology;
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t hdr[3];
    if (std::fread(hdr, 8, 3, f) != 3) return 2;
    std::vector<TopologyDocumentInput> docs(hdr[0]);
    for (uint64_t i = 0; i < hdr[0]; ++i) {
        uint32_t dim;
        if (std::fread(&dim, 4, 1, f) != 1) return 2;
        docs[i].embedding.resize(dim);
        if (dim && std::fread(docs[i].embedding.data(), 4, dim, f) != dim) return 2;
        char name[32];
        std::snprintf(name, sizeof name, "d%08llu", static_cast<unsigned long long>(i));
        docs[i].documentHash = name;
    }
    TopologyBuildConfig config;
    config.kmeansK = hdr[1];
    if (hdr[2] != ~0ull) config.kmeansMaxIterations = hdr[2];
    auto r = KMeansTopologyEngine().buildArtifacts(docs, config);
    if (!r) return 3;
    for (const auto& c : r.value().clusters) {
        for (const auto& h : c.memberDocumentHashes) std::printf("%llu ", std::stoull(h.substr(1)));
        std::printf("\n");
    }
    return 0;
}
'''
RAW_BITS_MAX = 256       # floats: cases up to this size carry their raw bits


def build_driver(ref, tmp):
    src = os.path.join(tmp, "kmeans_driver.cpp")
    with open(src, "w") as f:
        f.write(DRIVER)
    exe = os.path.join(tmp, "kmeans_driver")
    tus = [os.path.join(ref, "src", "topology", t) for t in
           ("topology_alternate_engines.cpp", "topology_representatives.cpp", "protected_relation_cover.cpp")]
    cmd = [os.environ.get("CXX", "g++"), "-std=c++20", "-O1", "-I" + os.path.join(ROOT, "oracle", "shim"), "-I" + os.path.join(ref, "include"),
           "-I" + os.path.join(ref, "src", "topology"), src, *tus, "-Wl,--unresolved-symbols=ignore-all", "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def run_reference(exe, tmp, embeddings, k, max_iterations):
    path = os.path.join(tmp, "case.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<QQQ", len(embeddings), k, max_iterations if max_iterations else 0xFFFFFFFFFFFFFFFF))
        for e in embeddings:
            f.write(struct.pack("<I", len(e))); f.write(np.asarray(e, np.float32).tobytes())
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, ("the reference driver failed (an unresolved symbol reached?)", r.returncode, r.stderr[-500:])
    return sorted(sorted(int(x) for x in line.split()) for line in r.stdout.splitlines() if line.strip())


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    cases = []
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(ref, tmp)
        for name, (k, it) in ko.CASES.items():
            emb = ko.case_rows(name)
            part = run_reference(exe, tmp, emb, k, it)
            assert sorted(i for g in part for i in g) == list(range(len(emb))), name
            case = {"name": name, "k": k, "max_iterations": it, "n": len(emb), "sha256": ko.rows_digest(emb), "partition": part}
            if sum(len(e) for e in emb) <= RAW_BITS_MAX:
                case["rows_bits"] = [np.asarray(e, np.float32).view(np.uint32).tolist() for e in emb]
            cases.append(case)
            print(name, len(emb), "rows ->", len(part), "clusters")
    out = os.path.join(HERE, "kmeans.json")
    with open(out, "w") as f:
        f.write('{"source": "KMeansTopologyEngine::buildArtifacts (kmeans_v1), default TopologyBuildConfig but kmeansK / kmeansMaxIterations",\n "cases": [\n')
        f.write(",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in cases))
        f.write("\n]}\n")
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
