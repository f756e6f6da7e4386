"""Regenerates tests/golden/semantic_neighbors.json from the reference's OWN pair loop.

    python tests/golden/make_semgraph_golden.py /path/to/reference

At generation time the reference's text is cut out of src/daemon/components/EmbeddingService.cpp by text anchors (a missing or
ambiguous anchor is an error) — the two score lambdas, CorpusVector, SourceDocRef, NeighborScore with its comparators, and the
candidate loop of the whole-corpus branch with its sort and effective threshold — and spliced into the driver below, which
defines the few locals those pieces name (semanticTopK, explicitSemanticThreshold, corpus, sources, the two counters), builds
the corpus as the streaming callback does (rows with inv <= 0 stay out) and prints what the loop left in topNeighbors.  The
program is compiled with g++ into a temporary directory and run once per case of _semgraph_oracle.golden_cases(); none of the
cut text is kept.  Only inputs and recorded results go into the JSON file."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _semgraph_oracle as so  # noqa: E402

SOURCE = os.path.join("src", "daemon", "components", "EmbeddingService.cpp")

# (name, first line of the piece, last line of the piece) — both matched after stripping, the first occurrence of `end` at or
# after `begin`; `begin` must occur exactly once
PIECES = [
    ("lambdas", "const auto inverseNorm = [](const std::vector<float>& v) {", "return static_cast<float>(dot * invNormA * invNormB);"),
    ("corpus_vector", "struct CorpusVector {", "};"),
    ("source_doc_ref", "struct SourceDocRef {", "};"),
    ("neighbor_score", "struct NeighborScore {", "return isBetterNeighbor(right, left);"),
    ("candidate_loop", "std::vector<NeighborScore> topNeighbors;", "explicitSemanticThreshold.value_or(topNeighbors.back().similarity);"),
]
CLOSERS = {"lambdas": 1, "neighbor_score": 1}      # pieces whose last matched line sits inside a lambda: take the closing `};` too

DRIVER = r"""
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <optional>
#include <string>
#include <unordered_set>
#include <vector>

int main(int argc, char** argv) {
    std::ifstream in(argv[1]);
    std::size_t n, dim, k, nSources;
    int hasThreshold;
    std::uint32_t thresholdBits;
    in >> n >> dim >> k >> hasThreshold >> thresholdBits >> nSources;
    float thresholdValue;
    std::memcpy(&thresholdValue, &thresholdBits, 4);
    const std::size_t semanticTopK = k;
    const std::optional<float> explicitSemanticThreshold = hasThreshold ? std::optional<float>(thresholdValue) : std::nullopt;
    std::vector<std::string> hashes(n);
    std::vector<std::vector<float>> rows(n, std::vector<float>(dim));
    for (std::size_t i = 0; i < n; ++i) {
        in >> hashes[i];
        for (std::size_t d = 0; d < dim; ++d) { std::uint32_t b; in >> b; std::memcpy(&rows[i][d], &b, 4); }
    }
    std::vector<std::size_t> sourceRows(nSources);
    for (auto& s : sourceRows) in >> s;

    //@lambdas@
    //@corpus_vector@
    // the streaming callback (first hash wins, rows with inv <= 0 stay out), written here: it is tied to the database
    std::vector<CorpusVector> corpus;
    corpus.reserve(n);
    std::unordered_set<std::string> corpusHashes;
    std::vector<float> allInv(n);
    for (std::size_t i = 0; i < n; ++i) {
        const float inv = inverseNorm(rows[i]);
        allInv[i] = inv;
        if (!corpusHashes.insert(hashes[i]).second) continue;
        if (inv <= 0.0f) continue;
        corpus.push_back(CorpusVector{hashes[i], std::string(), rows[i], inv});
    }
    std::printf("INV");
    for (std::size_t i = 0; i < n; ++i) { std::uint32_t b; std::memcpy(&b, &allInv[i], 4); std::printf(" %u", b); }
    std::printf("\n");
    if (corpus.size() < 2) { std::printf("COUNTS 0 0\n"); return 0; }
    //@source_doc_ref@
    std::vector<SourceDocRef> sources;
    for (std::size_t s : sourceRows)
        for (const auto& item : corpus)
            if (item.hash == hashes[s] && item.invNorm > 0.0f) sources.push_back(SourceDocRef{&item.hash, &item.filePath, &item.embedding, item.invNorm});
    //@neighbor_score@
    std::size_t similarityPairCount = 0;
    std::size_t candidateNeighborCount = 0;
    auto rowOf = [&](const std::string& h) { return static_cast<std::size_t>(std::find(hashes.begin(), hashes.end(), h) - hashes.begin()); };
    for (const auto& source : sources) {
        //@candidate_loop@
        std::uint32_t eb; std::memcpy(&eb, &effectiveThreshold, 4);
        std::printf("SRC %zu %u", rowOf(*source.hash), eb);
        for (const auto& t : topNeighbors) { std::uint32_t b; std::memcpy(&b, &t.similarity, 4); std::printf(" %zu:%u", rowOf(t.doc->hash), b); }
        std::printf("\n");
    }
    std::printf("COUNTS %zu %zu\n", similarityPairCount, candidateNeighborCount);
    return 0;
}
"""


def cut(text, name, begin, end):
    lines = text.splitlines()
    starts = [i for i, l in enumerate(lines) if l.strip() == begin]
    if len(starts) != 1:
        raise SystemExit(f"anchor for {name!r}: {len(starts)} matches of {begin!r}")
    for j in range(starts[0], len(lines)):
        if lines[j].strip() == end:
            break
    else:
        raise SystemExit(f"anchor for {name!r}: no {end!r} after its first line")
    if name in CLOSERS:
        j += 1
        if lines[j].strip() != "};":
            raise SystemExit(f"anchor for {name!r}: the lambda does not close where expected")
    return "\n".join(lines[starts[0]:j + 1])


def build(reference, tmp):
    text = open(os.path.join(reference, SOURCE)).read()
    prog = DRIVER
    for name, begin, end in PIECES:
        marker = f"//@{name}@"
        assert prog.count(marker) == 1, name
        prog = prog.replace(marker, cut(text, name, begin, end))
    src = os.path.join(tmp, "driver.cpp")
    open(src, "w").write(prog)
    exe = os.path.join(tmp, "driver")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++20", "-O2", "-ffp-contract=off", "-o", exe, src], check=True)
    return exe


def run(exe, tmp, v):
    rows = v["rows"]
    n, dim = rows.shape
    sources = list(range(n)) if v["sources"] is None else v["sources"]
    thr = v["threshold"]
    with open(os.path.join(tmp, "case.txt"), "w") as f:
        f.write(f"{n} {dim} {v['k']} {0 if thr is None else 1} {int(so.bits(np.float32(thr or 0.0))[0])} {len(sources)}\n")
        for h, r in zip(v["hashes"], so.bits(rows).tolist()):
            f.write(h + " " + " ".join(map(str, r)) + "\n")
        f.write(" ".join(map(str, sources)) + "\n")
    out = subprocess.run([exe, os.path.join(tmp, "case.txt")], check=True, capture_output=True, text=True).stdout.splitlines()
    rec = {"neighbors": {}, "effective_threshold_bits": {}}
    for line in out:
        w = line.split()
        if w[0] == "INV":
            rec["inv_bits"] = [int(b) for b in w[1:]]
        elif w[0] == "SRC":
            rec["neighbors"][w[1]] = [[int(p.split(":")[0]), int(p.split(":")[1])] for p in w[3:]]
            rec["effective_threshold_bits"][w[1]] = int(w[2])
        elif w[0] == "COUNTS":
            rec["pairs_scored"], rec["pairs_admitted"] = int(w[1]), int(w[2])
    return rec


def main():
    reference = sys.argv[1]
    cases = []
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(reference, tmp)
        for name, v in so.golden_cases().items():
            rec = run(exe, tmp, v)
            cases.append({"name": name, "dim": int(v["rows"].shape[1]), "k": v["k"],
                          "threshold_bits": None if v["threshold"] is None else int(so.bits(np.float32(v["threshold"]))[0]),
                          "sources": v["sources"], "hashes": v["hashes"], "rows_bits": so.bits(v["rows"]).tolist(), **rec})
    doc = {"source": SOURCE + ": updateSemanticNeighborGraphUnlocked, the whole-corpus branch's pair loop, cut out by anchors and run",
           "cases": cases}
    with open(os.path.join(HERE, "semantic_neighbors.json"), "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(len(cases), "cases")


if __name__ == "__main__":
    main()
