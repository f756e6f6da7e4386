"""Generates tests/golden/features.json from the REFERENCE'S OWN aggregateEmbedding, computeVarianceWeights, bucketCountSketch and
composeFeatureVector.

    python tests/golden/make_features_golden.py [reference checkout]     (default /root/reference; dev container only)

tests/cpp/features_shell_test.cpp — ours — built with -DFEATURES_WITH_REFERENCE includes the reference's
src/topology/topology_input_extractor.cpp as it is (the functions are local to that translation unit), reads the cases and
prints the bits the reference's functions return.  The absent simeon/minhash.hpp is a stub written into the same temporary
directory (the encoder is never called: the cases carry signatures); SQLite's header comes from the Python distribution's
include directory; the link ignores the unresolved symbols of the classes extract() talks to, which are never called.  It is
built twice: -ffp-contract=off (the SEPARATE form) and -ffp-contract=fast -mfma (FUSED, where this compiler emits the fma).
Which form a build has is judged on the recorded flip samples (tests/_features_oracle.py FLIP_SEEDS): a build whose weights
there are not the form's it was made for is replaced by the restatement, and the file says so.  Nothing of the reference, text
or binary, is written into the repository: the builds live in a temporary directory.

Per case and form the file holds the SHA-256 of the input bits and the bits of every output vector.  The generator asserts the
conditions the tests rely on, on what the REFERENCE returned:
  - the two forms give different weight bits in at least 4 of the flip cases;
  - aggregate: a lone -0.0f member stays -0.0f and two -0.0f members give -0.0f (a `0.0f +` start gives +0.0f in both);
  - var_tie_at_cut_t2: two equal variances straddle the cut, exactly one of the two dimensions is kept;
  - var_zero_inside_top_t3: a zero variance inside the top 3, so only 2 weights are positive;
  - compose: a sumSq == 0 row comes back as it is; a row whose norm rounds to inf becomes zeros; a NaN alpha gives a dense part
    of zeros; rows with each of the four (entityOn, minhashOn) combinations have the four lengths.
  NO ROW'S NORM CAN ROUND TO 0.0f: sumSq >= x^2 exactly for the largest |x| (products of floats are exact in fp64 and cannot
  underflow there), so sqrt(sumSq) >= |x| >= 2^-149, which float represents.  The case holds the nearest thing, a row whose norm
  IS 2^-149, and asserts that it normalises to 1.0f."""
import json
import os
import subprocess
import sys
import sysconfig
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _features_oracle as fo  # noqa: E402

MINHASH_STUB = """#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
namespace simeon {
struct MinHashConfig {};
class MinHashEncoder {
public:
    explicit MinHashEncoder(MinHashConfig) {}
    std::size_t k() const { return 0; }
    void encode(const std::string&, std::uint32_t*) {}
};
}
"""


def build(ref, tmp, name, flags):
    cxx = os.environ.get("CXX", "g++")
    os.makedirs(os.path.join(tmp, "simeon"), exist_ok=True)
    with open(os.path.join(tmp, "simeon", "minhash.hpp"), "w") as f:
        f.write(MINHASH_STUB)
    sqlite = [d for d in (sysconfig.get_paths()["include"] + "/..", "/opt/conda/include", "/usr/include") if os.path.exists(os.path.join(d, "sqlite3.h"))]
    inc = ["-I" + tmp, "-I" + os.path.join(ROOT, "oracle", "shim"), "-I" + os.path.join(ref, "include"), "-I" + os.path.join(ref, "src", "topology"),
           "-I" + os.path.join(ROOT, "include"), *["-I" + d for d in sqlite[:1]]]
    exe = os.path.join(tmp, name)
    subprocess.run([cxx, "-std=c++20", "-O2", *flags, "-DFEATURES_WITH_REFERENCE", *inc, os.path.join(ROOT, "tests", "cpp", "features_shell_test.cpp"),
                    "-Wl,--unresolved-symbols=ignore-all", "-o", exe], check=True)
    return exe


def vec(hexbits, dtype=np.float32):
    return np.frombuffer(bytes.fromhex(hexbits), dtype)


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    names = fo.case_names()
    out = {"source": "aggregateEmbedding, computeVarianceWeights, bucketCountSketch, composeFeatureVector "
                     "(src/topology/topology_input_extractor.cpp)", "forms": {}, "cases": []}
    returned = {}
    with tempfile.TemporaryDirectory() as tmp:
        cases = os.path.join(tmp, "cases.bin")
        fo.write_cases(cases)
        for form, flags in (("separate", ["-ffp-contract=off"]), ("fused", ["-ffp-contract=fast", "-mfma"])):
            exe = build(ref, tmp, "ref_" + form, flags)
            r = subprocess.run([exe, cases], capture_output=True, text=True)
            assert r.returncode == 0, (form, r.returncode, r.stderr[-500:])
            _, got = fo.parse_driver_output(r.stdout)
            assert len(got) == len(names)
            want = fo.restated(fo.FORMS[form])
            flips = [i for i, n in enumerate(names) if n.startswith("var_flip_")]
            if all(got[i] == want[i] for i in flips):
                out["forms"][form] = "the reference's translation unit, this compiler"
                returned[form] = got
            else:      # this compiler did not give the build that form: the restatement stands in, and the file says so
                other = fo.restated(1 - fo.FORMS[form])
                out["forms"][form] = "tests/_features_oracle.py (the reference build has the %s form)" % (
                    "other" if all(got[i] == other[i] for i in flips) else "neither")
                returned[form] = want
    sep, fus = returned["separate"], returned["fused"]
    at = {n: i for i, n in enumerate(names)}
    # ---- the conditions the tests rely on, on what came back ----
    differ = sum(sep[at[n]] != fus[at[n]] for n in names if n.startswith("var_flip_"))
    assert differ >= 4, "the two forms must give different weights in at least 4 flip cases, got %d" % differ
    for n in names:
        if not n.startswith("var_"):
            assert sep[at[n]] == fus[at[n]], (n, "aggregate and compose are form-free")
    agg = sep[at["aggregate"]]
    assert np.signbit(vec(agg[1])[[0, 2, 4]]).all() and np.signbit(vec(agg[2])[[0, 4]]).all() and not np.signbit(vec(agg[2])[2])
    tie = vec(sep[at["var_tie_at_cut_t2"]][0])
    sample, _ = fo.VARIANCE_CASES["var_tie_at_cut_t2"]
    _, var = fo.variance_py(np.stack(sample), None, fo.SEPARATE)
    assert var[1] == var[2] and tie[0] > 0 and (tie[1] > 0) != (tie[2] > 0) and tie[3] == 0, tie
    zer = vec(sep[at["var_zero_inside_top_t3"]][0])
    assert (zer > 0).sum() == 2, zer
    four = sep[at["compose_four_combinations"]]
    dense = fo.COMPOSE_CASES["compose_four_combinations"]["dense"]
    assert sorted(len(vec(v)) for v in four[:4]) == [9, 12, 16, 19]
    alloff = sep[at["compose_all_off"]]
    assert fo.same_bits(vec(alloff[1]), dense[1]), "a sumSq == 0 row is left as it is"
    assert vec(alloff[2])[4] == 1.0 and (np.delete(vec(alloff[2]), 4) == 0).all(), "the smallest norm there is"
    assert (vec(alloff[3]) == 0).all(), "a norm that rounds to inf"
    nan = sep[at["compose_nan_alpha"]]
    assert (vec(nan[1])[:9] == 0).all() and (vec(nan[5])[:9] == 0).all() and np.isnan(vec(nan[1])[9:12]).all(), "a NaN alpha: aD = 0.0f"
    assert len(vec(sep[at["compose_matryoshka_kept3"]][0])) == 3 and sep[at["compose_no_weight_kept"]][0] == ""
    digests = {"aggregate": fo.aggregate_digest()}
    digests.update({n: fo.variance_digest(n) for n in fo.VARIANCE_CASES})
    digests.update({n: fo.compose_digest(n) for n in fo.COMPOSE_CASES})
    for i, n in enumerate(names):
        out["cases"].append({"name": n, "sha256": digests[n], "separate": sep[i], "fused": fus[i], "forms_differ": sep[i] != fus[i]})
    path = os.path.join(HERE, "features.json")
    with open(path, "w") as f:
        f.write('{"source": %s,\n "forms": %s,\n "cases": [\n' % (json.dumps(out["source"]), json.dumps(out["forms"])))
        f.write(",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in out["cases"]))
        f.write("\n]}\n")
    print(path, os.path.getsize(path), "bytes", out["forms"], "flip cases whose forms differ:", differ)


if __name__ == "__main__":
    main()
