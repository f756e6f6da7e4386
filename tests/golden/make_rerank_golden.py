"""Generates tests/golden/colbert_maxsim.json from the REFERENCE'S OWN computeMaxSim, dot, maxPoolEmbeddings and
normalizeEmbedding.

    python tests/golden/make_rerank_golden.py [reference checkout]     (default /root/reference; dev container only)

The reference's translation unit (plugins/onnx/onnx_colbert_session.cpp) needs ONNX Runtime headers that a test machine does
not have, so the four member functions are CUT out of it by anchors at generation time — each from its signature line to the
closing brace at member indentation — into a file in a temporary directory; every anchor is asserted.
tests/cpp/rerank_shell_test.cpp — ours — built with -DRERANK_WITH_REFERENCE includes that file inside a struct, reads the cases
and prints the bits the reference's functions return.  It is built twice: -ffp-contract=off (the SEPARATE form) and
-ffp-contract=fast -mfma (FUSED, where this compiler emits the fma).  Which form a build really has is judged on the flip
cases: a build whose scores there are not the form's it was made for is replaced by the restatement, and the file says so.
Nothing of the reference, text or binary, is written into the repository.

Per case and form the file holds the SHA-256 of the input bits and the bits of the output.  The generator asserts the conditions
the tests rely on, on what the REFERENCE returned:
  - the two forms give different score bits in at least 4 of the flip cases;
  - an empty document scores -inf; an empty query scores +0.0f;
  - a NaN document token is skipped (the score is the one without it); a NaN query token gives -inf;
  - a +inf / -inf pair of row maxima gives NaN; the subnormal-only case is non-zero;
  - pooling maps an all-NaN dimension to 0.0f and a norm at or below 1e-8 to a row of zeros."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _rerank_oracle as ro  # noqa: E402

ANCHORS = ["std::vector<float> maxPoolEmbeddings(const ColbertEmbeddings& embeddings, size_t dim) const {",
           "void normalizeEmbedding(std::vector<float>& vec) const {",
           "float computeMaxSim(const ColbertEmbeddings& query, const ColbertEmbeddings& document) const {",
           "float dot(const std::vector<float>& a, const std::vector<float>& b) const {"]


def cut(ref, tmp):
    lines = open(os.path.join(ref, "plugins", "onnx", "onnx_colbert_session.cpp")).read().splitlines()
    out = []
    for anchor in ANCHORS:
        starts = [i for i, l in enumerate(lines) if l.strip() == anchor]
        assert len(starts) == 1, ("anchor not found exactly once", anchor, starts)
        end = next(i for i in range(starts[0] + 1, len(lines)) if lines[i] == "    }")
        assert end - starts[0] < 40, (anchor, "the member function is longer than expected")
        out += lines[starts[0]:end + 1] + [""]
    with open(os.path.join(tmp, "rerank_ref_cut.inc"), "w") as f:
        f.write("\n".join(out) + "\n")


def build(tmp, name, flags):
    cxx = os.environ.get("CXX", "g++")
    exe = os.path.join(tmp, name)
    subprocess.run([cxx, "-std=c++20", "-O2", *flags, "-DRERANK_WITH_REFERENCE", "-I" + tmp, os.path.join(ROOT, "tests", "cpp", "rerank_shell_test.cpp"),
                    "-o", exe], check=True)
    return exe


def vec(h):
    return ro.from_hex(h)


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    names = ro.case_names()
    flips = [i for i, n in enumerate(names) if n.startswith("flip_")]
    out = {"source": "computeMaxSim, dot, maxPoolEmbeddings, normalizeEmbedding (plugins/onnx/onnx_colbert_session.cpp)", "forms": {}}
    returned = {}
    with tempfile.TemporaryDirectory() as tmp:
        cut(ref, tmp)
        cases = os.path.join(tmp, "cases.bin")
        ro.write_cases(cases)
        for form, flags in (("separate", ["-ffp-contract=off"]), ("fused", ["-ffp-contract=fast", "-mfma"])):
            exe = build(tmp, "ref_" + form, flags)
            r = subprocess.run([exe, cases], capture_output=True, text=True)
            assert r.returncode == 0, (form, r.returncode, r.stderr[-500:])
            _, got = ro.parse_driver_output(r.stdout)
            assert len(got) == len(names)
            want = ro.restated(ro.FORMS[form])
            if all(got[i] == want[i] for i in flips):
                out["forms"][form] = "the reference's member functions, this compiler"
                returned[form] = got
            else:      # this compiler did not give the build that form: the restatement stands in, and the file says so
                other = ro.restated(1 - ro.FORMS[form])
                out["forms"][form] = "tests/_rerank_oracle.py (the reference build has the %s form)" % (
                    "other" if all(got[i] == other[i] for i in flips) else "neither")
                returned[form] = want
    sep, fus = returned["separate"], returned["fused"]
    at = {n: i for i, n in enumerate(names)}
    # ---- the conditions the tests rely on, on what came back ----
    differ = sum(sep[i] != fus[i] for i in flips)
    assert differ >= 4, "the two forms must give different scores in at least 4 flip cases, got %d" % differ
    ms = ro.maxsim_cases()
    for got in (sep, fus):
        assert vec(got[at["empty_document"]])[0] == -np.inf
        assert ro.hexbits(vec(got[at["empty_query"]])) == "00000000", "an empty query scores +0.0f"
        # the NaN tokens skipped: q0 = (1, 2) meets (1, 1) only -> 3; q1 = (3, -1) meets (1, 1) only -> 2
        assert vec(got[at["nan_document_token"]])[0] == 5.0, vec(got[at["nan_document_token"]])
        assert vec(got[at["nan_query_token"]])[0] == -np.inf
        assert np.isnan(vec(got[at["inf_pair"]])[0])
        assert vec(got[at["subnormal_only"]])[0] != 0 and abs(vec(got[at["subnormal_only"]])[0]) < 1e-37
        assert len(vec(got[at["window_mixed_lengths"]])) == 5 and vec(got[at["window_mixed_lengths"]])[1] == -np.inf
        pn = vec(got[at["pool_all_nan_dimension"]])
        assert pn[0] == 0.0 and not np.signbit(pn[0]) and pn[1] > 0
        assert not vec(got[at["pool_tiny_norm"]]).any(), "a norm at or below 1e-8: zeros"
        assert vec(got[at["pool_just_above"]])[0] > 0.9, "a norm just above 1e-8 is served"
        assert not vec(got[at["pool_nonfinite"]])[[0, 2]].any()
    for n in ro.pool_cases():
        assert sep[at[n]] == fus[at[n]], (n, "pooling is form-free")
    del ms
    with open(os.path.join(HERE, "colbert_maxsim.json"), "w") as f:
        f.write('{"source": %s,\n "forms": %s,\n "cases": [\n' % (json.dumps(out["source"]), json.dumps(out["forms"])))
        f.write(",\n".join("  " + json.dumps({"name": n, "sha256": ro.case_digest(n), "separate": sep[i], "fused": fus[i],
                                              "forms_differ": sep[i] != fus[i]}, separators=(",", ":")) for i, n in enumerate(names)))
        f.write("\n]}\n")
    path = os.path.join(HERE, "colbert_maxsim.json")
    print(path, os.path.getsize(path), "bytes", out["forms"], "flip cases whose forms differ:", differ)


if __name__ == "__main__":
    main()
