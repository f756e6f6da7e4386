"""Generates tests/golden/cluster_artifacts.json from the REFERENCE'S OWN selectDiverseRoutingRepresentatives,
applyOrthogonalBoundarySpill and detail::meanEmbedding.

    python tests/golden/make_artifacts_golden.py [reference checkout]     (default /root/reference; dev container only)

The reference's topology_representatives.cpp is compiled as it is and linked with tests/cpp/artifacts_shell_test.cpp built with
-DARTIFACTS_WITH_REFERENCE — ours: it reads a case, calls the reference's functions and prints what they return — and with that
file's stand-in StaticCosineAnnIndex, whose build fails: an admissible path (`if (built)` is false) on which every cluster is a
candidate.  Two builds: -ffp-contract=off (the SEPARATE form) and -ffp-contract=fast -mfma (FUSED, where this compiler emits
the fma; the driver's probe says which form each build really has, and a build whose probe does not say "fused" is replaced by
the restatement of tests/_artifacts_oracle.py, which the file then records).  Nothing of the reference, text or binary, is
written into the repository: the builds live in a temporary directory.

Per case (inputs: tests/_artifacts_oracle.py GOLDEN_CASES) and form the file holds the SHA-256 of the input bits, the bits of
every cluster's mean embedding, the selected hashes per cluster, the assignment count, the overlap ids per membership and the
member lists after the spill."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _artifacts_oracle as ao  # noqa: E402


def build(ref, tmp, name, flags):
    exe = os.path.join(tmp, name)
    cmd = [os.environ.get("CXX", "g++"), "-std=c++20", "-O2", *flags, "-DARTIFACTS_WITH_REFERENCE", "-DYAMS_ACCEL_USE_HOST_TYPES",
           "-I" + os.path.join(ROOT, "oracle", "shim"), "-I" + os.path.join(ref, "include"), "-I" + os.path.join(ref, "src", "topology"),
           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "artifacts_shell_test.cpp"),
           os.path.join(ref, "src", "topology", "topology_representatives.cpp"), "-ldl", "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def input_digest(docs, clusters, memberships, cfg):
    return ao.digest(*[np.asarray(d["emb"], np.float32) for d in docs],
                     np.frombuffer(json.dumps([[d["hash"] for d in docs], clusters, [[m["hash"], m["cluster"], m["role_outlier"]] for m in memberships],
                                               cfg], sort_keys=True).encode(), np.uint8))


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    out = {"source": "selectDiverseRoutingRepresentatives / applyOrthogonalBoundarySpill (src/topology/topology_representatives.cpp), "
                     "detail::meanEmbedding (src/topology/topology_build_utils.h); stand-in ANN index whose build fails",
           "forms": {}, "cases": []}
    with tempfile.TemporaryDirectory() as tmp:
        exes = {"separate": build(ref, tmp, "ref_separate", ["-ffp-contract=off"]),
                "fused": build(ref, tmp, "ref_fused", ["-ffp-contract=fast", "-mfma"])}
        for name, make in ao.GOLDEN_CASES.items():
            case = {"name": name}
            for form, exe in exes.items():
                docs, clusters, memberships, cfg = make()
                case["sha256"] = input_digest(docs, clusters, memberships, cfg)
                case["n"] = len(docs)
                path = os.path.join(tmp, "case.bin")
                ao.write_case(path, docs, clusters, memberships, cfg)
                r = subprocess.run([exe, path], capture_output=True, text=True)
                assert r.returncode == 0, (name, form, r.returncode, r.stderr[-500:])
                got = ao.parse_driver(r.stdout)
                probe = got.pop("probe")
                if probe == form:
                    out["forms"][form] = "the reference's translation unit, this compiler"
                else:      # this compiler did not give the build that form: the restatement stands in, and the file says so
                    out["forms"][form] = "tests/_artifacts_oracle.py (the reference build probed as '%s')" % probe
                    got = ao.run_case(docs, clusters, memberships, cfg, ao.FUSED if form == "fused" else ao.SEPARATE)
                case[form] = got
            cases_differ = case["separate"] != case["fused"]
            out["cases"].append(case)
            print(name, case["n"], "documents; forms differ in the result:", cases_differ)
    path = os.path.join(HERE, "cluster_artifacts.json")
    with open(path, "w") as f:
        f.write('{"source": %s,\n "forms": %s,\n "cases": [\n' % (json.dumps(out["source"]), json.dumps(out["forms"])))
        f.write(",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in out["cases"]))
        f.write("\n]}\n")
    print(path, os.path.getsize(path), "bytes", out["forms"])


if __name__ == "__main__":
    main()
