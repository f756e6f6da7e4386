"""Generates tests/golden/cluster_route.json from the REFERENCE'S OWN SparseGuidedClusterRouter::buildRouteIndex and ::route.

    python tests/golden/make_route_golden.py [reference checkout]     (default /root/reference; dev container only)

The reference's topology_baseline.cpp is compiled as it is (-O2 -ffp-contract=off, so that the blend is the uncontracted float
expression) and linked with tests/cpp/route_shell_test.cpp built with -DROUTE_WITH_REFERENCE — ours: it reads a case, calls the
reference's two functions and prints what they return — and with that file's stand-in StaticCosineAnnIndex: its build fails
unless the case asks for a candidate mask, and then it answers with the first clusters.  Nothing of the reference, text or
binary, is written into the repository: the build lives in a temporary directory.

Per case (inputs: tests/_route_oracle.py GOLDEN_CASES) the file holds the SHA-256 of the input bits, the bits of the index's
norms (centroidNorms and routingRepresentativeNorms, cluster after cluster), the full ordered route list (cluster id,
routeScore, semanticCost = 1 - dense, sparseCost; doubles as hex, absent = null: semanticCost present is denseObserved) and
the work counters."""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _route_oracle as ro  # noqa: E402


def build(ref, tmp):
    exe = os.path.join(tmp, "ref_route")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++20", "-O2", "-ffp-contract=off", "-DROUTE_WITH_REFERENCE",
           "-I" + os.path.join(ROOT, "oracle", "shim"), "-I" + os.path.join(ref, "include"), "-I" + os.path.join(ref, "src", "topology"),
           os.path.join(ROOT, "tests", "cpp", "route_shell_test.cpp"), os.path.join(ref, "src", "topology", "topology_baseline.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    cases = []
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(ref, tmp)
        for name, case in ro.GOLDEN_CASES.items():
            path = os.path.join(tmp, "case.bin")
            ro.write_case(path, case)
            r = subprocess.run([exe, path], capture_output=True, text=True)
            assert r.returncode == 0, (name, r.returncode, r.stderr[-500:])
            got = ro.parse_driver(r.stdout)
            assert "error" not in got, (name, got)
            cases.append({"name": name, "sha256": ro.case_digest(case), **got})
            print(name, len(got["routes"]), "routes", got["work"])
    path = os.path.join(HERE, "cluster_route.json")
    source = "SparseGuidedClusterRouter::buildRouteIndex / ::route (src/topology/topology_baseline.cpp), -O2 -ffp-contract=off; " \
             "stand-in ANN index (tests/cpp/route_shell_test.cpp)"
    with open(path, "w") as f:
        f.write('{"source": %s,\n "cases": [\n' % json.dumps(source))
        f.write(",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in cases))
        f.write("\n]}\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
