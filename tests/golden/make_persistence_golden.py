"""Generates tests/golden/persistence_h0.json from the REFERENCE'S OWN computePersistenceH0.

    python tests/golden/make_persistence_golden.py [reference checkout]     (default /root/reference; dev container only)

The reference's src/search/topological_quality.cpp is compiled as it is, twice — -ffp-contract=off (the SEPARATE form) and
-ffp-contract=fast -mfma (FUSED, where this compiler emits the fma) — and linked with tests/cpp/persistence_shell_test.cpp built
with -DPERSISTENCE_WITH_REFERENCE and -ffp-contract=off — ours: it reads the cases, calls the reference's function (both
overloads) and prints the bits it returns, after probing which chain form that build really has.  A build whose probe does not
report the form it was made for is replaced by the restatement of tests/_persistence_oracle.py, and the file says so.  Nothing
of the reference, text or binary, is written into the repository: the builds live in a temporary directory.

Per case (inputs: tests/_persistence_oracle.py GOLDEN_CASES) and form the file holds the SHA-256 of the input bits, the bits
the reference returned, and — marked as the restatement's — the restatement's value, percentile, index, merge count and the
digests of its distance matrix and merge weights.  The generator checks the conditions the tests rely on: the two forms return
different values in at least 4 of the small mixed-exponent cases, one lattice case has its percentile index strictly inside a
plateau, one duplicate case has norm = 0."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _persistence_oracle as po  # noqa: E402


def build(ref, tmp, name, flags):
    cxx = os.environ.get("CXX", "g++")
    inc = ["-I" + os.path.join(ROOT, "oracle", "shim"), "-I" + os.path.join(ref, "include"), "-I" + os.path.join(ROOT, "include")]
    tu, drv, exe = os.path.join(tmp, name + "_tu.o"), os.path.join(tmp, name + "_driver.o"), os.path.join(tmp, name)
    subprocess.run([cxx, "-std=c++20", "-O2", *flags, *inc, "-c", os.path.join(ref, "src", "search", "topological_quality.cpp"), "-o", tu], check=True)
    subprocess.run([cxx, "-std=c++20", "-O2", "-ffp-contract=off", "-DPERSISTENCE_WITH_REFERENCE", *inc, "-c",
                    os.path.join(ROOT, "tests", "cpp", "persistence_shell_test.cpp"), "-o", drv], check=True)
    subprocess.run([cxx, drv, tu, "-ldl", "-o", exe], check=True)
    return exe


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    out = {"source": "yams::search::computePersistenceH0 (src/search/topological_quality.cpp), both overloads", "forms": {}, "cases": []}
    names = list(po.GOLDEN_CASES)
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for i, name in enumerate(names):
            paths.append(os.path.join(tmp, "case_%03d.bin" % i))
            po.write_case(paths[-1], po.GOLDEN_CASES[name]())
        returned = {}
        for form, flags in (("separate", ["-ffp-contract=off"]), ("fused", ["-ffp-contract=fast", "-mfma"])):
            exe = build(ref, tmp, "ref_" + form, flags)
            r = subprocess.run([exe, *paths], capture_output=True, text=True)
            assert r.returncode == 0, (form, r.returncode, r.stderr[-500:])
            lines = r.stdout.split("\n")
            probe = lines[0].split()[1]
            values = [l.split()[1:] for l in lines[1:] if l.startswith("value")]
            assert len(values) == len(names) and all(a == b for a, b in values), "the two overloads disagree"
            if probe == form:
                out["forms"][form] = "the reference's translation unit, this compiler"
                returned[form] = [v[0] for v in values]
            else:      # this compiler did not give the build that form: the restatement stands in, and the file says so
                out["forms"][form] = "tests/_persistence_oracle.py (the reference build probed as '%s')" % probe
                returned[form] = [po.hex64(po.persistence_py(po.GOLDEN_CASES[n](), po.FORMS[form])["value"]) for n in names]
    differ = 0
    for i, name in enumerate(names):
        x = po.GOLDEN_CASES[name]()
        case = {"name": name, "m": int(x.shape[0]), "dim": int(x.shape[1]), "sha256": po.digest(x)}
        for form in ("separate", "fused"):
            case[form] = {"returned": returned[form][i], "restatement": po.golden_record(po.persistence_py(x, po.FORMS[form]))}
        case["forms_differ"] = case["separate"]["returned"] != case["fused"]["returned"]
        differ += case["forms_differ"] and name.startswith("mixed_")
        out["cases"].append(case)
        print(name, x.shape, "forms differ in the value:", case["forms_differ"])
    assert differ >= 4, "the two forms must return different values in at least 4 of the small mixed cases, got %d" % differ
    assert po.plateau_is_strictly_inside(po.GOLDEN_CASES["lattice_plateau_m30"]())
    assert po.persistence_py(po.GOLDEN_CASES["duplicates_norm_zero_m41"](), po.SEPARATE)["norm"] == 0.0
    path = os.path.join(HERE, "persistence_h0.json")
    with open(path, "w") as f:
        f.write('{"source": %s,\n "forms": %s,\n "cases": [\n' % (json.dumps(out["source"]), json.dumps(out["forms"])))
        f.write(",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in out["cases"]))
        f.write("\n]}\n")
    print(path, os.path.getsize(path), "bytes", out["forms"], "mixed cases whose forms differ:", differ)


if __name__ == "__main__":
    main()
