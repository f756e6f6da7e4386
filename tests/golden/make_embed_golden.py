"""Generates tests/golden/embed_pool.json from the REFERENCE'S OWN pooling head: the rank-3 batch block and the rank-2 block of
OnnxModelSession::runOnnxBatch.

    python tests/golden/make_embed_golden.py [reference checkout]     (default /root/reference; dev container only)

The reference's translation unit (plugins/onnx/onnx_model_pool.cpp) needs ONNX Runtime headers that a test machine does not
have, so the two blocks are CUT out of it by anchors at generation time — from the line that sizes `result` to the line in
front of `return result;` — into files in a temporary directory; every anchor is asserted.  tests/cpp/embed_shell_test.cpp —
ours — built with -DEMBED_WITH_REFERENCE includes those files inside two functions that declare data, B, SS, DD, hidden_dim,
masks, pooling_mode_, normalize_ and result, reads the cases and prints the bits the reference's loops leave in `result`.  It is
built twice: -ffp-contract=off and -ffp-contract=fast -mfma.  Nothing of the reference, text or binary, is written into the
repository.

Per case the file holds the SHA-256 of the input bits and the output bits.  The generator asserts, on what the REFERENCE
returned:
  - the two builds agree on every case (masks of 0 and 1: form-free);
  - at least four MEAN cases change bits when their tokens are summed in reverse order (the reference run on the reversed
    texts), at least four when the terms are summed pairwise, at least two when v / total becomes v * (1 / total);
  - a NaN or an infinity planted in a masked row changes nothing (the reference run with those rows zeroed gives the same bits);
  - a NaN in an active row gives a row of zeros under normalisation; an all-masked text gives zeros;
  - CLS copies a masked first token, and -0.0f keeps its sign through the normalisation;
  - MAX of all-negative tokens is +0.0f; a norm at or below 1e-8 gives zeros, one just above is served;
  - subnormal means are non-zero; a row of FLT_MAX / 4 values normalises to finite values."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _embed_oracle as eo  # noqa: E402

CUTS = [("embed_ref_rank3.inc", "result.resize(B, std::vector<float>(hidden_dim, 0.0f));", 60),
        ("embed_ref_rank2.inc", "result.resize(B);", 30)]


def cut(ref, tmp):
    lines = open(os.path.join(ref, "plugins", "onnx", "onnx_model_pool.cpp")).read().splitlines()
    for name, anchor, longest in CUTS:
        starts = [i for i, l in enumerate(lines) if l.strip() == anchor]
        assert len(starts) == 1, ("anchor not found exactly once", anchor, starts)
        end = next(i for i in range(starts[0] + 1, len(lines)) if lines[i].strip() == "return result;")
        assert end - starts[0] < longest, (anchor, "the block is longer than expected")
        block = lines[starts[0]:end]
        assert "normalize_" in "\n".join(block) and ("pooling_mode_" in "\n".join(block)) == (name == "embed_ref_rank3.inc"), anchor
        with open(os.path.join(tmp, name), "w") as f:
            f.write("\n".join(block) + "\n")


def build(tmp, name, flags):
    cxx = os.environ.get("CXX", "g++")
    exe = os.path.join(tmp, name)
    subprocess.run([cxx, "-std=c++20", "-O2", *flags, "-DEMBED_WITH_REFERENCE", "-I" + tmp, os.path.join(ROOT, "tests", "cpp", "embed_shell_test.cpp"),
                    "-o", exe], check=True)
    return exe


def run(exe, tmp, cases):
    path = os.path.join(tmp, "cases.bin")
    eo.write_case_list(path, cases)
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-500:])
    got = eo.parse_driver_output(r.stdout)[1]
    assert len(got) == len(cases)
    return got


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    names = eo.case_names()
    pool, rank2 = eo.pool_cases(), eo.rank2_cases()
    every = list(pool.values()) + list(rank2.values())
    means = [n for n, c in pool.items() if c["mode"] == eo.MEAN and c["mask"].shape[1] == c["hidden"].shape[1] and c["hidden"].shape[1] > 2]
    with tempfile.TemporaryDirectory() as tmp:
        cut(ref, tmp)
        builds = {form: build(tmp, "ref_" + form, flags) for form, flags in (("separate", ["-ffp-contract=off"]), ("fused", ["-ffp-contract=fast", "-mfma"]))}
        got = {form: run(exe, tmp, every) for form, exe in builds.items()}
        assert got["separate"] == got["fused"], [n for n, a, b in zip(names, got["separate"], got["fused"]) if a != b]
        ref_out = got["separate"]
        # the reference on the reversed texts, and on the texts whose masked rows are zeroed
        reversed_out = dict(zip(means, run(builds["separate"], tmp, [eo.reversed_case(pool[n]) for n in means])))
        planted = ["nan_masked_mean", "nan_masked_max"]
        zeroed = []
        for n in planted:
            c = dict(pool[n])
            x = c["hidden"].copy()
            x[c["mask"] <= 0] = 0.0
            assert np.isnan(c["hidden"]).any() and np.isinf(c["hidden"]).any() and np.isfinite(x).all()
            c["hidden"] = x
            zeroed.append(c)
        zeroed_out = dict(zip(planted, run(builds["separate"], tmp, zeroed)))
    at = {n: i for i, n in enumerate(names)}
    vec = lambda n: eo.from_hex(ref_out[at[n]])      # noqa: E731
    # ---- the conditions the tests rely on, on what came back ----
    order = sum(reversed_out[n] != ref_out[at[n]] for n in means)
    assert order >= 4, "reversing the tokens must change at least 4 MEAN cases, got %d" % order
    tree = sum(eo.hexbits(eo.pool_py(pool[n]["hidden"], pool[n]["mask"], eo.MEAN, pool[n]["normalize"], pairwise=True)) != ref_out[at[n]] for n in means)
    assert tree >= 4, "a pairwise sum must change at least 4 MEAN cases, got %d" % tree
    recip = sum(eo.hexbits(eo.pool_py(pool[n]["hidden"], pool[n]["mask"], eo.MEAN, pool[n]["normalize"], reciprocal=True)) != ref_out[at[n]] for n in means)
    assert recip >= 2, "v * (1 / total) must change at least 2 MEAN cases, got %d" % recip
    for n in planted:
        assert zeroed_out[n] == ref_out[at[n]] and np.isfinite(vec(n)).all(), (n, "a masked row reached the output")
    d = pool["nan_active_mean"]["hidden"].shape[2]
    assert not vec("nan_active_mean")[:d].any() and vec("nan_active_mean")[d:].any(), "a NaN norm: a row of zeros"
    assert np.isnan(vec("nan_active_mean_raw")[:d]).sum() == 1
    row = vec("inf_active_max")[:d]
    assert np.isnan(row).sum() == 1 and not row[~np.isnan(row)].any(), "an infinite norm: inf / inf is NaN, v / inf is zero"
    d = pool["all_masked_mean"]["hidden"].shape[2]
    assert not eo.bits(vec("all_masked_mean")[:d]).any() and vec("all_masked_mean")[d:].any()
    assert not eo.bits(vec("all_masked_max")[:d]).any() and not eo.bits(vec("no_mask_mean")).any()
    cls = vec("cls_masked_first")
    assert eo.bits(cls[:1])[0] == 0x80000000 and cls[1] == np.float32(0.6) and cls[3] == np.float32(-0.8), cls[:4]
    assert not eo.bits(vec("max_all_negative")).any(), "MAX of all-negative tokens is +0.0f"
    assert not vec("norm_tiny")[:3].any() and vec("norm_just_above")[0] > 0.9
    sub = vec("subnormal_mean")
    assert sub.all() and (np.abs(sub) < 1.2e-38).all(), sub
    big = vec("flt_max_quarter")
    assert np.isfinite(big).all() and big[0] > 0.4 and big[1] == 0
    r2 = vec("rank2_specials").reshape(-1, 3)
    assert not r2[0].any() and np.isnan(r2[1][0]) and not r2[1][1:].any() and eo.bits(r2[2])[0] == 0x80000000 and not r2[3].any() and r2[4][0] > 0.9 and np.isfinite(r2[5]).all()
    path = os.path.join(HERE, "embed_pool.json")
    with open(path, "w") as f:
        f.write('{"source": %s,\n "builds_agree": true,\n "cases": [\n' % json.dumps(
            "the rank-3 batch block and the rank-2 block of OnnxModelSession::runOnnxBatch (plugins/onnx/onnx_model_pool.cpp)"))
        f.write(",\n".join("  " + json.dumps({"name": n, "sha256": eo.case_digest(n), "out": ref_out[i]}, separators=(",", ":"))
                           for i, n in enumerate(names)))
        f.write("\n]}\n")
    print(path, os.path.getsize(path), "bytes; MEAN cases that tell: order", order, "pairwise", tree, "reciprocal", recip, "of", len(means))


if __name__ == "__main__":
    main()
