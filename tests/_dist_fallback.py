"""The Python merge tests/_dist_worker.py falls back to where no GPU is visible (the CPU suite): a restatement of the cosine
comparator without tie ranks, (similarity desc, row asc).  A fallback of THAT TEST only — the product has no CPU path;
tests/test_merge_model_cpu.py holds it to tests/_merge_model.py.  Works on numpy arrays and on torch tensors alike."""


def python_merge(g, out, world, nq, k):
    """g: gathered "scores" / "rows" [world][nq][k] and "counts" [world][nq]; out: "scores" / "rows" [nq][k], "counts" [nq]
    (slots behind a count are left as they were)."""
    for qi in range(nq):
        ent = [(-float(g["scores"][s, qi, i]), int(g["rows"][s, qi, i]))
               for s in range(world) for i in range(int(g["counts"][s, qi]))]
        ent.sort()
        ent = ent[:k]
        out["counts"][qi] = len(ent)
        for i, e in enumerate(ent):
            out["scores"][qi, i] = -e[0]; out["rows"][qi, i] = e[1]
