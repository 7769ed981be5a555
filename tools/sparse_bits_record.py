"""The bits of the sparse model's results on two small models, as hex strings of the fp64 words (one GPU; needs the built
library):

    python tools/sparse_bits_record.py tests/golden/sparse_own_bits.json

tests/test_gpu_sparse.py::test_own_y_and_targets_keep_the_recorded_bits computes the same quantities by results() below and
compares them to the file bit for bit.  The file in the tree was written by this script at commit abba926, the last one
with a kernel family of its own for the handle's y (k_sparse_wty, k_sparse_yy, k_sparse_h, k_sparse_finalize): it holds the
one family that replaced them to that commit's arithmetic.  Record it again only when a change of the arithmetic is meant.

The models (data: conftest.synth; Z: the first m rows scaled by 0.9; 5 test rows: the first 5 scaled by 0.5):
  a   SE isotropic, n = 300, m = 65, d = 3, chunk_rows = 128      three chunks with a ragged last one, mpad 128 with columns
                                                                  to mask, W recomputed in the gradient pass
  b   Matern 5/2 ARD, n = 200, m = 130, d = 3, chunk_rows = 256   one chunk (W is still there), mpad 256, two M tiles, the
                                                                  ARD trace sweeps
Per model: bound, bound_grad, bound_grad_z, predict, predict_joint, predict_grad for the handle's own y; for model a also
bound_grad_targets with p = 1 and p = 3 (the matrix route of the small solves, the weights and the final sums).
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

MODELS = {
    "a": dict(n=300, m=65, d=3, chunk_rows=128, kernel="se", ard=False, theta=[1.0, 0.2, -1.0], targets=(1, 3)),
    "b": dict(n=200, m=130, d=3, chunk_rows=256, kernel="matern52_ard", ard=False, theta=[1.2, 0.9, 1.1, 0.1, -0.8], targets=()),
}
NT = 5


def hexwords(a):
    return ["%016x" % w for w in np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64)]


def results(name):
    """{quantity: hex words} of model `name` on the loaded library."""
    import cugp_amd.gp as gp
    from conftest import synth
    c = MODELS[name]
    X, y = synth(c["n"], c["d"], seed=15618)
    Z, Xt = np.ascontiguousarray(X[:c["m"]] * 0.9), np.ascontiguousarray(X[:NT] * 0.5)
    Y = np.ascontiguousarray(np.column_stack([y, np.cos(X[:, 1]), 0.3 * X[:, 2]]))
    out = {}

    def fresh():
        s = gp.SparseGP(c["n"], c["m"], c["d"], kernel=c["kernel"], ard=c["ard"], chunk_rows=c["chunk_rows"])
        s.set_data(X, y)
        s.set_inducing(Z)
        s.set_loghyperparam(c["theta"])
        return s
    s = fresh()
    out["bound"] = hexwords(s.bound())
    for k, v in zip(("F", "g"), s.bound_grad()):
        out["bound_grad." + k] = hexwords(v)
    for k, v in zip(("F", "g", "gZ"), s.bound_grad_z()):
        out["bound_grad_z." + k] = hexwords(v)
    for k, v in zip(("mean", "var"), s.predict(Xt)):
        out["predict." + k] = hexwords(v)
    for k, v in zip(("mean", "cov"), s.predict_joint(Xt)):
        out["predict_joint." + k] = hexwords(v)
    for k, v in zip(("mean", "var", "dmean", "dvar"), s.predict_grad(Xt)):
        out["predict_grad." + k] = hexwords(v)
    s.close()
    s = fresh()                                                 # (a prediction first: it evaluates the bound itself)
    for k, v in zip(("mean", "var"), s.predict(Xt)):
        out["predict_first." + k] = hexwords(v)
    for p in c["targets"]:
        s.set_targets(Y[:, :p])
        for k, v in zip(("F", "g", "F_each"), s.bound_grad_targets()):
            out["bound_grad_targets_p%d.%s" % (p, k)] = hexwords(v)
    s.close()
    return out


if __name__ == "__main__":
    rec = {name: results(name) for name in MODELS}
    with open(sys.argv[1], "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %s" % (sys.argv[1], ", ".join("%s %d words" % (k, sum(len(v) for v in r.values())) for k, r in rec.items())))
