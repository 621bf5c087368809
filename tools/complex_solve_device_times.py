#!/usr/bin/env python3
"""Device time of the solves with a complex factor, sys = A, on a Hermitian matrix on Poisson's pattern.

    python tools/complex_solve_device_times.py [--out profiles/complex_solve_device_times.json] [--cases h3d_64,h3d_96]

Per case and nrhs in {1, 8, 16, 64}, stats [24] in ms (median of five after a warm-up) of
  device_cx_ms    Session.solve_device, the factor in complex storage (the CX forms of the column / panel kernels)
  device_twin_ms  the same with CHOLMOD_HIP_CX_TWIN=1: the full twin on the real kernels (twice the bytes of L)
  host_array_ms   Session.solve on the complex-storage factor: the host-array path, L read once per right-hand side
  real_device_ms  Session.solve_device of the REAL matrix on the same pattern
torch is imported before the engine library is loaded so that the two share one HIP runtime."""
import torch  # noqa: E402  (first)

import argparse
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from suitesparse_amd import cholmod as ch          # noqa: E402
from suitesparse_amd import generators as G        # noqa: E402

CASES = {
    "h3d_64": lambda: G.poisson3d(64) + (G.geometric_nd(64, 64, 64, 4),),
    "h3d_96": lambda: G.poisson3d(96) + (G.geometric_nd(96, 96, 96, 4),),
}
NRHS = [1, 8, 16, 64]


def hermitian_from(n, Ap, Ai, Ax, seed=0, scale=0.9):
    """every off-diagonal entry of the real SPD matrix turned by a random phase and shrunk (tests/test_complex.py)"""
    rng = np.random.default_rng(seed)
    Al = sp.tril(sp.csc_matrix((Ax, Ai, Ap), shape=(n, n))).tocsc()
    Al.sort_indices()
    vals = Al.data.astype(np.complex128)
    off = Al.indices != np.repeat(np.arange(n), np.diff(Al.indptr))
    vals[off] *= scale * np.exp(1j * rng.uniform(0, 2 * np.pi, int(off.sum())))
    return Al.indptr.astype(np.int64), Al.indices.astype(np.int64), vals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default=",".join(CASES))
    a = ap.parse_args()
    torch.cuda.init()
    res = {"device": torch.cuda.get_device_name(0), "timer": "stats [24], ms, median of five after a warm-up", "cases": {}}
    for name in a.cases.split(","):
        n, Ap, Ai, Ax, perm = CASES[name]()
        cAp, cAi, cAx = hermitian_from(n, Ap, Ai, Ax)
        rng = np.random.default_rng(0)
        rhs = {k: rng.standard_normal((k, n)) + 1j * rng.standard_normal((k, n)) for k in NRHS}
        cols = {k: {} for k in NRHS}
        info = {"n": n}
        for form in ("cx", "twin", "real"):
            if form == "twin":
                os.environ["CHOLMOD_HIP_CX_TWIN"] = "1"
            else:
                os.environ.pop("CHOLMOD_HIP_CX_TWIN", None)
            S = ch.Session(factor_on_device=True)
            A = S.sparse(n, Ap, Ai, Ax, -1) if form == "real" else S.sparse(n, cAp, cAi, cAx, -1)
            Lf = S.analyze(A, perm)
            assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
            info["xsize_complex_entries"] = int(Lf.contents.xsize)
            info[f"factor_bytes_{form}"] = float(S.hip_stats(Lf)[5])

            def med(run):
                run()
                t = []
                for _ in range(5):
                    run()
                    t.append(1e3 * float(S.hip_stats(Lf)[24]))
                return float(np.median(t))

            for k in NRHS:
                b = rhs[k].real.copy() if form == "real" else rhs[k]
                B = torch.from_numpy(b).cuda()
                key = {"cx": "device_cx_ms", "twin": "device_twin_ms", "real": "real_device_ms"}[form]
                cols[k][key] = med(lambda: S.solve_device(Lf, B))
                if form == "cx":
                    cols[k]["host_array_ms"] = med(lambda: S.solve(Lf, b))
                print(f"{name} {form:4s} nrhs={k:3d}: " + "  ".join(f"{q} {v:.3f}" for q, v in cols[k].items()), flush=True)
            torch.cuda.synchronize()
            S.free_factor(Lf)
            S.free_sparse(A)
            S.finish()
        rows = []
        for k in NRHS:
            c = cols[k]
            rows.append(dict(nrhs=k, **c, host_array_over_device_cx=c["host_array_ms"] / c["device_cx_ms"],
                             device_twin_over_device_cx=c["device_twin_ms"] / c["device_cx_ms"],
                             device_cx_over_real_device=c["device_cx_ms"] / c["real_device_ms"]))
        info["rows"] = rows
        res["cases"][name] = info
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
