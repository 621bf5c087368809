#!/usr/bin/env python3
"""Device time of the triangular solves, host-array path (Session.solve: the per-right-hand-side kernels) against the
device-resident path (Session.solve_device: panels of 16 on the MFMA block kernels), sys = A.

    python tools/solve_device_time.py [--out profiles/solve_device_times.json] [--cases p3d_64,p3d_100,...]

Per case and nrhs in {1, 2, 4, 8, 16, 32, 64}: stats [24] in ms (median of five after a warm-up) for both paths, the
HBM rate of the device path as 2 * 8 * xsize * ceil (nrhs / 16) bytes over its time against 8 TB/s, and the wall time of
one nrhs = 1 solve through each entry point.  torch is imported before the engine library is loaded so that the two
share one HIP runtime."""
import torch  # noqa: E402  (first)

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from suitesparse_amd import cholmod as ch          # noqa: E402
from suitesparse_amd import generators as G        # noqa: E402

CASES = {
    "p3d_64": lambda: G.poisson3d(64) + (G.geometric_nd(64, 64, 64, 4),),
    "p3d_100": lambda: G.poisson3d(100) + (G.geometric_nd(100, 100, 100, 4),),
    "box50_r3": lambda: G.box_stencil3d(50, 3) + (G.geometric_nd(50, 50, 50, 6, 3),),
    "p2d_1259": lambda: G.poisson2d(1259) + (G.geometric_nd(1259, 1259, 1, 4),),
}
NRHS = [1, 2, 4, 8, 16, 32, 64]
HBM = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--once", type=int, default=0, help="one device solve of this nrhs per case and nothing else (for a kernel trace)")
    a = ap.parse_args()
    torch.cuda.init()
    res = {}
    for name in a.cases.split(","):
        n, Ap, Ai, Ax, perm = CASES[name]()
        S = ch.Session()
        A = S.sparse(n, Ap, Ai, Ax, -1)
        Lf = S.analyze(A, perm)
        assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
        xsize = int(Lf.contents.xsize)
        rng = np.random.default_rng(0)
        if a.once:
            B = torch.from_numpy(rng.standard_normal((a.once, n))).cuda()
            S.solve_device(Lf, B)
            torch.cuda.synchronize()
            continue
        rows = []
        for nrhs in NRHS:
            b = rng.standard_normal((nrhs, n))
            B = torch.from_numpy(b).cuda()

            def med(run):
                run()
                t = []
                for _ in range(5):
                    run()
                    t.append(1e3 * float(S.hip_stats(Lf)[24]))
                return float(np.median(t))

            th = med(lambda: S.solve(Lf, b))
            td = med(lambda: S.solve_device(Lf, B))
            rate = 2 * 8 * xsize * ((nrhs + 15) // 16) / (1e-3 * td)
            rows.append(dict(nrhs=nrhs, host_path_ms=th, device_path_ms=td, ratio=th / td, device_path_hbm_fraction=rate / HBM))
            print(f"{name} nrhs={nrhs:3d}: host path {th:9.3f} ms  device path {td:9.3f} ms  x{th / td:5.2f}  HBM {rate / HBM:.3f}", flush=True)
        b = rng.standard_normal(n)
        B = torch.from_numpy(b).cuda()
        wall = {}
        for key, run in (("host_path", lambda: S.solve(Lf, b)), ("device_path", lambda: S.solve_device(Lf, B))):
            run()
            torch.cuda.synchronize()
            t = []
            for _ in range(5):
                t0 = time.perf_counter()
                run()
                torch.cuda.synchronize()
                t.append(1e3 * (time.perf_counter() - t0))
            wall[key] = float(np.median(t))
        print(f"{name} nrhs=1 wall: host path {wall['host_path']:.3f} ms, device path {wall['device_path']:.3f} ms", flush=True)
        res[name] = dict(n=n, xsize=xsize, rows=rows, wall_ms_nrhs1=wall)
        torch.cuda.synchronize()
        S.free_factor(Lf)
        S.free_sparse(A)
        S.finish()
    if a.out and res:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
