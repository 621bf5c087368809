#!/usr/bin/env python3
"""Time one step of a loop that factorizes new values of one pattern: the values-only path of cholmod_l_factorize (values in
a host array: staging copy, DMA, gather; for A*A' the host product ssamd_aat first) against Session.factorize_device (values
in device memory: gather, or product kernel + gather, on the device).  Both calls return when the factorization has finished
on the device, so a host clock around the call is the step; the two kinds of step alternate in one process, the median of
--steps of each after --warmup of each is reported with min and max (the spread).  The host path is not touched by the
device entry: its step here is the step of the commit before it.
    python tools/values_device_times.py [--steps 12] [--warmup 2] [--p2d 1259] [--p3d 100] [--aat 100] [--out FILE]
Cases: the 2D stand-in (poisson2d) and Poisson 3D of BASELINE.json, and A*A' for the edge-node matrix of the 3D grid with
one unit column per node: tril (A*A') has the pattern of the 7-point Poisson matrix (nnz (C) as in the 3D case), A has
7 m^3 entries in 4 m^3 columns, the lists are 1 .. 7 products long."""
import torch  # noqa: E402  (first: torch and the engine share one HIP runtime)

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from suitesparse_amd import cholmod as ch  # noqa: E402
from suitesparse_amd import generators as G  # noqa: E402


def grid_incidence(m):
    """(nrow, ncol, Ap, Ai, Ax): column i < m^3 is the unit vector of node i (value 1.5), then one column per grid edge
    (i, j), i < j, with entries +w at i and -w at j"""
    n = m ** 3
    idx = np.arange(n, dtype=np.int64).reshape(m, m, m)
    lo = [idx[:-1, :, :].ravel(), idx[:, :-1, :].ravel(), idx[:, :, :-1].ravel()]
    hi = [idx[1:, :, :].ravel(), idx[:, 1:, :].ravel(), idx[:, :, 1:].ravel()]
    lo, hi = np.concatenate(lo), np.concatenate(hi)
    ne = len(lo)
    Ai = np.concatenate([np.arange(n, dtype=np.int64), np.stack([lo, hi], axis=1).ravel()])
    Ap = np.concatenate([np.arange(n + 1, dtype=np.int64), n + 2 * np.arange(1, ne + 1, dtype=np.int64)])
    w = 0.75 + 0.5 * ((np.arange(ne) * 2654435761) % 1000) / 1000.0
    Ax = np.concatenate([np.full(n, 1.5), np.stack([w, -w], axis=1).ravel()])
    return n, n + ne, Ap, Ai, Ax


def stats(t):
    t = np.asarray(t) * 1e3
    return {"median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max()), "steps": len(t)}


def run_case(name, S, A, Lf, values, beta, steps, warmup):
    """values: the host array A->x is refreshed from; the device tensor holds the same numbers"""
    nz = len(values)
    ax = ch._view(A.contents.x, nz, C.c_double, np.float64)
    vd = torch.from_numpy(values).cuda()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    assert S.factorize_device(A, vd, Lf, beta) == 1 and S.cm.status == ch.OK      # (A*A': builds the product map)
    first_device_call = time.perf_counter() - t0
    th, td, tc = [], [], []
    for k in range(warmup + steps):
        scale = 1.0 + 0.01 * (k % 5)
        v = values * scale
        vd = torch.from_numpy(v).cuda()
        torch.cuda.synchronize()
        # host step: the values are in a host array already
        ax[:] = v
        t0 = time.perf_counter()
        ok = S.factorize(A, Lf, beta)
        t1 = time.perf_counter()
        assert ok == 1 and S.cm.status == ch.OK
        # host step as a PyTorch user pays it: the device tensor comes to the host first
        t2 = time.perf_counter()
        ax[:] = vd.cpu().numpy()
        ok = S.factorize(A, Lf, beta)
        t3 = time.perf_counter()
        assert ok == 1 and S.cm.status == ch.OK
        # device step
        t4 = time.perf_counter()
        ok = S.factorize_device(A, vd, Lf, beta)
        t5 = time.perf_counter()
        assert ok == 1 and S.cm.status == ch.OK
        if k >= warmup:
            th.append(t1 - t0)
            tc.append(t3 - t2)
            td.append(t5 - t4)
    dev_ms = float(S.hip_stats(Lf)[0]) * 1e3
    r = {"case": name, "n": int(Lf.contents.n), "nnz_A": nz, "nnz_resident_S": int(Lf.contents.hip_apat_nnz) if A.contents.stype == 0 else None,
         "host_values_only_step": stats(th), "host_step_after_values_cpu": stats(tc), "device_values_step": stats(td),
         "factorization_kernels_ms_last_step": dev_ms, "first_device_call_ms": first_device_call * 1e3}
    h, d = r["host_values_only_step"], r["device_values_step"]
    r["device_not_slower_than_host_beyond_its_spread"] = bool(d["median_ms"] <= h["median_ms"] + (h["max_ms"] - h["min_ms"]))
    print(json.dumps(r))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--p2d", type=int, default=1259)
    ap.add_argument("--p3d", type=int, default=100)
    ap.add_argument("--aat", type=int, default=100)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    torch.cuda.init()
    out = {"what": "wall time of one values-only factorization step, host clock around a call that returns when the "
                   "factorization has finished on the device; host and device steps alternate in one process",
           "command": "python tools/values_device_times.py " + " ".join(sys.argv[1:]),
           "device": torch.cuda.get_device_name(0), "cases": []}
    for wl, m in (("poisson2d", a.p2d), ("poisson3d", a.p3d)):
        if m <= 0:
            continue
        n, Ap, Ai, Ax = (G.poisson2d if wl == "poisson2d" else G.poisson3d)(m)
        perm = G.geometric_nd(m, m, 1 if wl == "poisson2d" else m, 4)
        S = ch.Session(factor_on_device=True)
        A = S.sparse(n, Ap, Ai, Ax, -1)
        Lf = S.analyze(A, perm)
        assert S.factorize(A, Lf) == 1 and S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
        out["cases"].append(run_case(f"{wl} {m}", S, A, Lf, np.asarray(Ax, dtype=np.float64).copy(), 0.0, a.steps, a.warmup))
        S.free_factor(Lf)
        S.free_sparse(A)
        S.finish()
    if a.aat > 0:
        m = a.aat
        nrow, ncol, Ap, Ai, Ax = grid_incidence(m)
        S = ch.Session(factor_on_device=True)
        A = S.L.cholmod_l_allocate_sparse(nrow, ncol, len(Ai), 1, 1, 0, ch.REAL, C.byref(S.cm))
        ch._view(A.contents.p, ncol + 1, C.c_int64, np.int64)[:] = Ap
        ch._view(A.contents.i, len(Ai), C.c_int64, np.int64)[:] = Ai
        ch._view(A.contents.x, len(Ai), C.c_double, np.float64)[:] = Ax
        Lf = S.analyze(A, G.geometric_nd(m, m, m, 4))
        assert S.factorize(A, Lf) == 1 and S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
        out["cases"].append(run_case(f"A*A', edge-node matrix of the {m}^3 grid", S, A, Lf, Ax.copy(), 0.0, a.steps, a.warmup))
        S.free_factor(Lf)
        S.free_sparse(A)
        S.finish()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
