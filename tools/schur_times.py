#!/usr/bin/env python3
"""Device time of the Schur complement onto the top separator (Session.schur_device: cholmod_hip_schur_device, the tile
kernel k_schur_tile) for Poisson 64^3 and 100^3 with the geometric nested dissection, m = the columns of the last supernode
(the top separator), beside the only route there was before it -- solve_device on m unit columns, then torch.linalg.inv of
the S rows -- and, as context, the rate of k_update3 in a profiled factorization of the same plan (stats [34] / stats [32]):
    python tools/schur_times.py [--out profiles/schur_device_times.json] [--cases p3d64,p3d100]
Times are torch events on the current stream around a window of calls (the calls are ordered on it), the median of seven
windows of five calls after a warm-up call (of two windows of one call for the m solves); one process per case.
Flops: the lower triangle of Sc, a multiply-add counted as two, without the zeros of the masked upper triangles; beside it
the bound sum over the trailing supernodes of (rows from the first trailing column down)^2 x (trailing columns)."""
import torch  # noqa: E402  (first: torch and the engine share one HIP runtime)

import argparse
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from suitesparse_amd import cholmod as ch  # noqa: E402
from suitesparse_amd import generators as G  # noqa: E402

CASES = {
    "p3d64": ("Poisson 64^3", lambda: G.poisson3d(64) + (G.geometric_nd(64, 64, 64, 4),)),
    "p3d100": ("Poisson 100^3", lambda: G.poisson3d(100) + (G.geometric_nd(100, 100, 100, 4),)),
}
WINDOWS = 7


def schur_flops(fv, m):
    """(flops of the lower triangle of Sc with the zeros of the masked upper triangles left out -- entry (i, j), i >= j, of a
    panel with k trailing columns contracts over min (j + 1, k) of them --, the bound sum rows^2 k that counts them)"""
    t0, fl, bound = fv.n - m, 0.0, 0.0
    s0 = int(np.searchsorted(fv.super, t0, side="right")) - 1
    for s in range(s0, fv.nsuper):
        c0 = max(0, t0 - int(fv.super[s]))
        rows, k = int(fv.pi[s + 1] - fv.pi[s]) - c0, int(fv.super[s + 1] - fv.super[s]) - c0
        j = np.arange(rows, dtype=np.float64)
        fl += float(np.sum(2.0 * (rows - j) * np.minimum(j + 1, k)))
        bound += float(rows) ** 2 * k
    return fl, bound


def _window_ms(call, reps, windows=WINDOWS):
    call()
    torch.cuda.synchronize()
    t = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        e1.synchronize()
        t.append(e0.elapsed_time(e1) / reps)
    return float(np.median(t)), float(min(t)), float(max(t))


def one(key):
    torch.cuda.init()
    name, make = CASES[key]
    n, Ap, Ai, Ax, perm = make()
    S = ch.Session(factor_on_device=True)
    A = S.sparse(n, Ap, Ai, Ax, -1)
    Lf = S.analyze(A, perm)
    assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
    fv = ch.FactorView(Lf)
    m = int(fv.super[-1] - fv.super[-2])
    S.set_profiling(Lf, True)
    assert S.refactorize_resident(Lf) == 1 and S.cm.status == ch.OK
    ps = S.hip_stats(Lf)
    S.set_profiling(Lf, False)
    assert S.refactorize_resident(Lf) == 1 and S.cm.status == ch.OK
    t_fact = float(S.hip_stats(Lf)[0])
    out = torch.empty((m, m), dtype=torch.float64, device="cuda")
    fbuf = torch.empty((m, m), dtype=torch.float64, device="cuda")
    t_sc = _window_ms(lambda: S.schur_device(Lf, m, out=out), 5)
    t_both = _window_ms(lambda: S.schur_device(Lf, m, factor=True, out=(out, fbuf)), 5)
    idx = torch.from_numpy(S.schur_index(Lf, m)).cuda()

    def m_solves():
        # m unit right-hand sides in panels of 512 (an n x m array at once would be 8 n m bytes), the S rows of each kept
        cols = []
        for j0 in range(0, m, 512):
            j1 = min(m, j0 + 512)
            E = torch.zeros((j1 - j0, n), dtype=torch.float64, device="cuda")
            E[torch.arange(j1 - j0, device="cuda"), idx[j0:j1]] = 1.0
            cols.append(S.solve_device(Lf, E)[:, idx])
        keep[0] = torch.cat(cols, 0)

    keep = [None]
    print(f"{key}: m={m}, schur_device {t_sc[0]:.3f} ms; timing the m solves ...", file=sys.stderr, flush=True)
    t_old = _window_ms(m_solves, 1, 2)
    Zss = keep[0]                                   # ((A + beta I)^-1)_SS, whose inverse is Sc
    eye_err = float((out @ Zss - torch.eye(m, dtype=torch.float64, device="cuda")).abs().max())
    try:
        t_inv = _window_ms(lambda: torch.linalg.inv(Zss), 1, 3)
        ref = torch.linalg.inv(Zss)
        err, inv_note = float((out - ref).abs().max() / ref.abs().max()), None
    except RuntimeError as e:                       # (the dense inverse is torch's; the m solves dominate the route anyway)
        t_inv, err, inv_note = (None, None, None), None, str(e)[:200]
    fl, bound = schur_flops(fv, m)
    r = {"case": name, "n": n, "nsuper": fv.nsuper, "m": m, "tiles": ((m + 63) // 64) * ((m + 63) // 64 + 1) // 2,
         "schur_device_ms": t_sc[0], "schur_device_ms_min_max": t_sc[1:], "schur_device_with_factor_ms": t_both[0],
         "schur_flops": fl, "schur_flops_bound_rows2_k": bound, "schur_TFLOPs": fl / (1e-3 * t_sc[0]) / 1e12,
         "k_update3_TFLOPs_same_factorization": (ps[34] / ps[32] / 1e12) if ps[32] > 0 else None,
         "factorize_resident_ms": 1e3 * t_fact,
         "m_solves_ms": t_old[0], "m_solves_ms_min_max": t_old[1:], "dense_inverse_ms": t_inv[0],
         "dense_inverse_failed": inv_note, "speedup_over_m_solves_alone": t_old[0] / t_sc[0],
         "max_abs_Sc_times_invA_SS_minus_I": eye_err, "max_rel_difference_from_the_inverse_route": err}
    print("RESULT " + json.dumps(r))
    S.free_factor(Lf)
    S.free_sparse(A)
    S.finish()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--one", default="")
    a = ap.parse_args()
    if a.one:
        return one(a.one)
    out = {"what": "device ms per call of Session.schur_device onto the top separator (torch events on the current stream, median of "
                   "seven windows of five calls after a warm-up), its flops and rate, k_update3's rate in a profiled factorization "
                   "of the same plan, and the route without it: solve_device on m unit columns (panels of 512; two windows of one "
                   "after a warm-up) and torch.linalg.inv of their S rows (three windows of one); one process per case",
           "command": "python tools/schur_times.py " + " ".join(sys.argv[1:]), "device": torch.cuda.get_device_name(0),
           "cases": []}
    for key in a.cases.split(","):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", key], stdout=subprocess.PIPE, text=True)
        res = [ln[7:] for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not res:
            print(p.stdout[-2000:])
            raise SystemExit(f"case {key} failed ({p.returncode})")
        print(res[-1], flush=True)
        out["cases"].append(json.loads(res[-1]))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
