#!/usr/bin/env python3
"""Device time of the selected inverse (cholmod_hip_selinv_device, info [0]) beside the resident factorization of the same
plan (stats [0], the yardstick), per case in a process of its own, the median of five after a warm-up:
    python tools/selinv_times.py [--out profiles/selinv_device_times.json] [--cases p3d64,p3d100,box42,p2d1259]
Also recorded: the launches (info [1]), the rate of the hot product Z [R, R] L [R, b] (info [2] / info [0]), the bytes of Zx
and of the scratch (info [4], info [5]), and the size-independent check |trace (A Z) - n| / n from the values on A's
pattern."""
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
    "box42": ("nd24k stand-in (box stencil 42^3, radius 3)", lambda: G.box_stencil3d(42, 3) + (G.geometric_nd(42, 42, 42, 6, 3),)),
    "p2d1259": ("Poisson 1259^2 (2D stand-in)", lambda: G.poisson2d(1259) + (G.geometric_nd(1259, 1259, 1, 4),)),
}
REPS = 5


def one(key):
    torch.cuda.init()
    name, make = CASES[key]
    n, Ap, Ai, Ax, perm = make()
    S = ch.Session(factor_on_device=True)
    A = S.sparse(n, Ap, Ai, Ax, -1)
    Lf = S.analyze(A, perm)
    assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
    plan = Lf.contents.hip_plan
    fact = []
    for k in range(REPS + 1):
        assert S.refactorize_resident(Lf) == 1 and S.cm.status == ch.OK
        if k:
            fact.append(float(S.hip_stats(Lf)[0]))
    info, sel = np.zeros(8), []
    for k in range(REPS + 1):
        assert S.L.cholmod_hip_selinv_device(plan, None) == ch.HIP_OK
        assert S.L.cholmod_hip_selinv_info(plan, info.ctypes.data) == ch.HIP_OK
        if k:
            sel.append(float(info[0]))
    Z, _ = S.selinv_device(A, Lf, diag=False)
    Z = Z.cpu().numpy()
    off = np.asarray(Ai) != np.repeat(np.arange(n), np.diff(Ap))
    tr = float(np.sum(Ax[~off] * Z[~off]) + 2.0 * np.sum(Ax[off] * Z[off]))
    t_sel, t_fact = float(np.median(sel)), float(np.median(fact))
    r = {"case": name, "n": n, "nsuper": int(Lf.contents.nsuper), "selinv_device_ms": 1e3 * t_sel,
         "factorize_resident_ms": 1e3 * t_fact, "selinv_over_factorization": t_sel / t_fact, "launches": int(info[1]),
         "hot_product_flops": info[2], "all_flops": info[3], "hot_product_TFLOPs": info[2] / t_sel / 1e12,
         "Zx_bytes": info[4], "scratch_bytes": info[5], "trace_identity_error": abs(tr - n) / n}
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
    out = {"what": "device ms of cholmod_hip_selinv_device (two events on the engine stream) and of the resident factorization "
                   "of the same plan (stats [0]); one process per case, median of five after a warm-up",
           "command": "python tools/selinv_times.py " + " ".join(sys.argv[1:]), "device": torch.cuda.get_device_name(0),
           "cases": []}
    for key in a.cases.split(","):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", key], capture_output=True, text=True)
        res = [ln[7:] for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not res:
            print(p.stdout[-2000:], p.stderr[-2000:])
            raise SystemExit(f"case {key} failed ({p.returncode})")
        print(res[-1], flush=True)
        out["cases"].append(json.loads(res[-1]))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
