#!/usr/bin/env python3
"""Device time of the factor gradient (cholmod_hip_factor_grad_device and cholmod_hip_factor_outer_grad_device with 16
right-hand sides, cholmod_hip_factor_grad_info [0]) beside the selected inverse of the same factor in the same run
(cholmod_hip_selinv_info [0]: the same launch program, the same hot product) and the resident factorization of the same
plan (stats [0]), per case in a process of its own, the median of five after a warm-up:
    python tools/factor_grad_times.py [--out profiles/factor_grad_times.json] [--cases p3d64,p3d100,box42,p2d1259]
Also recorded: the launches (info [1]), the rate of the hot product M [R, R] L [R, b] (info [2] / info [0]), the bytes of Gx and
of the scratch (info [4], info [5])."""
import torch  # noqa: E402  (first: torch and the engine share one HIP runtime)

import argparse
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from suitesparse_amd import cholmod as ch  # noqa: E402
from selinv_times import CASES, REPS  # noqa: E402  (the same four cases)


def _median(S, plan, call, info_fn):
    info, t = np.zeros(8), []
    for k in range(REPS + 1):
        assert call() == ch.HIP_OK
        assert info_fn(plan, info.ctypes.data) == ch.HIP_OK
        if k:
            t.append(float(info[0]))
    return float(np.median(t)), info


def one(key):
    torch.cuda.init()
    name, make = CASES[key]
    n, Ap, Ai, Ax, perm = make()
    S = ch.Session(factor_on_device=True)
    A = S.sparse(n, Ap, Ai, Ax, -1)
    Lf = S.analyze(A, perm)
    assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
    plan, lib = Lf.contents.hip_plan, S.L
    fact = []
    for k in range(REPS + 1):
        assert S.refactorize_resident(Lf) == 1 and S.cm.status == ch.OK
        if k:
            fact.append(float(S.hip_stats(Lf)[0]))
    gen = torch.Generator(device="cuda").manual_seed(1)
    Lbar = torch.randn(int(Lf.contents.xsize), dtype=torch.float64, device="cuda", generator=gen)
    PQ = torch.randn((32, n), dtype=torch.float64, device="cuda", generator=gen)
    torch.cuda.synchronize()
    t_sel, _ = _median(S, plan, lambda: lib.cholmod_hip_selinv_device(plan, None), lib.cholmod_hip_selinv_info)
    t_fg, info = _median(S, plan, lambda: lib.cholmod_hip_factor_grad_device(plan, Lbar.data_ptr(), None),
                         lib.cholmod_hip_factor_grad_info)
    t_out, _ = _median(S, plan, lambda: lib.cholmod_hip_factor_outer_grad_device(plan, -1.0, PQ[:16].data_ptr(), n,
                                                                                  PQ[16:].data_ptr(), n, 16, None),
                       lib.cholmod_hip_factor_grad_info)
    G, tr = S.factor_outer_grad_device(A, Lf, PQ[:16], PQ[16:])
    finite = bool(torch.isfinite(G).all()) and bool(torch.isfinite(tr))
    t_fact = float(np.median(fact))
    r = {"case": name, "n": n, "nsuper": int(Lf.contents.nsuper), "factor_grad_device_ms": 1e3 * t_fg,
         "factor_outer_grad_device_nrhs16_ms": 1e3 * t_out, "selinv_device_ms": 1e3 * t_sel, "factorize_resident_ms": 1e3 * t_fact,
         "factor_grad_over_selinv": t_fg / t_sel, "factor_outer_grad_over_selinv": t_out / t_sel, "launches": int(info[1]),
         "hot_product_flops": info[2], "hot_product_TFLOPs": info[2] / t_fg / 1e12, "Gx_bytes": info[4], "scratch_bytes": info[5],
         "finite": finite}
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
    out = {"what": "device ms of cholmod_hip_factor_grad_device / cholmod_hip_factor_outer_grad_device (two events on the engine "
                   "stream), of cholmod_hip_selinv_device on the same factor in the same run, and of the resident factorization "
                   "of the same plan (stats [0]); one process per case, median of five after a warm-up",
           "command": "python tools/factor_grad_times.py " + " ".join(sys.argv[1:]), "device": torch.cuda.get_device_name(0),
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
