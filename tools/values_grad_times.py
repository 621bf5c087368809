#!/usr/bin/env python3
"""Device times of the gradient kernels (cholmod_hip_values_grad_device, cholmod_hip_logdet_device) on Poisson m^3 with the
benchmark's ordering, for nrhs 1, 16 and 64, in one process:
    python tools/values_grad_times.py [--m 100] [--out profiles/values_grad_times.json]
Per nrhs: the sampled product at the engine level (values_grad_device_ms) and through the host layer, which hashes A's
pattern on the host in every call (host_layer_call_ms), its algorithmic bytes (the operands once, 2 n nrhs 8; the index of S, 16 bytes per entry plus
8 (n + 1); 8 nvalues out) and the GB/s they give; the torch-index formulation of the same gradient on the same tensors;
a whole backward (one solve_device + the sampled product) beside the forward solve.  Once: logdet_device beside
factor_checks (which waits for the stream: host clock).  Device times are torch events around INNER calls on the current
stream, after a warm-up; the median, the minimum and the maximum of SAMPLES such windows, per call."""
import torch  # noqa: E402  (first: torch and the engine share one HIP runtime)

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from suitesparse_amd import cholmod as ch  # noqa: E402
from suitesparse_amd import generators as G  # noqa: E402

SAMPLES, INNER = 7, 10


def device_ms(f, inner=INNER):
    """ms per call of f: [median, min, max] over SAMPLES windows of `inner` calls"""
    for _ in range(2):
        f()
    torch.cuda.synchronize()
    out = []
    for _ in range(SAMPLES):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            f()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / inner)
    return [float(np.median(out)), float(min(out)), float(max(out))]


def host_ms(f):
    for _ in range(2):
        f()
    out = []
    for _ in range(SAMPLES):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return [float(np.median(out)), float(min(out)), float(max(out))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=100)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    torch.cuda.init()
    m = a.m
    n, Ap, Ai, Ax = G.poisson3d(m)
    perm = G.geometric_nd(m, m, m, 4)
    S = ch.Session(factor_on_device=True)
    A = S.sparse(n, Ap, Ai, Ax, -1)
    Lf = S.analyze(A, perm)
    assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
    nnz = len(Ai)
    rows = torch.from_numpy(np.asarray(Ai, dtype=np.int64)).cuda()
    cols = torch.from_numpy(np.repeat(np.arange(n, dtype=np.int64), np.diff(Ap))).cuda()
    off = (rows != cols).to(torch.float64)
    gen = torch.Generator(device="cuda").manual_seed(5)
    out = {"what": __doc__.split("\n\n")[0].replace("\n", " "), "command": "python tools/values_grad_times.py " + " ".join(sys.argv[1:]),
           "device": torch.cuda.get_device_name(0), "case": f"Poisson {m}^3, geometric ND leaf 4", "n": n, "nnz": nnz,
           "samples": SAMPLES, "calls_per_sample": INNER, "times": "ms per call: [median, min, max]", "nrhs": {}}
    Gd = torch.empty(nnz, dtype=torch.float64, device="cuda")
    plan, stream = Lf.contents.hip_plan, torch.cuda.current_stream().cuda_stream
    for nrhs in (1, 16, 64):
        B = torch.randn((nrhs, n), dtype=torch.float64, device="cuda", generator=gen)
        X = S.solve_device(Lf, B)
        lam = S.solve_device(Lf, torch.randn((nrhs, n), dtype=torch.float64, device="cuda", generator=gen))

        def kernel():
            rc = S.L.cholmod_hip_values_grad_device(plan, 1, -1.0, lam.data_ptr(), n, X.data_ptr(), n, nrhs, Gd.data_ptr(), nnz, stream)
            assert rc == ch.HIP_OK

        def host_layer():       # ... through cholmod_l_hip_values_grad_device, which hashes A's pattern on the host every call
            S.values_grad_device(A, Lf, lam, X, alpha=-1.0, out=Gd)

        def torch_index():
            return -((lam[:, rows] * X[:, cols]).sum(0) + off * (lam[:, cols] * X[:, rows]).sum(0))

        def backward():
            S.values_grad_device(A, Lf, S.solve_device(Lf, B, out=lam), X, alpha=-1.0, out=Gd)

        inner = INNER if nrhs < 64 else 3
        t_k, t_t, t_h = device_ms(kernel, inner), device_ms(torch_index, inner), device_ms(host_layer, inner)
        t_f = device_ms(lambda: S.solve_device(Lf, B, out=lam), inner)
        t_b = device_ms(backward, inner)
        kernel()
        ref = torch_index()
        scale = float(((lam[:, rows] * X[:, cols]).abs().sum(0) + (lam[:, cols] * X[:, rows]).abs().sum(0)).max())
        err = float((Gd - ref).abs().max())
        by = 2 * n * nrhs * 8 + 16 * nnz + 8 * (n + 1) + 8 * nnz
        r = {"values_grad_device_ms": t_k, "algorithmic_bytes": by, "algorithmic_GBs": by / (t_k[0] * 1e-3) / 1e9,
             "torch_index_ms": t_t, "kernel_over_torch_index": t_k[0] / t_t[0], "host_layer_call_ms": t_h, "forward_solve_ms": t_f,
             "backward_solve_plus_grad_ms": t_b, "max_abs_difference_to_torch_index": err, "max_magnitude": scale}
        print(f"nrhs={nrhs}: " + json.dumps(r), flush=True)
        out["nrhs"][str(nrhs)] = r
        del B, X, lam, ref
        torch.cuda.empty_cache()
    t_l = device_ms(lambda: S.logdet_device(Lf))
    t_c = host_ms(lambda: S.factor_checks(Lf))
    ld, half = float(S.logdet_device(Lf)), S.factor_checks(Lf)["half_logdet"]
    out["logdet"] = {"logdet_device_ms": t_l, "factor_checks_host_ms": t_c, "logdet_device": ld, "twice_factor_checks": 2 * half,
                     "closed_form": G.poisson_logdet(m, m, m)}
    print("logdet: " + json.dumps(out["logdet"]), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    torch.cuda.synchronize()
    S.free_factor(Lf)
    S.free_sparse(A)
    S.finish()


if __name__ == "__main__":
    main()
