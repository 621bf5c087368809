#!/usr/bin/env python3
"""Device times of the gradients through A*A' + beta*I (cholmod_hip_product_values_grad_device,
cholmod_hip_product_logdet_grad_device) for A = J' of a 2-D grid least-squares problem, in one process:
    python tools/aat_grad_times.py [--m 384] [--out profiles/aat_grad_times.json] [--kernel-stats CSV] [--commit ID]
The unknowns are the m x m nodes of a grid; the measurements (columns of A) are the differences along every edge (2
entries), a prior on every node (1), the weighted mean of every 4 x 4 block (16) and of 8 whole grid rows (m): the lists
of the transposed product map are 3, 2, 17 and m + 1 half-pairs long, so k_product_grad runs in its three classes.
Device times are torch events around INNER calls on the current stream, after a warm-up: the median, the minimum and the
maximum of SAMPLES such windows, per call -- the engine's two entry points at nrhs 1 and 16, a whole backward (one
solve_device + the gradient through the host layer, which hashes A's pattern) beside the forward solve, and the forward
factorize_device (k_product_values, the gather and the factorization).
Kernel times come from a run of their own: `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python
tools/aat_grad_times.py --quick`, whose *_kernel_stats.csv a second, unprofiled run takes as --kernel-stats and records
per kernel (k_product_values, the forward on the same map: same pairs, 16 bytes per pair; k_gr_columns / k_gr_panel, the
sampled product into the scratch; k_si_gather_logdet_grad; k_product_grad per class) with the ratio of the transposed kernel to the forward one."""
import torch  # noqa: E402  (first: torch and the engine share one HIP runtime)

import argparse
import csv
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from suitesparse_amd import cholmod as ch  # noqa: E402

SAMPLES, INNER = 7, 10
BETA = 1e-2


def grid_least_squares(m, seed=3):
    """A = J' (m^2 rows) as scipy CSC with sorted indices"""
    rng = np.random.default_rng(seed)
    node = np.arange(m * m).reshape(m, m)
    cols = []
    for a, b in ((node[:, :-1], node[:, 1:]), (node[:-1, :], node[1:, :])):          # edges
        cols += [np.stack([a.ravel(), b.ravel()], axis=1)]
    cols += [node.reshape(-1, 1)]                                                       # priors
    blocks = node[:m - m % 4, :m - m % 4].reshape(m // 4, 4, m // 4, 4).transpose(0, 2, 1, 3).reshape(-1, 16)
    cols += [blocks]
    cols += [node[np.linspace(0, m - 1, 8).astype(int)]]                                # 8 whole rows
    rows, indptr = [], [0]
    for c in cols:
        rows.append(np.sort(c, axis=1).ravel())
        indptr.append(indptr[-1] + c.shape[0] * c.shape[1])
    lens = np.concatenate([np.full(c.shape[0], c.shape[1]) for c in cols])
    Ap = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    Ai = np.concatenate(rows).astype(np.int64)
    Ax = rng.uniform(0.5, 2.0, len(Ai)) * rng.choice([-1.0, 1.0], len(Ai))
    return sp.csc_matrix((Ax, Ai, Ap), shape=(m * m, len(lens)))


def device_ms(f, inner=INNER, samples=SAMPLES):
    """ms per call of f: [median, min, max] over `samples` windows of `inner` calls"""
    for _ in range(2):
        f()
    torch.cuda.synchronize()
    out = []
    for _ in range(samples):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            f()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / inner)
    return [float(np.median(out)), float(min(out)), float(max(out))]


def kernel_stats(path):
    """rocprofv3's *_kernel_stats.csv -> {kernel: {calls, average_us, min_us, max_us}} for the kernels of this path"""
    keep = re.compile(r"k_product_values|k_product_grad|k_gr_columns|k_gr_panel|k_gr_zero_fill|k_si_gather_logdet_grad|k_gather_values")
    out = {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            name = row["Name"]
            if keep.search(name):
                short = re.sub(r"^void |sship::|\(.*$", "", name)
                out[short] = {"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) * 1e-3,
                              "min_us": float(row["MinNs"]) * 1e-3, "max_us": float(row["MaxNs"]) * 1e-3}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=384)
    ap.add_argument("--out", default="")
    ap.add_argument("--kernel-stats", default="")
    ap.add_argument("--commit", default="")
    ap.add_argument("--quick", action="store_true", help="few calls: the run rocprofv3 traces")
    a = ap.parse_args()
    torch.cuda.init()
    samples, inner = (2, 3) if a.quick else (SAMPLES, INNER)
    M = grid_least_squares(a.m)
    n, nnz = M.shape[0], M.nnz
    ck = np.diff(M.indptr)
    npairs = int((ck * (ck + 1) // 2).sum())
    S = ch.Session(ordering="default", factor_on_device=True)
    A = S.L.cholmod_l_allocate_sparse(n, M.shape[1], nnz, 1, 1, 0, ch.REAL, C.byref(S.cm))
    ch._view(A.contents.p, M.shape[1] + 1, C.c_int64, np.int64)[:] = M.indptr
    ch._view(A.contents.i, nnz, C.c_int64, np.int64)[:] = M.indices
    ch._view(A.contents.x, nnz, C.c_double, np.float64)[:] = M.data
    Lf = S.L.cholmod_l_analyze(A, C.byref(S.cm))
    assert Lf and S.factorize(A, Lf, BETA) == 1 and S.cm.status == ch.OK
    vd = torch.from_numpy(M.data).cuda()
    assert S.factorize_device(A, vd, Lf, BETA) == 1 and S.cm.status == ch.OK
    lens = np.repeat(ck, ck) + 1
    classes = {"1": int((lens <= 8).sum()), "16": int(((lens > 8) & (lens <= 128)).sum()), "64": int((lens > 128).sum())}
    halves = {"1": int(lens[lens <= 8].sum()), "16": int(lens[(lens > 8) & (lens <= 128)].sum()), "64": int(lens[lens > 128].sum())}
    out = {"what": __doc__.split("\n")[0] + " " + __doc__.split("\n")[1], "command": "python tools/aat_grad_times.py " + " ".join(sys.argv[1:]),
           "commit": a.commit, "device": torch.cuda.get_device_name(0),
           "case": f"A = J' of a {a.m} x {a.m} grid least-squares problem, beta = {BETA}", "n": n, "columns": int(M.shape[1]),
           "nnz_A": nnz, "pairs": npairs, "map_bytes": 16 * npairs, "values_per_class": classes, "half_pairs_per_class": halves,
           "samples": samples, "calls_per_sample": inner, "times": "ms per call: [median, min, max]", "nrhs": {}}
    plan, stream = Lf.contents.hip_plan, torch.cuda.current_stream().cuda_stream
    Gd = torch.empty(nnz, dtype=torch.float64, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(5)
    out["forward_factorize_device_ms"] = device_ms(lambda: S.factorize_device(A, vd, Lf, BETA), 3, samples)
    for nrhs in (1, 16):
        B = torch.randn((nrhs, n), dtype=torch.float64, device="cuda", generator=gen)
        X = S.solve_device(Lf, B)
        lam = S.solve_device(Lf, torch.randn((nrhs, n), dtype=torch.float64, device="cuda", generator=gen))

        def engine():
            rc = S.L.cholmod_hip_product_values_grad_device(plan, 1, -1.0, lam.data_ptr(), n, X.data_ptr(), n, nrhs, vd.data_ptr(),
                                                            Gd.data_ptr(), nnz, stream)
            assert rc == ch.HIP_OK

        def backward():
            S.aat_values_grad_device(A, Lf, vd, S.solve_device(Lf, B, out=lam), X, alpha=-1.0, out=Gd)

        r = {"product_values_grad_device_ms": device_ms(engine, inner, samples),
             "forward_solve_ms": device_ms(lambda: S.solve_device(Lf, B, out=lam), inner, samples),
             "backward_solve_plus_grad_ms": device_ms(backward, inner, samples)}
        print(f"nrhs={nrhs}: " + json.dumps(r), flush=True)
        out["nrhs"][str(nrhs)] = r
    assert S.L.cholmod_hip_selinv_device(plan, stream) == ch.HIP_OK
    out["product_logdet_grad_device_ms"] = device_ms(
        lambda: S.L.cholmod_hip_product_logdet_grad_device(plan, vd.data_ptr(), Gd.data_ptr(), nnz, stream), inner, samples)
    print("logdet gradient: " + json.dumps(out["product_logdet_grad_device_ms"]), flush=True)
    if a.kernel_stats:
        ks = kernel_stats(a.kernel_stats)
        fwd = sum(v["average_us"] for k, v in ks.items() if k.startswith("k_product_values"))
        bwd = sum(v["average_us"] for k, v in ks.items() if k.startswith("k_product_grad"))
        out["kernels"] = {"source": "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/aat_grad_times.py --quick "
                                    f"--m {a.m} (a run of its own)", "per_kernel": ks,
                          "k_product_values_all_classes_us": fwd, "k_product_grad_all_classes_us": bwd,
                          "transposed_over_forward": bwd / fwd if fwd else None,
                          "forward_GBs_of_map": 16 * npairs / (fwd * 1e-6) / 1e9 if fwd else None,
                          "transposed_GBs_of_map": 16 * npairs / (bwd * 1e-6) / 1e9 if bwd else None}
        print("kernels: " + json.dumps(out["kernels"]), flush=True)
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
