"""The body of tests/test_gpu_mixed_streams.py, run in a process of its own: `python mixed_streams_cases.py`, torch imported
FIRST (see solve_device_cases.py).  Exit status 0 and a line `CASE OK` = every assertion held.

Every device-resident entry point orders the engine stream against its caller's with the plan's one pair of events
(stream_enter / stream_leave, csrc/hip/plan.hip.h).  Here the features take turns on TWO side streams, each turn behind a
large matmul on its stream and behind an event from the turn before, with no host wait of the test's own in between: an
event of the pair is recorded again while the other stream's wait on its earlier record is still outstanding.  Every
result is checked as the feature's own side-stream case checks it: same reference, same bar."""
import torch  # noqa: E402  (first)

import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import factor_grad_cases as FG
import factorize_device_cases as FD
import grad_cases as GC
import grad_reference as GR
import residual_device_cases as RD
import schur_reference as SR
import selinv_reference as R
from suitesparse_amd import cholmod as ch
from suitesparse_amd.autograd import DeviceCholesky

M_SCHUR = 300


def main():
    case = R.CASES["p3d_12_nd"]()
    n, Ap, Ai, Ax = case["n"], case["Lp"], case["Li"], case["Lx"]
    S, A, Lf = R.factorized(case, use_gpu=1)
    chol = DeviceCholesky(S, A, Lf)
    perm = FG._host_factor(S, Lf).Perm.copy()
    rng = np.random.default_rng(71)
    b, c = rng.standard_normal((3, n)), rng.standard_normal((3, n))
    Bg, Wg = GR.inputs(n, 19, 9)
    Zf, Bf, Wf, W2f = (rng.standard_normal((3, n)) for _ in range(4))
    dev = FD._dev
    src, Bh, Ch, Bgd, Wgd, Zfd, Bfd, Wfd, W2fd = (dev(a) for a in (Ax, b, c, Bg, Wg, Zf, Bf, Wf, W2f))
    big = torch.full((4096, 4096), 1.0 / 4096, dtype=torch.float64, device="cuda")
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for rep in range(2):
        scale = 1.0 + 0.5 * rep             # rep 0: A itself, rep 1: 1.5 A
        turn, last = [0], [None]

        def take_turn(body):
            """body (zero) on the next stream: behind a large matmul of that stream (zero is a device scalar 0.0 that
            comes out of it) and behind the turn before"""
            s = streams[turn[0] % 2]
            turn[0] += 1
            with torch.cuda.stream(s):
                Z = big
                for _ in range(3):
                    Z = Z @ big
                if last[0] is not None:
                    s.wait_event(last[0])
                out = body(0.0 * Z[0, 0])
                last[0] = s.record_event()
            return out

        def factorize(zero):
            vals = torch.full((len(Ax),), FD.NAN, dtype=torch.float64, device="cuda")     # (read too early: NaN everywhere)
            vals.copy_(src * scale + zero)
            return vals, S.factorize_device(A, vals, Lf), S.cm.status

        def solve(zero):
            X = S.solve_device(Lf, Bh + zero)
            return X, X + 0.0

        def selinv(zero):
            _, d = S.selinv_device(A, Lf)
            return d * 2.0 + zero

        def values_grad(zero):
            v, Bd = (vals + zero).requires_grad_(), (Bgd * 1.0).requires_grad_()
            ((Wgd * chol.solve(v, Bd)).sum() + 0.3 * chol.logdet(v)).backward()
            return v.grad * 2.0, Bd.grad * 2.0

        def factor_grad(zero):
            v, Zd, Bd = (vals + zero).requires_grad_(), (Zfd * 1.0).requires_grad_(), (Bfd * 1.0).requires_grad_()
            Xt, Y = chol.solve_Lt(v, Zd), chol.solve_L(v, Bd)
            ((Wfd * Xt).sum() + (W2fd * Y).sum()).backward()
            return dict(X=Xt.detach() * 2.0, Y=Y.detach() * 2.0, gv=v.grad * 2.0, gZ=Zd.grad * 2.0, gB=Bd.grad * 2.0)

        def schur(zero):
            return S.schur_device(Lf, M_SCHUR) * 2.0 + zero

        def residual(zero):
            return S.residual_device(Lf, X, Ch + zero) * 2.0

        vals, ok, status = take_turn(factorize)
        X, Xc = take_turn(solve)
        d2 = take_turn(selinv)
        gv2, gb2 = take_turn(values_grad)
        fg2 = take_turn(factor_grad)
        Sc2 = take_turn(schur)
        R2 = take_turn(residual)
        for s in streams:
            s.synchronize()
        assert turn[0] == 7 and ok == 1 and status == ch.OK
        tag = f"mixed rep {rep}"
        # factorize_values_device + solve_device: tests/factorize_device_cases.py, case_stream
        xs = np.linalg.solve(FD._lower_of(n, Ap, Ai, Ax * scale).toarray(), b.T).T
        e = FD._relcols(Xc.cpu().numpy(), xs)
        print(f"{tag}: x vs numpy {e:.3e}")
        assert e < FD.TOL, e
        # selinv_device: tests/selinv_cases.py, case_stream
        Zd = np.linalg.inv(R.dense_symmetric(n, Ap, Ai, Ax * scale))
        fv = FG._host_factor(S, Lf)
        tol = R.tolerance(R.factor_rcond(fv))
        err = np.abs(d2.cpu().numpy() - 2.0 * np.diag(Zd)).max()
        print(f"{tag}: diagonal {err:.2e} tol {2 * tol * np.abs(Zd).max():.2e}")
        assert err <= 2 * tol * np.abs(Zd).max(), (rep, err, tol)
        # values_grad_device (and the log-determinant): tests/grad_cases.py, case_stream
        GC._check_grads(tag, gv2 * 0.5, gb2 * 0.5, GR.torch_reference(n, Ap, Ai, Ax * scale, -1, 0.0, Bg, Wg), tol, 19)
        # factor_outer_grad_device and the L-solves: tests/factor_grad_cases.py, case_stream
        ref = FG._torch_reference(n, Ap, Ai, Ax * scale, perm, 0.0, Zf, Bf, Wf, W2f)
        ref["gbeta"] = 0.0
        FG._check_autograd(tag, dict({k: 0.5 * t.cpu().numpy() for k, t in fg2.items()}, gbeta=0.0), ref, tol)
        # schur_device: tests/schur_cases.py, case_stream
        sref = SR.dense_schur(SR.permuted_dense(dict(case, Lx=Ax * scale), fv.Perm), M_SCHUR)
        err = np.abs(Sc2.cpu().numpy() - 2.0 * sref).max() / np.abs(2.0 * sref).max()
        print(f"{tag}: schur {err:.2e} tol {tol:.2e}")
        assert err <= tol, (rep, err, tol)
        # residual_device: tests/residual_device_cases.py, case_stream
        rref, bound = RD.Sym(n, Ap, Ai, Ax * scale).residual(X.cpu().numpy(), c)
        w = RD._worst(R2.cpu().numpy(), 2.0 * rref, 2.0 * bound)
        print(f"{tag}: residual worst / bound {w:.3e}")
        assert w <= 1.0, (rep, w)
    FG._done(S, A, Lf)
    print("CASE OK")


if __name__ == "__main__":
    main()
