"""The device-array part of tests/test_gpu_pivot_range.py, run in a process of its own: `python pivot_range_device_cases.py
NAME`, torch imported FIRST (see solve_device_cases.py).  For the matrix NAME of scaling_cases.py and each exponent profile:
the factor of D A D, solve_device with 3 (column kernels) and 20 (MFMA panel kernels) right-hand sides for A, L and L',
residual_device against the componentwise bound of residual_device_cases.py on the scaled data, and one refinement step.
Every profile gets its own verdict in the line `RESULT <json>`: "ok" or the assertion that failed.

In the factor's ordering L_s = D_p L, D_p = D in the order of Perm.  A x = D c gives x = D^-1 A^-1 c; L_s y = D_p c gives
y = L^-1 c, the unscaled solve itself; L_s' z = c gives z = D_p^-1 L^-T c -- the right-hand side for which the solve with L'
is the scaled image of the unscaled one."""
import torch  # noqa: E402  (first)

import json
import sys
import traceback

import numpy as np

import solve_device_cases as SD  # noqa: F401  (puts the repository root and tests/ on sys.path)
from solve_device_cases import TOL, _dev, _done, _relcols
from residual_device_cases import Sym, _check1
import scaling_cases as SC
from suitesparse_amd import cholmod as ch
from suitesparse_amd import generators as G


def run(name, profile):
    ref, e, Axs = SC.sparse_case(name, profile)
    n, ep = ref.n, e[ref.struct["Perm"]]
    S = ch.Session()
    A = S.sparse(n, ref.Ap, ref.Ai, Axs, -1)
    Lf = S.analyze(A, ref.perm)
    assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
    fv = ch.FactorView(Lf)
    m = ref.mask
    err = np.linalg.norm((SC.descale_factor(fv.x, ref, e) - ref.x)[m]) / np.linalg.norm(ref.x[m])
    print(f"{name} {profile}: factor {err:.2e}")
    assert err < 1e-12 and np.all(fv.x[~m] == 0)
    M = Sym(n, ref.Ap, ref.Ai, Axs)
    rng = np.random.default_rng(31)
    for nrhs in (3, 20):
        c = rng.standard_normal((nrhs, n))
        Dc = np.ldexp(c, e[None, :])
        x = np.ldexp(S.solve_device(Lf, _dev(Dc)).cpu().numpy(), e[None, :])
        ex = _relcols(x, ref.O.solve(c))
        for k in range(nrhs):
            r = G.sym_matvec(n, ref.Ap, ref.Ai, ref.Ax, -1, x[k]) - c[k]
            assert np.linalg.norm(r) / np.linalg.norm(c[k]) < TOL, (nrhs, k)
        y = S.solve_device(Lf, _dev(np.ldexp(c, ep[None, :])), ch.SYS_L).cpu().numpy()
        ey = _relcols(y, ref.O.lsolve(c))
        z = np.ldexp(S.solve_device(Lf, _dev(c), ch.SYS_Lt).cpu().numpy(), ep[None, :])
        ez = _relcols(z, ref.O.ltsolve(c))
        print(f"{name} {profile} nrhs={nrhs}: A {ex:.2e} L {ey:.2e} Lt {ez:.2e}")
        assert ex < 1e-10 and ey < TOL and ez < TOL, (nrhs, ex, ey, ez)
        # the residual of arbitrary X and B in the units of the scaled system
        xs, bs = np.ldexp(rng.standard_normal((nrhs, n)), -e[None, :]), np.ldexp(rng.standard_normal((nrhs, n)), e[None, :])
        R, nrm = S.residual_device(Lf, _dev(xs), _dev(bs), norms=True)
        _check1(M, R, nrm, xs, bs, f"{name} {profile} nrhs={nrhs}")
        # one refinement step from a solution that is off by 1e-3: no column norm goes up, and the solution is reached
        B = _dev(Dc)
        X = S.solve_device(Lf, B) * _dev(1.0 + 1e-3 * rng.standard_normal((nrhs, n)))
        _, n0 = S.refine_device(Lf, B, X, steps=0, norms=True)
        n0 = n0.cpu().numpy().copy()
        _, n1 = S.refine_device(Lf, B, X, steps=1, norms=True)
        n1 = n1.cpu().numpy()
        print(f"{name} {profile} nrhs={nrhs}: residual norms after / before one step, largest ratio {(n1 / n0).max():.2e}")
        assert np.all(np.isfinite(n0)) and np.all(n1 <= n0), (n0, n1)
        assert _relcols(np.ldexp(X.cpu().numpy(), e[None, :]), ref.O.solve(c)) < 1e-10
    _done(S, A, Lf)


if __name__ == "__main__":
    torch.cuda.init()
    name = sys.argv[1]
    out = {}
    for profile in (["mixed"] if name == "big_supernode" else SC.PROFILES):
        try:
            run(name, profile)
            out[profile] = "ok"
        except AssertionError:
            out[profile] = traceback.format_exc()[-1500:]
            print(out[profile])
    print("RESULT " + json.dumps(out))
