"""The numpy reference of the device-side factor checks (tests/factor_check_reference.py) against two identities that
know nothing of supernodes, on the CPU path's factor (Common->useGPU = 0: no GPU needed):

    ||L||_F^2 = trace (A)              2 sum_j log L_jj = log det (A)

so that the GPU tests (tests/test_gpu_factor_checks.py) compare the kernels with index sets that are themselves
checked."""
import math

import numpy as np
import pytest

import factor_check_reference as R
from suitesparse_amd import cholmod as ch

U = 2.0 ** -53          # unit roundoff of fp64


def _dense_lower(n, Ap, Ai, Ax):
    A = np.zeros((n, n))
    cols = np.repeat(np.arange(n), np.diff(Ap))
    A[Ai, cols] = Ax
    return A + np.tril(A, -1).T


def _dense_L(fv, shape, x):
    Ld = np.zeros((fv.n, fv.n))
    for k in range(fv.nsuper):
        nscol, nsrow = int(shape.nscol[k]), int(shape.nsrow[k])
        blk = x[fv.px[k]:fv.px[k] + nscol * nsrow].reshape(nscol, nsrow)
        rows = fv.s[fv.pi[k]:fv.pi[k + 1]]
        for j in range(nscol):
            Ld[rows[j:], fv.super[k] + j] = blk[j, j:]
    return Ld


@pytest.mark.parametrize("name", R.REAL_CASES)
def test_reference_agrees_with_trace_and_logdet(name):
    n, Ap, Ai, Ax, perm = R.matrix(name)
    S = ch.Session(use_gpu=0)
    A = S.sparse(n, Ap, Ai, Ax, -1)
    Lf = S.analyze(A, perm)
    assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK and not Lf.contents.hip_plan
    fv = ch.FactorView(Lf)
    shape = R.FactorShape(fv.super, fv.pi, fv.px, fv.xsize)
    R.assert_front_shapes(name, shape)
    x = fv.x.copy()
    ref = R.factor_checks(shape, x)
    assert ref["upper_nonzeros"] == 0 and ref["nonfinite"] == 0 and ref["nonpositive_diag"] == 0
    assert len(shape.diag) == n and len(shape.lower) + len(shape.dead) == int((shape.nscol * shape.nsrow).sum())

    Ad = _dense_lower(n, Ap, Ai, Ax)
    # ||L||_F^2 = trace (L L') = trace (A + E), and the computed factor has |E| <= g |L||L'|, g = (n+1) u / (1 - (n+1) u)
    # (Higham, Accuracy and Stability of Numerical Algorithms, theorem 10.3), whose trace is g ||L||_F^2: no condition
    # number.  The reference sums exactly (fsum) and trace (A) is an exact sum as well; n 2^-52 = 2 n u >= g for n >= 1.
    trace = math.fsum(np.diag(Ad))
    e_fro = abs(ref["fro2"] - trace)
    b_fro = n * R.EPS * trace
    # log det (A + E) - log det (A) = trace (A^-1 E) to first order, at most g tau with
    # tau = sum_ij |A^-1|_ij (|L||L'|)_ij, computed here from the factor itself instead of guessing a condition number.
    # numpy's slogdet is an LU factorization of the same matrix: no row is exchanged (the diagonal dominates every
    # column), L_lu U = A + E2 with |E2| <= g |L_lu||U| and |L_lu||U| = |L||L'|, the same tau; it then adds n logarithms
    # log u_jj = 2 log L_jj in floating point, (n - 1) u + u relative to sum |log u_jj|.  The reference's own sum is
    # exact.  Together, with (n+1) 2^-52 >= 2 g:
    P = fv.Perm
    Ld = _dense_L(fv, shape, x)
    tau = float(np.sum(np.abs(np.linalg.inv(Ad[np.ix_(P, P)])) * (np.abs(Ld) @ np.abs(Ld).T)))
    sign, logdet = np.linalg.slogdet(Ad)
    assert sign == 1.0
    e_log = abs(2.0 * ref["half_logdet"] - logdet)
    b_log = (n + 1) * R.EPS * (tau + 2.0 * R.sum_abs_log_diag(shape, x))
    print(f"{name}: |fro2 - trace A| = {e_fro:.3e} = {e_fro / b_fro:.3f} of the bound; "
          f"|2 half_logdet - logdet A| = {e_log:.3e} = {e_log / b_log:.3f} of the bound (tau = {tau:.1f}, n = {n})")
    assert e_fro <= b_fro
    assert e_log <= b_log
    # the diagonal scan's reference on the same factor: the extremes of diag (L), nothing counted
    lo, hi, bad = R.diag_minmax(shape, x)
    d = np.diag(Ld)
    assert (lo, hi, bad) == (d.min(), d.max(), 0)
    S.free_factor(Lf)
    S.free_sparse(A)
    S.finish()


def test_reference_counts_what_is_planted():
    """The counting rules on a hand-made 3-column panel over 4 rows followed by a 1 x 1 one."""
    shape = R.FactorShape([0, 3, 4], [0, 4, 5], [0, 12, 13], 13)
    assert shape.diag.tolist() == [0, 5, 10, 12] and sorted(shape.dead.tolist()) == [4, 8, 9]
    assert sorted(shape.lower.tolist()) == [0, 1, 2, 3, 5, 6, 7, 10, 11, 12]
    x = np.zeros(13)
    x[shape.lower] = 2.0
    good = R.factor_checks(shape, x)
    assert good == dict(half_logdet=4 * math.log(2.0), upper_nonzeros=0, nonfinite=0, fro2=40.0, nonpositive_diag=0)
    y = x.copy()
    y[[4, 8, 9]] = [-0.0, np.nan, 3.0]                   # dead: -0.0 is no entry, a NaN is one
    y[[1, 2]] = [np.inf, -np.inf]
    y[[0, 5, 10]] = [-0.0, np.nan, -1.0]                 # diagonal: none of them is > 0; the NaN is also non-finite
    got = R.factor_checks(shape, y)
    assert got == dict(half_logdet=math.log(2.0), upper_nonzeros=2, nonfinite=3, fro2=4.0 * 5 + 1.0, nonpositive_diag=3)
    assert R.diag_minmax(shape, y) == (0.0, 2.0, 2) and math.copysign(1.0, R.diag_minmax(shape, y)[0]) == 1.0
    y[shape.diag] = np.nan
    assert R.diag_minmax(shape, y) == (math.inf, 0.0, 4)
    # a complex 1 x 1 supernode (2 - 3i) as its twin
    ts, t = R.twin_of_complex([0, 1], [0, 1], [0, 1], 1, np.array([2 - 3j]))
    assert t.tolist() == [2.0, -3.0, 3.0, 2.0] and ts.dead.tolist() == [2] and ts.diag.tolist() == [0, 3]
