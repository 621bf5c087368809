"""The pivot code of the front kernels over the whole range of doubles (run with -m gpu on an MI355X).

Every front kernel takes its square roots and reciprocals from hand-written sequences (sqrt_rsqrt: a v_rsq_f64 seed, a
coupled Goldschmidt iteration and a rescale by 2^+-512 outside [1e-290, 1e290]; v_rcp_f64 plus a Newton step for the LDL'
elimination on unscaled columns) and pads its panels with literal 1.0.  Four parts:

 1. the square root and its reciprocal measured in ulps against math.sqrt, one pivot per 1 x 1 front, through
    k_thin_front, k_leaf_pair and k_potrf_mfma;
 2. dense fronts, 3. sparse factorizations, solves and residuals of D M D for D = diag(2^e_i), held against LAPACK's /
    the oracle's results for the UNSCALED M at the suite's existing tolerances (scaling_cases.py has the argument,
    test_scaling_reference.py ties it down on the CPU);
 4. the failure boundary d <= 0 by value: +0.0, -0.0 and the smallest denormals of either sign.

The device-array solves need torch imported before the engine library: their bodies live in
tests/pivot_range_device_cases.py and run in a child process per matrix, as those of test_gpu_solve_device.py do."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import scaling_cases as SC
from oracle.oracle import OracleFactor
from suitesparse_amd import cholmod as ch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TOL_L, TOL_RES = 1e-12, 1e-11           # test_gpu_parity.py
EPS = 2.0 ** -53
NO_SMALL_FRONTS, NO_LEAF_PAIRS = 16, 4096      # plan flags (include/cholmod_hip.h)


@pytest.fixture(scope="module")
def L():
    lib = ch.lib()
    assert lib.cholmod_hip_probe() == 1, "no HIP device visible"
    return lib


def _set_values(A, Ax):
    ch._view(A.contents.x, len(Ax), C.c_double, np.float64)[:] = Ax


def _ulps(a, b):
    """distance in units of the last place between positive doubles"""
    return np.abs(np.ascontiguousarray(a).view(np.int64) - np.ascontiguousarray(b).view(np.int64))


# ---- 1. sqrt and 1 / sqrt, measured ----------------------------------------------------------------------------------------

N1 = 4096


def sqrt_values():
    """4096 pivots: mantissas 1 + eps, 2 - eps, 4 - eps at exponents around every branch, the neighbours of both rescale
    thresholds, DBL_MIN, DBL_MAX, 64 denormals with 5e-324 among them, and a log-uniform sweep of normal doubles
    2^-1021 .. 2^1023 with random mantissas"""
    rng = np.random.default_rng(2024)
    v = []
    for k in (-1021, -1020, -965, -964, -963, -962, -513, -512, -511, -2, -1, 0, 1, 2, 511, 512, 513, 962, 963, 964, 965, 1019, 1020):
        v += [math.ldexp(1.0 + 2.0 ** -52, k), math.ldexp(2.0 - 2.0 ** -52, k), math.ldexp(4.0 - 2.0 ** -51, k)]
    for t in (SC.LO, SC.HI):
        v += [t, np.nextafter(t, 0.0), np.nextafter(t, np.inf), np.nextafter(np.nextafter(t, 0.0), 0.0)]
    v += [SC.DBL_MIN, np.nextafter(SC.DBL_MIN, 1.0), SC.DBL_MAX, np.nextafter(SC.DBL_MAX, 0.0)]
    den = np.concatenate([[1, 2, 3, 2 ** 52 - 1, 2 ** 51, 2 ** 26], rng.integers(1, 2 ** 52, 58)]).astype(np.int64)
    assert len(den) == 64
    v += list(den.view(np.float64))
    v = np.array(v, dtype=np.float64)
    m = N1 - len(v)
    sweep = np.ldexp(1.0 + rng.integers(0, 2 ** 52, m).astype(np.float64) * 2.0 ** -52, rng.integers(-1021, 1023, m))
    d = np.concatenate([v, sweep])
    d = d[rng.permutation(N1)]
    assert d[0] != 5e-324 and np.all(d > 0) and np.all(np.isfinite(d)) and (d == 5e-324).any()
    assert (d < SC.DBL_MIN).sum() == 64 and (d < SC.LO).sum() > 100 and (d > SC.HI).sum() > 100
    return d


def _diag_session(d, flags):
    n = len(d)
    S = ch.Session(hip_flags=flags)
    A = S.sparse(n, np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int64), d, -1)
    Lf = S.analyze(A, np.arange(n, dtype=np.int64))
    return S, A, Lf


def _kinds(S, Lf):
    return sorted(set(int(k) for k in S.launch_profile(Lf)["kind"]))


def _sqrt_check(S, Lf, d, what):
    fv = ch.FactorView(Lf)
    assert fv.nsuper == len(d) and fv.minor == len(d)                 # one 1 x 1 front per pivot
    u = _ulps(fv.x, np.sqrt(d))
    w = int(np.argmax(u))
    assert float(np.sqrt(d[w])) == math.sqrt(d[w])
    print(f"sqrt through {what}: largest distance {int(u.max())} ulp (at d = {d[w]!r}); "
          f"normal d: {int(u[d >= SC.DBL_MIN].max())} ulp, denormal d: {int(u[d < SC.DBL_MIN].max())} ulp; "
          f"{int((u > 0).sum())} of {len(d)} differ from the correctly rounded root")
    assert u.max() <= 1, (what, d[w], fv.x[w], math.sqrt(d[w]))
    # The final step g + (d - g^2) h of sqrt_rsqrt is what makes the root more than "within 1 ulp".  d - g^2 is exact in the
    # fma (g is within 1 ulp of the root), h is 1 / (2 sqrt (d)) to about 2^-51, so the sum before its one rounding is within
    # 2^-49 ulp of sqrt (d): the result is the correctly rounded root unless sqrt (d) lies that close to the midpoint of two
    # doubles -- for a random mantissa a chance of 2^-48, over these 4096 values 2^-36.  Without the step g carries the
    # roundings of the iteration, half an ulp or so, and is off by one ulp for a fixed fraction of the mantissas (the model of
    # the sequence in exact fma arithmetic, tests/test_scaling_reference.py::test_model_of_the_square_root_sequence: none
    # with the step, more than one in twenty without).  One in a hundred separates the two by a wide margin on either side.
    # (Measured on an MI355X, every path: 0 of 4096 with the step; 794 of 4096, each by 1 ulp, in a build without it.)
    assert (u > 0).sum() <= len(d) // 100, (what, int((u > 0).sum()))
    return int(u.max())


def test_sqrt_within_one_ulp_in_every_front_kernel(L):
    """L_ii against math.sqrt (d_i), d_i over the whole range of positive doubles, denormals included: at most 1 ulp -- the
    contract above sqrt_rsqrt -- in the first factorization (k_thin_front, search path), in a refactorization with new
    values (k_leaf_pair through the assembly map), with CHOLMOD_HIP_NO_LEAF_PAIRS (k_thin_front, mapped) and with
    CHOLMOD_HIP_NO_SMALL_FRONTS (k_potrf_mfma / pf_eliminate).
    Which kernel a run is attributed to is INFERRED from the engine's dispatch, not observed: the launch list
    (cholmod_hip_get_launch_profile) is the plan's, it tells thin-front launches (kind 8) from the panel chain but not
    k_thin_front from k_leaf_pair, which the engine picks at launch time -- leaf fronts of a plan without
    CHOLMOD_HIP_NO_LEAF_PAIRS, once the assembly map of a resident S exists (the second factorization on).  What IS
    observed at run time: every factorization produced the new values' roots (d2 is d rotated: a factor left over from the
    run before, or values that never arrived, are off by hundreds of binades)."""
    d = sqrt_values()
    d2 = np.roll(d, 1237)                                              # other values on the same pattern
    S, A, Lf = _diag_session(d, 0)
    assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
    assert 8 in _kinds(S, Lf) and not {2, 3, 9, 10, 13, 14, 16} & set(_kinds(S, Lf))      # thin-front launches, no panel chain
    _sqrt_check(S, Lf, d, "k_thin_front (first factorization)")
    _set_values(A, d2)
    assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
    _sqrt_check(S, Lf, d2, "k_leaf_pair (values-only refactorization)")
    S.free_factor(Lf); S.free_sparse(A); S.finish()
    S, A, Lf = _diag_session(d, NO_LEAF_PAIRS)
    assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
    _set_values(A, d2)
    assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
    assert 8 in _kinds(S, Lf) and not {2, 3, 9, 10, 13, 14, 16} & set(_kinds(S, Lf))
    _sqrt_check(S, Lf, d2, "k_thin_front (mapped, no leaf pairs)")
    S.free_factor(Lf); S.free_sparse(A); S.finish()
    S, A, Lf = _diag_session(d, NO_SMALL_FRONTS)
    assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
    assert 8 not in _kinds(S, Lf) and {2, 9, 10} & set(_kinds(S, Lf))   # generic kernels: the panel chain
    _sqrt_check(S, Lf, d, "k_potrf_mfma (no thin fronts)")
    S.free_factor(Lf); S.free_sparse(A); S.finish()



def two_by_two_values():
    """2048 blocks [[d, a], [a, d2]]: d from the sweep of part 1 (normal, >= DBL_MIN / eps so that 1 / d is finite),
    |a| = sqrt(d) 2^k for small k and either sign, d2 = 4 a^2 / d -- of order one whatever d is: the block mixes magnitudes"""
    rng = np.random.default_rng(77)
    nb = 2048
    d = np.ldexp(1.0 + rng.integers(0, 2 ** 52, nb).astype(np.float64) * 2.0 ** -52, rng.integers(-969, 1023, nb))
    d[:8] = [SC.LO, np.nextafter(SC.LO, 0.0), np.nextafter(SC.LO, 1.0), SC.HI, np.nextafter(SC.HI, 0.0), np.nextafter(SC.HI, np.inf),
             SC.DBL_MIN * 2.0 ** 53, 2.0 ** 1022]
    assert np.all(d >= SC.DBL_MIN * 2.0 ** 53)
    a = np.ldexp(np.sqrt(d), rng.integers(-3, 4, nb)) * rng.choice([-1.0, 1.0], nb)
    dl, al = d.astype(np.longdouble), a.astype(np.longdouble)
    d2 = (4 * al * al / dl).astype(np.float64)
    assert np.all(np.isfinite(d2)) and np.all(d2 >= 2.0 ** -5) and np.all(d2 <= 2.0 ** 9)
    return d, a, d2


def _blocks_csc(d, a, d2):
    nb = len(d)
    Ap = np.zeros(2 * nb + 1, dtype=np.int64)
    Ap[1::2] = 3 * np.arange(nb) + 2
    Ap[2::2] = 3 * np.arange(nb) + 3
    Ai = np.stack([2 * np.arange(nb), 2 * np.arange(nb) + 1, 2 * np.arange(nb) + 1], axis=1).reshape(-1).astype(np.int64)
    Ax = np.stack([d, a, d2], axis=1).reshape(-1)
    return 2 * nb, Ap, Ai, Ax


@pytest.mark.parametrize("flags", [0, NO_LEAF_PAIRS, NO_SMALL_FRONTS])
def test_two_by_two_blocks(L, flags):
    """L21 = a / sqrt (d) against numpy's long double within 2 ulp: ri = 1 / sqrt (d) is within 1 ulp and the product adds
    one rounding.  L22 = sqrt (d2 - a^2 / d) within 8 eps relative, eps = 2^-53: the kernels form t = a (1 / d) with 1 / d
    within 1.5 ulp = 3 eps (v_rcp_f64 and one Newton step, or 4 eps where 1 / d is subnormal, d > 2^1022) and one rounding,
    then fma (-t, a, d2): the subtrahend a^2 / d = l^2 <= d2 / 4 (1 + eps) carries at most 5 eps, against a difference of
    3 d2 / 4 that is 5/3 eps, plus the rounding of the fma 8/3 eps; the square root halves it, 4/3 eps, and adds its own
    1 ulp = 2 eps: under 4 eps -- 8 eps leaves a factor of two.  First factorization and values-only refactorization."""
    d, a, d2 = two_by_two_values()
    n, Ap, Ai, Ax = _blocks_csc(d, a, d2)
    dl, al, d2l = (v.astype(np.longdouble) for v in (d, a, d2))
    assert np.finfo(np.longdouble).nmant >= 63
    l21 = al / np.sqrt(dl)
    l22 = np.sqrt(d2l - al * al / dl)
    S = ch.Session(hip_flags=flags)
    A = S.sparse(n, Ap, Ai, Ax, -1)
    Lf = S.analyze(A, np.arange(n, dtype=np.int64))
    for rnd in range(2):
        assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
        fv = ch.FactorView(Lf)
        assert fv.nsuper == len(d) and fv.minor == n and np.all(np.diff(fv.px) == 4)
        x = fv.x.reshape(-1, 4)                                        # (L11, L21, dead, L22) of every block
        assert _ulps(x[:, 0], np.sqrt(d)).max() <= 1
        u21 = _ulps(np.abs(x[:, 1]), np.abs(l21).astype(np.float64))
        assert np.array_equal(np.sign(x[:, 1]), np.sign(a))
        r22 = np.abs((x[:, 3].astype(np.longdouble) - l22) / l22).astype(np.float64)
        print(f"2 x 2 blocks, flags {flags}, factorization {rnd}: L21 at most {int(u21.max())} ulp from the rounded exact value, "
              f"L22 at most {r22.max() / EPS:.2f} eps")
        assert u21.max() <= 2, (d[np.argmax(u21)], a[np.argmax(u21)])
        assert r22.max() <= 8 * EPS, (d[np.argmax(r22)], a[np.argmax(r22)])
        assert np.all(x[:, 2] == 0)
    S.free_factor(Lf); S.free_sparse(A); S.finish()


# ---- 2. dense fronts under scaling -----------------------------------------------------------------------------------------

_dense_unscaled = {}


def _dense_check(L, nsrow, nscol, flags, profile):
    Fm, L11, L21, Sc, e, Fs = SC.dense_case(nsrow, nscol, profile)
    F = np.asfortranarray(Fs.copy())
    info = C.c_int64(-1)
    rc = L.cholmod_hip_dense_partial_factor(F.ctypes.data, nsrow, nscol, flags, C.byref(info))
    assert rc == 0 and info.value == 0
    # strictly upper part of the diagonal block is never written
    assert np.array_equal(np.triu(F[:nscol, :nscol], 1), np.triu(Fs[:nscol, :nscol], 1))
    assert np.all(np.isfinite(F))
    B = SC.descale_front(F, nscol, e)
    e11 = np.linalg.norm(np.tril(B[:nscol, :nscol]) - L11) / np.linalg.norm(L11)
    e21 = np.linalg.norm(B[nscol:, :nscol] - L21) / np.linalg.norm(L21)
    esc = np.linalg.norm(np.tril(B[nscol:, nscol:]) - Sc) / np.linalg.norm(Sc)
    key = (nsrow, nscol, flags, os.environ.get("CHOLMOD_HIP_NO_CHAINF"))
    if key not in _dense_unscaled:                                  # the engine's own result for the unscaled front, once
        F0 = np.asfortranarray(Fm.copy())
        assert L.cholmod_hip_dense_partial_factor(F0.ctypes.data, nsrow, nscol, flags, C.byref(info)) == 0 and info.value == 0
        _dense_unscaled[key] = F0
    same = np.array_equal(np.tril(B[:, :nscol]), np.tril(_dense_unscaled[key][:, :nscol]))
    print(f"dense {nsrow} x {nscol} flags {flags} {profile}: L11 {e11:.2e} L21 {e21:.2e} Schur {esc:.2e}; "
          f"COVARIANT {profile} bit for bit with the engine's own unscaled [L11; L21]: {same}")
    assert e11 < 1e-13 and e21 < 1e-12 and esc < 1e-12             # test_dense_partial_factorization's


@pytest.mark.parametrize("profile", SC.PROFILES)
@pytest.mark.parametrize("flags", [0, 512, 1024, 512 | 1024, 8192])
@pytest.mark.parametrize("nsrow,nscol", SC.DENSE_SHAPES)
def test_dense_front_under_scaling(L, nsrow, nscol, flags, profile):
    """cholmod_hip_dense_partial_factor on D (M M' + n I) D: L11 and L21 descaled by D_i, the Schur block by D_i D_j, against
    LAPACK on the unscaled front; the fused chain, potrf / trsm launches of their own, and the 256-column chain"""
    _dense_check(L, nsrow, nscol, flags, profile)


def _chain_kinds(L, nsrow, nscol):
    """launch kinds of a host-only CHOLMOD_HIP_CHAIN256 plan whose first front is nsrow x nscol (a dense root below it)"""
    n = nsrow
    sup = np.array([0, nscol, n], dtype=np.int64)
    pi = np.array([0, nsrow, nsrow + n - nscol], dtype=np.int64)
    px = np.array([0, nsrow * nscol, nsrow * nscol + (n - nscol) ** 2], dtype=np.int64)
    s = np.concatenate([np.arange(n), np.arange(nscol, n)]).astype(np.int64)
    st = C.c_int(0)
    P = L.cholmod_hip_plan_create(n, 2, sup.ctypes.data, pi.ctypes.data, px.ctypes.data, s.ctypes.data,
                                  8192 | ch.HIP_PLAN_HOST_ONLY, C.byref(st))
    assert P and st.value == 0
    nl = L.cholmod_hip_get_launch_profile(P, 0, None, None, None, None, None, None)
    kind = np.zeros(nl, dtype=np.int32)
    L.cholmod_hip_get_launch_profile(P, nl, kind.ctypes.data, None, None, None, None, None)
    L.cholmod_hip_plan_destroy(P)
    return set(int(k) for k in kind)


@pytest.mark.parametrize("profile", SC.PROFILES)
def test_dense_front_under_scaling_two_kernel_chain256(L, monkeypatch, profile):
    """the 256-column chain as k_diag + k_rowsolve (CHOLMOD_HIP_NO_CHAINF in the environment, as test_dist.py sets it).  The
    dense entry point exposes no plan, so that the variable is spelled as the scheduler reads it is checked on a host-only
    plan of the same front: launch kinds 13 / 14 take the place of 16."""
    assert 16 in _chain_kinds(L, 700, 530) and not {13, 14} & _chain_kinds(L, 700, 530)
    monkeypatch.setenv("CHOLMOD_HIP_NO_CHAINF", "1")
    assert {13, 14} <= _chain_kinds(L, 700, 530) and 16 not in _chain_kinds(L, 700, 530)
    _dense_check(L, 700, 530, 8192, profile)


# ---- 3. sparse factor and host-array solves under scaling ------------------------------------------------------------------

def _rel(x, ref):
    return np.linalg.norm(x - ref) / np.linalg.norm(ref)


def _factor_check(S, Lf, ref, e, tag):
    fv = ch.FactorView(Lf)
    for k, v in ref.struct.items():
        assert np.array_equal(getattr(fv, k), v), k
    assert fv.minor == ref.n
    m = ref.mask
    assert np.all(np.isfinite(fv.x))
    err = _rel(SC.descale_factor(fv.x, ref, e)[m], ref.x[m])
    print(f"{tag}: ||D^-1 L - L_ref|| / ||L_ref|| = {err:.2e}")
    assert err < TOL_L, (tag, err)
    assert np.all(fv.x[~m] == 0)                                       # dead upper triangles stay zero
    return err


@pytest.mark.parametrize("profile", SC.PROFILES)
@pytest.mark.parametrize("flags", [0, 16, 512 | 1024, 8192])
@pytest.mark.parametrize("name", SC.SPARSE_NAMES)
def test_sparse_factor_and_solves_under_scaling(L, name, flags, profile):
    """The factor of D A D, descaled row by row, against the oracle's factor of A: the first factorization (search path),
    then -- after a values-only factorization of A itself -- D A D again through the assembly map (leaf fronts two to a
    wave).  Session.solve: A x = D c gives x = D^-1 A^-1 c, L y = D c gives y = L_ref^-1 c, L' z = c gives z = D^-1 L_ref^-T c
    (the right-hand side for which the solve with L' is the scaled image of the unscaled one)."""
    ref, e, Axs = SC.sparse_case(name, profile)
    zero = np.zeros(ref.n, dtype=np.int64)
    S = ch.Session(hip_flags=flags)
    A = S.sparse(ref.n, ref.Ap, ref.Ai, Axs, -1)
    Lf = S.analyze(A, ref.perm)
    assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
    _factor_check(S, Lf, ref, e, f"{name} flags {flags} {profile} first")
    _set_values(A, ref.Ax)
    assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
    _factor_check(S, Lf, ref, zero, f"{name} flags {flags} unscaled, mapped")
    x0 = ch.FactorView(Lf).x.copy()
    _set_values(A, Axs)
    assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
    _factor_check(S, Lf, ref, e, f"{name} flags {flags} {profile} mapped")
    # reported, not asserted: is the engine's factor of D A D bit for bit D times its own factor of A?
    same = np.array_equal(SC.descale_factor(ch.FactorView(Lf).x, ref, e)[ref.mask], x0[ref.mask])
    print(f"{name} flags {flags}: COVARIANT {profile} bit for bit with the engine's own unscaled factor: {same}")
    rng = np.random.default_rng(5)
    c = rng.standard_normal((3, ref.n))
    ep = e[ref.struct["Perm"]]                                         # D in the factor's ordering
    x = np.ldexp(S.solve(Lf, np.ldexp(c, e[None, :])), e[None, :])
    assert _rel(x, ref.O.solve(c)) < 1e-10
    for k in range(3):
        r = SC.G.sym_matvec(ref.n, ref.Ap, ref.Ai, ref.Ax, -1, x[k]) - c[k]
        assert np.linalg.norm(r) / np.linalg.norm(c[k]) < TOL_RES
    y = S.solve(Lf, np.ldexp(c, ep[None, :]), ch.SYS_L)
    assert _rel(y, ref.O.lsolve(c)) < 1e-11
    z = np.ldexp(S.solve(Lf, c, ch.SYS_Lt), ep[None, :])
    assert _rel(z, ref.O.ltsolve(c)) < 1e-11
    S.free_factor(Lf); S.free_sparse(A); S.finish()


@pytest.mark.parametrize("profile", ["down", "mixed"])
def test_complex_hermitian_under_real_scaling(L, profile):
    """a complex Hermitian matrix through the GPU path of test_complex.py (complex storage: the PHI / CX pivot code), real D"""
    ref, e, Axs = SC.sparse_case("cx_p3d_9_nd", profile)
    S = ch.Session(use_gpu=1)
    A = S.sparse(ref.n, ref.Ap, ref.Ai, Axs, -1)
    Lf = S.analyze(A, ref.perm)
    assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
    fv = ch.FactorView(Lf)
    assert fv.xtype == ch.COMPLEX
    _factor_check(S, Lf, ref, e, f"complex {profile}")
    rng = np.random.default_rng(7)
    c = rng.standard_normal((2, ref.n)) + 1j * rng.standard_normal((2, ref.n))
    x = SC._ldexp(S.solve(Lf, SC._ldexp(c, e[None, :])), e[None, :])
    xo = ref.O.solve_complex(c)
    assert _rel(x, xo) < 1e-10
    S.free_factor(Lf); S.free_sparse(A); S.finish()


# ---- 3b. device-array solves, residual and refinement (child processes) -------------------------------------------------------

_device_results = {}


def _device(name):
    if name not in _device_results:
        p = subprocess.run([sys.executable, os.path.join(HERE, "pivot_range_device_cases.py"), name],
                           capture_output=True, text=True, timeout=120)      # (torch's start, then well under a second per profile and nrhs)
        print(p.stdout)
        print(p.stderr[-4000:])
        res = [ln[7:] for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        _device_results[name] = json.loads(res[-1]) if (p.returncode == 0 and res) else {"child": f"exit status {p.returncode}"}
    return _device_results[name]


@pytest.mark.parametrize("profile", SC.PROFILES)
@pytest.mark.parametrize("name", SC.SPARSE_NAMES)
def test_device_solves_residual_and_refinement_under_scaling(name, profile):
    """solve_device with 3 (column kernels) and 20 (MFMA panel kernels) right-hand sides for A, L and L', residual_device
    within its componentwise bound on the scaled data, one refinement step that increases no column norm.  One child
    process per matrix runs the four profiles; every profile has its own verdict."""
    r = _device(name)
    assert profile in r, r
    assert r[profile] == "ok", r[profile]


def test_big_supernode_block_walk_under_mixed_scaling():
    """the 1400-column supernode of test_big_supernode_block_walk_solves_multi_rhs under `mixed`: the explicit 64 x 64
    inverses and the block walk of the solves (k_diag_inv64, Winv, k_solve_*_diag, k_sd_*_diag)"""
    r = _device("big_supernode")
    assert r.get("mixed") == "ok", r


# ---- 4. the failure boundary, by value ---------------------------------------------------------------------------------------

BAD = {"+0.0": 0.0, "-0.0": -0.0, "-5e-324": -5e-324}
COLS = [0, 15, 16, 63, 64, N1 - 1]


def _planted_check(S, A, Lf, d, col, v):
    n = len(d)
    dd = d.copy()
    dd[col] = v
    O = OracleFactor(n, np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int64), -1, perm=np.arange(n, dtype=np.int64),
                     postorder=True)
    assert O.factorize(dd) == 1 and O.minor == col                     # LAPACK's test: ajj <= 0
    _set_values(A, dd)
    assert S.factorize(A, Lf) == 1                                      # TRUE, as the reference
    assert S.cm.status == ch.NOT_POSDEF
    fv = ch.FactorView(Lf)
    assert fv.minor == col, (col, v, fv.minor)
    assert np.array_equal(fv.x != 0, O.x != 0)
    assert np.all(fv.x[col:] == 0)
    assert _ulps(fv.x[:col], np.sqrt(dd[:col])).max(initial=0) <= 1


@pytest.mark.parametrize("path", ["first", "mapped", "generic"])
@pytest.mark.parametrize("bad", list(BAD))
def test_zero_and_negative_denormal_pivots_fail_at_their_column(L, bad, path):
    """+0.0, -0.0 and -5e-324 planted in the diagonal matrix of part 1 at column 0, 15, 16, 63, 64 or the last: minor is that
    column, status NOT_POSDEF, zeros from it on -- minor and the zero pattern as the oracle's.  first: every case the first
    factorization of its plan (k_thin_front, search path); mapped: values-only refactorizations (k_leaf_pair); generic:
    CHOLMOD_HIP_NO_SMALL_FRONTS (pf_eliminate)."""
    d = sqrt_values()
    d[COLS] = [3.0, 1e300, 1e-300, 2.0, 5.0, 7.0]                      # (no denormal at a planted column's place)
    if path == "first":
        for col in COLS:
            S, A, Lf = _diag_session(d, 0)
            _planted_check(S, A, Lf, d, col, BAD[bad])
            S.free_factor(Lf); S.free_sparse(A); S.finish()
        return
    S, A, Lf = _diag_session(d, NO_SMALL_FRONTS if path == "generic" else 0)
    assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
    for col in COLS:
        _planted_check(S, A, Lf, d, col, BAD[bad])
    _set_values(A, d)                                                  # and positive definite again
    assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK and ch.FactorView(Lf).minor == len(d)
    S.free_factor(Lf); S.free_sparse(A); S.finish()


@pytest.mark.parametrize("path", ["first", "mapped", "generic"])
def test_smallest_positive_pivots_succeed(L, path):
    """+5e-324 and DBL_MIN on 1 x 1 fronts at the same columns: a success, L_ii within 1 ulp of the square root"""
    d = sqrt_values()
    d[COLS] = [5e-324, SC.DBL_MIN, 5e-324, SC.DBL_MIN, 5e-324, SC.DBL_MIN]
    S, A, Lf = _diag_session(d, NO_SMALL_FRONTS if path == "generic" else 0)
    for _ in range(2 if path == "mapped" else 1):
        assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
    fv = ch.FactorView(Lf)
    assert fv.minor == len(d)
    assert _ulps(fv.x, np.sqrt(d)).max() <= 1
    S.free_factor(Lf); S.free_sparse(A); S.finish()


@pytest.mark.parametrize("bad", list(BAD))
def test_dense_front_zero_and_negative_denormal_pivots(L, bad):
    """the same values as a pivot of the (200, 100) dense front: row and column `col` of the front are cleared and its
    diagonal entry set to the value, so that the pivot the kernel meets at that column is the value itself, whatever came
    before.  info is LAPACK's (ajj <= 0), the columns from it on are zero, the leading block is LAPACK's."""
    Fm, L11, _, _ = SC.dense_reference(200, 100)
    nsrow, nscol = 200, 100
    for flags in (0, 512 | 1024, 8192):
        for col in (0, 15, 16, 63, 64, nscol - 1):
            Fb = Fm.copy()
            Fb[col, :] = 0.0
            Fb[:, col] = 0.0                                        # (column `col` decoupled: its pivot is its diagonal entry, exactly)
            Fb[col, col] = BAD[bad]
            F = np.asfortranarray(Fb.copy())
            info = C.c_int64(-1)
            assert L.cholmod_hip_dense_partial_factor(F.ctypes.data, nsrow, nscol, flags, C.byref(info)) == 0
            assert info.value == col + 1, (flags, col, info.value)      # 1-based failing column, LAPACK convention
            if col:
                lead = np.linalg.cholesky(Fb[:col, :col])
                assert np.linalg.norm(np.tril(F[:col, :col]) - lead) / np.linalg.norm(lead) < 1e-13
            ii, jj = np.indices((nsrow, nscol))
            assert np.all(F[:, :nscol][(jj >= col) & (ii >= jj)] == 0), (flags, col)
