"""The device-side verification kernels shown factors that are wrong (run with -m gpu on an MI355X).

cholmod_hip_factor_checks, cholmod_hip_factor_checks_local and cholmod_hip_diag_minmax are what the suite relies on at
sizes without a CPU oracle, and every other test compares their counters with zero only.  Here a factor is computed
once, downloaded, and edited copies go back through cholmod_hip_upload_factor: planted NaN / inf / zeros / dead-triangle
entries must be counted exactly, and the two sums must stay within bounds derived below, against the numpy reference of
tests/factor_check_reference.py (itself tied to trace (A) and log det (A) in tests/test_factor_check_reference.py).

Bounds on the two sums (the counters are integers far below 2^53: exact):
  fro2         every term is one fused multiply-add into a sum of non-negative terms, so any order of summation is
               within (N - 1) 2^-53 relative to first order, N = entries of the lower trapezoids.  Bound: N 2^-52 fro2.
  half_logdet  n logarithms, each taken as at most 1 ulp off (the figure of the ROCm device library's documentation for
               the fp64 log), summed in some order: (n - 1) 2^-53 + 2^-52 relative to sum |log L_jj|.
               Bound: (n + 2) 2^-52 sum |log L_jj|.
Both leave a factor of two over those worst cases.  Each comparison prints the observed error as a fraction of its bound."""
import ctypes as C
import math

import numpy as np
import pytest

import factor_check_reference as R
from suitesparse_amd import cholmod as ch

pytestmark = pytest.mark.gpu

KEYS = ("half_logdet", "upper_nonzeros", "nonfinite", "fro2", "nonpositive_diag")
COUNTS = ("upper_nonzeros", "nonfinite", "nonpositive_diag")
WORST = {"fro2": 0.0, "half_logdet": 0.0}       # largest observed error / bound, printed by every comparison


def _bits(*v):
    return np.array(v, dtype=np.float64).view(np.uint64).tolist()


class Resident:
    """A matrix factorized once by the engine; edited copies of its factor go up and the checks are read back."""

    def __init__(self, name, factor_on_device=False):
        assert ch.lib().cholmod_hip_probe() == 1, "no HIP device visible"
        self.name = name
        n, Ap, Ai, Ax, perm = R.matrix(name)
        self.n = n
        self.S = S = ch.Session(factor_on_device=factor_on_device)
        self.A = S.sparse(n, Ap, Ai, Ax, -1)
        self.Lf = S.analyze(self.A, perm)
        assert S.factorize(self.A, self.Lf) == 1 and S.cm.status == ch.OK
        fv = ch.FactorView(self.Lf)
        assert fv.minor == n and fv.xtype == ch.REAL
        self.plan = self.Lf.contents.hip_plan
        assert self.plan
        self.shape = R.FactorShape(fv.super, fv.pi, fv.px, fv.xsize)
        R.assert_front_shapes(name, self.shape)
        self.good = self.download()
        self.good.flags.writeable = False

    def download(self):
        x = np.full(self.shape.xsize, -7.0)
        assert self.S.L.cholmod_hip_download_factor(self.plan, x.ctypes.data) == 0
        return x

    def upload(self, x):
        assert x.dtype == np.float64 and x.flags.c_contiguous and len(x) == self.shape.xsize
        assert self.S.L.cholmod_hip_upload_factor(self.plan, x.ctypes.data) == 0

    def checks(self, local=False):
        out = np.full(5, -1.0)
        f = self.S.L.cholmod_hip_factor_checks_local if local else self.S.L.cholmod_hip_factor_checks
        assert f(self.plan, out.ctypes.data) == 0
        assert all(out[q] == int(out[q]) for q in (1, 2, 4))
        return dict(half_logdet=float(out[0]), upper_nonzeros=int(out[1]), nonfinite=int(out[2]), fro2=float(out[3]),
                    nonpositive_diag=int(out[4]))

    def minmax(self):
        out = np.full(3, -1.0)
        assert self.S.L.cholmod_hip_diag_minmax(self.plan, out.ctypes.data) == 0
        return float(out[0]), float(out[1]), int(out[2])

    def close(self):
        self.S.free_factor(self.Lf)
        self.S.free_sparse(self.A)
        self.S.finish()


@pytest.fixture(scope="module")
def resident():
    made = {}

    def get(name, factor_on_device=False):
        key = (name, factor_on_device)
        if key not in made:
            made[key] = Resident(name, factor_on_device)
        return made[key]

    yield get
    for r in made.values():
        r.close()


def assert_matches(got, shape, x, what, ref=None):
    """The three counters equal the reference exactly, the two sums within the bounds of the module docstring."""
    ref = R.factor_checks(shape, x) if ref is None else ref
    for k in COUNTS:
        assert got[k] == ref[k], (what, k, got, ref)
    bounds = {"fro2": len(shape.lower) * R.EPS * ref["fro2"],
              "half_logdet": (shape.n + 2) * R.EPS * R.sum_abs_log_diag(shape, x)}
    for k, b in bounds.items():
        if not math.isfinite(ref[k]):                    # (+inf on the diagonal: log (+inf) = +inf, nothing to bound)
            assert got[k] == ref[k], (what, k, got, ref)
            continue
        err = abs(got[k] - ref[k])
        frac = err / b if b > 0 else 0.0
        WORST[k] = max(WORST[k], frac)
        print(f"{what}: {k} = {got[k]!r}, reference {ref[k]!r}, error {err:.3e} = {frac:.4f} of the bound {b:.3e} "
              f"(largest so far {WORST[k]:.4f})")
        assert err <= b, (what, k, got, ref, b)
    return ref


# ---- cholmod_hip_factor_checks, real storage --------------------------------------------------------------------------

@pytest.mark.parametrize("name", R.REAL_CASES)
def test_good_factor(resident, name):
    r = resident(name)
    r.upload(r.good)
    got = r.checks()
    assert (got["upper_nonzeros"], got["nonfinite"], got["nonpositive_diag"]) == (0, 0, 0)
    assert_matches(got, r.shape, r.good, f"{name} good")


@pytest.mark.parametrize("name", R.REAL_CASES)
def test_everything_planted(resident, name):
    r = resident(name)
    sh = r.shape
    x = r.good.copy()
    x[sh.lower] = np.nan
    r.upload(x)
    got = r.checks()
    assert got == dict(half_logdet=0.0, upper_nonzeros=0, nonfinite=len(sh.lower), fro2=0.0, nonpositive_diag=sh.n)
    x = r.good.copy()
    x[sh.dead] = 1.0
    r.upload(x)
    got = r.checks()
    assert got["upper_nonzeros"] == len(sh.dead) and got["nonfinite"] == 0 and got["nonpositive_diag"] == 0
    assert_matches(got, sh, x, f"{name} dead triangles full")
    r.upload(r.good)


def _draw(sh, good, seed, inf_on_diagonal):
    """NaN / +inf / -inf on a random half of the lower entries, a nonzero / NaN / -0.0 on a random half of the dead ones,
    0.0 / -0.0 / a negative / NaN on a random third of the diagonal.  +inf on the diagonal makes half_logdet +inf (its
    logarithm is summed), which would leave nothing of that sum to compare: only the draws with inf_on_diagonal keep it
    there, the others turn it into -inf."""
    rng = np.random.default_rng(seed)
    x = good.copy()
    sel = rng.permutation(sh.lower)[:(len(sh.lower) + 1) // 2]
    v = np.array([np.nan, np.inf, -np.inf])[rng.integers(0, 3, len(sel))]
    if not inf_on_diagonal:
        v[np.isin(sel, sh.diag) & (v == np.inf)] = -np.inf
    x[sel] = v
    sel = rng.permutation(sh.dead)[:(len(sh.dead) + 1) // 2]
    x[sel] = np.array([1.5, np.nan, -0.0])[rng.integers(0, 3, len(sel))]
    sel = rng.permutation(sh.diag)[:(len(sh.diag) + 2) // 3]
    x[sel] = np.array([0.0, -0.0, -2.5, np.nan])[rng.integers(0, 4, len(sel))]
    return x


@pytest.mark.parametrize("name", R.REAL_CASES)
def test_random_subsets(resident, name):
    r = resident(name)
    for seed in range(6):
        x = _draw(r.shape, r.good, 100 * len(name) + seed, inf_on_diagonal=(seed == 5))
        r.upload(x)
        ref = assert_matches(r.checks(), r.shape, x, f"{name} draw {seed}")
        if r.n > 1:     # (n = 1: no dead entry, and the one diagonal entry is always among the planted third)
            assert ref["nonfinite"] > 0 and ref["nonpositive_diag"] > 0 and ref["upper_nonzeros"] > 0
            assert math.isfinite(ref["half_logdet"]) == (seed != 5)
    r.upload(r.good)


def _fronts_for_single_defects(name, sh):
    if name == "blocks70_135":
        return [0, 1]
    return sorted({int(np.argmax(sh.nscol)), int(np.argmax(sh.nsrow))})     # 214 x 214 and 75 x 219


@pytest.mark.parametrize("name", ["blocks70_135", "p3d_12_nd"])
def test_one_defect_at_a_time(resident, name):
    r = resident(name)
    sh = r.shape
    x = r.good.copy()
    zero = dict(upper_nonzeros=0, nonfinite=0, nonpositive_diag=0)
    uploads = 0

    def counts_with(idx, value):
        nonlocal uploads
        keep = x[idx]
        x[idx] = value
        r.upload(x)
        x[idx] = keep
        uploads += 1
        got = r.checks()
        return {k: got[k] for k in COUNTS}

    for k in _fronts_for_single_defects(name, sh):
        nscol, nsrow = int(sh.nscol[k]), int(sh.nsrow[k])
        rows = sorted({i for i in (0, 63, 64, 127, 128, nsrow - 1) if i < nsrow})
        cols = sorted({j for j in (0, 3, 4, 63, 64, 127, 128, nscol - 1) if j < nscol})
        for j in cols:
            for i in rows:
                if i < j:
                    continue
                want = dict(zero, nonfinite=1, nonpositive_diag=1 if i == j else 0)
                assert counts_with(sh.at(k, i, j), np.nan) == want, (name, k, i, j)
            assert counts_with(sh.at(k, j, j), 0.0) == dict(zero, nonpositive_diag=1), (name, k, j)
        dead = {(0, 1), (0, nscol - 1), (nscol - 2, nscol - 1), (63, 64), (64, 65)}
        for i, j in sorted(p for p in dead if 0 <= p[0] < p[1] < nscol):
            assert counts_with(sh.at(k, i, j), 7.0) == dict(zero, upper_nonzeros=1), (name, k, i, j)
    print(f"{name}: {uploads} single defects")
    assert np.array_equal(x.view(np.uint64), r.good.view(np.uint64))
    r.upload(r.good)


def assert_same_call(a, b, shape, x, what):
    """Two calls on the same factor.  The counters agree exactly.  The sums need not agree to the bit: every workgroup
    adds its partial sums to the result with an atomic, in the order the workgroups finish.  Both calls add the same T
    partial sums (T = workgroups = 64-column tasks), each order within (T - 1) 2^-53 of their exact sum relative to
    sum |partial| <= fro2 resp. sum |log L_jj|: they differ by at most (T - 1) 2^-52 of that."""
    tasks = int(np.sum((shape.nscol + 63) // 64))
    for k in COUNTS:
        assert a[k] == b[k], (what, k, a, b)
    for k, scale in (("fro2", max(a["fro2"], b["fro2"])), ("half_logdet", R.sum_abs_log_diag(shape, x))):
        d, bound = abs(a[k] - b[k]), (tasks - 1) * R.EPS * scale
        print(f"{what}: {k} of two calls differs by {d:.3e}, bound {bound:.3e} ({tasks} tasks)")
        assert d <= bound, (what, k, a, b, bound)


@pytest.mark.parametrize("name", R.REAL_CASES)
def test_state(resident, name):
    r = resident(name)
    sh = r.shape
    # The accumulators start from zero on every call: a second call returns the same numbers (left uncleared, all five
    # would double) -- the counters exactly, the sums as far as the order of the atomic additions allows.
    r.upload(r.good)
    first = r.checks()
    good_ref = assert_matches(first, sh, r.good, f"{name} good, first call")
    second = r.checks()
    assert_matches(second, sh, r.good, f"{name} good, second call", good_ref)
    assert_same_call(first, second, sh, r.good, f"{name} good")
    x = _draw(sh, r.good, 7, inf_on_diagonal=False)
    r.upload(x)
    planted = r.checks()
    planted_ref = assert_matches(planted, sh, x, f"{name} planted, first call")
    second = r.checks()
    assert_matches(second, sh, x, f"{name} planted, second call", planted_ref)
    assert_same_call(planted, second, sh, x, f"{name} planted")
    assert planted["nonfinite"] + planted["nonpositive_diag"] > 0
    # one rank: the local checks are "the same numbers" (include/cholmod_hip.h)
    loc = r.checks(local=True)
    assert {k: loc[k] for k in COUNTS} == {k: planted[k] for k in COUNTS}
    assert_matches(loc, sh, x, f"{name} local, planted", planted_ref)
    # the kernels only read: what comes back is what went up, bit for bit
    assert np.array_equal(r.download().view(np.uint64), x.view(np.uint64))
    r.upload(r.good)
    again = r.checks()
    assert (again["upper_nonzeros"], again["nonfinite"], again["nonpositive_diag"]) == (0, 0, 0)
    assert_matches(again, sh, r.good, f"{name} good again", good_ref)
    loc = r.checks(local=True)
    assert (loc["upper_nonzeros"], loc["nonfinite"], loc["nonpositive_diag"]) == (0, 0, 0)
    assert_matches(loc, sh, r.good, f"{name} local, good", good_ref)
    assert np.array_equal(r.download().view(np.uint64), r.good.view(np.uint64))


# ---- cholmod_hip_diag_minmax and cholmod_l_rcond ------------------------------------------------------------------------

def _diagonals(sh, seed=3):
    """(label, diagonal) pairs: seeded positive values with the extremes and the special values moved around"""
    n = sh.n
    rng = np.random.default_rng(seed)
    base = rng.uniform(1.0, 2.0, n)
    k = int(np.argmax(sh.nscol))
    places = sorted({c for c in (0, 63, 64, 255, 256, 511, 512, n - 1, int(sh.col0[k]), int(sh.col0[k] + sh.nscol[k] - 1))
                     if 0 <= c < n})
    yield "seeded", base.copy(), True
    for c in places:
        d = base.copy(); d[c] = 0.25
        yield f"min at {c}", d, True
        d = base.copy(); d[c] = 7.5
        yield f"max at {c}", d, True
    mid = n // 2
    d = base.copy(); d[mid] = 5e-324
    yield "denormal min", d, True
    d = base.copy(); d[mid] = np.inf
    yield "inf max", d, True
    d = base.copy()
    bad = rng.permutation(n)[:min(5, n)]
    d[bad[:3]] = np.nan; d[bad[3:]] = -3.0               # (below every positive entry and NaN: none may reach the extremes)
    yield "3 NaN, 2 negative", d, False
    d = base.copy(); d[places[-1]] = np.nan
    yield "one NaN", d, True
    yield "all NaN", np.full(n, np.nan), True
    d = base.copy(); d[mid] = 0.0
    yield "+0.0 min", d, False
    for c in places:
        # -0.0 and, in the same wave, the maximum: the result compares equal to 0 and the maximum is not disturbed
        d = base.copy(); d[c] = -0.0
        if n > 1:
            d[c ^ 1 if (c ^ 1) < n else c - 1] = 7.5
        yield f"-0.0 min at {c}", d, False


def _check_minmax(r, label, d):
    sh = r.shape
    x = r.good.copy()
    x[sh.diag] = d
    r.upload(x)
    got, ref = r.minmax(), R.diag_minmax(sh, x)
    # no arithmetic is involved: the extremes are diagonal entries bit for bit (a zero of either sign: +0.0)
    assert _bits(got[0], got[1]) == _bits(ref[0], ref[1]) and got[2] == ref[2], (r.name, label, got, ref)
    return got


@pytest.mark.parametrize("name", R.REAL_CASES)
def test_diag_minmax(resident, name):
    r = resident(name)
    seen = 0
    for label, d, _ in _diagonals(r.shape):
        got = _check_minmax(r, label, d)
        if label.startswith("-0.0") or label.startswith("+0.0"):
            assert got[0] == 0.0 and math.copysign(1.0, got[0]) == 1.0 and got[2] == 0
        if label == "all NaN":
            assert got == (math.inf, 0.0, r.n)
        seen += 1
    print(f"{name}: {seen} diagonals")
    r.upload(r.good)
    assert r.minmax() == R.diag_minmax(r.shape, r.good)


@pytest.mark.parametrize("name", R.REAL_CASES)
def test_rcond_of_a_resident_factor(resident, name):
    """cholmod_l_rcond on a factor that lives in HBM only takes the device path (k_diag_minmax): (min / max)^2 of the
    diagonal, 0 with a NaN on it -- CHOLMOD/Cholesky/cholmod_rcond.c, restated by the host branch.  One division and one
    square: 1e-15 relative."""
    r = resident(name, factor_on_device=True)
    f = r.Lf.contents
    assert f.hip_on_device and not f.hip_host_valid and not f.x
    for label, d, possible in _diagonals(r.shape):
        if not possible:                                 # (only what a successful factorization could leave)
            continue
        _check_minmax(r, label, d)
        got = r.S.L.cholmod_l_rcond(r.Lf, C.byref(r.S.cm))
        assert r.S.cm.status == ch.OK and not f.hip_host_valid and not f.x
        if np.isnan(d).any():
            want = 0.0
        else:
            q = float(d.min()) / float(d.max())
            want = q * q
        if math.isnan(want):                             # (n = 1 with an infinite entry: inf / inf, on either path)
            assert math.isnan(got), (name, label, got)
        else:
            assert abs(got - want) <= 1e-15 * want, (name, label, got, want)
    r.upload(r.good)


# ---- complex storage ----------------------------------------------------------------------------------------------------

def test_complex_storage(golden_dir):
    """The checks on a complex factor in its own storage are those of the real twin it stands for."""
    from test_complex import _case as complex_case
    n, Ap, Ai, Ax, perm = complex_case("p3d_9_nd", golden_dir)
    S = ch.Session()
    A = S.sparse(n, Ap, Ai, Ax, -1)
    Lf = S.analyze(A, perm)
    assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
    T = C.cast(Lf.contents.cx_twin, C.POINTER(ch.Factor)).contents
    assert T.hip_is_twin == 2 and T.hip_plan and T.xsize == 2 * Lf.contents.xsize
    plan = T.hip_plan
    fv = ch.FactorView(Lf)
    assert fv.xtype == ch.COMPLEX

    def checks():
        out = np.full(5, -1.0)
        assert S.L.cholmod_hip_factor_checks(plan, out.ctypes.data) == 0
        return dict(zip(KEYS, (float(out[0]), int(out[1]), int(out[2]), float(out[3]), int(out[4]))))

    zf = np.full(2 * fv.xsize, -7.0)
    assert S.L.cholmod_hip_download_even_columns(plan, zf.ctypes.data) == 0
    twin, t = R.twin_of_complex(fv.super, fv.pi, fv.px, fv.xsize, zf.view(np.complex128))
    first = checks()
    assert (first["upper_nonzeros"], first["nonfinite"], first["nonpositive_diag"]) == (0, 0, 0)
    good = assert_matches(first, twin, t, "complex p3d_9_nd good")

    csh = R.FactorShape(fv.super, fv.pi, fv.px, fv.xsize)          # (in complex entries)
    k = int(np.argmax(csh.nsrow - csh.nscol + (csh.nscol >= 3) * 10000))
    nscol, nsrow = int(csh.nscol[k]), int(csh.nsrow[k])
    assert nscol >= 3 and nsrow > nscol
    cases = []
    for i, j in ((2, 1), (nsrow - 1, nscol - 1)):                    # inside the diagonal block, below it
        cases.append((2 * csh.at(k, i, j), np.nan, dict(nonfinite=2)))                  # real part
        cases.append((2 * csh.at(k, i, j) + 1, np.nan, dict(nonfinite=2)))              # imaginary part
    for j in (0, nscol - 1):
        cases.append((2 * csh.at(k, j, j), np.nan, dict(nonfinite=2, nonpositive_diag=2)))
        cases.append((2 * csh.at(k, j, j) + 1, 0.375, dict(upper_nonzeros=1)))
    for idx, value, want in cases:
        y = zf.copy()
        y[idx] = value
        assert S.L.cholmod_hip_upload_factor(plan, y.ctypes.data) == 0
        got = checks()
        assert {q: got[q] for q in COUNTS} == dict(dict(upper_nonzeros=0, nonfinite=0, nonpositive_diag=0), **want), (idx, got)
        twin, t = R.twin_of_complex(fv.super, fv.pi, fv.px, fv.xsize, y.view(np.complex128))
        assert_matches(got, twin, t, f"complex, {value} at {idx}")
        if value == 0.375:
            # an imaginary part on the diagonal is a lower entry of the twin: the device's fro2 grows by its square, as
            # far as the two device sums are known (each within N 2^-52 fro2 of the exact one)
            growth, tol = got["fro2"] - first["fro2"], 2 * len(twin.lower) * R.EPS * got["fro2"]
            print(f"complex: fro2 grows by {growth!r} for an imaginary part 0.375 (0.375^2 = {0.375 ** 2}), +- {tol:.3e}")
            assert tol < 1e-3 * 0.375 ** 2 and abs(growth - 0.375 ** 2) <= tol
    assert S.L.cholmod_hip_upload_factor(plan, zf.ctypes.data) == 0
    assert_matches(checks(), *R.twin_of_complex(fv.super, fv.pi, fv.px, fv.xsize, zf.view(np.complex128)),
                   "complex p3d_9_nd good again", good)
    back = np.zeros_like(zf)
    assert S.L.cholmod_hip_download_even_columns(plan, back.ctypes.data) == 0
    assert np.array_equal(back.view(np.uint64), zf.view(np.uint64))
    S.free_factor(Lf)
    S.free_sparse(A)
    S.finish()


# ---- the solves follow an uploaded factor ------------------------------------------------------------------------------

def test_solves_follow_an_uploaded_factor(resident):
    """A supernode of more than 1024 columns is solved in 64-column blocks with cached inverses of the diagonal blocks;
    cholmod_hip_upload_factor must void them.  L -> 2 L is exact, so the solution halves; stale inverses would be off
    by a factor of two in whole blocks.  1e-11 column-wise: the project's bound for a solve, only the order of the
    atomic additions differs between the runs."""
    r = resident("blocks1400_200")
    b = np.random.default_rng(3).standard_normal((3, r.n))
    r.upload(r.good)
    y1 = r.S.solve(r.Lf, b, ch.SYS_L)                    # (caches the inverses)
    twice = 2.0 * r.good
    r.upload(twice)
    y2 = r.S.solve(r.Lf, b, ch.SYS_L)
    r.upload(r.good)
    y3 = r.S.solve(r.Lf, b, ch.SYS_L)
    for q in range(3):
        e2 = np.linalg.norm(y2[q] - 0.5 * y1[q]) / np.linalg.norm(0.5 * y1[q])
        e3 = np.linalg.norm(y3[q] - y1[q]) / np.linalg.norm(y1[q])
        print(f"right-hand side {q}: after 2 L {e2:.2e}, after L again {e3:.2e}")
        assert e2 < 1e-11 and e3 < 1e-11
