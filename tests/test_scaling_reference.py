"""The reference of tests/test_gpu_pivot_range.py, tied down without a GPU: for every matrix, dense front and exponent
profile used there, the CPU factor of D M D, descaled by the exact powers of two, IS the CPU factor of M -- bit for bit --
and the preconditions of the case hold (scaling_cases.py).  The GPU tests may therefore hold the engine's factor of the
scaled matrix against the oracle's / LAPACK's factor of the unscaled one at the suite's usual tolerances."""
import numpy as np
import pytest

import scaling_cases as SC


def _same_bits(a, b):
    if np.iscomplexobj(a):
        return _same_bits(np.real(a), np.real(b)) and _same_bits(np.imag(a), np.imag(b))
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


@pytest.mark.parametrize("profile", SC.PROFILES)
@pytest.mark.parametrize("name", SC.SPARSE_NAMES + ["big_supernode", "cx_p3d_9_nd"])
def test_oracle_factor_is_covariant(name, profile):
    ref, e, Axs = SC.sparse_case(name, profile)                 # (asserts the preconditions)
    O = ref.factor(Axs)
    for k, v in ref.struct.items():
        assert np.array_equal(getattr(O, k), v), k
    xs = O.xc if ref.cx else O.x
    m = ref.mask
    assert _same_bits(SC.descale_factor(xs, ref, e)[m], ref.x[m])


@pytest.mark.parametrize("profile", SC.PROFILES)
@pytest.mark.parametrize("nsrow,nscol", SC.DENSE_SHAPES)
def test_lapack_front_is_covariant(nsrow, nscol, profile):
    Fm, L11, L21, Sc, e, Fs = SC.dense_case(nsrow, nscol, profile)
    L11s = np.linalg.cholesky(Fs[:nscol, :nscol])
    assert _same_bits(np.ldexp(L11s, -e[:nscol, None]), L11)
    # descale_front on the front a partial factorization of D Fm D leaves in exact arithmetic: D L11 under the untouched
    # upper triangle, D L21, D Sc D
    done = Fs.copy()
    done[:nscol, :nscol] = np.triu(Fs[:nscol, :nscol], 1) + np.ldexp(L11, e[:nscol, None])
    done[nscol:, :nscol] = np.ldexp(L21, e[nscol:, None])
    done[nscol:, nscol:] = np.ldexp(Sc, e[nscol:, None] + e[None, nscol:])
    back = SC.descale_front(done, nscol, e)
    assert _same_bits(back[:nscol, :nscol], np.triu(Fm[:nscol, :nscol], 1) + L11)
    assert _same_bits(back[nscol:, :nscol], L21) and _same_bits(back[nscol:, nscol:], Sc)


def test_exponent_choices():
    """E_up is the largest exponent that keeps 2^(2E) max|A| below 2^1020, E_down the largest that puts the largest pivot
    below 1e-290"""
    for amax in (1.0, 4.0, 125.0, 0.75, 2.0 ** 40 - 1.0, 1e9):
        E = SC._e_up(amax)
        assert np.ldexp(amax, 2 * E) < 2.0 ** 1020 and not np.ldexp(amax, 2 * (E + 1)) < 2.0 ** 1020
    for pmax in (1.0, 6.0, 1400.0, 1e12):
        E = SC._e_down(pmax)
        assert np.ldexp(pmax, 2 * E) < SC.LO and not np.ldexp(pmax, 2 * (E + 1)) < SC.LO


# ---- a host model of sqrt_rsqrt (csrc/hip/kernels.hip.h), instruction by instruction ------------------------------------------
# What tests/test_gpu_pivot_range.py asserts about the correctly rounded fraction of the roots rests on it.  Every fma is
# exact (rational arithmetic, one rounding); the v_rsq_f64 seed is the rounded 1 / sqrt (d) put off by a relative error of
# up to 2^-26, the accuracy the kernel's comment gives for it.

def _fma(a, b, c):
    from fractions import Fraction
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def sqrt_rsqrt_model(d, seed_error, lo=1e-290, correct=True):
    import math
    sh = -512 if d > 1e290 else (512 if d < lo else 0)
    d = math.ldexp(d, sh)
    y = (1.0 / math.sqrt(d)) * (1.0 + seed_error)
    g, h = d * y, 0.5 * y
    e = _fma(-h, g, 0.5)
    g, h = _fma(g, e, g), _fma(h, e, h)
    e = _fma(-h, g, 0.5)
    g, h = _fma(g, e, g), _fma(h, e, h)
    t = _fma(-g, g, d)
    if correct:
        g = _fma(t, h, g)
    ri = h + h
    u = _fma(-g, ri, 1.0)
    ri = _fma(u, ri, ri)
    return math.ldexp(g, -(sh >> 1)), math.ldexp(ri, sh >> 1)


def test_model_of_the_square_root_sequence():
    """With the final step g + (d - g^2) h every root of the sample is the correctly rounded one, whatever the seed's error
    within 2^-26; without it the root stays within 1 ulp -- a `within 1 ulp` assertion cannot see the step go -- but more
    than one root in twenty is off by that ulp.  The bound of one in a hundred in the GPU test lies between the two."""
    import math
    rng = np.random.default_rng(11)
    n = 1500
    d = np.ldexp(1.0 + rng.integers(0, 2 ** 52, n).astype(np.float64) * 2.0 ** -52, rng.integers(-1021, 1023, n))
    d[:64] = rng.integers(1, 2 ** 52, 64).astype(np.int64).view(np.float64)          # denormals
    err = rng.uniform(-1.0, 1.0, n) * 2.0 ** -26
    err[::7] = 2.0 ** -26
    err[3::7] = -2.0 ** -26
    off = {True: 0, False: 0}
    for correct in (True, False):
        for k in range(n):
            r, _ = sqrt_rsqrt_model(float(d[k]), float(err[k]), correct=correct)
            u = abs(int(np.float64(r).view(np.int64)) - int(np.float64(math.sqrt(d[k])).view(np.int64)))
            assert u <= 1
            off[correct] += u
    assert off[True] == 0
    assert off[False] > n // 20, off


def test_model_rescale_threshold_has_slack():
    """Between 1e-300 and 1e-290 the rescale by 2^512 changes neither result, bit for bit: without it only the residual
    t = d - g^2 is subnormal, off by at most 2^-1075, which reaches the root as less than 2^-27 ulp.  A threshold of 1e-300 in
    place of 1e-290 is therefore invisible to any test of values."""
    rng = np.random.default_rng(12)
    n = 600
    d = np.ldexp(1.0 + rng.integers(0, 2 ** 52, n).astype(np.float64) * 2.0 ** -52, rng.integers(-996, -964, n))
    assert np.all((d >= 1e-300) & (d < 1e-290))
    for k in range(n):
        err = float(rng.uniform(-1.0, 1.0)) * 2.0 ** -26
        assert sqrt_rsqrt_model(float(d[k]), err) == sqrt_rsqrt_model(float(d[k]), err, lo=1e-300)
