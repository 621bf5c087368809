"""The Schur complement on the device-resident factor (Session.schur_device / schur_reduce_device / schur_expand_device,
cholmod_hip_schur_device, cholmod_hip_trailing_multiply_device): Sc = L22 L22' entry by entry against the dense
M_SS - M_SI inv (M_II) M_IS of M = P (A + beta I) P' at the project's parity bar max (1e-12, 20 eps / rcond) max |ref|
(tests/schur_reference.py; the numpy restatement holds it 4 x or more inside, tests/test_schur_api.py), for every m of the
list -- 0, 1, 2, 15, 16, 17, 63, 64, 65, n // 2, n - 1, n, an m whose boundary is the first column of a supernode and one
whose boundary lies strictly inside the last supernode of at least 3 columns (every case of the table has one) --, the dense
L22 bit for bit, nesting, the condensed solve, a chosen subset, Poisson 24^3, the stream contract and the refusals.

The bodies live in tests/schur_cases.py and run in a fresh child process each, as those of tests/test_gpu_selinv.py do: torch
has to be imported before the engine library is loaded."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
# the names of tests/selinv_reference.py: CASES (kept literal here so that collection needs no scipy work)
NAMES = ["arrow300", "arrow300_norelax", "bcsstk01", "bcsstk02", "box9r2_nd", "dense200", "forest148", "forest148_norelax",
         "p2d_60_nd", "p3d_10x7x5_nd", "p3d_12_nd", "p3d_9_natural_norelax", "p3d_9_random_nopost"]
NO_SMALL_FRONTS = 16


def _child(case, *args, timeout=900):
    p = subprocess.run([sys.executable, os.path.join(HERE, "schur_cases.py"), case, *map(str, args)],
                       capture_output=True, text=True, timeout=timeout)
    print(p.stdout)
    print(p.stderr[-4000:])
    assert p.returncode == 0 and "CASE OK" in p.stdout, (case, args, p.returncode)
    res = [ln[7:] for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    return json.loads(res[-1]) if res else None


_entries = {}


def _entry(name, beta, flags):
    """one child process factorizes all of them and forms every Sc and F; every case has its own verdict"""
    if not _entries:
        _entries.update(_child("entries") or {"failed": 1})
    key = f"{name}|{beta}|{flags}"
    assert key in _entries
    return _entries[key]


@pytest.mark.parametrize("beta", [0.0, 0.375])
@pytest.mark.parametrize("name", NAMES)
def test_entry_by_entry(name, beta):
    """Sc for every m of the list against the dense Schur complement at the bar (the figure is the worst error over the
    list in units of the bar), bitwise symmetric, nothing written outside the m x m corner of an over-allocated, poisoned
    array"""
    r = _entry(name, beta, 0)
    assert r["err"] <= 1.0, (name, beta, r)
    assert r["sym"] and r["untouched"], (name, beta, r)


@pytest.mark.parametrize("name", ["p3d_12_nd", "box9r2_nd"])
def test_entry_by_entry_generic_kernels_only(name):
    """CHOLMOD_HIP_NO_SMALL_FRONTS: the factor from the generic kernels, the same checks"""
    r = _entry(name, 0.0, NO_SMALL_FRONTS)
    assert r["err"] <= 1.0 and r["sym"] and r["untouched"], (name, r)


@pytest.mark.parametrize("beta", [0.0, 0.375])
@pytest.mark.parametrize("name", NAMES)
def test_m_equal_n_is_the_matrix_itself(name, beta):
    """Sc (m = n) against the dense P (A + beta I) P': a check that needs no reference elimination"""
    r = _entry(name, beta, 0)
    assert r["mn"] is not None and r["mn"] <= 1.0, (name, beta, r)


@pytest.mark.parametrize("beta", [0.0, 0.375])
@pytest.mark.parametrize("name", NAMES)
def test_the_factor_of_sc(name, beta):
    """F for every m of the list: its lower triangle bit for bit the entries of the downloaded factor, exact +0.0 above
    the diagonal and outside the pattern of L; F F' against Sc at the bar"""
    r = _entry(name, beta, 0)
    assert r["fbits"], (name, beta, r)
    assert r["fft"] <= 1.0, (name, beta, r)


def test_nesting():
    """the dense Schur complement of Sc (m2) onto its last m1 variables against Sc (m1): forest148 with m2 = 110 (L22 is
    block-sparse), arrow300 and dense200 with m2 = 137 (a supernode with more than 64 contributing columns)"""
    _child("nesting")


def test_same_bits():
    """two calls give the same bits (Sc and F); L22' V twice gives the same bits; both products against numpy at the bar;
    after factorize_device with new values Sc is the new matrix's"""
    _child("samebits")


_condensed = {}


@pytest.mark.parametrize("nrhs", [1, 7, 8, 17])
@pytest.mark.parametrize("name,m", [("p3d_12_nd", "half"), ("p3d_12_nd", 65), ("forest148", 100), ("bcsstk01", 17)])
def test_condensed_solve(name, m, nrhs):
    """reduce -> torch.cholesky_solve with F on the interface -> expand.  G against the dense B_S - A_SI inv (A_II) B_I at
    the bar relative to max |ref|; X against solve_device at the bar, its trailing rows x_S; the residual norms of X
    (refine_device, steps=0) within the bar times max |B|.

    Which residual check: the norms of solve_device's own X on these cases are 2.2e-15 .. 1e-14 (p3d_12_nd, forest148;
    max |B| is 3 .. 4, so 3 .. 13 ulps of it) and 1.2e-13 .. 6.2e-13 (bcsstk01) -- the rounding floor, where a ratio of two
    such norms moves in steps of a quarter to a half from the order of the atomic adds in the forward sweep alone.  That
    leaves no room to fix a factor 4 against them, so the norm is held to tolerance (rcond) max |B| instead, the bar
    every other figure here is held to.  (Measured: the condensed route's norms are 0.64 .. 2.0 x solve_device's.)"""
    if not _condensed:
        _condensed.update(_child("condensed") or {"failed": 1})
    eg, ex, exs, tol, r1, r0, rbar = _condensed[f"{name}|{m}|{nrhs}"]
    assert eg <= tol and ex <= tol and exs <= tol, (name, m, nrhs, eg, ex, exs, tol)
    assert r1 <= rbar, (name, m, nrhs, r1, r0, rbar)


def test_subset_in_the_callers_order():
    """an ordering from Session.schur_perm for a scrambled subset of p3d_9: with postorder=False the rows and columns of Sc
    come back in the subset's order, against the dense reference; the same on a session with postorder=True either passes
    or raises the ValueError that names postorder=False -- never a wrong answer; a subset that is not ordered last raises"""
    out = _child("subset")
    assert out["False"] == "passed" and out["True"] in ("passed", "refused"), out
    print("postorder=True:", out["True"])


def test_larger_case_poisson24():
    """Poisson 24^3 (n = 13 824), m = the top separator's supernode and m = 2000 (sibling separators that are not in each
    other's row lists): Sc (inv (A) e_j)_S against e_j on S for 16 j in S at the bar -- Sc^-1 = ((A + beta I)^-1)_SS --, no
    dense reference of n^2"""
    out = _child("larger", 24)
    for m, (err, tol) in out.items():
        assert err <= tol, (m, err, tol)


def test_stream_contract():
    """on a side stream behind the work that produces the values; a consumer enqueued after it sees Sc; no allocation and
    no host synchronisation inside the engine's calls once the first has run"""
    _child("stream")


def test_refusals_on_a_live_device():
    """a complex factor: CHOLMOD_NOT_INSTALLED; a factorization that was not positive definite (2lo.tri): refused, L as it
    was; the engine's own argument checks; m = 0 and nrhs = 0 touch nothing; an m = 0 expansion is the plain L' solve"""
    _child("refusals")
