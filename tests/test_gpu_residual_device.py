"""Session.residual_device / Session.refine_device (cholmod_l_hip_residual_device, cholmod_l_hip_refine_device) on the GPU:
R = B - (A + beta I) X and iterative refinement on the matrix that is resident in HBM, X, B and R in HBM, ordered on the
caller's stream.  The residual is checked entry by entry against numpy with the dot-product bound
2 (m + 3) eps (|B| + |beta| |X| + |A| |X|) (derived in tests/residual_device_cases.py: nothing measured), its norms and
its repeatability bit for bit; the refinement against Session.solve with the project's 1e-11 per column.

The bodies live in tests/residual_device_cases.py and run in a fresh child process each, as those of
tests/test_gpu_solve_device.py do: torch has to be imported before the engine library is loaded."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _child(case, *args, timeout=900):
    p = subprocess.run([sys.executable, os.path.join(HERE, "residual_device_cases.py"), case, *map(str, args)],
                       capture_output=True, text=True, timeout=timeout)
    print(p.stdout)
    print(p.stderr[-4000:])
    assert p.returncode == 0 and "CASE OK" in p.stdout, (case, args, p.returncode)
    res = [ln[7:] for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    return json.loads(res[-1]) if res else None


@pytest.mark.parametrize("beta", [0.0, 0.375])
@pytest.mark.parametrize("name", ["box9r2_nd", "p2d_60_nd", "p3d_12_nd"])
def test_residual_componentwise(name, beta):
    """nrhs in {1, 2, 7, 8, 15, 16, 17, 40}, random X and B: every entry within the bound, the norms equal to
    abs(R).max(axis=1) bit for bit; with beta = 0 and with a beta passed to the factorization"""
    _child("residual", name, beta)


def test_two_calls_give_the_same_bits():
    _child("reproducible")


@pytest.mark.parametrize("nrhs", [3, 20])
def test_residual_follows_a_values_only_upload(nrhs):
    _child("values", nrhs)


def test_layout_contract():
    """ld = n + 7 with sentinel padding in X, B and R; R is B; nrhs == 0; R == X refused"""
    _child("layout")


def test_stream_contract_and_workspace_growth():
    _child("stream")


@pytest.mark.parametrize("name", ["box9r2_nd", "p2d_60_nd", "p3d_12_nd"])
def test_refinement(name):
    """nrhs in {3, 16, 20} from a solution perturbed by 1e-3: one step lands within 1e-11 of Session.solve and of the host
    restatement; steps = 0 leaves X alone and reports the norms; two more steps keep the norm within twice the bound"""
    _child("refine", name)


# the list of tests/solve_device_cases.py (kept literal here so that collection needs no torch)
REFERENCE_INPUTS = [
    ("tcov", "1_0"), ("tcov", "1e99"), ("tcov", "2.tri"), ("tcov", "20lo"), ("tcov", "2_3"), ("tcov", "2diag.tri"),
    ("tcov", "3_2"), ("tcov", "3b"), ("tcov", "4"), ("tcov", "4lo"), ("tcov", "5"), ("tcov", "5by50"), ("tcov", "C9840"),
    ("tcov", "a2"), ("tcov", "afiro"), ("tcov", "diag"), ("tcov", "ex5lo"), ("tcov", "galenet"), ("tcov", "ibm32"),
    ("tcov", "itest2"), ("tcov", "itest6"), ("tcov", "k01up"), ("tcov", "pi"), ("tcov", "plskz362.mtx"), ("tcov", "r5lo"),
    ("tcov", "r5lo2"), ("tcov", "r5up"), ("tcov", "r5up2"), ("tcov", "rza.mtx"), ("demo", "bcsstk01.tri"),
    ("demo", "bcsstk02.tri"), ("demo", "can___24.mtx"), ("demo", "lp_afiro.tri"), ("demo", "one.tri"),
    ("demo", "pts5ldd03.mtx"), ("demo", "two.tri"),
]
_ref_results = {}


@pytest.mark.parametrize("d,f", REFERENCE_INPUTS)
def test_reference_inputs(d, f):
    """nrhs = 5 on every real file the solve test runs, each with its beta: the componentwise bound and the norms.  One
    child process runs all of them; every file has its own verdict."""
    if not _ref_results:
        _ref_results.update(_child("reference_inputs") or {"failed": 1})
    assert f"{d}/{f}" in _ref_results
    worst, norms_equal = _ref_results[f"{d}/{f}"]
    assert worst <= 1.0, worst
    assert norms_equal


def test_residual_costs_less_than_half_a_solve_poisson100():
    """Poisson 100^3, 16 right-hand sides, torch events, median of five after a warm-up: residual_device takes less
    than half of solve_device in the same process (the traffic argument gives well over 10 : 1)."""
    r = _child("poisson100")
    assert r["residual_device_ms"] > 0 and r["solve_device_ms"] > 0
    assert r["residual_device_ms"] < 0.5 * r["solve_device_ms"], r
