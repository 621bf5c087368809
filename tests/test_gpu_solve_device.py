"""Session.solve_device / cholmod_l_hip_solve_device on the GPU: right-hand sides and solutions in HBM, ordered on the
caller's stream; two or more right-hand sides travel in panels of 16 through the MFMA block kernels.  Every case is an
ordinary solve.  The bound against the oracle and against the host-array path (Session.solve, unchanged) is the
project's 1e-11 relative, per column (1e-10 against the oracle at 64^3, the bar of tests/test_gpu_scale.py).

The bodies live in tests/solve_device_cases.py and run in a fresh child process each: torch has to be imported before
the engine library is loaded for the two to share one HIP runtime, and the pytest process has long loaded the engine."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-11


def _child(case, *args, timeout=900):
    p = subprocess.run([sys.executable, os.path.join(HERE, "solve_device_cases.py"), case, *map(str, args)],
                       capture_output=True, text=True, timeout=timeout)
    print(p.stdout)
    print(p.stderr[-4000:])
    assert p.returncode == 0 and "CASE OK" in p.stdout, (case, args, p.returncode)
    res = [ln[7:] for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    return json.loads(res[-1]) if res else None


@pytest.mark.parametrize("name", ["box9r2_nd", "p2d_60_nd", "p3d_12_nd"])
def test_parity_all_systems(name):
    """nrhs in {1, 2, 3, 15, 16, 17, 40}, all nine systems: L / L' against the oracle, A by its residual, P / Pt / D
    bit-equal to the host path, every column within 1e-11 of the host path."""
    _child("parity", name)


@pytest.mark.parametrize("nrhs", [3, 20])
def test_big_supernode_walk_and_rebuilt_inverses(nrhs):
    _child("big_supernode", nrhs)


def test_layout_contract():
    """ld = n + 7 with sentinel padding, in place, nrhs == 0"""
    _child("layout")


def test_stream_contract_and_workspace_growth():
    _child("stream")


# the real-valued files of tests/test_tcov_matrices.py whose factorization returns CHOLMOD_OK (fixed on the CPU path)
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
    """nrhs = 5, sys = A, set up as run_case of tests/test_tcov_matrices.py does: within 1e-11 of the host path per
    column.  One child process solves all of them; every file has its own verdict."""
    if not _ref_results:
        _ref_results.update(_child("reference_inputs") or {"failed": 1})
    assert f"{d}/{f}" in _ref_results
    assert _ref_results[f"{d}/{f}"] < TOL, _ref_results[f"{d}/{f}"]


def test_baseline_size_poisson64():
    """Poisson 64^3, 16 right-hand sides: every column within 1e-10 of the oracle, columns 0 and 15 within 1e-11 of
    the host path"""
    _child("poisson64")


def test_l_is_read_once_poisson100():
    """Poisson 100^3, 16 right-hand sides, device time from stats [24] (median of five after a warm-up): the device
    path takes less than half of the host-array path on the same factor (the traffic argument gives 16 : 1)."""
    r = _child("poisson100")
    assert r["host_ms"] > 0 and r["device_ms"] > 0
    assert r["device_ms"] < 0.5 * r["host_ms"], r
