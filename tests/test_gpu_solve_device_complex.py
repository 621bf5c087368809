"""Session.solve_device / residual_device / refine_device with a complex factor on the GPU
(cholmod_l_hip_solve_device_complex and its two companions): interleaved complex right-hand sides and solutions in HBM,
solved on the twin's plan -- in complex storage through the CX forms of the column and panel kernels, with
CHOLMOD_HIP_CX_TWIN=1 on the full twin through the real ones.  Bars: P / Pt / D bit-equal to the host-array path
(Session.solve, unchanged), every other system within 1e-11 relative per column of it, L and L^H within 1e-11 of a dense
triangular solve, A by its residual against the full Hermitian matrix at 1e-11 and within 1e-10 of the oracle.

The bodies live in tests/solve_device_complex_cases.py and run in a fresh child process each: torch has to be imported
before the engine library is loaded for the two to share one HIP runtime."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _child(case, *args, timeout=600):
    p = subprocess.run([sys.executable, os.path.join(HERE, "solve_device_complex_cases.py"), case, *map(str, args)],
                       capture_output=True, text=True, timeout=timeout)
    print(p.stdout)
    print(p.stderr[-4000:])
    assert p.returncode == 0 and "CASE OK" in p.stdout, (case, args, p.returncode)
    res = [ln[7:] for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    return json.loads(res[-1]) if res else None


@pytest.mark.parametrize("storage", ["cx", "twin"])
@pytest.mark.parametrize("name", ["p3d_9_nd", "box7r2_nd", "bcsstk01"])
def test_parity_all_systems(name, storage):
    """nrhs in {1, 2, 7, 8, 15, 16, 17, 40} (7 | 8: columns / panels, 16 | 17: the panel edge), all nine systems, in
    complex storage and on the full twin; bcsstk01 has odd supernode widths (twin widths that are no multiple of 16)."""
    _child("parity", name, storage)


@pytest.mark.parametrize("nrhs", [3, 20])
def test_big_supernode_walk_and_rebuilt_inverses(nrhs):
    """a complex supernode of 700 columns with 50 rows below it and a dense root of 100, complex storage: the walk in
    256-column blocks (the last one 120 = 64 + 56 twin columns) with the explicit inverses, which follow a second
    factorization"""
    _child("big_supernode", nrhs)


@pytest.mark.parametrize("storage", ["cx", "twin"])
def test_layout_contract(storage):
    """ld = n + 3 with sentinel padding that survives bit for bit, in place, a single vector (n,), nrhs == 0, and a
    TypeError for a dtype that does not match the factor"""
    _child("layout", storage)


@pytest.mark.parametrize("storage", ["cx", "twin"])
@pytest.mark.parametrize("nrhs", [3, 16])
def test_residual_and_refinement(nrhs, storage):
    """R within 1e-11 (relative to |B|) of B - A X formed with scipy, the same bits from two calls, norms = the largest
    |re| or |im| of the returned R exactly; one refinement step from an X perturbed by 1e-6 brings the relative
    residual below 1e-11; steps = 0 leaves X bit-identical"""
    _child("residual_refine", storage, nrhs)


def test_l_is_read_once_hermitian64():
    """Hermitian 64^3, 16 right-hand sides, complex storage, device time from stats [24] (median of five after a
    warm-up): the device path takes less time than the host-array complex solve on the same factor, which reads L
    sixteen times.  No margin beyond that."""
    r = _child("hermitian64")
    print(f"host-array path {r['host_ms']:.2f} ms, device path {r['device_ms']:.2f} ms, ratio {r['host_ms'] / r['device_ms']:.2f}")
    assert r["host_ms"] > 0 and r["device_ms"] > 0
    assert r["device_ms"] < r["host_ms"], r
