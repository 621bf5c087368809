"""The selected inverse on the GPU (Session.selinv_host / Session.selinv_device, cholmod_hip_selinv_*): Z = (A + beta I)^-1
on the pattern of L, entry by entry against the dense inverse at the project's parity bar
max (1e-12, 20 eps / rcond) max |Z_ref| (tests/selinv_reference.py; the numpy restatement of the recurrence holds it 18 x
or more inside, tests/test_selinv_api.py), the gather bit for bit against Zx, staleness, the size-independent identities
at Poisson 40^3, the launch bound and the stream contract.

The bodies live in tests/selinv_cases.py and run in a fresh child process each, as those of tests/test_gpu_residual_device.py
do: torch has to be imported before the engine library is loaded."""
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
    p = subprocess.run([sys.executable, os.path.join(HERE, "selinv_cases.py"), case, *map(str, args)],
                       capture_output=True, text=True, timeout=timeout)
    print(p.stdout)
    print(p.stderr[-4000:])
    assert p.returncode == 0 and "CASE OK" in p.stdout, (case, args, p.returncode)
    res = [ln[7:] for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    return json.loads(res[-1]) if res else None


_entries = {}


def _entry(name, beta, flags):
    """one child process factorizes and inverts all of them; every case has its own verdict"""
    if not _entries:
        _entries.update(_child("entries") or {"failed": 1})
    key = f"{name}|{beta}|{flags}"
    assert key in _entries
    err, tol, dead = _entries[key]
    assert err <= tol, (key, err, tol)
    assert dead == 0, (key, dead)


@pytest.mark.parametrize("beta", [0.0, 0.375])
@pytest.mark.parametrize("name", NAMES)
def test_entry_by_entry(name, beta):
    """Session.selinv_host against the dense inverse of P (A + beta I) P' over every stored lower-trapezoid entry; the dead
    upper triangles of the diagonal blocks exact zeros"""
    _entry(name, beta, 0)


@pytest.mark.parametrize("name", ["p3d_12_nd", "box9r2_nd"])
def test_entry_by_entry_generic_kernels_only(name):
    """CHOLMOD_HIP_NO_SMALL_FRONTS: the factor from the generic kernels, the same bar"""
    _entry(name, 0.0, NO_SMALL_FRONTS)


def test_gather_is_bit_identical_to_zx():
    """selinv_device on lower-stored, upper-stored and junk-carrying input: values and diagonal are entries of Zx bit for
    bit, NaN exactly where A is not read, the dense inverse at the bar; the diagonal in both orderings at the engine level"""
    _child("gather")


def test_stale_and_fresh():
    """two calls and a call after release give the same bits; after factorize_device the inverse is the new matrix's;
    info [6] goes 1 -> 0 -> 1; gather and download without a current Zx are refused; a 0.25 MB scratch budget changes the
    launches, not the bits"""
    _child("stale")


def test_size_independent_identities_poisson40():
    """n = 64 000: |trace (A Z) - n| / n <= 1e-11 from the values on A's pattern, the diagonal sum against the closed form
    within 1e-12, 16 columns of Z against Session.solve (e_j) at the bar, the launch bound"""
    _child("poisson40")


@pytest.mark.parametrize("name", ["p2d_60_nd", "p2d_300_nd"])
def test_launch_bound(name):
    """info [1] <= 8 sum over the batches of (max ceil (nscol / 64)) + 8 batches + 16, the batches from
    cholmod_hip_get_batches; the diagonal sum against the closed form"""
    _child("launches", name)


def test_stream_contract():
    _child("stream")


def test_refusals_on_a_live_device():
    """a complex factor: CHOLMOD_NOT_INSTALLED; a factorization that was not positive definite (2lo.tri): refused, L as it
    was"""
    _child("refusals")
