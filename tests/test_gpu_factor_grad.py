"""The gradient through the factor on the GPU (Session.factor_grad_device / factor_outer_grad_device / factor_grad_host,
cholmod_hip_factor_grad_*, DeviceCholesky.solve_Lt / solve_L): reverse-mode Cholesky on the pattern of L, entry by entry
against the dense formula at the project's parity bar max (1e-12, 20 eps / rcond) max |G_ref| (tests/selinv_reference.py;
the numpy restatement of the recurrence holds it three orders of magnitude inside, tests/test_factor_grad_api.py), the
selected inverse as its special case, the outer-product entry, the gather bit for bit against Gx, torch.autograd against a
dense torch reference, staleness, the stream contract and the refusals.

The bodies live in tests/factor_grad_cases.py and run in a fresh child process each, as those of tests/test_gpu_selinv.py
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
    p = subprocess.run([sys.executable, os.path.join(HERE, "factor_grad_cases.py"), case, *map(str, args)],
                       capture_output=True, text=True, timeout=timeout)
    print(p.stdout)
    print(p.stderr[-4000:])
    assert p.returncode == 0 and "CASE OK" in p.stdout, (case, args, p.returncode)
    res = [ln[7:] for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    return json.loads(res[-1]) if res else None


_entries = {}


def _entry(name, beta, flags):
    """one child process factorizes and differentiates all of them; every case has its own verdict"""
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
    """Session.factor_grad_host for a seeded standard-normal Lbar (1e30 in the dead triangles) against the dense formula on
    P (A + beta I) P' over every stored lower-trapezoid entry; the dead upper triangles of the diagonal blocks exact zeros.
    dense200: blocks 64/64/64/8 with no R at the last; arrow300: a partial 64-row slice of R and K no multiple of 64;
    forest148: 1 x 1 and thin-only fronts; _norelax / _nopost: ancestors found by search, not by order"""
    _entry(name, beta, 0)


@pytest.mark.parametrize("name", ["p3d_12_nd", "box9r2_nd"])
def test_entry_by_entry_generic_kernels_only(name):
    """CHOLMOD_HIP_NO_SMALL_FRONTS: everything through the generic kernels, the same bar"""
    _entry(name, 0.0, NO_SMALL_FRONTS)


@pytest.mark.parametrize("name", ["p3d_12_nd", "p2d_60_nd"])
def test_selected_inverse_is_the_special_case(name):
    """Lbar = diag (2 / L_jj): the gathered G equals m Z from selinv_device (m = 1 on the diagonal, 2 off it), the trace
    equals sum Z_ii, both within tol max |Z|"""
    _child("selinv_special", name)


@pytest.mark.parametrize("name", ["p3d_12_nd", "arrow300"])
def test_outer_product_entry(name):
    """Lbar = alpha tril (P Q') formed on the device, nrhs 1, 3, 16, 17, ld > n once, P and Q the same array once: the dense
    formula at the bar, two calls the same bits, nrhs = 0 all zeros"""
    _child("outer", name)


def test_gather_is_bit_identical_to_gx():
    """lower-stored, upper-stored and junk-carrying input: G is the entries of Gx bit for bit and +0.0 exactly where the
    selected inverse's gather gives NaN; the trace within (n + 2) eps sum |G_jj| of math.fsum; a wrong nvalues is refused"""
    _child("gather")


@pytest.mark.parametrize("name", ["p3d_9_random_nopost", "forest148", "arrow300"])
def test_autograd_against_dense_torch(name):
    """(W . solve_Lt (v, Z)).sum () + (W2 . solve_L (v, B)).sum () with a tensor beta (0 and 0.375), nrhs 1 and 19: the
    forward and the gradients with respect to values, right-hand sides and beta against torch.linalg.cholesky /
    solve_triangular of the dense permuted matrix at the bar; a second backward after the factor was replaced"""
    _child("autograd", name)


def test_stale_and_fresh():
    """gather and download are refused before the first call and after factorize_device and correct again after a new
    call; release followed by a new call and a 0.25 MB scratch budget (more launches) give the same bits"""
    _child("stale")


def test_stream_contract_and_launch_bound():
    """forward and backward on a side stream without a host wait; three engine-level calls of each entry point leave
    torch.cuda.mem_get_info () unchanged; the launch count within the selected inverse's bound on p2d_60_nd"""
    _child("stream")


def test_refusals_on_a_live_device():
    """a complex factor: CHOLMOD_NOT_INSTALLED; a factorization that was not positive definite (2lo.tri): CHOLMOD_INVALID, L
    as it was"""
    _child("refusals")
