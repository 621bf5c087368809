"""Session.factorize_device (cholmod_l_hip_factorize_values_device) on the GPU: a values-only factorization whose values
already live in device memory, ordered on the caller's stream.  Symmetric A: the resident S equals the permuted values
exactly and L is bit-identical to what cholmod_l_factorize gives for the same values in a second session; A*A' (stype 0):
the values of tril (A*A') are formed on the device, each within the dot-product bound (len + 2) 2^-53 sum |a_p| |a_q| of the
exact sum, and L is within 1e-12 of the host's.

The bodies live in tests/factorize_device_cases.py and run in a fresh child process each, as those of
tests/test_gpu_solve_device.py do: torch has to be imported before the engine library is loaded."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _child(case, *args, timeout=300):
    p = subprocess.run([sys.executable, os.path.join(HERE, "factorize_device_cases.py"), case, *map(str, args)],
                       capture_output=True, text=True, timeout=timeout)
    print(p.stdout)
    print(p.stderr[-4000:])
    assert p.returncode == 0 and "CASE OK" in p.stdout, (case, args, p.returncode)


@pytest.mark.parametrize("stype", [-1, 1])
def test_symmetric_bit_identical_to_the_host_path(stype):
    """poisson3d (12), geometric_nd: host factorization, then new values (diagonal shifted, off-diagonals scaled) made on
    the device; S and L bit for bit, two calls on one tensor included; the host values-only path afterwards"""
    _child("symmetric", stype)


@pytest.mark.parametrize("kind", ["natural", "both"])
def test_identity_map_and_ignored_entries(kind):
    """natural ordering with packed lower A (S is A, the identity map); both triangles stored under stype -1 (more values
    than S has entries, the ignored ones NaN on the device)"""
    _child("shape", kind)


def test_beta_and_the_residual_of_the_new_matrix():
    _child("beta")


@pytest.mark.parametrize("which", ["afiro", "engineered"])
def test_aat_product_on_the_device(which):
    """lp_afiro (beta = 1e-3 max |C|) and the engineered 70-row matrix (lists of 1 .. 131 products): every value of S
    against the exact sum, L against the host, solve + refine + residual on the device against numpy"""
    _child("aat", which)


def test_not_positive_definite_then_good_values():
    _child("not_posdef")


def test_stream_order():
    _child("stream")


def test_another_pattern_is_refused_and_nothing_is_touched():
    _child("pattern")


def test_n_equal_one():
    _child("n1")
