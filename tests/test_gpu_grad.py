"""Gradients through the device path on the GPU (Session.values_grad_device / Session.logdet_device,
suitesparse_amd.autograd.DeviceCholesky): the sampled product exact, entry by entry, on integer inputs and within its
rounding bar on badly scaled ones, +0.0 exactly where the factorization does not read A, the whole backward pass against
dense torch autograd on the CPU at the project's parity bar, the log-determinant against the downloaded diagonal and the
closed form, the stream contract and the refusals.  Formulas and references: tests/grad_reference.py.

The bodies live in tests/grad_cases.py and run in a fresh child process each, as those of tests/test_gpu_selinv.py do:
torch has to be imported before the engine library is loaded."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _child(case, *args, timeout=600):
    p = subprocess.run([sys.executable, os.path.join(HERE, "grad_cases.py"), case, *map(str, args)],
                       capture_output=True, text=True, timeout=timeout)
    print(p.stdout)
    print(p.stderr[-4000:])
    assert p.returncode == 0 and "CASE OK" in p.stdout, (case, args, p.returncode)


@pytest.mark.parametrize("name", ["arrow300", "forest148", "p3d_9_random_nopost", "p3d_12_nd", "bcsstk01"])
def test_exact_entry_by_entry(name):
    """small integers (|.| <= 8), alpha = -1: G equals the numpy reference exactly, nrhs 1, 3, 7, 8, 16, 19, 33, through the
    host layer and the engine with perm 1 and 0, once with ld > n, once with U and V the same array; dG pre-filled with NaN"""
    _child("exact", name)


def test_rounded_inputs_and_same_bits():
    """rows scaled by 2^+-20: per entry within 2 (2 nrhs + 2) eps |alpha| sum_r (|U_i V_j| + |U_j V_i|); two calls, the same
    bits"""
    _child("rounded")


def test_what_is_not_read_gets_plus_zero():
    """upper-stored input and junk in the ignored triangle: +0.0 exactly where selinv_device gives NaN"""
    _child("unread")


@pytest.mark.parametrize("name", ["p3d_12_nd", "arrow300", "forest148", "bcsstk02", "dense200"])
def test_autograd_against_dense_torch_on_the_cpu(name):
    """loss = (W . solve (v, B)).sum () + 0.3 logdet (v), beta 0 and 0.375, nrhs 1 and 19: gradients and forward values at
    the bars, one factorization for logdet + solve, the stale-factor guard"""
    _child("autograd", name)


def test_not_positive_definite_raises_in_the_forward():
    _child("not_posdef")


def test_logdet():
    """2 fsum (log d) of the downloaded diagonal within (n + 2) eps sum |2 log L_jj|, Poisson 24^3 against the closed form
    at 1e-11, the same bits across two calls and across a refactorization, refused after 2lo.tri with L left as it was"""
    _child("logdet")


def test_stream_contract():
    _child("stream")


def test_refusals_on_a_live_device():
    """a complex factor: CHOLMOD_NOT_INSTALLED; a wrong nvalues, ld < n, nrhs < 0, a product map set: CHOLMOD_HIP_INVALID,
    dG untouched; a matrix of another pattern: refused by the host layer"""
    _child("refusals")
