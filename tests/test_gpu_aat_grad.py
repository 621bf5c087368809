"""Gradients through A*A' + beta*I and with respect to beta on the GPU (Session.aat_values_grad_device /
Session.aat_logdet_grad_device, the engine's cholmod_hip_product_*_grad_device, DeviceCholesky with an unsymmetric A or a
tensor beta): the chain rule through the product map exact, value by value, on integer inputs, bit for bit against the
kernel's documented summation order on the device's own selected inverse, within its rounding bar on badly scaled inputs,
the whole backward pass against dense torch autograd on the CPU at bars derived from the chain rule, the stream contract
and the refusals.  Formulas and references: tests/aat_grad_reference.py; matrices: tests/aat_grad_matrices.py.

The bodies live in tests/aat_grad_cases.py and run in a fresh child process each, as those of tests/test_gpu_grad.py do:
torch has to be imported before the engine library is loaded."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
THREE = ["afiro", "engineered", "classes160"]


def _child(case, *args, timeout=600):
    p = subprocess.run([sys.executable, os.path.join(HERE, "aat_grad_cases.py"), case, *map(str, args)],
                       capture_output=True, text=True, timeout=timeout)
    print(p.stdout)
    print(p.stderr[-4000:])
    assert p.returncode == 0 and "CASE OK" in p.stdout, (case, args, p.returncode)


@pytest.mark.parametrize("name", THREE)
def test_exact_value_by_value(name):
    """small integers, alpha = -1: dGa equals the numpy reference exactly, nrhs 1, 7, 8, 16, 19, 33, through the host layer
    and the engine with perm 1 and 0, once with ld > n, once with U and V the same array; dGa pre-filled with NaN; the first
    call builds the product map and its transpose; nrhs = 0 zero-fills"""
    _child("exact", name)


@pytest.mark.parametrize("name", THREE)
def test_logdet_gradient_isolates_the_chain_step(name):
    """integer values, Gv from the device's own Zx: bit for bit the sums in the kernel's order, and within
    (len_q + 2) 2^-53 sum |Gv_c| |a_partner| of numpy; the engine's entry with other integers as dA"""
    _child("logdet_grad", name)


@pytest.mark.parametrize("name", THREE)
def test_rounded_inputs_and_same_bits(name):
    """rows scaled by 2^+-20, a in [0.5, 2): the chain step's bar plus the sampled product's carried through the chain; two
    calls, and a call after the product map was dropped and set again, give the same bits"""
    _child("rounded", name)


@pytest.mark.parametrize("name", THREE + ["one_by_one"])
def test_autograd_against_dense_torch_on_the_cpu(name):
    """loss = (W . solve (v, B)).sum () + 0.3 logdet (v) with a tensor beta that requires grad: the gradients with respect
    to values, B and beta and the forward values at the bars, one factorization for logdet + solve, the stale-factor guard,
    a Python-float beta bit for bit"""
    _child("autograd", name)


def test_symmetric_matrix_with_a_tensor_beta():
    _child("symmetric_beta")


def test_stream_contract():
    _child("stream")


def test_refusals_on_a_live_device():
    """no product map, a wrong navalues, ld < n, nrhs < 0, a stale Zx, a factor that is not positive definite:
    CHOLMOD_HIP_INVALID; a complex factor: CHOLMOD_NOT_INSTALLED; dGa untouched; the old entry points still refuse a plan
    with a product map"""
    _child("refusals")
