"""What NaN and Inf values do to the factor, the solves and the residual on the GPU (run with -m gpu on an MI355X): the table
of tests/nonfinite_cases.py through the first factorization of a plan, the values-only refactorization and
Session.factorize_device, each followed by the clean values.

Two things finite data cannot show.  The PROTOCOL: every pivot kernel says "NaN does not trip", as dpotrf -- `!(d > 0.0)`
for `d <= 0.0`, an fmax or a select that drops a NaN would pass every other test.  CONTAINMENT: the kernels predicate by
select-to-zero and by full MFMA tiles over triangles whose other half is zero, and 0 * NaN is NaN, so a poisoned value
shows every lane and tile that reads what it has no business reading -- fronts that share a launch or a wave
(k_leaf_pair), siblings under the extend-add, the right-hand sides of a 16-wide solve panel, and the caches a
refactorization must refresh.  The bar (tests/nonfinite_cases.py): must <= non-finite entries <= may, every supernode
outside may BIT-IDENTICAL to the plan's clean factor, status, minor and the finite entries the oracle's; after the clean
values every factor and solve is the clean bits again.

One thing the device does NOT repeat bit for bit, poisoned or not: the forward solves add the contributions of sibling
supernodes into their ancestor rows with floating-point atomics, so two clean calls differ in those rows (20 repeats of a
16-wide SYS_L panel on the 437-column arrow: up to 23 words, all root rows).  The solve checks compare bits in the rows
that are reproducible (nonfinite_cases.reproducible_rows: every row under SYS_Lt, the rows below any sum over siblings
otherwise) and hold the others to twice the solve bar against the clean call; the NaN row sets are exact everywhere.

The bodies live in tests/nonfinite_device_cases.py and run in a fresh child process each, under a timeout of their own,
as those of tests/test_gpu_not_posdef.py do.  The runner there starts its own script only, so this module has the same
dozen lines once more -- but ONE stop list with it: a child of either module that faults, aborts or runs into its
timeout ends the GPU work of both."""
import json
import os
import subprocess
import sys

import pytest

import nonfinite_cases as NF
import test_gpu_not_posdef as T

pytestmark = pytest.mark.gpu

SCRIPT = os.path.join(T.HERE, "nonfinite_device_cases.py")


def _child(body, *args, timeout=120):
    if T._stopped:
        pytest.fail(f"not started: {T._stopped[0]}")
    cmd = [sys.executable, SCRIPT, body, *map(str, args)]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        T._stopped.append(f"{body} {args} ran into its timeout of {timeout} s")
        raise
    print(p.stdout[-20000:])
    print(p.stderr[-4000:])
    if p.returncode < 0 or p.returncode in (124, 134, 137, 139) or "illegal memory access" in p.stderr:
        T._stopped.append(f"{body} {args} ended with status {p.returncode}")
    assert p.returncode == 0 and "CASE OK" in p.stdout, (body, args, p.returncode)
    return [json.loads(ln[7:]) for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]


def _group(group, flags, storage="-", timeout=120):
    r = _child("group", group, flags, storage, timeout=timeout)
    w = r["worst"]
    print(f"{group} flags {flags}: {r['cases']} cases; worst {w['name']}: must {w['must']} <= device {w['nonfinite']} <= may {w['may']}")
    assert w["must"] <= w["nonfinite"] <= w["may"]
    return r


@pytest.mark.parametrize("flags", NF.DEEP_FLAGS)
def test_nan_on_the_diagonal_of_a_leaf(flags):
    """"deep": leaf (129, 136) at its columns 0, 64 and 128, leaf (65, 71) at 64; status OK, minor n.  The kernel that meets
    the NaN pivot: the fused 64-column chain, potrf / trsm launches of their own, k_chainf, the generic kernels for the
    (65, 71) leaf as well, the four-wave thin front"""
    assert _group("leafdiag", flags)["cases"] == 4


def test_nan_pivot_in_the_two_kernel_chain():
    """leaf (129, 136)@64 under flags 8192 with CHOLMOD_HIP_NO_CHAINF in the child's environment: k_diag factors the diagonal
    sub-block and leaves its inverses, k_rowsolve solves the rows below; the plan's launches are checked to be those"""
    assert _group("twokernel", 8192)["cases"] == 1


@pytest.mark.parametrize("flags", [0, 8192])
def test_nan_off_the_diagonal(flags):
    """one below-row entry (a root row) of column 64 of leaf (129, 136), one entry inside its triangle"""
    assert _group("offdiag", flags)["cases"] == 2


@pytest.mark.parametrize("flags", NF.THIN_FLAGS)
def test_nan_in_one_front_of_a_shared_launch(flags):
    """"thin": four leaves in one 136-row four-wave launch.  "pair": each member of a wave pair of k_leaf_pair in turn (the
    values-only and factorize_device paths under flags 0); the partner front in the same wave is bit-identical"""
    assert _group("sharedlaunch", flags)["cases"] == 6


def test_nan_together_with_a_failing_pivot():
    """the plant trips unless the NaN has reached its pivot; -inf trips; both values of quick_return_if_not_posdef"""
    assert _group("mixed", 0)["cases"] == 10


def test_nan_in_a_leaf_of_the_poisson_tree():
    """n = 576, relaxed supernodes: 5 of 49 supernodes on the path, the other 44 the clean bits"""
    assert _group("levels", 0)["cases"] == 1


@pytest.mark.parametrize("storage", ["cx", "twin"])
def test_nan_in_a_complex_hermitian_arrow(storage):
    """the imaginary part of an off-diagonal entry, a real diagonal entry; complex storage and the full twin"""
    assert _group("complex", 0, storage)["cases"] == 2


@pytest.mark.parametrize("flags", [0, 16])
def test_inf_on_a_diagonal_stays_on_its_path(flags):
    """+Inf on the diagonal of (65, 71)@7: status OK, minor n, the non-finite entries inside may, everything outside may
    bit-identical.  The values inside may are not compared: the oracle gives L (j, j) = +inf and zeros below it, the
    device's sqrt_rsqrt NaN"""
    assert _group("inf", flags)["cases"] == 1


def test_resident_checks_solves_and_residual():
    """on the NaN factor: rcond 0, the diagonal and entry counts between must and may, a NaN log-determinant; solves with
    1, 3, 16 and 17 right-hand sides, host arrays and device tensors: the tree of the NaN all NaN, the other tree the clean
    bits; after the recovery the clean bits everywhere.  On the clean factor: a NaN in one row of one right-hand side
    under SYS_A, SYS_L and SYS_Lt, a NaN in one row of one column of X in the residual and its norm"""
    r = _child("resident", timeout=120)
    for k, (lo, got, hi) in r["worst"].items():
        assert lo <= got <= hi, (k, lo, got, hi)
