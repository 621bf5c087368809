"""The not-positive-definite protocol with SEVERAL failing pivots on the GPU (run with -m gpu on an MI355X): the table of
tests/not_posdef_cases.py -- two leaves of a block arrow at once, a leaf and the root, a pivot deep in a 129- or 65-column
front that has rows below it while a later leaf fails too, the root alone, thin fronts (four waves per front), an arrow
of small leaves (one wave per front, and two fronts to a wave in k_leaf_pair), a small column high in one subtree of a
Poisson tree against a larger one in a leaf of another, a complex Hermitian arrow in both storages -- through the first factorization of a plan, the values-only refactorization and Session.factorize_device.

What a single failing pivot cannot show: which of several reporting supernodes k_first_fail picks (the smallest, not the
largest and not the last writer), that the valid columns of a big failing front are solved through ALL their rows while
its later columns and every later supernode are zero, that the zeroed tail does not reach into earlier supernodes of
other subtrees, and that nothing of a factorization that failed in several places survives into the next one.  minor,
the zero pattern and the values by entry (TOL_L = 1e-12, the worst supernode) against the oracle and against a dense
numpy restatement of the protocol; tests/test_not_posdef_cases.py holds the two references within a tenth of that bar.

The bodies live in tests/not_posdef_device_cases.py and run in a fresh child process each (torch has to be imported
before the engine library is loaded), under a timeout of their own; a child runs its cases under both values of
quick_return_if_not_posdef.  A child that faults, aborts or runs into its timeout ends the GPU work of this module: the
tests after it fail without starting anything.

Measured on one MI355X: 138 cases, the worst by-entry figure 5.6e-16 (the complex arrow), every failed factor the same
bits on the three value paths."""
import json
import os
import subprocess
import sys

import pytest

import not_posdef_cases as NP

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_stopped = []


def _child(body, *args, timeout=120):
    if _stopped:
        pytest.fail(f"not started: {_stopped[0]}")
    cmd = [sys.executable, os.path.join(HERE, "not_posdef_device_cases.py"), body, *map(str, args)]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        _stopped.append(f"{body} {args} ran into its timeout of {timeout} s")
        raise
    print(p.stdout[-20000:])
    print(p.stderr[-4000:])
    if p.returncode < 0 or p.returncode in (124, 134, 137, 139) or "illegal memory access" in p.stderr:
        _stopped.append(f"{body} {args} ended with status {p.returncode}")
    assert p.returncode == 0 and "CASE OK" in p.stdout, (body, args, p.returncode)
    r = [json.loads(ln[7:]) for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    print(f"{body} {args}: {r['cases']} cases, worst by-entry figure {r['worst']:.3e}")
    return r


def test_two_leaves_and_the_root_fail_at_once():
    """block arrow (17, 72) (64, 72) (65, 71) (129, 136) (16, 0) (1, 1): the middle column of an early leaf and column 0 of a
    later one (info == 1 there), the two swapped, an early leaf that is a tree of its own, a third plant in the root"""
    assert _child("group", "two", 0)["cases"] == 8


@pytest.mark.parametrize("flags", NP.DEEP_FLAGS)
def test_failure_deep_in_a_generic_front_with_rows_below(flags):
    """leaf (129, 136) at its columns 63, 64, 65 and 128, leaf (65, 71) at 64 and 1, a later leaf failing as well: the
    columns before the failing one hold the solved values in all 136 / 71 rows below, the later columns and every later
    supernode are zero; fused chain, potrf / trsm launches of their own, the 256-column chain, no thin-front kernel,
    128-wide tiles with 2048-column outer blocks"""
    assert _child("group", "deep", flags)["cases"] == 12


def test_failure_in_the_root_leaves_every_leaf_intact():
    """root columns 0, 63, 64 and 139: every leaf by entry"""
    assert _child("group", "root", 0)["cases"] == 8


@pytest.mark.parametrize("flags", NP.THIN_FLAGS)
def test_two_thin_fronts_fail_at_once(flags):
    """leaves (1, 1) (15, 63) (16, 64) (64, 72): the first, a middle and the last column of two of them at once.  The four
    share one launch whose widest member has 136 rows: the four-wave k_thin_front on every value path, and
    CHOLMOD_HIP_NO_LEAF_PAIRS changes nothing for them (tests/test_not_posdef_cases.py pins that launch)"""
    assert _child("group", "thin", flags)["cases"] == 12


@pytest.mark.parametrize("flags", NP.THIN_FLAGS)
def test_two_leaf_pair_fronts_fail_at_once(flags):
    """leaves (1, 1) (4, 8) (12, 20) (16, 16), all of at most 32 rows and 16 columns: one thin launch that the values-only
    refactorization and factorize_device run as k_leaf_pair, two fronts to a wave, and the first factorization -- with
    CHOLMOD_HIP_NO_LEAF_PAIRS every path -- as the one-wave k_thin_front.  The first, a middle and the last column of two
    leaves at once, the two in different waves and in the same wave; the pair kernel holds the winning failure"""
    assert _child("group", "pair", flags)["cases"] == 16


def test_small_column_high_in_the_tree_beats_a_larger_one_in_a_leaf():
    """poisson2d (24): supernode a at level >= 2 and a leaf b of another subtree with larger columns; b reports in the
    first batch, long before a: minor is in a (sparent and the levels from cholmod_hip_get_maps, as the table's)"""
    assert _child("group", "levels", 0)["cases"] == 2


@pytest.mark.parametrize("storage", ["cx", "twin"])
def test_complex_hermitian_arrow(storage):
    """two plants in a Hermitian block arrow, in complex storage and as the full twin (CHOLMOD_HIP_CX_TWIN=1): minor in
    complex columns, the reference OracleFactor.factorize_complex"""
    assert _child("group", "complex", 0, storage)["cases"] == 2


def test_device_resident_calls_after_the_recovery():
    _child("resident")


@pytest.mark.parametrize("flags", [0, 512 | 1024, 8192])
def test_dense_front_rows_below_the_valid_columns(flags):
    """cholmod_hip_dense_partial_factor on the (200, 100) front with a decoupled bad column at 15, 64 and 99: rows
    100 .. 199 of the columns BEFORE it (not_posdef_device_cases.body_dense says what the probe promises there)"""
    assert _child("dense", flags, timeout=60)["cases"] == 3
