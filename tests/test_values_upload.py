"""The values-only path of cholmod_l_factorize (host/numeric.c: factorize_values_only, values.hip: cholmod_hip_values_begin /
_push_chunk) under every team shape of its roles table, in batch order and in S order, and the state of L when the long way
after a hash mismatch fails.  The sequence of calls is test_factorize_again_with_new_values_and_with_a_new_pattern's; run
as a script this module is the child process of the tests below:
    python tests/test_values_upload.py <CHOLMOD_API_THREADS values, comma-separated>"""
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import pytest  # noqa: E402

from oracle.oracle import OracleFactor  # noqa: E402
from suitesparse_amd import cholmod as ch  # noqa: E402
from suitesparse_amd import generators as G  # noqa: E402
from test_gpu_edge_and_demo import test_factorize_again_with_new_values_and_with_a_new_pattern as sequence  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("threads", ["1", "2", "3", None])
def test_sequence_in_process(monkeypatch, threads):
    """CHOLMOD_API_THREADS is read on every call: teams of 1, 2 and 3 threads and the default one"""
    if threads is None:
        monkeypatch.delenv("CHOLMOD_API_THREADS", raising=False)
    else:
        monkeypatch.setenv("CHOLMOD_API_THREADS", threads)
    for stype in (-1, 1):
        sequence(stype)


def _child(threads, order, **env):
    """the sequence in a child process (what it reads once per process comes from env); CHOLMOD_API_TIMING names the order
    of every values-only call that got through"""
    env = dict(os.environ, CHOLMOD_API_TIMING="1", **env)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), threads], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "sequence ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "(values only, in %s order)" % order in r.stderr
    assert "(values only, in %s order)" % ("batch" if order == "S" else "S") not in r.stderr


def test_sequence_in_s_order():
    """no batch order: every chunk of A->x as it is, gathered into S by the push of the last one"""
    _child("1,2,4", "S", CHOLMOD_HIP_VALUES_IN_BATCH_ORDER="0")


@pytest.mark.parametrize("order", ["batch", "S"])
def test_team_smaller_than_asked_for(order):
    """four threads asked for, one given: that thread stages, pushes, factorizes and hashes in turn"""
    _child("4", order, OMP_THREAD_LIMIT="1", CHOLMOD_HIP_VALUES_IN_BATCH_ORDER="1" if order == "batch" else "0")


def _two_patterns():
    """poisson3d(14), lower, strictly diagonally dominant: A2 = one off-diagonal entry removed, A3 = A2 with one row index
    moved (the same count, inside L's pattern), as the sequence builds them"""
    n, Ap, Ai, Ax = G.poisson3d(14)
    cols = np.repeat(np.arange(n), np.diff(Ap))
    diag = Ai == cols
    vals = Ax.copy()
    vals[diag] += 2.0
    keep = np.ones(len(Ai), dtype=bool)
    keep[np.where(~diag)[0][(len(Ai) - n) // 2]] = False
    Ap2 = np.concatenate([[0], np.cumsum(np.bincount(cols[keep], minlength=n))]).astype(np.int64)
    Ai2, Ax2, cols2 = Ai[keep].copy(), vals[keep].copy(), cols[keep]
    # the last entry that can move one row up: off the diagonal, the column kept sorted
    q = next(q for q in range(len(Ai2) - 1, 0, -1)
             if Ai2[q] - 1 > cols2[q] and (cols2[q - 1] != cols2[q] or Ai2[q] - 1 > Ai2[q - 1]))
    Ai3 = Ai2.copy()
    Ai3[q] -= 1
    return n, Ap, Ai, vals, Ap2, Ai2, Ai3, Ax2


@pytest.mark.parametrize("on_device", [False, True])
def test_failed_long_way_after_a_hash_mismatch(on_device):
    """Same count, another pattern: the values-only path has already factorized on the device when the hash says no.  If
    the long way then fails (the k-th host allocation of the call, k = 1, 2, ...: the first is the values-only path's own),
    L must not claim a device factor: it is symbolic, or numeric with its host values only."""
    from test_memory_faults import FaultAllocator
    n, Ap, Ai, Ax, Ap2, Ai2, Ai3, Ax2 = _two_patterns()
    perm = G.geometric_nd(14, 14, 14, 4)
    S = ch.Session(factor_on_device=on_device)
    S.cm.error_handler = ch.ERRFUNC(0)
    A = S.sparse(n, Ap, Ai, Ax, -1)
    Lf = S.analyze(A, perm)                 # (L's symbolic structure is A's, as in the sequence)
    S.free_sparse(A)
    A2 = S.sparse(n, Ap2, Ai2, Ax2, -1)
    A3 = S.sparse(n, Ap2, Ai3, Ax2, -1)
    failures = 0
    with FaultAllocator(S.L) as fa:
        for k in range(1, 200):
            # (the map of A2, then a call through its values-only path)
            assert S.factorize(A2, Lf) == 1 and S.factorize(A2, Lf) == 1 and S.cm.status == ch.OK
            assert Lf.contents.hip_apat_valid == 1 and Lf.contents.hip_on_device == 1
            fa.arm(k)
            ok = S.factorize(A3, Lf)
            failed = fa.failed
            fa.arm(-1)
            if not failed:
                assert ok == 1
                break
            if ok:
                continue            # (an allocation the call can do without)
            failures += 1
            L = Lf.contents
            assert S.cm.status == ch.OUT_OF_MEMORY, (k, S.cm.status)
            assert not L.hip_on_device, k
            assert L.xtype == ch.PATTERN or (L.x and L.hip_host_valid), (k, L.xtype, L.hip_host_valid)
            S.cm.status = ch.OK
    assert not failed and failures > 0
    assert S.factorize(A3, Lf) == 1 and S.cm.status == ch.OK
    O = OracleFactor(n, Ap, Ai, -1, perm=perm, postorder=True)
    assert O.factorize(Ax2, Ap=Ap2, Ai=Ai3) == 0
    mask = O.lower_mask()
    assert S.L.cholmod_l_factor_to_host(Lf, C.byref(S.cm)) == 1
    x = ch.FactorView(Lf).x
    assert np.linalg.norm((x - O.x)[mask]) / np.linalg.norm(O.x[mask]) < 1e-12
    S.free_factor(Lf)
    S.free_sparse(A2)
    S.free_sparse(A3)
    assert S.cm.malloc_count == 0
    S.finish()


if __name__ == "__main__":
    # CHOLMOD_API_THREADS is read on every call; what else the environment holds (OMP_THREAD_LIMIT,
    # CHOLMOD_HIP_VALUES_IN_BATCH_ORDER) is read once per process and comes from the parent
    for t in sys.argv[1].split(","):
        os.environ["CHOLMOD_API_THREADS"] = t
        for stype in (-1, 1):
            sequence(stype)
    print("sequence ok")
