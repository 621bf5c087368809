"""The bodies of tests/test_gpu_solve_device_complex.py, run in a process of their own:
`python solve_device_complex_cases.py CASE [ARG ...]`.  torch is imported FIRST, before the engine library is loaded, so
that torch and the engine share one HIP runtime (see tests/solve_device_cases.py).  Exit status 0 = every assertion held;
a line `RESULT <json>` carries figures back.

STORAGE is "cx" (the engine keeps the complex factor in its own storage and the solve kernels rebuild the odd twin
columns: the default on one GPU) or "twin" (CHOLMOD_HIP_CX_TWIN=1: the full real twin on the real kernels)."""
import torch  # noqa: E402  (first: see above)

import ctypes as C
import json
import os
import sys

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle.oracle import OracleFactor
from suitesparse_amd import cholmod as ch
from suitesparse_amd import generators as G

TOL = 1e-11             # per column, against Session.solve and the dense triangular solves (tests/test_gpu_solve_device.py)
TOL_RES = 1e-11         # residual against the full Hermitian matrix (tests/test_complex.py)
TOL_ORACLE = 1e-10      # against OracleFactor.solve_complex (tests/test_complex.py)
NRHS = [1, 2, 7, 8, 15, 16, 17, 40]         # 7 | 8: columns / panels; 16 | 17: the panel edge
GOLDEN = os.path.join(ROOT, "tests", "golden")


def hermitian_from(n, Ap, Ai, Ax, stype=-1, seed=0, scale=0.9):
    """(a copy of the helper of tests/test_complex.py) A Hermitian positive definite matrix on the pattern of a real SPD
    one: every off-diagonal entry is turned by a random phase and shrunk (the diagonal keeps dominating).  Returns the
    lower-stored CSC (Ap, Ai, complex Ax), sorted."""
    rng = np.random.default_rng(seed)
    A = sp.csc_matrix((Ax, Ai, Ap), shape=(n, n))
    Al = (sp.tril(A) if stype < 0 else sp.triu(A).T).tocsc()
    Al.sort_indices()
    vals = Al.data.astype(np.complex128)
    cols = np.repeat(np.arange(n), np.diff(Al.indptr))
    off = Al.indices != cols
    vals[off] *= scale * np.exp(1j * rng.uniform(0, 2 * np.pi, int(off.sum())))
    return Al.indptr.astype(np.int64), Al.indices.astype(np.int64), vals


def full_hermitian(n, Ap, Ai, Ax):
    Al = sp.csc_matrix((Ax, Ai, Ap), shape=(n, n))
    return (Al + sp.tril(Al, -1).conj().T).tocsr()


def dense_L(fv, x):
    n = fv.n
    Ld = np.zeros((n, n), dtype=x.dtype)
    sup, pi, px, s = (np.asarray(getattr(fv, k)) for k in ("super", "pi", "px", "s"))
    for k in range(len(sup) - 1):
        nscol, nsrow = int(sup[k + 1] - sup[k]), int(pi[k + 1] - pi[k])
        blk = x[px[k]:px[k] + nsrow * nscol].reshape(nscol, nsrow).T
        r = s[pi[k]:pi[k + 1]]
        for j in range(nscol):
            Ld[r[j:], sup[k] + j] = blk[j:, j]
    return Ld


def _matrix(name):
    """the cases of tests/test_complex.py: (n, Ap, Ai, complex Ax, perm)"""
    if name == "bcsstk01":          # odd supernode widths: twin widths that are no multiple of 16
        rec = json.load(open(os.path.join(GOLDEN, "reference_recorded.json")))["bcsstk01"]
        n, Ap, Ai, Ax, stype = G.read_triplet(os.path.join(GOLDEN, "bcsstk01.tri"))
        return (n,) + hermitian_from(n, Ap, Ai, Ax, stype, scale=0.5) + (np.array(rec["Perm"]),)
    if name == "p3d_9_nd":
        n, Ap, Ai, Ax = G.poisson3d(9)
        return (n,) + hermitian_from(n, Ap, Ai, Ax) + (G.geometric_nd(9, 9, 9, 3),)
    if name == "box7r2_nd":
        n, Ap, Ai, Ax = G.box_stencil3d(7, 2)
        return (n,) + hermitian_from(n, Ap, Ai, Ax, scale=0.3) + (G.geometric_nd(7, 7, 7, 3),)
    raise KeyError(name)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _relcols(X, R):
    """largest relative 2-norm error over the columns (rows of the (nrhs, n) arrays)"""
    X, R = np.atleast_2d(X), np.atleast_2d(R)
    return max(np.linalg.norm(X[k] - R[k]) / np.linalg.norm(R[k]) for k in range(R.shape[0]))


def _rhs(rng, nrhs, n):
    return rng.standard_normal((nrhs, n)) + 1j * rng.standard_normal((nrhs, n))


def _factor(n, Ap, Ai, Ax, perm, storage, **kw):
    assert storage in ("cx", "twin")
    if storage == "twin":
        os.environ["CHOLMOD_HIP_CX_TWIN"] = "1"
    else:
        os.environ.pop("CHOLMOD_HIP_CX_TWIN", None)
    S = ch.Session(**kw)
    A = S.sparse(n, Ap, Ai, Ax, -1)
    Lf = S.analyze(A, perm)
    assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
    assert Lf.contents.xtype == ch.COMPLEX
    T = C.cast(Lf.contents.cx_twin, C.POINTER(ch.Factor))
    assert T.contents.hip_is_twin == (2 if storage == "cx" else 1)      # the form that was asked for
    return S, A, Lf


def _done(S, A, Lf):
    torch.cuda.synchronize()
    S.free_factor(Lf)
    S.free_sparse(A)
    S.finish()


def _check_systems(S, Lf, b, Ld, Af, O, tag):
    """all nine systems for the right-hand sides b (nrhs, n): the bars of the module"""
    nrhs, n = b.shape
    B = _dev(b)
    for sys_ in range(9):
        xh = np.atleast_2d(S.solve(Lf, b, sys_))        # the unchanged host-array path
        xd = S.solve_device(Lf, B, sys_)
        assert xd.dtype == torch.complex128 and tuple(xd.shape) == (nrhs, n)
        xd = xd.cpu().numpy()
        if sys_ in (ch.SYS_P, ch.SYS_Pt, ch.SYS_D):
            assert np.array_equal(xd, xh), (tag, nrhs, sys_)
            continue
        e = _relcols(xd, xh)
        print(f"{tag} nrhs={nrhs} sys={sys_}: device vs host path {e:.2e}")
        assert e < TOL, (tag, nrhs, sys_, e)
        if sys_ in (ch.SYS_L, ch.SYS_LD):
            e = _relcols(xd, sla.solve_triangular(Ld, b.T, lower=True).T)
            print(f"{tag} nrhs={nrhs} sys={sys_}: vs dense L {e:.2e}")
            assert e < TOL, (tag, nrhs, sys_, e)
        elif sys_ in (ch.SYS_Lt, ch.SYS_DLt):
            e = _relcols(xd, sla.solve_triangular(Ld, b.T, lower=True, trans="C").T)
            print(f"{tag} nrhs={nrhs} sys={sys_}: vs dense L^H {e:.2e}")
            assert e < TOL, (tag, nrhs, sys_, e)
        elif sys_ == ch.SYS_A:
            r = (Af @ xd.T).T - b
            e = max(np.linalg.norm(r[k]) / np.linalg.norm(b[k]) for k in range(nrhs))
            eo = np.linalg.norm(xd - O.solve_complex(b)) / np.linalg.norm(xd)
            print(f"{tag} nrhs={nrhs} sys=A: residual {e:.2e}, vs oracle {eo:.2e}")
            assert e < TOL_RES, (tag, nrhs, e)
            assert eo < TOL_ORACLE, (tag, nrhs, eo)
    return S.solve_device(Lf, B).cpu().numpy()


def case_parity(name, storage):
    n, Ap, Ai, Ax, perm = _matrix(name)
    S, A, Lf = _factor(n, Ap, Ai, Ax, perm, storage)
    O = OracleFactor(n, Ap, Ai, -1, perm=perm, postorder=True)
    assert O.factorize_complex(Ax) == 0
    fv = ch.FactorView(Lf)
    Ld = dense_L(fv, fv.x)
    Af = full_hermitian(n, Ap, Ai, Ax)
    rng = np.random.default_rng(11)
    for nrhs in NRHS:
        _check_systems(S, Lf, _rhs(rng, nrhs, n), Ld, Af, O, f"{name}/{storage}")
    _done(S, A, Lf)


def _big_supernode_matrix(scale):
    """the shape of _big_supernode_matrix of tests/solve_device_cases.py at half the size, Hermitian: a 700-column
    supernode with 50 rows below it, followed by a dense 100-column root; random phases on the off-diagonal entries, the
    same diagonal dominance.  Twin: 1400 columns = five 256-column blocks and a last one of 120 = 64 + 56."""
    n1, n2 = 700, 100
    n = n1 + n2
    rng = np.random.default_rng(7)
    M = rng.standard_normal((n, n)) * 0.05
    Ad = M @ M.T + np.eye(n) * 4.0
    mask = np.zeros((n, n), dtype=bool)
    mask[:n1, :n1] = True
    mask[n1:, n1:] = True
    mask[n1 + 50:, :n1] = True
    mask[:n1, n1 + 50:] = True
    Ad = np.where(mask, Ad, 0.0)
    Ad += np.eye(n) * (np.abs(Ad).sum(axis=1).max())
    Ad[:350, :350] *= scale                      # (scale != 1: other values on the same pattern, still diagonally dominant)
    ph = np.exp(1j * rng.uniform(0, 2 * np.pi, (n, n)))
    ph = np.tril(ph, -1)
    ph = ph + ph.conj().T + np.eye(n)            # Hermitian phases, a real diagonal
    Ac = Ad * ph
    ii, jj = np.nonzero(np.tril(mask))
    order = np.lexsort((ii, jj))
    Ai, cols = ii[order].astype(np.int64), jj[order]
    Ax = Ac[Ai, cols]
    Ap = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(cols, minlength=n), out=Ap[1:])
    return n, Ap, Ai, Ax


def case_big_supernode(nrhs):
    nrhs = int(nrhs)
    n, Ap, Ai, Ax = _big_supernode_matrix(1.0)
    perm = np.arange(n, dtype=np.int64)
    S, A, Lf = _factor(n, Ap, Ai, Ax, perm, "cx")
    fv = ch.FactorView(Lf)
    assert np.diff(fv.super).max() >= 700 - 32
    b = _rhs(np.random.default_rng(3), nrhs, n)

    def check(Ax_now):
        O = OracleFactor(n, Ap, Ai, -1, perm=perm, postorder=True)
        assert O.factorize_complex(Ax_now) == 0
        f = ch.FactorView(Lf)
        return _check_systems(S, Lf, b, dense_L(f, f.x), full_hermitian(n, Ap, Ai, Ax_now), O, "big")

    x_a = check(Ax)
    # a second factorization with other values: the cached inverses must follow them
    _, _, _, Ax2 = _big_supernode_matrix(1.5)
    S.free_sparse(A)
    A = S.sparse(n, Ap, Ai, Ax2, -1)
    assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
    x_b = check(Ax2)
    assert _relcols(x_b, x_a) > 1e-6             # the result follows the new values
    _done(S, A, Lf)


def case_layout(storage):
    name = "p3d_9_nd"
    n, Ap, Ai, Ax, perm = _matrix(name)
    S, A, Lf = _factor(n, Ap, Ai, Ax, perm, storage)
    rng = np.random.default_rng(5)
    for nrhs in (1, 5, 18):
        b = _rhs(rng, nrhs, n)
        ref = S.solve(Lf, b)
        ld = n + 3
        Bp = torch.full((nrhs, ld), -777.0 + 333.0j, dtype=torch.complex128, device="cuda")
        Xp = torch.full((nrhs, ld), 555.0 - 111.0j, dtype=torch.complex128, device="cuda")
        Bp[:, :n] = _dev(b)
        B0 = Bp.clone()
        out = S.solve_device(Lf, Bp[:, :n], out=Xp[:, :n])
        assert out.data_ptr() == Xp.data_ptr()
        assert torch.equal(Bp, B0)                                   # B and its padding rows unchanged
        assert bool((Xp[:, n:] == 555.0 - 111.0j).all())             # padding rows of X unchanged, bit for bit
        x = Xp[:, :n].cpu().numpy()
        assert _relcols(x, ref) < TOL
        # in place (the forward sweeps add into shared ancestor rows atomically, so two runs agree to rounding)
        S.solve_device(Lf, Bp[:, :n], out=Bp[:, :n])
        assert _relcols(Bp[:, :n].cpu().numpy(), x) < TOL
        assert bool((Bp[:, n:] == -777.0 + 333.0j).all())
        # a single vector of shape (n,)
        x1 = S.solve_device(Lf, _dev(b[0]))
        assert tuple(x1.shape) == (n,) and x1.dtype == torch.complex128
        assert _relcols(x1.cpu().numpy(), np.atleast_2d(ref)[0]) < TOL
    # nrhs == 0: TRUE, nothing touched
    E = torch.empty((0, n), dtype=torch.complex128, device="cuda")
    assert tuple(S.solve_device(Lf, E).shape) == (0, n)
    assert tuple(S.residual_device(Lf, E, E.clone()).shape) == (0, n)
    Bk = torch.full((2, n), 3.0 + 1.0j, dtype=torch.complex128, device="cuda")
    Xk = torch.full((2, n), 4.0 - 2.0j, dtype=torch.complex128, device="cuda")
    ok = S.L.cholmod_l_hip_solve_device_complex(ch.SYS_A, Lf, Bk.data_ptr(), n, Xk.data_ptr(), n, 0, None, C.byref(S.cm))
    torch.cuda.synchronize()
    assert ok == 1 and S.cm.status == ch.OK
    assert bool((Bk == 3.0 + 1.0j).all()) and bool((Xk == 4.0 - 2.0j).all())
    # a dtype that does not match the factor
    for bad in (torch.zeros((2, n), dtype=torch.float64, device="cuda"), torch.zeros((2, n), dtype=torch.complex64, device="cuda")):
        for call in (lambda t: S.solve_device(Lf, t), lambda t: S.residual_device(Lf, t, t.clone()),
                     lambda t: S.refine_device(Lf, t, t.clone())):
            try:
                call(bad)
            except TypeError:
                continue
            raise AssertionError("a tensor of the wrong dtype was accepted")
    _done(S, A, Lf)


def case_residual_refine(storage, nrhs):
    nrhs = int(nrhs)
    n, Ap, Ai, Ax, perm = _matrix("p3d_9_nd")
    S, A, Lf = _factor(n, Ap, Ai, Ax, perm, storage)
    Af = full_hermitian(n, Ap, Ai, Ax)
    rng = np.random.default_rng(13)
    b = _rhs(rng, nrhs, n)
    x = _rhs(rng, nrhs, n)                       # any X: the residual is a matrix product
    B, X = _dev(b), _dev(x)
    R, nrm = S.residual_device(Lf, X, B, norms=True)
    assert R.dtype == torch.complex128 and nrm.dtype == torch.float64 and tuple(nrm.shape) == (nrhs,)
    r = R.cpu().numpy()
    ref = b - (Af @ x.T).T
    e = max(np.linalg.norm(r[k] - ref[k]) / np.linalg.norm(b[k]) for k in range(nrhs))
    print(f"residual {storage} nrhs={nrhs}: vs scipy {e:.2e} (relative to |B|)")
    assert e < 1e-11, e
    R2, nrm2 = S.residual_device(Lf, X, B, norms=True)
    assert torch.equal(R, R2) and torch.equal(nrm, nrm2)            # the same bits
    want = np.maximum(np.abs(r.real).max(axis=1), np.abs(r.imag).max(axis=1))
    assert np.array_equal(nrm.cpu().numpy(), want)
    # in place on B
    Bc = B.clone()
    assert S.residual_device(Lf, X, Bc, out=Bc).data_ptr() == Bc.data_ptr()
    assert torch.equal(Bc, R)
    # refinement: one step from a solution perturbed by 1e-6
    xs = S.solve_device(Lf, B).cpu().numpy()
    xp = xs * (1.0 + 1e-6 * _rhs(rng, nrhs, n))
    before = max(np.linalg.norm(b[k] - Af @ xp[k]) / np.linalg.norm(b[k]) for k in range(nrhs))
    Xp = _dev(xp)
    X0 = Xp.clone()
    out, n0 = S.refine_device(Lf, B, Xp, steps=0, norms=True)
    assert out.data_ptr() == Xp.data_ptr() and torch.equal(Xp, X0)  # steps = 0: X bit-identical
    r0 = b - (Af @ xp.T).T
    w0 = np.maximum(np.abs(r0.real).max(axis=1), np.abs(r0.imag).max(axis=1))
    assert np.allclose(n0.cpu().numpy(), w0, rtol=1e-6, atol=0)
    _, n1 = S.refine_device(Lf, B, Xp, steps=1, norms=True)
    xr = Xp.cpu().numpy()
    after = max(np.linalg.norm(b[k] - Af @ xr[k]) / np.linalg.norm(b[k]) for k in range(nrhs))
    print(f"refine {storage} nrhs={nrhs}: relative residual {before:.2e} -> {after:.2e}")
    assert before > 1e-9 and after < 1e-11, (before, after)
    assert bool((n1 < n0).all())
    _done(S, A, Lf)


def case_hermitian64():
    """Hermitian matrix on the pattern of Poisson 64^3, 16 right-hand sides, complex storage: device time (stats [24],
    median of five after a warm-up) of the device path against the host-array complex solve on the same factor, which
    reads L once per right-hand side.  No margin: a panel path that loses to it is not working."""
    n, Ap, Ai, Ax = G.poisson3d(64)
    perm = G.geometric_nd(64, 64, 64, 4)
    Ap, Ai, Ax = hermitian_from(n, Ap, Ai, Ax)
    S, A, Lf = _factor(n, Ap, Ai, Ax, perm, "cx", factor_on_device=True)
    b = _rhs(np.random.default_rng(4), 16, n)
    B = _dev(b)

    def median(run):
        run()
        t = []
        for _ in range(5):
            run()
            t.append(float(S.hip_stats(Lf)[24]))
        return float(np.median(t))

    keep = {}
    t_host = median(lambda: keep.__setitem__("h", S.solve(Lf, b)))
    t_dev = median(lambda: keep.__setitem__("d", S.solve_device(Lf, B)))
    print(f"Hermitian 64^3 nrhs=16: host-array path {1e3 * t_host:.2f} ms, device path {1e3 * t_dev:.2f} ms, "
          f"ratio {t_host / max(t_dev, 1e-30):.2f}")
    print("RESULT " + json.dumps({"host_ms": 1e3 * t_host, "device_ms": 1e3 * t_dev}))
    assert t_host > 0 and t_dev > 0
    xd = keep["d"].cpu().numpy()
    assert _relcols(xd, keep["h"]) < TOL
    Af = full_hermitian(n, Ap, Ai, Ax)
    assert max(np.linalg.norm(Af @ xd[k] - b[k]) / np.linalg.norm(b[k]) for k in range(16)) < TOL_RES
    assert t_dev < t_host, (t_dev, t_host)
    _done(S, A, Lf)


if __name__ == "__main__":
    torch.cuda.init()
    globals()["case_" + sys.argv[1]](*sys.argv[2:])
    print("CASE OK")
