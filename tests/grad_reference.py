"""Test-side reference of the gradients through the device path (tests/test_grad_api.py, tests/grad_cases.py): the numpy
formulas of the sampled product and of the whole backward pass, and the same loss built from a dense symmetric matrix with
torch.linalg.solve / torch.logdet in float64 on the CPU.  No GPU.

For a symmetric A given by the entries (i, j) it is read at (one triangle), M = A + beta I, X = M^-1 B, a loss
    loss = (W . X).sum () + 0.3 log det M
has, with Lambda = M^-1 W and Z = M^-1,
    d loss / d B = Lambda
    d loss / d a_ij = -sum_r (Lambda [i, r] X [j, r] + [i != j] Lambda [j, r] X [i, r]) + 0.3 (Z_ii if i == j else 2 Z_ij)
and zero at every entry A is not read at.  Right-hand sides are ROWS here, as in Session.solve_device: U [r, i]."""
import numpy as np

EPS = np.finfo(float).eps


def columns_of(Ap):
    return np.repeat(np.arange(len(Ap) - 1, dtype=np.int64), np.diff(Ap))


def read_mask(Ap, Ai, stype):
    """the entries of A (CSC, sorted, no duplicates) the factorization reads: the stored triangle"""
    cols = columns_of(Ap)
    return (Ai >= cols) if stype < 0 else (Ai <= cols)


def values_grad(Ap, Ai, stype, U, V, alpha):
    """G [k] = alpha sum_r (U [r, i] V [r, j] + [i != j] U [r, j] V [r, i]) at the entries read, +0.0 elsewhere; r ascending"""
    U, V = np.atleast_2d(U), np.atleast_2d(V)
    cols, read = columns_of(Ap), read_mask(Ap, Ai, stype)
    off = (Ai != cols).astype(np.float64)
    s = np.zeros(len(Ai))
    for r in range(U.shape[0]):
        s += U[r, Ai] * V[r, cols]
        s += off * (U[r, cols] * V[r, Ai])
    return np.where(read, alpha * s, 0.0)


def values_grad_magnitude(Ap, Ai, U, V):
    """sum_r (|U_i V_j| + |U_j V_i|) per entry: what the rounding bar of the sampled product scales with"""
    U, V = np.abs(np.atleast_2d(U)), np.abs(np.atleast_2d(V))
    cols = columns_of(Ap)
    return (U[:, Ai] * V[:, cols] + U[:, cols] * V[:, Ai]).sum(axis=0)


def logdet_multiplier(Ap, Ai, stype):
    """1 on the diagonal, 2 off it, 0 where A is not read"""
    cols = columns_of(Ap)
    return np.where(read_mask(Ap, Ai, stype), np.where(Ai == cols, 1.0, 2.0), 0.0)


def dense_of(n, Ap, Ai, Ax, stype, beta=0.0):
    """the symmetric matrix the stored triangle of (Ap, Ai, Ax) stands for, plus beta I, dense"""
    cols, read = columns_of(Ap), read_mask(Ap, Ai, stype)
    M = np.zeros((n, n))
    M[Ai[read], cols[read]] = Ax[read]
    off = read & (Ai != cols)
    M[cols[off], Ai[off]] = Ax[off]
    return M + beta * np.eye(n)


def loss_gradients(n, Ap, Ai, Ax, stype, beta, B, W):
    """the numpy restatement: -> (grad_values, grad_B) of loss = (W . X).sum () + 0.3 log det M"""
    M = dense_of(n, Ap, Ai, Ax, stype, beta)
    B2, W2 = np.atleast_2d(B), np.atleast_2d(W)
    X = np.linalg.solve(M, B2.T).T
    lam = np.linalg.solve(M, W2.T).T
    Z = np.linalg.inv(M)
    gv = values_grad(Ap, Ai, stype, lam, X, -1.0) + 0.3 * logdet_multiplier(Ap, Ai, stype) * Z[Ai, columns_of(Ap)]
    return gv, lam.reshape(np.shape(B))


def torch_reference(n, Ap, Ai, Ax, stype, beta, B, W):
    """the same loss from a dense symmetric matrix with torch.linalg.solve / torch.logdet in float64 on the CPU, through
    torch.autograd -> dict (loss, X, logdet, grad_values, grad_B, and max |Lambda|, max |X|, max |Z| for the bars)"""
    import torch
    cols, read = columns_of(Ap), read_mask(Ap, Ai, stype)
    off = read & (Ai != cols)
    v = torch.tensor(Ax, dtype=torch.float64, requires_grad=True)
    Bt = torch.tensor(np.atleast_2d(B), dtype=torch.float64, requires_grad=True)
    Wt = torch.tensor(np.atleast_2d(W), dtype=torch.float64)
    rows_t = torch.tensor(np.concatenate([Ai[read], cols[off]]))
    cols_t = torch.tensor(np.concatenate([cols[read], Ai[off]]))
    vals = torch.cat([v[torch.tensor(np.flatnonzero(read))], v[torch.tensor(np.flatnonzero(off))]])
    M = torch.zeros((n, n), dtype=torch.float64).index_put((rows_t, cols_t), vals) + beta * torch.eye(n, dtype=torch.float64)
    X = torch.linalg.solve(M, Bt.T).T
    ld = torch.logdet(M)
    loss = (Wt * X).sum() + 0.3 * ld
    loss.backward()
    with torch.no_grad():
        lam = torch.linalg.solve(M, Wt.T).T
        Z = torch.linalg.inv(M)
        half = float(torch.log(torch.diagonal(torch.linalg.cholesky(M))).abs().sum())
    return dict(loss=float(loss.detach()), X=X.detach().numpy().reshape(np.shape(B)), logdet=float(ld.detach()), logdet_scale=2.0 * half,
                grad_values=v.grad.numpy(), grad_B=Bt.grad.numpy().reshape(np.shape(B)),
                lam_max=float(lam.abs().max()), x_max=float(X.detach().abs().max()), z_max=float(Z.abs().max()))


def bars(ref, tol, nrhs):
    """(bar of grad_values, bar of grad_B): each of the two solves carries tol relative to its maximum, and their errors
    pass through 2 nrhs products per entry; the selected inverse carries tol max |Z| and enters with 0.3 * 2"""
    return tol * (4 * nrhs * ref["lam_max"] * ref["x_max"] + 0.6 * ref["z_max"]), tol * ref["lam_max"]


def inputs(n, nrhs, seed):
    """(B, W) of the end-to-end cases: standard normal, shape (nrhs, n), or (n,) for one right-hand side"""
    rng = np.random.default_rng(seed)
    shape = (n,) if nrhs == 1 else (nrhs, n)
    return rng.standard_normal(shape), rng.standard_normal(shape)
