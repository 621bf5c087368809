"""Test-side reference of the gradients through M = A A' + beta I for an unsymmetric A (tests/test_aat_grad_api.py,
tests/aat_grad_cases.py): the product map of tril (A A') and its transpose restated in numpy, the chain rule through it,
the whole backward pass, and the same loss from a dense matrix with torch.linalg.solve / torch.logdet in float64 on the
CPU.  No GPU.

vals [c] = sum over the pairs p of list c of a [ia [p]] a [ib [p]] is entry c of tril (A A') (CSC order).  With
Gv [c] = d loss / d vals [c] -- the sampled product of tests/grad_reference.py on the pattern of tril (A A') for a solve, Z_ii
on the diagonal and 2 Z_ij off it for log det M --
    g [q] = sum_{p : ia [p] = q} Gv [c (p)] a [ib [p]]  +  sum_{p : ib [p] = q} Gv [c (p)] a [ia [p]]
and d loss / d beta = trace (d loss / d M).  Right-hand sides are ROWS, as in Session.solve_device."""
from fractions import Fraction

import numpy as np

import grad_reference as GR

EPS53 = 2.0 ** -53
PM_LEN1, PM_LEN16 = 8, 128


def product_map(M):
    """(Cp, Ci, cp, ia, ib) of the scipy CSC matrix M (sorted indices): the pattern of tril (M M') by columns, and per entry
    c = (i, j), i >= j, the pairs (position of M (i, k), position of M (j, k)) over the columns k both rows have, k ascending
    -- the map of cholmod_l_hip_aat_product_map"""
    m, ncol = M.shape
    lists = {}
    for k in range(ncol):
        q0, q1 = int(M.indptr[k]), int(M.indptr[k + 1])
        r = M.indices[q0:q1]
        for b in range(q1 - q0):
            for a in range(b, q1 - q0):
                lists.setdefault((int(r[b]), int(r[a])), []).append((q0 + a, q0 + b))       # key (column j, row i)
    keys = sorted(lists)
    Cp = np.zeros(m + 1, dtype=np.int64)
    for j, _ in keys:
        Cp[j + 1] += 1
    Cp = np.cumsum(Cp)
    Ci = np.array([i for _, i in keys], dtype=np.int64)
    cp = np.concatenate([[0], np.cumsum([len(lists[k]) for k in keys])]).astype(np.int64)
    pairs = [p for k in keys for p in lists[k]]
    ia = np.array([p[0] for p in pairs], dtype=np.int64)
    ib = np.array([p[1] for p in pairs], dtype=np.int64)
    return Cp, Ci, cp, ia, ib


def transpose_map(cp, ia, ib, navalues):
    """(tp, tc, tpart): per value q the half-pairs (entry c, partner value), tp [q] .. tp [q + 1], pairs in ascending p, the
    ia half of a pair before its ib half"""
    lists = [[] for _ in range(navalues)]
    for c in range(len(cp) - 1):
        for p in range(cp[c], cp[c + 1]):
            lists[ia[p]].append((c, ib[p]))
            lists[ib[p]].append((c, ia[p]))
    tp = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    tc = np.array([h[0] for x in lists for h in x], dtype=np.int64)
    tpart = np.array([h[1] for x in lists for h in x], dtype=np.int64)
    return tp, tc, tpart


def product_values(cp, ia, ib, a):
    return np.add.reduceat(np.append(a[ia] * a[ib], 0.0), cp[:-1]) * (np.diff(cp) > 0)


def product_grad(tp, tc, tpart, Gv, a):
    """g [q] = sum over the half-pairs of q of Gv [c] a [partner], in list order; +0.0 for an empty list"""
    g = np.zeros(len(tp) - 1)
    for q in range(len(g)):
        s = 0.0
        for h in range(tp[q], tp[q + 1]):
            s += Gv[tc[h]] * a[tpart[h]]
        g[q] = s
    return g


def product_grad_magnitude(tp, tc, tpart, Gv, a):
    """sum |Gv [c]| |a [partner]| per value: what the rounding bar of the chain step scales with"""
    t = np.abs(Gv)[tc] * np.abs(a)[tpart]
    return np.array([t[tp[q]:tp[q + 1]].sum() for q in range(len(tp) - 1)])


def _fma(x, y, z):
    return float(Fraction(x) * Fraction(y) + Fraction(z))       # one rounding, to nearest even


def product_grad_in_kernel_order(tp, tc, tpart, Gv, a):
    """the same sums in the order k_product_grad documents, rounding for rounding: a group of G = 1, 16 or 64 lanes by the
    length of the list (<= PM_LEN1, <= PM_LEN16, longer), lane l adds the half-pairs l, l + G, ... with a fused multiply-add
    from 0.0, then acc [l] += acc [l ^ w] for w = G / 2 .. 1 on all lanes at once; lane 0 holds the result.  Finite input."""
    g = np.zeros(len(tp) - 1)
    for q in range(len(g)):
        h0, h1 = int(tp[q]), int(tp[q + 1])
        G = 1 if h1 - h0 <= PM_LEN1 else 16 if h1 - h0 <= PM_LEN16 else 64
        acc = [0.0] * G
        for lane in range(G):
            for h in range(h0 + lane, h1, G):
                acc[lane] = _fma(float(Gv[tc[h]]), float(a[tpart[h]]), acc[lane])
        w = G // 2
        while w:
            acc = [acc[lane] + acc[lane ^ w] for lane in range(G)]
            w //= 2
        g[q] = acc[0]
    return g


def dense_of(M, a, beta):
    D = np.zeros(M.shape)
    D[M.indices, GR.columns_of(M.indptr)] = a
    return D @ D.T + beta * np.eye(M.shape[0])


def loss_gradients(M, a, beta, B, W, maps=None):
    """the numpy restatement: -> (grad_values, grad_B, grad_beta) of loss = (W . X).sum () + 0.3 log det (A A' + beta I)"""
    Cp, Ci, cp, ia, ib = maps if maps is not None else product_map(M)
    tp, tc, tpart = transpose_map(cp, ia, ib, M.nnz)
    Md = dense_of(M, a, beta)
    B2, W2 = np.atleast_2d(B), np.atleast_2d(W)
    X = np.linalg.solve(Md, B2.T).T
    lam = np.linalg.solve(Md, W2.T).T
    Z = np.linalg.inv(Md)
    Gv = GR.values_grad(Cp, Ci, -1, lam, X, -1.0) + 0.3 * GR.logdet_multiplier(Cp, Ci, -1) * Z[Ci, GR.columns_of(Cp)]
    gbeta = -float((lam * X).sum()) + 0.3 * float(np.trace(Z))
    return product_grad(tp, tc, tpart, Gv, a), lam.reshape(np.shape(B)), gbeta


def symmetric_beta_gradient(n, Ap, Ai, Ax, stype, beta, B, W):
    """d loss / d beta of the same loss for a symmetric A (tests/grad_reference.py), M = A + beta I"""
    Md = GR.dense_of(n, Ap, Ai, Ax, stype, beta)
    X = np.linalg.solve(Md, np.atleast_2d(B).T).T
    lam = np.linalg.solve(Md, np.atleast_2d(W).T).T
    return -float((lam * X).sum()) + 0.3 * float(np.trace(np.linalg.inv(Md)))


def _finish(Md, v, Bt, Wt, bt, B):
    import torch
    X = torch.linalg.solve(Md, Bt.T).T
    ld = torch.logdet(Md)
    loss = (Wt * X).sum() + 0.3 * ld
    loss.backward()
    with torch.no_grad():
        lam = torch.linalg.solve(Md, Wt.T).T
        Z = torch.linalg.inv(Md)
        half = float(torch.log(torch.diagonal(torch.linalg.cholesky(Md))).abs().sum())
    return dict(loss=float(loss.detach()), X=X.detach().numpy().reshape(np.shape(B)), logdet=float(ld.detach()), logdet_scale=2.0 * half,
                grad_values=v.grad.numpy(), grad_B=Bt.grad.numpy().reshape(np.shape(B)), grad_beta=float(bt.grad),
                lam_max=float(lam.abs().max()), x_max=float(X.detach().abs().max()), z_max=float(Z.abs().max()))


def torch_reference(M, a, beta, B, W):
    """the loss from the dense M = D D' + beta I, D built from the values with index_put, through torch.autograd in float64
    on the CPU -> dict as grad_reference.torch_reference gives, plus grad_beta"""
    import torch
    v = torch.tensor(a, dtype=torch.float64, requires_grad=True)
    bt = torch.tensor(float(beta), dtype=torch.float64, requires_grad=True)
    Bt = torch.tensor(np.atleast_2d(B), dtype=torch.float64, requires_grad=True)
    Wt = torch.tensor(np.atleast_2d(W), dtype=torch.float64)
    idx = (torch.tensor(M.indices.astype(np.int64)), torch.tensor(GR.columns_of(M.indptr)))
    D = torch.zeros(M.shape, dtype=torch.float64).index_put(idx, v)
    return _finish(D @ D.T + bt * torch.eye(M.shape[0], dtype=torch.float64), v, Bt, Wt, bt, B)


def torch_reference_symmetric(n, Ap, Ai, Ax, stype, beta, B, W):
    """the same for a symmetric A given by its stored triangle, M = A + beta I: the dict with grad_beta"""
    import torch
    cols, read = GR.columns_of(Ap), GR.read_mask(Ap, Ai, stype)
    off = read & (Ai != cols)
    v = torch.tensor(Ax, dtype=torch.float64, requires_grad=True)
    bt = torch.tensor(float(beta), dtype=torch.float64, requires_grad=True)
    Bt = torch.tensor(np.atleast_2d(B), dtype=torch.float64, requires_grad=True)
    Wt = torch.tensor(np.atleast_2d(W), dtype=torch.float64)
    rows_t = torch.tensor(np.concatenate([Ai[read], cols[off]]))
    cols_t = torch.tensor(np.concatenate([cols[read], Ai[off]]))
    vals = torch.cat([v[torch.tensor(np.flatnonzero(read))], v[torch.tensor(np.flatnonzero(off))]])
    Md = torch.zeros((n, n), dtype=torch.float64).index_put((rows_t, cols_t), vals) + bt * torch.eye(n, dtype=torch.float64)
    return _finish(Md, v, Bt, Wt, bt, B)


def column_weight(M, a):
    """max over the values q of || A [:, col (q)] ||_1 + |a_q|: what an error of the gradient with respect to M is multiplied
    by on its way to a value of A (one half-pair per entry of the column, and the value itself once more)"""
    cols = GR.columns_of(M.indptr)
    norm1 = np.add.reduceat(np.append(np.abs(a), 0.0), M.indptr[:-1]) * (np.diff(M.indptr) > 0)
    return float((norm1[cols] + np.abs(a)).max()) if M.nnz else 0.0


def bars(M, a, ref, tol, nrhs):
    """(bar of grad_values, of grad_B, of grad_beta) of the end-to-end comparison, from the chain rule: the gradient with
    respect to M holds the bar of grad_reference.bars entry by entry; a value of A collects it over its column
    (column_weight); beta collects the m diagonal entries, each with 2 nrhs products of the two solves and 0.3 Z_ii"""
    bv, bb = GR.bars(ref, tol, nrhs)
    return bv * column_weight(M, a), bb, tol * M.shape[0] * (2 * nrhs * ref["lam_max"] * ref["x_max"] + 0.3 * ref["z_max"])
