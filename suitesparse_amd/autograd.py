"""torch.autograd through the device-resident Cholesky path: a solve and a log-determinant whose backward passes stay on
the device and on torch's current stream.

    chol = DeviceCholesky(session, A, Lf, beta=0.0)
    X = chol.solve(values, B)           # M^-1 B; differentiable in values, B and (a tensor) beta
    ld = chol.logdet(values)            # log det M; differentiable in values and (a tensor) beta
    X = chol.solve_Lt(values, Z)        # P' L^-T Z, the reparameterised sample from N (0, M^-1); symmetric A only
    Y = chol.solve_L(values, B)         # L^-1 P B, whitening; both differentiable in values, the right-hand side and beta

`A` gives the pattern, `values` (a 1-D torch.float64 device tensor of length nnz (A), A's entry order) the numbers, `Lf` is a
factor that was factorized once from a host matrix of A's pattern -- the precondition of Session.factorize_device.  For a
symmetric A (stype != 0) M = A (values) + beta I; for an unsymmetric one (stype == 0) M = A (values) A (values)' + beta I,
the normal equations of a least-squares problem with A = J' and beta the damping.

With X = M^-1 B and an incoming gradient gX:  Lambda = M^-1 gX  is the gradient with respect to B, and
-(Lambda X' + X Lambda') is the one with respect to M: sampled on the entries of A the factorization reads
(Session.values_grad_device) it is the gradient with respect to the values of a symmetric A -- a value the factorization
does not read (the ignored triangle) has gradient zero --, carried through the product map (Session.aat_values_grad_device)
the one with respect to the values of an unsymmetric A; its trace, -(Lambda . X).sum (), the one with respect to beta.
The gradient of log det M with respect to M is Z = M^-1 from Session.selinv_device: Z_ii on the diagonal and 2 Z_ij off it
for the value of a symmetric A at (i, j), Session.aat_logdet_grad_device for an unsymmetric A, Z's trace for beta.

solve_Lt and solve_L are functions of the factor L L' = P M P' itself, and their gradient with respect to M is neither low
rank nor the inverse: it is reverse-mode Cholesky (Session.factor_outer_grad_device, the sweep of the selected inverse with
another recurrence).  With Xt = L^-T Z and an incoming gradient gXt (the factor's ordering), U = L^-1 gXt is the gradient
with respect to Z and Lbar = -tril (Xt U') the one with respect to L; with Y = L^-1 P B and gY, V = L^-T gY gives P' V for B
and Lbar = -tril (V Y').  The sweep turns Lbar into the gradient with respect to the values of A -- zero where the
factorization does not read A -- and its trace, the gradient with respect to beta.

beta is a Python float, or a 0-dim torch.float64 tensor on either device; a tensor that requires grad receives its
gradient (two torch reductions on the current stream).  The factorization reads float (beta) -- it waits for the host
anyway --, once per version of the tensor.

The wrapper OWNS Lf: a factorization of Lf behind its back is detected (the engine counts factorizations,
cholmod_hip_progress out [0]) and answered by factorizing again from the values a backward pass saved, but values handed to
Session.factorize_device directly are not seen by `solve` / `logdet` calls that follow with the tensor factorized last.
All functions are differentiable once; real factors, one rank."""
import ctypes as C

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import cholmod as ch


class DeviceCholesky:
    def __init__(self, session, A, Lf, beta=0.0):
        self.S, self.A, self.Lf = session, A, Lf
        self.aat = A.contents.stype == 0        # M = A A' + beta I
        self.beta = beta
        self._values = None         # the tensor factorized last (kept alive: its address cannot be handed out again)
        self._key = None            # (data_ptr, _version, beta) of that factorization
        self._fact = -1             # the engine's count of factorizations right after it
        self._mult = None
        self.factorizations = 0     # ... and the wrapper's own

    # ---- beta: a float, or a 0-dim float64 tensor that is read once per version
    @property
    def beta(self):
        return self._beta

    @beta.setter
    def beta(self, beta):
        if isinstance(beta, torch.Tensor):
            if beta.dim() != 0 or beta.dtype != torch.float64:
                raise TypeError("DeviceCholesky: a tensor beta must be 0-dim and torch.float64")
            self._beta, self._beta_read = beta, None
        else:
            self._beta, self._beta_read = float(beta), None

    def _beta_value(self):
        b = self._beta
        if not isinstance(b, torch.Tensor):
            return b
        if self._beta_read is None or self._beta_read[0] != b._version:
            self._beta_read = (b._version, float(b.detach()))
        return self._beta_read[1]

    def _beta_input(self):
        """what the autograd functions take as their beta input: the tensor, or None for a float"""
        return self._beta if isinstance(self._beta, torch.Tensor) else None

    # ---- the factor
    def _count(self):
        plan = self.Lf.contents.hip_plan
        if not plan:
            return -1
        out = np.zeros(12, dtype=np.int64)
        if self.S.L.cholmod_hip_progress(plan, out.ctypes.data) != ch.HIP_OK:
            return -1
        return int(out[0])

    def _factorize(self, values):
        self._key = self._values = None
        beta = self._beta_value()
        ok = self.S.factorize_device(self.A, values, self.Lf, beta)
        if not ok or self.S.cm.status != ch.OK or self.Lf.contents.minor < self.Lf.contents.n:
            raise RuntimeError(f"DeviceCholesky: the matrix is not positive definite or the factorization failed "
                               f"(status {self.S.cm.status}, minor {self.Lf.contents.minor})")
        self.factorizations += 1
        self._values, self._key, self._fact = values, (values.data_ptr(), values._version, beta), self._count()

    def _ensure(self, values):
        """the factor of `values`: reused when `values` is the tensor factorized last, unchanged, and Lf still holds it"""
        values = values.detach()
        if self._key != (values.data_ptr(), values._version, self._beta_value()) or self._count() != self._fact:
            self._factorize(values)
        return self._fact

    def _restore(self, values, fact):
        """a backward pass whose factor was replaced since its forward factorizes again from the values it saved"""
        return fact if self._count() == fact else self._ensure(values)

    def _multiplier(self, device):
        """1 on the diagonal, 2 off it, 0 where A is not read (the ignored triangle)"""
        if self._mult is None or self._mult.device != device:
            a = self.A.contents
            n = int(a.ncol)
            Ap = ch._view(a.p, n + 1, C.c_int64, np.int64)
            Ai = ch._view(a.i, int(Ap[-1]), C.c_int64, np.int64)
            cols = np.repeat(np.arange(n, dtype=np.int64), np.diff(Ap))
            read = (Ai >= cols) if a.stype < 0 else (Ai <= cols)
            m = np.where(read, np.where(Ai == cols, 1.0, 2.0), 0.0)
            self._mult = torch.from_numpy(m).to(device)
        return self._mult

    # ---- the differentiable functions
    def solve(self, values, B):
        """X = M^-1 B; B of shape (nrhs, n) or (n,), rows are right-hand sides (Session.solve_device)"""
        return _Solve.apply(self, values, B, self._beta_input())

    def logdet(self, values):
        """log det M as a 0-dim device tensor"""
        return _LogDet.apply(self, values, self._beta_input())

    def solve_Lt(self, values, Z):
        """X = P' L^-T Z with L L' = P M P'; Z of shape (nrhs, n) or (n,), rows are right-hand sides.  For Z ~ N (0, I) the
        rows of X are samples from N (0, M^-1).  A symmetric A (stype != 0) only."""
        if self.aat:
            raise NotImplementedError("DeviceCholesky.solve_Lt: A*A' input (stype == 0) is not supported")
        return _SolveFactor.apply(self, values, Z, self._beta_input(), True)

    def solve_L(self, values, B):
        """Y = L^-1 P B with L L' = P M P': whitening, |Y|^2 = B' M^-1 B; B as for `solve_Lt`.  A symmetric A only."""
        if self.aat:
            raise NotImplementedError("DeviceCholesky.solve_L: A*A' input (stype == 0) is not supported")
        return _SolveFactor.apply(self, values, B, self._beta_input(), False)


class _SolveFactor(torch.autograd.Function):
    """transposed: P' L^-T Z, else L^-1 P B"""

    @staticmethod
    def forward(ctx, chol, values, B, beta, transposed):
        ctx.chol, ctx.fact, ctx.transposed = chol, chol._ensure(values), transposed
        ctx.beta_device = None if beta is None else beta.device
        S, Lf = chol.S, chol.Lf
        B = B.detach().contiguous()
        if transposed:
            inner = S.solve_device(Lf, B, ch.SYS_Lt)            # Xt, the factor's ordering
            out = S.solve_device(Lf, inner, ch.SYS_Pt)
        else:
            out = inner = S.solve_device(Lf, S.solve_device(Lf, B, ch.SYS_P), ch.SYS_L)
        ctx.save_for_backward(values, inner)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        chol = ctx.chol
        values, inner = ctx.saved_tensors
        need_v, need_b, need_beta = ctx.needs_input_grad[1:4]
        if not (need_v or need_b or need_beta):
            return None, None, None, None, None
        chol._restore(values, ctx.fact)
        S, Lf = chol.S, chol.Lf
        g = g.contiguous()
        if ctx.transposed:
            gb = other = S.solve_device(Lf, S.solve_device(Lf, g, ch.SYS_P), ch.SYS_L)      # U = L^-1 P gX
            P, Q = inner, other                                                             # Lbar = -tril (Xt U')
        else:
            other = S.solve_device(Lf, g, ch.SYS_Lt)                                        # V = L^-T gY
            gb = S.solve_device(Lf, other, ch.SYS_Pt)
            P, Q = other, inner                                                             # Lbar = -tril (V Y')
        gv = gbeta = None
        if need_v or need_beta:
            gv, tr = S.factor_outer_grad_device(chol.A, Lf, P, Q, alpha=-1.0)
            gbeta = tr.to(ctx.beta_device) if need_beta else None
        return None, (gv if need_v else None), (gb if need_b else None), gbeta, None


class _Solve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, chol, values, B, beta):
        ctx.chol, ctx.fact = chol, chol._ensure(values)
        ctx.beta_device = None if beta is None else beta.device
        X = chol.S.solve_device(chol.Lf, B.detach().contiguous())
        ctx.save_for_backward(values, X)
        return X

    @staticmethod
    @once_differentiable
    def backward(ctx, gX):
        chol = ctx.chol
        values, X = ctx.saved_tensors
        need_v, need_b, need_beta = ctx.needs_input_grad[1:4]
        if not (need_v or need_b or need_beta):
            return None, None, None, None
        chol._restore(values, ctx.fact)
        lam = chol.S.solve_device(chol.Lf, gX.contiguous())
        gv = None
        if need_v and chol.aat:
            gv = chol.S.aat_values_grad_device(chol.A, chol.Lf, values.detach(), lam, X, alpha=-1.0)
        elif need_v:
            gv = chol.S.values_grad_device(chol.A, chol.Lf, lam, X, alpha=-1.0)
        gbeta = (-(lam * X).sum()).to(ctx.beta_device) if need_beta else None
        return None, gv, (lam if need_b else None), gbeta


class _LogDet(torch.autograd.Function):
    @staticmethod
    def forward(ctx, chol, values, beta):
        ctx.chol, ctx.fact = chol, chol._ensure(values)
        ctx.beta_device = None if beta is None else beta.device
        ctx.save_for_backward(values)
        return chol.S.logdet_device(chol.Lf)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        chol = ctx.chol
        (values,) = ctx.saved_tensors
        need_v, need_beta = ctx.needs_input_grad[1:3]
        if not (need_v or need_beta):
            return None, None, None
        chol._restore(values, ctx.fact)
        gv = gbeta = None
        if need_v and chol.aat:
            gv = g * chol.S.aat_logdet_grad_device(chol.A, chol.Lf, values.detach())
        elif need_v:
            Z, _ = chol.S.selinv_device(chol.A, chol.Lf, diag=False)
            Z = torch.where(torch.isnan(Z), torch.zeros_like(Z), Z)
            gv = g * chol._multiplier(Z.device) * Z
        if need_beta:
            gbeta = (g * chol.S.selinv_device(None, chol.Lf, values=False, diag=True)[1].sum()).to(ctx.beta_device)
        return None, gv, gbeta
