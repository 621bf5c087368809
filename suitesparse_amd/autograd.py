"""torch.autograd through the device-resident Cholesky path: a solve and a log-determinant whose backward passes stay on
the device and on torch's current stream.

    chol = DeviceCholesky(session, A, Lf, beta=0.0)
    X = chol.solve(values, B)           # (A (values) + beta I)^-1 B; differentiable in values and B
    ld = chol.logdet(values)            # log det (A (values) + beta I); differentiable in values

`A` gives the pattern, `values` (a 1-D torch.float64 device tensor of length nnz (A), A's entry order) the numbers, `Lf` is a
factor that was factorized once from a host matrix of A's pattern -- the precondition of Session.factorize_device.

With X = M^-1 B, M = A + beta I, and an incoming gradient gX:  Lambda = M^-1 gX  is the gradient with respect to B, and
-(Lambda X' + X Lambda') sampled on the entries of A the factorization reads (Session.values_grad_device) the one with
respect to the values; a value the factorization does not read (the ignored triangle of a symmetric A) has gradient zero.
The gradient of log det M with respect to the value at (i, j) is Z_ii on the diagonal and 2 Z_ij off it, Z = M^-1 from
Session.selinv_device.

The wrapper OWNS Lf: a factorization of Lf behind its back is detected (the engine counts factorizations,
cholmod_hip_progress out [0]) and answered by factorizing again from the values a backward pass saved, but values handed to
Session.factorize_device directly are not seen by `solve` / `logdet` calls that follow with the tensor factorized last.
beta is a Python float and is not differentiated; both functions are differentiable once; real factors, one rank."""
import ctypes as C

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import cholmod as ch


class DeviceCholesky:
    def __init__(self, session, A, Lf, beta=0.0):
        self.S, self.A, self.Lf, self.beta = session, A, Lf, float(beta)
        self._values = None         # the tensor factorized last (kept alive: its address cannot be handed out again)
        self._key = None            # (data_ptr, _version, beta) of that factorization
        self._fact = -1             # the engine's count of factorizations right after it
        self._mult = None
        self.factorizations = 0     # ... and the wrapper's own

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
        ok = self.S.factorize_device(self.A, values, self.Lf, self.beta)
        if not ok or self.S.cm.status != ch.OK or self.Lf.contents.minor < self.Lf.contents.n:
            raise RuntimeError(f"DeviceCholesky: the matrix is not positive definite or the factorization failed "
                               f"(status {self.S.cm.status}, minor {self.Lf.contents.minor})")
        self.factorizations += 1
        self._values, self._key, self._fact = values, (values.data_ptr(), values._version, self.beta), self._count()

    def _ensure(self, values):
        """the factor of `values`: reused when `values` is the tensor factorized last, unchanged, and Lf still holds it"""
        values = values.detach()
        if self._key != (values.data_ptr(), values._version, self.beta) or self._count() != self._fact:
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
        """X = (A (values) + beta I)^-1 B; B of shape (nrhs, n) or (n,), rows are right-hand sides (Session.solve_device)"""
        return _Solve.apply(self, values, B)

    def logdet(self, values):
        """log det (A (values) + beta I) as a 0-dim device tensor"""
        return _LogDet.apply(self, values)


class _Solve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, chol, values, B):
        ctx.chol, ctx.fact = chol, chol._ensure(values)
        X = chol.S.solve_device(chol.Lf, B.detach().contiguous())
        ctx.save_for_backward(values, X)
        return X

    @staticmethod
    @once_differentiable
    def backward(ctx, gX):
        chol = ctx.chol
        values, X = ctx.saved_tensors
        need_v, need_b = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if not (need_v or need_b):
            return None, None, None
        chol._restore(values, ctx.fact)
        lam = chol.S.solve_device(chol.Lf, gX.contiguous())
        gv = chol.S.values_grad_device(chol.A, chol.Lf, lam, X, alpha=-1.0) if need_v else None
        return None, gv, (lam if need_b else None)


class _LogDet(torch.autograd.Function):
    @staticmethod
    def forward(ctx, chol, values):
        ctx.chol, ctx.fact = chol, chol._ensure(values)
        ctx.save_for_backward(values)
        return chol.S.logdet_device(chol.Lf)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        chol = ctx.chol
        (values,) = ctx.saved_tensors
        if not ctx.needs_input_grad[1]:
            return None, None
        chol._restore(values, ctx.fact)
        Z, _ = chol.S.selinv_device(chol.A, chol.Lf, diag=False)
        Z = torch.where(torch.isnan(Z), torch.zeros_like(Z), Z)
        return None, g * chol._multiplier(Z.device) * Z
