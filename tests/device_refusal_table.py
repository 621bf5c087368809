"""The table of refusals of the device-resident entry points of the host layer: every cholmod_l_hip_* function that takes
device pointers or reads the resident factor, called on a CPU-path factor (integers stand in for device pointers: nothing
here may dereference them) with one fault or two at a time -- the pairs pin the ORDER of the checks.  A row is
(return value, Common->status, the messages handed to Common->error_handler); file and line are not part of it.

A CPU-path factor never passes "L was not factorized on the device", so every row is a refusal and no device is touched:
the table runs, and gives the same rows, with and without a GPU.  (cholmod_l_hip_solve_device alone would upload a host
factor: its rows all keep Common->useGPU = 0, which it refuses before that.)

tests/test_device_refusals.py compares rows () with tests/golden/device_refusals.json, tools/record_device_refusals.py
writes that file."""
import ctypes as C
import itertools

import numpy as np

import aat_grad_matrices as AM
import schur_reference as R
from suitesparse_amd import cholmod as ch

M = 5                       # the m of the Schur entries
P = ("ptr",)                # a device pointer: an integer stands in; fault: NULL
LDN, LDM = ("ldn",), ("ldm",)   # a leading dimension, at least n / at least m; fault: one too small


# entry -> (which factor, the arguments in C order as (name, kind)); "A", "L", "stream", "cm" are filled in by call ()
ENTRIES = {
    "cholmod_l_hip_solve_device": ("real", (("sys", "sys"), "L", ("B", P), ("ldb", LDN), ("X", P), ("ldx", LDN),
                                                 ("nrhs", "nrhs"), "stream", "cm")),
    "cholmod_l_hip_residual_device": ("real", ("L", ("X", P), ("ldx", LDN), ("B", P), ("ldb", LDN), ("R", P), ("ldr", LDN),
                                                    ("nrhs", "nrhs"), ("Rnorm", P), "stream", "cm")),
    "cholmod_l_hip_refine_device": ("real", ("L", ("B", P), ("ldb", LDN), ("X", P), ("ldx", LDN), ("nrhs", "nrhs"),
                                                  ("steps", "steps"), ("Rnorm", P), "stream", "cm")),
    "cholmod_l_hip_solve_device_complex": ("complex", (("sys", "sys"), "L", ("B", P), ("ldb", LDN), ("X", P), ("ldx", LDN),
                                                            ("nrhs", "nrhs"), "stream", "cm")),
    "cholmod_l_hip_residual_device_complex": ("complex", ("L", ("X", P), ("ldx", LDN), ("B", P), ("ldb", LDN), ("R", P),
                                                               ("ldr", LDN), ("nrhs", "nrhs"), ("Rnorm", P), "stream", "cm")),
    "cholmod_l_hip_refine_device_complex": ("complex", ("L", ("B", P), ("ldb", LDN), ("X", P), ("ldx", LDN), ("nrhs", "nrhs"),
                                                             ("steps", "steps"), ("Rnorm", P), "stream", "cm")),
    "cholmod_l_hip_factorize_values_device": ("real", ("A", ("Ax", P), ("beta", "beta"), "L", "stream", "cm")),
    "cholmod_l_hip_selinv_device": ("real", ("A", "L", ("Z", P), ("diag", P), "stream", "cm")),
    "cholmod_l_hip_selinv_to_host": ("real", ("L", ("Zx", P), "cm")),
    "cholmod_l_hip_values_grad_device": ("real", ("A", "L", ("alpha", "val"), ("U", P), ("ldu", LDN), ("V", P), ("ldv", LDN),
                                                       ("nrhs", "nrhs"), ("G", P), "stream", "cm")),
    "cholmod_l_hip_logdet_device": ("real", ("L", ("out", P), "stream", "cm")),
    "cholmod_l_hip_aat_values_grad_device": ("aat", ("A", "L", ("alpha", "val"), ("U", P), ("ldu", LDN), ("V", P), ("ldv", LDN),
                                                          ("nrhs", "nrhs"), ("Avalues", P), ("G", P), "stream", "cm")),
    "cholmod_l_hip_aat_logdet_grad_device": ("aat", ("A", "L", ("Avalues", P), ("G", P), "stream", "cm")),
    "cholmod_l_hip_factor_grad_device": ("real", ("A", "L", ("Lbar", P), ("G", P), ("trace", P), "stream", "cm")),
    "cholmod_l_hip_factor_outer_grad_device": ("real", ("A", "L", ("alpha", "val"), ("P", P), ("ldp", LDN), ("Q", P),
                                                             ("ldq", LDN), ("nrhs", "nrhs"), ("G", P), ("trace", P), "stream", "cm")),
    "cholmod_l_hip_factor_grad_to_host": ("real", ("L", ("Gx", P), "cm")),
    "cholmod_l_hip_schur_device": ("real", ("L", ("m", "m"), ("S", P), ("lds", LDM), ("F", P), ("ldf", LDM), "stream", "cm")),
    "cholmod_l_hip_schur_reduce_device": ("real", ("L", ("m", "m"), ("B", P), ("ldb", LDN), ("Y", P), ("ldy", LDN), ("G", P),
                                                        ("ldg", LDM), ("nrhs", "nrhs"), "stream", "cm")),
    "cholmod_l_hip_schur_expand_device": ("real", ("L", ("m", "m"), ("Y", P), ("ldy", LDN), ("XS", P), ("ldxs", LDM), ("X", P),
                                                        ("ldx", LDN), ("nrhs", "nrhs"), "stream", "cm")),
}
# outputs that must not alias an input: (entry suffix, output, input)
ALIASES = (("residual_device", "R", "X"), ("residual_device_complex", "R", "X"), ("schur_expand_device", "X", "Y"))


class Factors:
    """The three CPU-path factors of the table: p3d_12_nd (real), the same pattern with Hermitian values (complex) and the
    engineered unsymmetric matrix, factorized as A*A' (aat).  Every error lands in self.messages."""

    def __init__(self):
        self.messages = []
        self._cb = ch.ERRFUNC(lambda status, file, line, msg: self.messages.append((msg or b"").decode()))
        case = R.CASES["p3d_12_nd"]()
        n, Lp, Li, Lx = case["n"], case["Lp"], case["Li"], case["Lx"]
        cols = np.repeat(np.arange(n), np.diff(Lp))
        Lz = np.where(Li == cols, Lx, 0.9 * Lx * np.exp(1j * np.arange(len(Lx)))).astype(np.complex128)
        self.of = {}
        for kind, vals in (("real", Lx), ("complex", Lz)):
            S = ch.Session(use_gpu=0)
            A = S.sparse(n, Lp, Li, vals, -1)
            Lf = S.analyze(A, case["perm"])
            assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
            assert Lf.contents.xtype == (ch.COMPLEX if kind == "complex" else ch.REAL)
            self.of[kind] = (S, A, Lf)
        Mu = AM.engineered()
        S = ch.Session(use_gpu=0, ordering="default")
        A = S.L.cholmod_l_allocate_sparse(Mu.shape[0], Mu.shape[1], Mu.nnz, 1, 1, 0, ch.REAL, C.byref(S.cm))
        ch._view(A.contents.p, Mu.shape[1] + 1, C.c_int64, np.int64)[:] = Mu.indptr
        ch._view(A.contents.i, Mu.nnz, C.c_int64, np.int64)[:] = Mu.indices
        ch._view(A.contents.x, Mu.nnz, C.c_double, np.float64)[:] = Mu.data
        Lf = S.L.cholmod_l_analyze(A, C.byref(S.cm))
        assert Lf and S.factorize(A, Lf, 0.375) == 1 and S.cm.status == ch.OK
        self.of["aat"] = (S, A, Lf)
        for S, A, Lf in self.of.values():
            assert not Lf.contents.hip_plan and Lf.contents.is_super     # the CPU path: nothing on a device
            S.cm.error_handler = self._cb

    def close(self):
        for S, A, Lf in self.of.values():
            S.cm.error_handler = ch.ERRFUNC(0)
            S.free_factor(Lf)
            S.free_sparse(A)
            S.finish()


def _set(target, field, value):
    return lambda st: st[target].__setitem__(field, value)


def faults_of(entry, kind, spec, n):
    """-> [(label, the (target, field) keys it writes, what it does to a state)]; two faults that write the same key are not
    paired"""
    out = []

    def add(label, *writes):
        out.append((label, {(t, f) for t, f, _ in writes}, [_set(t, f, v) for t, f, v in writes]))

    has_A = "A" in spec
    for a in spec:
        if a == "L" or a == "A":
            add(f"{a}=NULL", ("args", a, None))
        if isinstance(a, str):
            continue
        name, k = a
        if k == P:
            add(f"{name}=NULL", ("args", name, None))
        elif k == LDN:
            add(f"{name}=n-1", ("args", name, n - 1))
        elif k == LDM:
            add(f"{name}=m-1", ("args", name, M - 1))
        elif k == "m":
            add("m=n+1", ("args", "m", n + 1))
            add("m=0", ("args", "m", 0))
        elif k == "nrhs":
            add("nrhs=0", ("args", "nrhs", 0))
        elif k == "sys":
            add("sys=-1", ("args", "sys", -1))
            add("sys=9", ("args", "sys", 9))
        elif k == "steps":
            add("steps=-1", ("args", "steps", -1))
        elif k == "beta":
            add("beta=NULL", ("args", "beta", None))
    for suffix, o, i in ALIASES:
        if entry.endswith("hip_" + suffix):
            out.append((f"{o}=={i}", {("args", o)}, [lambda st, o=o, i=i: st["args"].__setitem__(o, st["args"][i])]))
    for label, xt in (("L real", ch.REAL), ("L complex", ch.COMPLEX), ("L zomplex", ch.ZOMPLEX), ("L pattern", ch.PATTERN)):
        if xt != (ch.COMPLEX if kind == "complex" else ch.REAL):
            add(label, ("L", "xtype", xt))
    add("L simplicial", ("L", "is_super", 0))
    add("L.minor=n-1", ("L", "minor", n - 1))
    if entry != "cholmod_l_hip_solve_device":       # (its rows all keep useGPU = 0: see the module's docstring)
        add("useGPU=0", ("cm", "useGPU", 0), ("cm", "hip_cpu_fallback", 0))
    add("useGPU=0 with hip_cpu_fallback", ("cm", "useGPU", 0), ("cm", "hip_cpu_fallback", 1))
    add("hip_world=2", ("cm", "hip_world", 2))
    if has_A:
        add("A complex", ("A", "xtype", ch.COMPLEX))
        add("A stype", ("A", "stype", -1 if kind == "aat" else 0))
        add("A unpacked", ("A", "packed", 0))
        add("A.nrow-1", ("A", "nrow", n - 1))
        add("A.i=NULL", ("A", "i", None))
    return out


def _defaults(entry, spec, n):
    args, k = {}, 0
    for a in spec:
        if isinstance(a, str):
            continue
        name, kind = a
        if kind == P:
            k += 1
            args[name] = 0x1000 * k
        else:
            args[name] = {LDN: n, LDM: M, "m": M, "nrhs": 3, "sys": ch.SYS_A, "steps": 2, "val": -1.0,
                          "beta": (C.c_double * 2)(0.25, 0.0)}[kind]
    return args


def _call(F, entry, kind, spec, state):
    S, A, Lf = F.of[kind]
    saved = []
    for target, obj in (("L", Lf.contents), ("A", A.contents), ("cm", S.cm)):
        for field, value in state[target].items():
            saved.append((obj, field, getattr(obj, field)))
            setattr(obj, field, value)
    S.cm.status = ch.OK
    del F.messages[:]
    argv = []
    for a in spec:
        if a == "cm":
            argv.append(C.byref(S.cm))
        elif a == "stream":
            argv.append(None)
        elif a in ("A", "L"):
            argv.append(state["args"].get(a, A if a == "A" else Lf))
        else:
            argv.append(state["args"][a[0]])
    ret = getattr(S.L, entry)(*argv)
    status = S.cm.status
    for obj, field, value in reversed(saved):
        setattr(obj, field, value)
    assert ret == 0, (entry, state)                 # every row is a refusal: nothing may get as far as a device
    return [ret, status, " | ".join(F.messages)]


def rows():
    """-> {entry: {label: [return value, Common->status, message]}}: no fault ("-"), every fault, every pair of faults"""
    F = Factors()
    table = {}
    for entry, (kind, spec) in ENTRIES.items():
        S, A, Lf = F.of[kind]
        n = int(Lf.contents.n)
        faults = faults_of(entry, kind, spec, n)
        base_cm = {"useGPU": 0 if entry == "cholmod_l_hip_solve_device" else 1, "hip_cpu_fallback": 0, "hip_world": 1}
        combos = [()] + [(f,) for f in faults] + [c for c in itertools.combinations(faults, 2) if not (c[0][1] & c[1][1])]
        t = table[entry] = {}
        for combo in combos:
            state = {"args": _defaults(entry, spec, n), "L": {}, "A": {}, "cm": dict(base_cm)}
            for _, _, writes in combo:
                for w in writes:
                    w(state)
            t[" + ".join(f[0] for f in combo) or "-"] = _call(F, entry, kind, spec, state)
    F.close()
    return table


def pack(table):
    """the table as it is stored: the messages once, the rows by index"""
    messages = sorted({r[2] for t in table.values() for r in t.values()})
    at = {m: k for k, m in enumerate(messages)}
    return {"messages": messages, "rows": {e: {label: [r[0], r[1], at[r[2]]] for label, r in t.items()} for e, t in table.items()}}


def unpack(stored):
    msg = stored["messages"]
    return {e: {label: [r[0], r[1], msg[r[2]]] for label, r in t.items()} for e, t in stored["rows"].items()}
