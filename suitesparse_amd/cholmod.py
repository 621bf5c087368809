"""ctypes binding of libcholmod_amd.so -- the host-side mirror of the reference's
cholmod_l_* C API (include/cholmod.h) plus the engine shim (include/cholmod_hip.h).

This module is plumbing for tests and bench.py: it declares the C structs,
loads the in-tree shared library and fails loudly if it is missing.  All
numeric work happens in the library (HIP engine); nothing here computes.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CHOLMOD_AMD_LIB") or os.path.join(_HERE, "lib", "libcholmod_amd.so")   # (override: A/B builds while tuning)
# the same library with the engine's test hooks compiled in (CHOLMOD_HIP_TEST_*): tests only, see csrc/Makefile
HOOKS_LIB_PATH = os.path.join(_HERE, "lib", "libcholmod_amd_testhooks.so")
CSRC = os.path.join(_HERE, "csrc")

CHOLMOD_MAXMETHODS = 9
CHOLMOD_HIP_NSTATS = 41

# constants (include/cholmod.h)
PATTERN, REAL, COMPLEX, ZOMPLEX = 0, 1, 2, 3
OK, NOT_INSTALLED, OUT_OF_MEMORY, TOO_LARGE, INVALID, GPU_PROBLEM = 0, -1, -2, -3, -4, -5
NOT_POSDEF = 1
NATURAL, GIVEN, POSTORDERED = 0, 1, 6
SIMPLICIAL, AUTO, SUPERNODAL = 0, 1, 2
SYS_A, SYS_LDLt, SYS_LD, SYS_DLt, SYS_L, SYS_Lt, SYS_D, SYS_P, SYS_Pt = range(9)
HIP_PLAN_HOST_ONLY = 2
# plan flags (include/cholmod_hip.h)
HIP_WIDE_OB, HIP_NO_FUSED_POTRF, HIP_NO_FUSED_TRSM, HIP_PHI_TWIN = 128, 512, 1024, 16384
HIP_NO_SMALL_FRONTS = 16
HIP_FUSED_CB_EA = 65536
HIP_OK = 0
HIP_INVALID = -4
HIP_NO_DEVICE = -1


class Method(C.Structure):
    _fields_ = [("lnz", C.c_double), ("fl", C.c_double), ("ordering", C.c_int)]


ERRFUNC = C.CFUNCTYPE(None, C.c_int, C.c_char_p, C.c_int, C.c_char_p)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p)


class Common(C.Structure):
    _fields_ = [
        ("supernodal", C.c_int), ("supernodal_switch", C.c_double),
        ("final_asis", C.c_int), ("final_super", C.c_int), ("final_ll", C.c_int),
        ("final_pack", C.c_int), ("final_monotonic", C.c_int), ("final_resymbol", C.c_int),
        ("zrelax", C.c_double * 3), ("nrelax", C.c_size_t * 3),
        ("prefer_upper", C.c_int), ("quick_return_if_not_posdef", C.c_int),
        ("print", C.c_int), ("nmethods", C.c_int), ("current", C.c_int), ("selected", C.c_int),
        ("method", Method * (CHOLMOD_MAXMETHODS + 1)),
        ("postorder", C.c_int), ("try_catch", C.c_int),
        ("error_handler", ERRFUNC),
        ("itype", C.c_int), ("dtype", C.c_int), ("status", C.c_int),
        ("fl", C.c_double), ("lnz", C.c_double), ("anz", C.c_double), ("modfl", C.c_double),
        ("malloc_count", C.c_size_t), ("memory_usage", C.c_size_t), ("memory_inuse", C.c_size_t),
        ("nrealloc_col", C.c_double), ("nrealloc_factor", C.c_double), ("ndbounds_hit", C.c_double),
        ("rowfacfl", C.c_double), ("aatfl", C.c_double),
        ("called_nd", C.c_int), ("blas_ok", C.c_int),
        ("useGPU", C.c_int), ("maxGpuMemBytes", C.c_size_t), ("maxGpuMemFraction", C.c_double),
        ("gpuMemorySize", C.c_size_t), ("gpuKernelTime", C.c_double), ("gpuFlops", C.c_int64),
        ("gpuNumKernelLaunches", C.c_int), ("devBuffSize", C.c_size_t), ("ibuffer", C.c_int),
        ("syrkStart", C.c_double),
        ("cholmod_cpu_gemm_time", C.c_double), ("cholmod_cpu_syrk_time", C.c_double),
        ("cholmod_cpu_trsm_time", C.c_double), ("cholmod_cpu_potrf_time", C.c_double),
        ("cholmod_gpu_gemm_time", C.c_double), ("cholmod_gpu_syrk_time", C.c_double),
        ("cholmod_gpu_trsm_time", C.c_double), ("cholmod_gpu_potrf_time", C.c_double),
        ("cholmod_assemble_time", C.c_double), ("cholmod_assemble_time2", C.c_double),
        ("cholmod_cpu_gemm_calls", C.c_size_t), ("cholmod_cpu_syrk_calls", C.c_size_t),
        ("cholmod_cpu_trsm_calls", C.c_size_t), ("cholmod_cpu_potrf_calls", C.c_size_t),
        ("cholmod_gpu_gemm_calls", C.c_size_t), ("cholmod_gpu_syrk_calls", C.c_size_t),
        ("cholmod_gpu_trsm_calls", C.c_size_t), ("cholmod_gpu_potrf_calls", C.c_size_t),
        ("hip_factor_on_device", C.c_int), ("hip_flags", C.c_int), ("hip_profile", C.c_int),
        ("hip_rank", C.c_int), ("hip_world", C.c_int),
        ("hip_allreduce", C.c_void_p), ("hip_allreduce_user", C.c_void_p),
        ("hip_cpu_fallback", C.c_int), ("prefer_zomplex", C.c_int), ("prefer_binary", C.c_int),
        ("hip_lazy_plan", C.c_int), ("hip_plan_seconds", C.c_double),
    ]


class Sparse(C.Structure):
    _fields_ = [("nrow", C.c_size_t), ("ncol", C.c_size_t), ("nzmax", C.c_size_t),
                ("p", C.c_void_p), ("i", C.c_void_p), ("nz", C.c_void_p), ("x", C.c_void_p),
                ("z", C.c_void_p), ("stype", C.c_int), ("itype", C.c_int), ("xtype", C.c_int),
                ("dtype", C.c_int), ("sorted", C.c_int), ("packed", C.c_int)]


class Triplet(C.Structure):
    _fields_ = [("nrow", C.c_size_t), ("ncol", C.c_size_t), ("nzmax", C.c_size_t), ("nnz", C.c_size_t),
                ("i", C.c_void_p), ("j", C.c_void_p), ("x", C.c_void_p), ("z", C.c_void_p),
                ("stype", C.c_int), ("itype", C.c_int), ("xtype", C.c_int), ("dtype", C.c_int)]


class Dense(C.Structure):
    _fields_ = [("nrow", C.c_size_t), ("ncol", C.c_size_t), ("nzmax", C.c_size_t),
                ("d", C.c_size_t), ("x", C.c_void_p), ("z", C.c_void_p),
                ("xtype", C.c_int), ("dtype", C.c_int)]


class Factor(C.Structure):
    _fields_ = [("n", C.c_size_t), ("minor", C.c_size_t),
                ("Perm", C.c_void_p), ("ColCount", C.c_void_p), ("IPerm", C.c_void_p),
                ("nzmax", C.c_size_t),
                ("p", C.c_void_p), ("i", C.c_void_p), ("x", C.c_void_p), ("z", C.c_void_p),
                ("nz", C.c_void_p), ("next", C.c_void_p), ("prev", C.c_void_p),
                ("nsuper", C.c_size_t), ("ssize", C.c_size_t), ("xsize", C.c_size_t),
                ("maxcsize", C.c_size_t), ("maxesize", C.c_size_t),
                ("super", C.c_void_p), ("pi", C.c_void_p), ("px", C.c_void_p), ("s", C.c_void_p),
                ("ordering", C.c_int), ("is_ll", C.c_int), ("is_super", C.c_int),
                ("is_monotonic", C.c_int), ("itype", C.c_int), ("xtype", C.c_int),
                ("dtype", C.c_int), ("useGPU", C.c_int),
                ("hip_plan", C.c_void_p), ("hip_on_device", C.c_int), ("hip_host_valid", C.c_int),
                ("cx_twin", C.c_void_p), ("hip_apat_hash", C.c_uint64), ("hip_apat_nnz", C.c_size_t),
                ("hip_apat_valid", C.c_int), ("hip_apat_hash2", C.c_uint64), ("hip_is_twin", C.c_int),
                ("bset_work", C.c_void_p), ("hip_plan_ahead", C.c_int), ("hip_perm_set", C.c_int),
                ("hip_aat_hash", C.c_uint64), ("hip_aat_hash2", C.c_uint64), ("hip_aat_nnz", C.c_size_t),
                ("hip_aat_valid", C.c_int)]


# every symbol include/cholmod.h and include/cholmod_hip.h declare
API_SYMBOLS = [
    "cholmod_l_start", "cholmod_l_finish", "cholmod_l_defaults", "cholmod_l_error",
    "cholmod_l_malloc", "cholmod_l_calloc", "cholmod_l_free",
    "cholmod_l_allocate_sparse", "cholmod_l_free_sparse", "cholmod_l_copy_sparse",
    "cholmod_l_nnz", "cholmod_l_ptranspose", "cholmod_l_transpose",
    "cholmod_l_allocate_triplet", "cholmod_l_free_triplet", "cholmod_l_triplet_to_sparse",
    "cholmod_l_allocate_dense", "cholmod_l_zeros", "cholmod_l_ones", "cholmod_l_copy_dense",
    "cholmod_l_free_dense", "cholmod_l_free_factor",
    "cholmod_l_read_sparse", "cholmod_l_read_triplet", "cholmod_l_read_dense", "cholmod_l_read_matrix", "cholmod_l_check_factor", "cholmod_l_check_sparse",
    "cholmod_gpu_memorysize", "cholmod_gpu_probe", "cholmod_gpu_deallocate", "cholmod_gpu_end", "cholmod_gpu_allocate",
    "cholmod_l_gpu_stats", "cholmod_l_sdmult", "cholmod_l_norm_dense", "cholmod_l_norm_sparse",
    "cholmod_l_analyze", "cholmod_l_analyze_p", "cholmod_l_analyze_p2",
    "cholmod_l_factorize", "cholmod_l_factorize_p", "cholmod_l_solve", "cholmod_l_solve2",
    "cholmod_l_rcond", "cholmod_l_change_factor", "cholmod_l_realloc",
    "SuiteSparse_start", "SuiteSparse_finish", "SuiteSparse_malloc", "SuiteSparse_calloc", "SuiteSparse_realloc", "SuiteSparse_free",
    "cholmod_l_etree", "cholmod_l_postorder", "cholmod_l_rowcolcounts",
    "cholmod_l_super_symbolic", "cholmod_l_super_symbolic2", "cholmod_l_super_numeric",
    "cholmod_l_super_lsolve", "cholmod_l_super_ltsolve",
    "cholmod_l_gpu_memorysize", "cholmod_l_gpu_probe", "cholmod_l_gpu_deallocate",
    "cholmod_l_gpu_end", "cholmod_l_gpu_allocate",
    "cholmod_l_factor_to_host", "cholmod_l_hip_stats", "cholmod_l_refactorize_resident",
    "cholmod_l_gather_factor", "cholmod_l_hip_prepare", "cholmod_l_hip_front_reach",
    "cholmod_l_hip_solve_device", "cholmod_l_hip_residual_device", "cholmod_l_hip_refine_device",
    "cholmod_l_hip_solve_device_complex", "cholmod_l_hip_residual_device_complex", "cholmod_l_hip_refine_device_complex",
    "cholmod_l_hip_factorize_values_device", "cholmod_l_hip_aat_product_map",
    "cholmod_l_hip_selinv_device", "cholmod_l_hip_selinv_to_host",
    "cholmod_l_hip_schur_device", "cholmod_l_hip_schur_reduce_device", "cholmod_l_hip_schur_expand_device",
    "cholmod_l_hip_values_grad_device", "cholmod_l_hip_logdet_device",
    "cholmod_l_hip_aat_values_grad_device", "cholmod_l_hip_aat_logdet_grad_device",
    "cholmod_l_hip_factor_grad_device", "cholmod_l_hip_factor_outer_grad_device", "cholmod_l_hip_factor_grad_to_host",
]
HIP_SYMBOLS = [
    "cholmod_hip_probe", "cholmod_hip_memorysize", "cholmod_hip_set_device", "cholmod_hip_device_count",
    "cholmod_hip_plan_create", "cholmod_hip_plan_destroy", "cholmod_hip_factorize",
    "cholmod_hip_plan_create_dist", "cholmod_hip_plan_create_reach", "cholmod_hip_set_allreduce", "cholmod_hip_get_partition",
    "cholmod_hip_get_groups", "cholmod_hip_get_batches", "cholmod_hip_progress_enable", "cholmod_hip_progress", "cholmod_hip_debug_schedule_hash", "cholmod_hip_diag_minmax", "cholmod_hip_values_begin", "cholmod_hip_values_push_chunk", "cholmod_hip_debug_routing",
    "cholmod_hip_gather_factor",
    "cholmod_hip_upload_matrix", "cholmod_hip_factorize_resident",
    "cholmod_hip_set_value_map",
    "cholmod_hip_factorize_values_device", "cholmod_hip_set_product_map", "cholmod_hip_download_matrix_values",
    "cholmod_hip_download_factor", "cholmod_hip_download_even_columns", "cholmod_hip_upload_factor", "cholmod_hip_solve",
    "cholmod_hip_set_perm", "cholmod_hip_solve_device", "cholmod_hip_residual_device", "cholmod_hip_refine_device",
    "cholmod_hip_get_maps", "cholmod_hip_get_stats", "cholmod_hip_set_profiling",
    "cholmod_hip_selinv_device", "cholmod_hip_selinv_gather_device", "cholmod_hip_selinv_download",
    "cholmod_hip_selinv_release", "cholmod_hip_selinv_info",
    "cholmod_hip_schur_device", "cholmod_hip_trailing_multiply_device",
    "cholmod_hip_factor_grad_device", "cholmod_hip_factor_outer_grad_device", "cholmod_hip_factor_grad_gather_device",
    "cholmod_hip_factor_grad_download", "cholmod_hip_factor_grad_release", "cholmod_hip_factor_grad_info",
    "cholmod_hip_values_grad_device", "cholmod_hip_logdet_device",
    "cholmod_hip_product_values_grad_device", "cholmod_hip_product_logdet_grad_device",
    "cholmod_hip_dense_partial_factor", "cholmod_hip_factor_checks", "cholmod_hip_factor_checks_local", "cholmod_hip_get_launch_profile", "cholmod_hip_debug_thin_cycles", "cholmod_hip_debug_launch_regions",
    "cholmod_hip_debug_cb_extend_add", "cholmod_hip_debug_fused_pair",
    "cholmod_hip_rccl_unique_id", "cholmod_hip_rccl_attach", "cholmod_hip_rccl_detach",
    "cholmod_hip_version",
]

PROBES_PATH = os.path.join(_HERE, "lib", "libcholmod_amd_probes.so")
PROBE_SYMBOLS = [
    "cholmod_hip_bench_update_kernel", "cholmod_hip_bench_update_pair", "cholmod_hip_bench_mfma_peak", "cholmod_hip_bench_mfma_peak2",
    "cholmod_hip_bench_mixed", "cholmod_hip_debug_potrf_cycles", "cholmod_hip_debug_panel_cycles",
    "cholmod_hip_debug_latency", "cholmod_hip_bench_mfma_ceiling", "cholmod_hip_probe_cu_mask", "cholmod_hip_probe_overlap", "cholmod_hip_debug_update_diff", "cholmod_hip_debug_diag_cycles", "cholmod_hip_bench_handoff",
]

_probes = None


def build(force: bool = False) -> str:
    """Compile the host C layer and the HIP engine for gfx950 (in-tree)."""
    if force:
        subprocess.check_call(["make", "-C", CSRC, "-s", "clean"])
    subprocess.check_call(["make", "-C", CSRC, "-s", "-j3"])
    return LIB_PATH


_libs = {}


def lib(hooks=None):
    """The product library; hooks=True: its twin with the engine's test hooks compiled in (tests that inject jitter,
    poison, failures).  hooks=None: the product library unless SSAMD_TEST_HOOKS_LIB=1 (worker processes of such tests)."""
    if hooks is None:
        hooks = os.environ.get("SSAMD_TEST_HOOKS_LIB") == "1"
    path = HOOKS_LIB_PATH if hooks else LIB_PATH
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` (hipcc --offload-arch=gfx950).  There is no fallback path.")
    L = C.CDLL(path)
    vp, i64, dbl, sz = C.c_void_p, C.c_int64, C.c_double, C.c_size_t
    cm = C.POINTER(Common)
    sp, dn, fc = C.POINTER(Sparse), C.POINTER(Dense), C.POINTER(Factor)

    def sig(name, res, args):
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args

    sig("cholmod_l_start", C.c_int, [cm])
    sig("cholmod_l_finish", C.c_int, [cm])
    sig("cholmod_l_defaults", C.c_int, [cm])
    sig("cholmod_l_allocate_sparse", sp, [sz, sz, sz, C.c_int, C.c_int, C.c_int, C.c_int, cm])
    sig("cholmod_l_free_sparse", C.c_int, [C.POINTER(sp), cm])
    sig("cholmod_l_copy_sparse", sp, [sp, cm])
    sig("cholmod_l_nnz", i64, [sp, cm])
    sig("cholmod_l_ptranspose", sp, [sp, C.c_int, vp, vp, sz, cm])
    sig("cholmod_l_transpose", sp, [sp, C.c_int, cm])
    sig("cholmod_l_allocate_dense", dn, [sz, sz, sz, C.c_int, cm])
    sig("cholmod_l_zeros", dn, [sz, sz, C.c_int, cm])
    sig("cholmod_l_ones", dn, [sz, sz, C.c_int, cm])
    sig("cholmod_l_copy_dense", dn, [dn, cm])
    sig("cholmod_l_free_dense", C.c_int, [C.POINTER(dn), cm])
    sig("cholmod_l_free_factor", C.c_int, [C.POINTER(fc), cm])
    sig("cholmod_l_check_factor", C.c_int, [fc, cm])
    sig("cholmod_l_check_sparse", C.c_int, [sp, cm])
    sig("cholmod_l_gpu_stats", C.c_int, [cm])
    sig("cholmod_l_sdmult", C.c_int, [sp, C.c_int, C.POINTER(dbl * 2), C.POINTER(dbl * 2), dn, dn, cm])
    sig("cholmod_l_norm_dense", dbl, [dn, C.c_int, cm])
    sig("cholmod_l_norm_sparse", dbl, [sp, C.c_int, cm])
    sig("cholmod_l_analyze", fc, [sp, cm])
    sig("cholmod_l_analyze_p", fc, [sp, vp, vp, sz, cm])
    sig("cholmod_l_analyze_p2", fc, [C.c_int, sp, vp, vp, sz, cm])
    sig("cholmod_l_factorize", C.c_int, [sp, fc, cm])
    sig("cholmod_l_factorize_p", C.c_int, [sp, C.POINTER(dbl * 2), vp, sz, fc, cm])
    sig("cholmod_l_solve", dn, [C.c_int, fc, dn, cm])
    sig("cholmod_l_solve2", C.c_int, [C.c_int, fc, dn, sp, C.POINTER(dn), C.POINTER(sp), C.POINTER(dn), C.POINTER(dn), cm])
    sig("cholmod_l_rcond", dbl, [fc, cm])
    sig("cholmod_l_change_factor", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, fc, cm])
    sig("cholmod_l_etree", C.c_int, [sp, vp, cm])
    sig("cholmod_l_postorder", i64, [vp, sz, vp, vp, cm])
    sig("cholmod_l_rowcolcounts", C.c_int, [sp, vp, sz, vp, vp, vp, vp, vp, vp, cm])
    sig("cholmod_l_super_symbolic", C.c_int, [sp, sp, vp, fc, cm])
    sig("cholmod_l_super_numeric", C.c_int, [sp, sp, C.POINTER(dbl * 2), fc, cm])
    sig("cholmod_l_super_lsolve", C.c_int, [fc, dn, dn, cm])
    sig("cholmod_l_super_ltsolve", C.c_int, [fc, dn, dn, cm])
    sig("cholmod_l_gpu_memorysize", C.c_int, [C.POINTER(sz), C.POINTER(sz), cm])
    sig("cholmod_l_gpu_probe", C.c_int, [cm])
    sig("cholmod_l_gpu_allocate", C.c_int, [cm])
    sig("cholmod_l_gpu_deallocate", C.c_int, [cm])
    sig("cholmod_l_factor_to_host", C.c_int, [fc, cm])
    sig("cholmod_l_hip_stats", C.c_int, [fc, C.POINTER(dbl * CHOLMOD_HIP_NSTATS), cm])
    sig("cholmod_l_refactorize_resident", C.c_int, [C.POINTER(dbl * 2), fc, cm])
    sig("cholmod_l_read_sparse", sp, [vp, cm])
    sig("cholmod_l_read_dense", dn, [vp, cm])
    sig("cholmod_l_read_triplet", vp, [vp, cm])
    sig("cholmod_l_free_triplet", C.c_int, [C.POINTER(vp), cm])
    sig("cholmod_l_read_matrix", vp, [vp, C.c_int, C.POINTER(C.c_int), cm])
    # engine shim
    sig("cholmod_hip_probe", C.c_int, [])
    sig("cholmod_hip_set_device", C.c_int, [C.c_int])
    sig("cholmod_hip_memorysize", C.c_int, [C.POINTER(sz), C.POINTER(sz)])
    sig("cholmod_hip_plan_create", vp, [i64, i64, vp, vp, vp, vp, C.c_int, C.POINTER(C.c_int)])
    sig("cholmod_hip_plan_destroy", None, [vp])
    sig("cholmod_hip_plan_create_dist", vp, [i64, i64, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int,
                                             C.POINTER(C.c_int)])
    sig("cholmod_hip_plan_create_reach", vp, [i64, i64, vp, vp, vp, vp, C.c_int, vp, vp, C.POINTER(C.c_int)])
    sig("cholmod_l_hip_front_reach", i64, [sp, fc, vp, vp, cm])
    sig("cholmod_hip_set_allreduce", C.c_int, [vp, ALLREDUCE_FN, vp])
    sig("cholmod_hip_get_partition", C.c_int, [vp, vp])
    sig("cholmod_hip_get_groups", C.c_int, [vp, vp, vp])
    sig("cholmod_hip_get_batches", i64, [vp, vp, vp])
    sig("cholmod_hip_progress_enable", C.c_int, [vp, C.c_int])
    sig("cholmod_hip_progress", C.c_int, [vp, vp])
    sig("cholmod_hip_debug_schedule_hash", C.c_int, [vp, vp])
    sig("cholmod_hip_debug_routing", C.c_int64, [vp, C.c_int64, vp, vp, vp, vp])
    sig("cholmod_hip_gather_factor", C.c_int, [vp])
    sig("cholmod_l_gather_factor", C.c_int, [fc, cm])
    sig("cholmod_l_hip_prepare", C.c_int, [fc, cm])
    sig("cholmod_hip_factorize", C.c_int, [vp, vp, vp, vp, vp, dbl, C.c_int, vp, C.POINTER(i64)])
    sig("cholmod_hip_upload_matrix", C.c_int, [vp, vp, vp, vp, vp])
    sig("cholmod_hip_factorize_resident", C.c_int, [vp, dbl, C.c_int, C.POINTER(i64)])
    sig("cholmod_hip_download_factor", C.c_int, [vp, vp])
    sig("cholmod_hip_upload_factor", C.c_int, [vp, vp])
    sig("cholmod_hip_download_even_columns", C.c_int, [vp, vp])
    sig("cholmod_hip_diag_minmax", C.c_int, [vp, vp])
    sig("cholmod_hip_solve", C.c_int, [vp, C.c_int, vp, i64, i64])
    sig("cholmod_hip_set_perm", C.c_int, [vp, vp])
    sig("cholmod_hip_solve_device", C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, i64, vp, i64, i64, vp])
    sig("cholmod_l_hip_solve_device", C.c_int, [C.c_int, fc, vp, sz, vp, sz, sz, vp, cm])
    sig("cholmod_hip_residual_device", C.c_int, [vp, C.c_int, vp, i64, vp, i64, vp, i64, i64, vp, vp])
    sig("cholmod_hip_refine_device", C.c_int, [vp, C.c_int, vp, i64, vp, i64, i64, C.c_int, vp, vp])
    sig("cholmod_l_hip_residual_device", C.c_int, [fc, vp, sz, vp, sz, vp, sz, sz, vp, vp, cm])
    sig("cholmod_l_hip_refine_device", C.c_int, [fc, vp, sz, vp, sz, sz, C.c_int, vp, vp, cm])
    sig("cholmod_l_hip_solve_device_complex", C.c_int, [C.c_int, fc, vp, sz, vp, sz, sz, vp, cm])
    sig("cholmod_l_hip_residual_device_complex", C.c_int, [fc, vp, sz, vp, sz, vp, sz, sz, vp, vp, cm])
    sig("cholmod_l_hip_refine_device_complex", C.c_int, [fc, vp, sz, vp, sz, sz, C.c_int, vp, vp, cm])
    sig("cholmod_hip_factorize_values_device", C.c_int, [vp, vp, i64, dbl, C.c_int, vp, C.POINTER(i64)])
    sig("cholmod_hip_set_product_map", C.c_int, [vp, vp, vp, vp, i64, i64])
    sig("cholmod_hip_download_matrix_values", C.c_int, [vp, vp])
    sig("cholmod_l_hip_factorize_values_device", C.c_int, [sp, vp, C.POINTER(dbl * 2), fc, vp, cm])
    sig("cholmod_l_hip_aat_product_map", i64, [sp, vp, vp, vp, cm])
    sig("cholmod_hip_selinv_device", C.c_int, [vp, vp])
    sig("cholmod_hip_selinv_gather_device", C.c_int, [vp, vp, i64, vp, C.c_int, vp])
    sig("cholmod_hip_selinv_download", C.c_int, [vp, vp])
    sig("cholmod_hip_selinv_release", C.c_int, [vp])
    sig("cholmod_hip_selinv_info", C.c_int, [vp, vp])
    sig("cholmod_l_hip_selinv_device", C.c_int, [sp, fc, vp, vp, vp, cm])
    sig("cholmod_l_hip_selinv_to_host", C.c_int, [fc, vp, cm])
    sig("cholmod_hip_schur_device", C.c_int, [vp, i64, vp, i64, vp, i64, vp])
    sig("cholmod_hip_trailing_multiply_device", C.c_int, [vp, i64, C.c_int, vp, i64, vp, i64, i64, vp])
    sig("cholmod_l_hip_schur_device", C.c_int, [fc, sz, vp, sz, vp, sz, vp, cm])
    sig("cholmod_l_hip_schur_reduce_device", C.c_int, [fc, sz, vp, sz, vp, sz, vp, sz, sz, vp, cm])
    sig("cholmod_l_hip_schur_expand_device", C.c_int, [fc, sz, vp, sz, vp, sz, vp, sz, sz, vp, cm])
    sig("cholmod_hip_factor_grad_device", C.c_int, [vp, vp, vp])
    sig("cholmod_hip_factor_outer_grad_device", C.c_int, [vp, dbl, vp, i64, vp, i64, i64, vp])
    sig("cholmod_hip_factor_grad_gather_device", C.c_int, [vp, vp, i64, vp, vp])
    sig("cholmod_hip_factor_grad_download", C.c_int, [vp, vp])
    sig("cholmod_hip_factor_grad_release", C.c_int, [vp])
    sig("cholmod_hip_factor_grad_info", C.c_int, [vp, vp])
    sig("cholmod_l_hip_factor_grad_device", C.c_int, [sp, fc, vp, vp, vp, vp, cm])
    sig("cholmod_l_hip_factor_outer_grad_device", C.c_int, [sp, fc, dbl, vp, sz, vp, sz, sz, vp, vp, vp, cm])
    sig("cholmod_l_hip_factor_grad_to_host", C.c_int, [fc, vp, cm])
    sig("cholmod_hip_values_grad_device", C.c_int, [vp, C.c_int, dbl, vp, i64, vp, i64, i64, vp, i64, vp])
    sig("cholmod_hip_logdet_device", C.c_int, [vp, vp, vp])
    sig("cholmod_l_hip_values_grad_device", C.c_int, [sp, fc, dbl, vp, sz, vp, sz, sz, vp, vp, cm])
    sig("cholmod_l_hip_logdet_device", C.c_int, [fc, vp, vp, cm])
    sig("cholmod_hip_product_values_grad_device", C.c_int, [vp, C.c_int, dbl, vp, i64, vp, i64, i64, vp, vp, i64, vp])
    sig("cholmod_hip_product_logdet_grad_device", C.c_int, [vp, vp, vp, i64, vp])
    sig("cholmod_l_hip_aat_values_grad_device", C.c_int, [sp, fc, dbl, vp, sz, vp, sz, sz, vp, vp, vp, cm])
    sig("cholmod_l_hip_aat_logdet_grad_device", C.c_int, [sp, fc, vp, vp, vp, cm])
    sig("cholmod_hip_get_maps", C.c_int, [vp, vp, vp, vp])
    sig("cholmod_hip_get_stats", C.c_int, [vp, vp])
    sig("cholmod_hip_set_profiling", C.c_int, [vp, C.c_int])
    sig("cholmod_hip_dense_partial_factor", C.c_int, [vp, i64, i64, C.c_int, C.POINTER(i64)])
    sig("cholmod_hip_factor_checks", C.c_int, [vp, vp])
    sig("cholmod_hip_factor_checks_local", C.c_int, [vp, vp])
    sig("cholmod_hip_get_launch_profile", i64, [vp, i64, vp, vp, vp, vp, vp, vp])
    sig("cholmod_hip_debug_thin_cycles", C.c_int, [vp, i64, vp])
    sig("cholmod_hip_debug_launch_regions", i64, [vp, i64, i64, vp])
    sig("cholmod_hip_debug_cb_extend_add", i64, [vp, i64, vp])
    sig("cholmod_hip_debug_fused_pair", i64, [vp, i64, vp, vp, vp])
    sig("cholmod_hip_rccl_unique_id", C.c_int, [vp])
    sig("cholmod_hip_rccl_attach", C.c_int, [vp, vp])
    sig("cholmod_hip_rccl_detach", C.c_int, [vp])
    sig("cholmod_hip_version", C.c_char_p, [])
    _libs[path] = L
    return L


def probes():
    """Micro-benchmarks / tuning probes (include/cholmod_hip_probes.h): a library of
    their own, not part of the product."""
    global _probes
    if _probes is not None:
        return _probes
    if not os.path.exists(PROBES_PATH):
        raise RuntimeError(f"{PROBES_PATH} is missing: build it with __graft_entry__.build()")
    L = C.CDLL(PROBES_PATH)
    vp, i64, dbl = C.c_void_p, C.c_int64, C.c_double
    for name, res, args in (
            ("cholmod_hip_bench_update_kernel", dbl, [i64, i64, i64, C.c_int, C.c_int]),
            ("cholmod_hip_bench_update_pair", dbl, [i64, i64, i64, i64, i64, C.c_int, C.c_int]),
            ("cholmod_hip_bench_mfma_peak", dbl, [C.c_int, C.c_int]),
            ("cholmod_hip_bench_mfma_peak2", dbl, [C.c_int, C.c_int, C.c_int, C.c_int]),
            ("cholmod_hip_bench_mixed", dbl, [C.c_int, C.c_int, C.c_int]),
            ("cholmod_hip_bench_mfma_ceiling", dbl, [C.c_int, C.c_int, C.c_int, C.c_int, vp]),
            ("cholmod_hip_probe_cu_mask", dbl, [vp, C.c_int, C.c_int, C.c_int, vp]),
            ("cholmod_hip_probe_overlap", C.c_int, [vp, vp, C.c_int, i64, i64, C.c_int, C.c_int, C.c_int, vp]),
            ("cholmod_hip_debug_update_diff", dbl, [i64, i64, i64, C.c_int, C.c_int, C.c_int]),
            ("cholmod_hip_debug_diag_cycles", C.c_int, [vp, C.c_int, C.c_int]),
            ("cholmod_hip_debug_potrf_cycles", C.c_int, [vp]),
            ("cholmod_hip_debug_panel_cycles", C.c_int, [vp]),
            ("cholmod_hip_debug_latency", C.c_int, [vp, C.c_int])):
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _probes = L
    return L


def _view(ptr, n, ctype, dtype):
    if not ptr or n == 0:
        return np.zeros(0, dtype=dtype)
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(int(n),))


class Session:
    """One cholmod_common plus convenience wrappers (tests / bench harness)."""

    def __init__(self, supernodal=SUPERNODAL, use_gpu=1, print_level=0, postorder=True,
                 factor_on_device=False, hip_flags=0, rank=0, world=1, allreduce=None,
                 ordering="natural", hooks=None):
        """ordering (used by analyze() when no permutation is passed): "natural"
        (the harness default: tests pin results to the oracle's natural order),
        "default" (cholmod_l_start's strategy: the built-in nested dissection) or
        "nesdis".  hooks=True: the library with the engine's test hooks (lib ())."""
        self.L = lib(hooks)
        self.cm = Common()
        self.L.cholmod_l_start(C.byref(self.cm))
        if ordering == "natural":
            self.cm.nmethods = 1
            self.cm.method[0].ordering = 0          # CHOLMOD_NATURAL
        elif ordering == "nesdis":
            self.cm.nmethods = 1
            self.cm.method[0].ordering = 4          # CHOLMOD_NESDIS
        elif ordering != "default":
            raise ValueError(ordering)
        self.cm.supernodal = supernodal
        self.cm.useGPU = use_gpu
        self.cm.print = print_level
        self.cm.postorder = int(postorder)
        self.cm.hip_factor_on_device = int(factor_on_device)
        self.cm.hip_flags = hip_flags
        self._keep = []
        if world > 1 or allreduce is not None:
            # allreduce: a ctypes ALLREDUCE_FN (see suitesparse_amd/dist.py); with
            # world == 1 it is only used by the CHOLMOD_HIP_SHARE_AS_WORLD self test
            self.cm.hip_rank, self.cm.hip_world = rank, world
            self._keep.append(allreduce)
            self.cm.hip_allreduce = C.cast(allreduce, C.c_void_p)

    @property
    def status(self):
        return self.cm.status

    def finish(self):
        self.L.cholmod_l_finish(C.byref(self.cm))

    # ---- object helpers
    def sparse(self, n, Ap, Ai, Ax, stype, zomplex=False):
        """Copy numpy CSC arrays into a library-owned cholmod_sparse.  Complex values
        (numpy complex128) make a CHOLMOD_COMPLEX matrix, or CHOLMOD_ZOMPLEX on request."""
        nz = int(Ap[-1])
        cx = np.iscomplexobj(Ax)
        xtype = (ZOMPLEX if zomplex else COMPLEX) if cx else REAL
        A = self.L.cholmod_l_allocate_sparse(n, n, max(nz, 1), 1, 1, stype, xtype, C.byref(self.cm))
        if not A:
            raise MemoryError("cholmod_l_allocate_sparse")
        a = A.contents
        _view(a.p, n + 1, C.c_int64, np.int64)[:] = Ap
        if nz:
            _view(a.i, nz, C.c_int64, np.int64)[:] = Ai
            if not cx:
                _view(a.x, nz, C.c_double, np.float64)[:] = Ax
            elif zomplex:
                _view(a.x, nz, C.c_double, np.float64)[:] = np.real(Ax)
                _view(a.z, nz, C.c_double, np.float64)[:] = np.imag(Ax)
            else:
                _view(a.x, 2 * nz, C.c_double, np.float64)[:] = np.ascontiguousarray(Ax, dtype=np.complex128).view(np.float64)
        return A

    def dense(self, arr, zomplex=False):
        cx = np.iscomplexobj(arr)
        arr = np.asarray(arr, dtype=np.complex128 if cx else np.float64)
        n = arr.shape[-1] if arr.ndim > 1 else arr.shape[0]
        nrhs = arr.shape[0] if arr.ndim > 1 else 1
        xtype = (ZOMPLEX if zomplex else COMPLEX) if cx else REAL
        X = self.L.cholmod_l_allocate_dense(n, nrhs, n, xtype, C.byref(self.cm))
        if not cx:
            _view(X.contents.x, n * nrhs, C.c_double, np.float64)[:] = arr.reshape(-1)
        elif zomplex:
            _view(X.contents.x, n * nrhs, C.c_double, np.float64)[:] = arr.real.reshape(-1)
            _view(X.contents.z, n * nrhs, C.c_double, np.float64)[:] = arr.imag.reshape(-1)
        else:
            _view(X.contents.x, 2 * n * nrhs, C.c_double, np.float64)[:] = arr.reshape(-1).view(np.float64)
        return X

    def dense_to_numpy(self, X):
        x = X.contents
        if x.xtype == COMPLEX:
            out = _view(x.x, 2 * x.d * x.ncol, C.c_double, np.float64).copy().view(np.complex128)
        elif x.xtype == ZOMPLEX:
            out = (_view(x.x, x.d * x.ncol, C.c_double, np.float64)
                   + 1j * _view(x.z, x.d * x.ncol, C.c_double, np.float64))
        else:
            out = _view(x.x, x.d * x.ncol, C.c_double, np.float64).copy()
        return out.reshape(x.ncol, x.d)[:, :x.nrow] if x.ncol > 1 else out[:x.nrow]

    def free_sparse(self, A):
        self.L.cholmod_l_free_sparse(C.byref(A), C.byref(self.cm))

    def free_dense(self, X):
        self.L.cholmod_l_free_dense(C.byref(X), C.byref(self.cm))

    def free_factor(self, Lf):
        self.L.cholmod_l_free_factor(C.byref(Lf), C.byref(self.cm))

    # ---- the path
    def analyze(self, A, perm=None):
        if perm is None:
            Lf = self.L.cholmod_l_analyze(A, C.byref(self.cm))
        else:
            p = np.ascontiguousarray(perm, dtype=np.int64)
            Lf = self.L.cholmod_l_analyze_p(A, p.ctypes.data, None, 0, C.byref(self.cm))
        if not Lf:
            raise RuntimeError(f"cholmod_l_analyze failed, status {self.cm.status}")
        return Lf

    def factorize(self, A, Lf, beta=0.0):
        b = (C.c_double * 2)(beta, 0.0)
        return self.L.cholmod_l_factorize_p(A, C.byref(b), None, 0, Lf, C.byref(self.cm))

    def factorize_device(self, A, values, Lf, beta=0.0):
        """cholmod_l_hip_factorize_values_device: `factorize` for new values of A that live on the device.  A gives the
        pattern (its host values are not read); values: a 1-D contiguous torch.float64 device tensor of length nnz (A), in
        A's entry order.  Lf must have been factorized from a host matrix of this pattern before.  Enqueued after torch's
        current stream; returns what `factorize` returns, when the factorization has finished on the device."""
        import torch
        a = A.contents
        nz = int(_view(a.p, a.ncol + 1, C.c_int64, np.int64)[-1]) if a.p else 0
        if not (isinstance(values, torch.Tensor) and values.is_cuda and values.dtype == torch.float64):
            raise TypeError("factorize_device: values must be a torch.float64 tensor on the device")
        if values.dim() != 1 or values.shape[0] != nz or not values.is_contiguous():
            raise ValueError(f"factorize_device: values must be 1-D, contiguous and of length nnz (A) = {nz}")
        b = (C.c_double * 2)(beta, 0.0)
        stream = torch.cuda.current_stream(values.device).cuda_stream
        return self.L.cholmod_l_hip_factorize_values_device(A, values.data_ptr() or 1, C.byref(b), Lf, stream,
                                                            C.byref(self.cm))

    def refactorize_resident(self, Lf, beta=0.0):
        b = (C.c_double * 2)(beta, 0.0)
        return self.L.cholmod_l_refactorize_resident(C.byref(b), Lf, C.byref(self.cm))

    def solve(self, Lf, b, sys=SYS_A, zomplex=False):
        B = self.dense(b, zomplex=zomplex)
        X = self.L.cholmod_l_solve(sys, Lf, B, C.byref(self.cm))
        self.free_dense(B)
        if not X:
            raise RuntimeError(f"cholmod_l_solve failed, status {self.cm.status}")
        out = self.dense_to_numpy(X)
        self.free_dense(X)
        return out

    @staticmethod
    def _device_dtype(Lf):
        """(dtype of the device tensors that go with the factor Lf, suffix of its entry points): torch.complex128 and the
        `_complex` entry points for a complex factor, torch.float64 and the real ones for every other."""
        import torch
        return (torch.complex128, "_complex") if Lf.contents.xtype == COMPLEX else (torch.float64, "")

    @staticmethod
    def _device_layout(what, n, t, like=None, dtype=None):
        """(leading dimension, right-hand sides) of the column-major n-by-nrhs matrix the rows of the device tensor t
        are: torch.float64 (or `dtype`), shape (nrhs, n) or (n,), unit stride along a row, any row stride >= n, both in
        elements of the tensor; `like`: a tensor whose shape and device t must share."""
        import torch
        dtype = dtype or torch.float64
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype):
            raise (TypeError if like is None else ValueError)(f"{what} must be a {dtype} tensor on the device")
        if t.dim() not in (1, 2) or t.shape[-1] != n:
            raise ValueError(f"{what} must have shape (nrhs, {n}) or ({n},)")
        if like is not None and (t.shape != like.shape or t.device != like.device):
            raise ValueError(f"{what} must have the shape and the device of the other arrays")
        if n > 1 and t.stride(-1) != 1:
            raise ValueError(f"{what}: the entries of a right-hand side must be contiguous")
        if t.dim() == 1 or t.shape[0] <= 1:
            return n, (1 if t.dim() == 1 else int(t.shape[0]))
        if t.stride(0) < n:
            raise ValueError(f"{what}: row stride smaller than n")
        return int(t.stride(0)), int(t.shape[0])

    def solve_device(self, Lf, B, sys=SYS_A, out=None):
        """cholmod_l_hip_solve_device: solve with right-hand sides that live on the device.  B: a torch.float64 device
        tensor of shape (nrhs, n) or (n,) -- rows are right-hand sides, as in `solve` -- with unit stride along a row
        and any row stride >= n.  Returns a device tensor of the same shape, or writes into `out` (`out is B`: in
        place).  The solve is enqueued on torch's current stream; nothing is copied to the host and the host does not
        wait for it.  torch must have been imported before the library was loaded (before the first Session), so that
        the two share one HIP runtime.  A complex factor takes torch.complex128 tensors of the same shapes (strides in
        complex elements) and goes through cholmod_l_hip_solve_device_complex; a dtype that does not match the factor
        is a TypeError."""
        import torch
        n = int(Lf.contents.n)
        dt, sfx = self._device_dtype(Lf)
        ldb, nrhs = self._device_layout("solve_device: B", n, B, dtype=dt)
        if out is None:
            out = torch.empty(B.shape, dtype=dt, device=B.device)
        ldx, _ = self._device_layout("solve_device: out", n, out, like=B, dtype=dt)
        stream = torch.cuda.current_stream(B.device).cuda_stream
        fn = getattr(self.L, "cholmod_l_hip_solve_device" + sfx)
        ok = fn(sys, Lf, B.data_ptr() or 1, ldb, out.data_ptr() or 1, ldx, nrhs, stream, C.byref(self.cm))
        if not ok:
            raise RuntimeError(f"cholmod_l_hip_solve_device{sfx} failed, status {self.cm.status}")
        return out

    def residual_device(self, Lf, X, B, out=None, norms=False):
        """cholmod_l_hip_residual_device: R = B - A X on the device, A being the matrix Lf was last factorized from
        (plus beta I).  X, B: device tensors as for `solve_device`, of one shape.  Returns R as a new tensor or in `out`
        (`out is B`: in place; never X); with norms=True, (R, norms): norms a device tensor of length nrhs holding
        max |R| of every right-hand side.  Enqueued on torch's current stream; two calls on the same inputs give the same
        bits.  A complex factor: torch.complex128 tensors (cholmod_l_hip_residual_device_complex); norms stays
        torch.float64 and holds the largest |re| or |im| of every right-hand side of R."""
        import torch
        n = int(Lf.contents.n)
        dt, sfx = self._device_dtype(Lf)
        ldx, nrhs = self._device_layout("residual_device: X", n, X, dtype=dt)
        ldb, _ = self._device_layout("residual_device: B", n, B, like=X, dtype=dt)
        if out is None:
            out = torch.empty(X.shape, dtype=dt, device=X.device)
        ldr, _ = self._device_layout("residual_device: out", n, out, like=X, dtype=dt)
        nrm = torch.empty(nrhs, dtype=torch.float64, device=X.device) if norms else None
        stream = torch.cuda.current_stream(X.device).cuda_stream
        # (empty tensors have no address: distinct stand-ins, R must not be X)
        fn = getattr(self.L, "cholmod_l_hip_residual_device" + sfx)
        ok = fn(Lf, X.data_ptr() or 1, ldx, B.data_ptr() or 2, ldb, out.data_ptr() or 3, ldr, nrhs,
                nrm.data_ptr() if norms and nrhs else None, stream, C.byref(self.cm))
        if not ok:
            raise RuntimeError(f"cholmod_l_hip_residual_device{sfx} failed, status {self.cm.status}")
        return (out, nrm) if norms else out

    def refine_device(self, Lf, B, X, steps=1, norms=False):
        """cholmod_l_hip_refine_device: `steps` rounds of X += A^-1 (B - A X) with the factor Lf, in place on the device
        tensor X, which is returned; with norms=True, (X, norms): the residual norms of the final X (steps=0: X is left
        alone and only its norms are formed).  Tensors, stream and complex factors as for `residual_device`."""
        import torch
        n = int(Lf.contents.n)
        dt, sfx = self._device_dtype(Lf)
        ldb, nrhs = self._device_layout("refine_device: B", n, B, dtype=dt)
        ldx, _ = self._device_layout("refine_device: X", n, X, like=B, dtype=dt)
        nrm = torch.empty(nrhs, dtype=torch.float64, device=X.device) if norms else None
        stream = torch.cuda.current_stream(X.device).cuda_stream
        fn = getattr(self.L, "cholmod_l_hip_refine_device" + sfx)
        ok = fn(Lf, B.data_ptr() or 2, ldb, X.data_ptr() or 1, ldx, nrhs, int(steps),
                nrm.data_ptr() if norms and nrhs else None, stream, C.byref(self.cm))
        if not ok:
            raise RuntimeError(f"cholmod_l_hip_refine_device{sfx} failed, status {self.cm.status}")
        return (X, nrm) if norms else X

    def selinv_device(self, A, Lf, values=True, diag=True):
        """cholmod_l_hip_selinv_device: the selected inverse of the matrix Lf was last factorized from on the device
        (plus beta I).  Returns (Z, d) as torch.float64 device tensors, None for the part not asked for: Z of length
        nnz (A), the inverse at the entries of A in A's entry order (NaN where the factorization does not read A), d of
        length n, its diagonal in A's ordering.  A gives the pattern only (None is allowed with values=False).  Enqueued
        on torch's current stream; two calls on the same factor give the same bits."""
        import torch
        n = int(Lf.contents.n)
        dev = torch.device("cuda", torch.cuda.current_device())
        Z = d = None
        if values:
            a = A.contents
            nz = int(_view(a.p, a.ncol + 1, C.c_int64, np.int64)[-1]) if a.p else 0
            Z = torch.empty(nz, dtype=torch.float64, device=dev)
        if diag:
            d = torch.empty(n, dtype=torch.float64, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        ok = self.L.cholmod_l_hip_selinv_device(A, Lf, (Z.data_ptr() or 1) if values else None,
                                                (d.data_ptr() or 2) if diag else None, stream, C.byref(self.cm))
        if not ok:
            raise RuntimeError(f"cholmod_l_hip_selinv_device failed, status {self.cm.status}")
        return Z, d

    def values_grad_device(self, A, Lf, U, V, alpha=1.0, out=None):
        """cholmod_l_hip_values_grad_device: alpha sum_r (U [i, r] V [j, r] + [i != j] U [j, r] V [i, r]) at every entry
        (i, j) of A the factorization reads, exact +0.0 at every other entry; with U = A^-1 gX, V = X = A^-1 B and
        alpha = -1 the gradient of a scalar with respect to A's values through the solve.  U, V: device tensors as for
        `solve_device`, of one shape, in A's ordering (they may be the same tensor).  Returns a 1-D tensor of length
        nnz (A) in A's entry order, or writes into `out`.  Enqueued on torch's current stream; the same inputs give the
        same bits."""
        import torch
        n = int(Lf.contents.n)
        ldu, nrhs = self._device_layout("values_grad_device: U", n, U)
        ldv, _ = self._device_layout("values_grad_device: V", n, V, like=U)
        a = A.contents
        nz = int(_view(a.p, a.ncol + 1, C.c_int64, np.int64)[-1]) if a.p else 0
        if out is None:
            out = torch.empty(nz, dtype=torch.float64, device=U.device)
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float64 and out.device == U.device):
            raise ValueError("values_grad_device: out must be a torch.float64 tensor on the device of U")
        if out.dim() != 1 or out.shape[0] != nz or not out.is_contiguous():
            raise ValueError(f"values_grad_device: out must be 1-D, contiguous and of length nnz (A) = {nz}")
        stream = torch.cuda.current_stream(U.device).cuda_stream
        ok = self.L.cholmod_l_hip_values_grad_device(A, Lf, float(alpha), U.data_ptr() or 1, ldu, V.data_ptr() or 1, ldv,
                                                     nrhs, out.data_ptr() or 2, stream, C.byref(self.cm))
        if not ok:
            raise RuntimeError(f"cholmod_l_hip_values_grad_device failed, status {self.cm.status}")
        return out

    @staticmethod
    def _aat_values(what, A, values, out):
        """(nnz (A), out) for the gradients through A*A': `values` and `out` 1-D contiguous torch.float64 tensors of
        length nnz (A) on one device; out=None: a new tensor"""
        import torch
        a = A.contents
        nz = int(_view(a.p, a.ncol + 1, C.c_int64, np.int64)[-1]) if a.p else 0
        if not (isinstance(values, torch.Tensor) and values.is_cuda and values.dtype == torch.float64):
            raise TypeError(f"{what}: values must be a torch.float64 tensor on the device")
        if values.dim() != 1 or values.shape[0] != nz or not values.is_contiguous():
            raise ValueError(f"{what}: values must be 1-D, contiguous and of length nnz (A) = {nz}")
        if out is None:
            out = torch.empty(nz, dtype=torch.float64, device=values.device)
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float64 and out.device == values.device):
            raise ValueError(f"{what}: out must be a torch.float64 tensor on the device of values")
        if out.dim() != 1 or out.shape[0] != nz or not out.is_contiguous():
            raise ValueError(f"{what}: out must be 1-D, contiguous and of length nnz (A) = {nz}")
        return nz, out

    def aat_values_grad_device(self, A, Lf, values, U, V, alpha=1.0, out=None):
        """cholmod_l_hip_aat_values_grad_device: for an unsymmetric A (stype 0) and M = A A' + beta I, the chain rule from
        G = alpha (U V' + V U') sampled on tril (M) to the values of A: out [q] = sum_j G (i, j) a (j, k) over column k of
        the entry q = (i, k).  With U = M^-1 gX, V = X = M^-1 B and alpha = -1 the gradient of a scalar with respect to
        A's values through the solve.  values: the 1-D device tensor Lf was factorized from (factorize_device); U, V as
        for `values_grad_device`.  Returns a 1-D tensor of length nnz (A) in A's entry order, or writes into `out`.
        Enqueued on torch's current stream; the same inputs give the same bits.  The first call after a new pattern
        builds the transposed product map on the host and waits for it."""
        import torch
        n = int(Lf.contents.n)
        ldu, nrhs = self._device_layout("aat_values_grad_device: U", n, U)
        ldv, _ = self._device_layout("aat_values_grad_device: V", n, V, like=U)
        _, out = self._aat_values("aat_values_grad_device", A, values, out)
        if values.device != U.device:
            raise ValueError("aat_values_grad_device: values must be on the device of U")
        stream = torch.cuda.current_stream(U.device).cuda_stream
        ok = self.L.cholmod_l_hip_aat_values_grad_device(A, Lf, float(alpha), U.data_ptr() or 1, ldu, V.data_ptr() or 1, ldv,
                                                         nrhs, values.data_ptr() or 3, out.data_ptr() or 2, stream,
                                                         C.byref(self.cm))
        if not ok:
            raise RuntimeError(f"cholmod_l_hip_aat_values_grad_device failed, status {self.cm.status}")
        return out

    def aat_logdet_grad_device(self, A, Lf, values, out=None):
        """cholmod_l_hip_aat_logdet_grad_device: the gradient of log det (A A' + beta I) with respect to the values of the
        unsymmetric A, 2 (Z A) sampled on A with Z the selected inverse (computed if the resident one is stale).  Tensors,
        stream and result as for `aat_values_grad_device`."""
        import torch
        _, out = self._aat_values("aat_logdet_grad_device", A, values, out)
        stream = torch.cuda.current_stream(values.device).cuda_stream
        ok = self.L.cholmod_l_hip_aat_logdet_grad_device(A, Lf, values.data_ptr() or 3, out.data_ptr() or 2, stream,
                                                         C.byref(self.cm))
        if not ok:
            raise RuntimeError(f"cholmod_l_hip_aat_logdet_grad_device failed, status {self.cm.status}")
        return out

    def logdet_device(self, Lf):
        """cholmod_l_hip_logdet_device: log det (A + beta I) = 2 sum log L_jj of the factor resident on the device, as a
        0-dim torch.float64 device tensor.  Enqueued on torch's current stream, no host wait; the same factor gives the
        same bits."""
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        out = torch.empty((), dtype=torch.float64, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        if not self.L.cholmod_l_hip_logdet_device(Lf, out.data_ptr(), stream, C.byref(self.cm)):
            raise RuntimeError(f"cholmod_l_hip_logdet_device failed, status {self.cm.status}")
        return out

    def selinv_host(self, Lf):
        """cholmod_l_hip_selinv_to_host: the selected inverse in the layout of L->x (FactorView.x), xsize doubles, in
        the factor's ordering; computed on the device if the resident one is stale."""
        out = np.zeros(max(int(Lf.contents.xsize), 1))
        if not self.L.cholmod_l_hip_selinv_to_host(Lf, out.ctypes.data, C.byref(self.cm)):
            raise RuntimeError(f"cholmod_l_hip_selinv_to_host failed, status {self.cm.status}")
        return out[:int(Lf.contents.xsize)]

    def _factor_grad_outputs(self, A, dev):
        """(G, trace) for the two factor-gradient calls: new torch.float64 tensors on `dev`, nnz (A) long and 0-dim"""
        import torch
        a = A.contents
        nz = int(_view(a.p, a.ncol + 1, C.c_int64, np.int64)[-1]) if a.p else 0
        return torch.zeros(nz, dtype=torch.float64, device=dev), torch.zeros((), dtype=torch.float64, device=dev)

    def factor_grad_device(self, A, Lf, Lbar):
        """cholmod_l_hip_factor_grad_device: reverse-mode Cholesky on the device.  Lbar: a 1-D contiguous torch.float64
        device tensor of length L->xsize, df/dL in the layout of L->x (FactorView.x; the dead upper triangles of the
        diagonal blocks are ignored).  Returns (G, trace): G a 1-D tensor of length nnz (A) in A's entry order, df/d (the
        value of A at that entry), exact +0.0 where the factorization does not read A; trace a 0-dim tensor, df/dbeta.  A
        gives the pattern only.  Enqueued on torch's current stream; the same inputs give the same bits."""
        import torch
        xsize = int(Lf.contents.xsize)
        if not (isinstance(Lbar, torch.Tensor) and Lbar.is_cuda and Lbar.dtype == torch.float64):
            raise TypeError("factor_grad_device: Lbar must be a torch.float64 tensor on the device")
        if Lbar.dim() != 1 or Lbar.shape[0] != xsize or not Lbar.is_contiguous():
            raise ValueError(f"factor_grad_device: Lbar must be 1-D, contiguous and of length L->xsize = {xsize}")
        G, tr = self._factor_grad_outputs(A, Lbar.device)
        stream = torch.cuda.current_stream(Lbar.device).cuda_stream
        ok = self.L.cholmod_l_hip_factor_grad_device(A, Lf, Lbar.data_ptr() or 1, G.data_ptr() or 2, tr.data_ptr(), stream,
                                                     C.byref(self.cm))
        if not ok:
            raise RuntimeError(f"cholmod_l_hip_factor_grad_device failed, status {self.cm.status}")
        return G, tr

    def factor_outer_grad_device(self, A, Lf, P, Q, alpha=-1.0):
        """cholmod_l_hip_factor_outer_grad_device: the same with Lbar = alpha sum_r P [:, r] Q [:, r]' sampled on the pattern
        of L, formed on the device.  P, Q: device tensors as for `solve_device` (rows are right-hand sides), of one
        shape, in the FACTOR's ordering -- what `solve_device` returns for sys=SYS_L and SYS_Lt --; they may be the same
        tensor.  For Xt = solve_device (Lf, Z, SYS_Lt) and an incoming gradient gXt, with U = solve_device (Lf, gXt, SYS_L):
        P = Xt, Q = U, alpha = -1 (and the gradient with respect to Z is U); for Y = solve_device (Lf, B, SYS_L) and gY, with
        V = solve_device (Lf, gY, SYS_Lt):  P = V, Q = Y, alpha = -1 (and the gradient with respect to B is V).  Returns
        (G, trace) as `factor_grad_device`."""
        import torch
        n = int(Lf.contents.n)
        ldp, nrhs = self._device_layout("factor_outer_grad_device: P", n, P)
        ldq, _ = self._device_layout("factor_outer_grad_device: Q", n, Q, like=P)
        G, tr = self._factor_grad_outputs(A, P.device)
        stream = torch.cuda.current_stream(P.device).cuda_stream
        ok = self.L.cholmod_l_hip_factor_outer_grad_device(A, Lf, float(alpha), P.data_ptr() or 1, ldp, Q.data_ptr() or 1, ldq,
                                                           nrhs, G.data_ptr() or 2, tr.data_ptr(), stream, C.byref(self.cm))
        if not ok:
            raise RuntimeError(f"cholmod_l_hip_factor_outer_grad_device failed, status {self.cm.status}")
        return G, tr

    def factor_grad_host(self, Lf):
        """cholmod_l_hip_factor_grad_to_host: Gx = df/dS on the pattern of L of the last factor_grad_device /
        factor_outer_grad_device, in the layout of L->x (FactorView.x), xsize doubles, in the factor's ordering; waits for
        it.  A factorization since then makes it stale: RuntimeError."""
        out = np.zeros(max(int(Lf.contents.xsize), 1))
        if not self.L.cholmod_l_hip_factor_grad_to_host(Lf, out.ctypes.data, C.byref(self.cm)):
            raise RuntimeError(f"cholmod_l_hip_factor_grad_to_host failed, status {self.cm.status}")
        return out[:int(Lf.contents.xsize)]

    # ---- the Schur complement onto the last m variables of the factor's ordering
    @staticmethod
    def schur_index(Lf, m):
        """The variables of A the rows of `schur_device`, of G and of XS stand for: Perm [n - m:], as an np.int64 array."""
        f = Lf.contents
        n, m = int(f.n), int(m)
        if not 0 <= m <= n:
            raise ValueError(f"schur_index: m must lie in 0 .. n = {n}")
        return _view(f.Perm, n, C.c_int64, np.int64)[n - m:].copy()

    @staticmethod
    def _square_layout(what, m, t, dev):
        """leading dimension of the (m, m) torch.float64 device tensor t: unit stride along a row, row stride >= m"""
        import torch
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.device == dev):
            raise ValueError(f"{what} must be a torch.float64 tensor on the current device")
        if t.dim() != 2 or tuple(t.shape) != (m, m) or (m > 1 and (t.stride(1) != 1 or t.stride(0) < m)):
            raise ValueError(f"{what} must have shape ({m}, {m}), unit stride along a row and a row stride >= {m}")
        return int(t.stride(0)) if m > 1 else max(m, 1)

    def schur_device(self, Lf, m=None, subset=None, factor=False, out=None):
        """cholmod_l_hip_schur_device: the Schur complement Sc of the matrix Lf was last factorized from on the device (plus
        beta I) onto the LAST m variables of the factor's ordering -- the variables `schur_index (Lf, m)` of A, in that
        order -- as an (m, m) torch.float64 device tensor, both triangles, bitwise symmetric.  factor=True: (Sc, F) with
        F [i, j] = L22 (i, j), the Cholesky factor of Sc (F @ F.T is Sc; torch.cholesky_solve (g, F) solves with it): a
        transposed view of the column-major array, exact +0.0 above the diagonal.  subset: a sequence of distinct
        variables of A instead of m; it must be the set of the last len (subset) variables of the factor's ordering (see
        `schur_perm`), and rows and columns come back in ITS order.  out: a tensor for Sc, or with factor=True a pair
        (tensor for Sc, tensor for the column-major array behind F); shape (m, m), unit stride along a row, any row
        stride >= m -- nothing outside the (m, m) block is written; not with subset.  Enqueued on torch's current stream;
        the same factor gives the same bits."""
        import torch
        n = int(Lf.contents.n)
        order = None
        if subset is not None:
            sub = np.asarray(subset, dtype=np.int64).reshape(-1)
            if m is not None and int(m) != len(sub):
                raise ValueError("schur_device: m and len (subset) differ")
            if out is not None:
                raise ValueError("schur_device: out cannot be combined with subset")
            m = len(sub)
            if m > n or len(set(sub.tolist())) != m or (m and (sub.min() < 0 or sub.max() >= n)):
                raise ValueError("schur_device: subset must hold distinct variables 0 .. n-1 of A")
            tail = self.schur_index(Lf, m)
            if set(tail.tolist()) != set(sub.tolist()):
                raise ValueError("schur_device: subset is not the set of the last len (subset) variables of the factor's "
                                 "ordering; analyze with schur_perm (A, subset) on a Session with postorder=False (the "
                                 "weighted postorder may move a variable of the subset)")
            pos = {int(v): k for k, v in enumerate(tail)}
            order = np.array([pos[int(v)] for v in sub], dtype=np.int64)
        if m is None:
            raise ValueError("schur_device: m or subset is needed")
        m = int(m)
        if not 0 <= m <= n:
            raise ValueError(f"schur_device: m must lie in 0 .. n = {n}")
        dev = torch.device("cuda", torch.cuda.current_device())
        So, Fo = (out if isinstance(out, (tuple, list)) else (out, None)) if out is not None else (None, None)
        Sc = torch.empty((m, m), dtype=torch.float64, device=dev) if So is None else So
        lds = self._square_layout("schur_device: out", m, Sc, dev)
        Fb, ldf = None, max(m, 1)
        if factor:
            Fb = torch.empty((m, m), dtype=torch.float64, device=dev) if Fo is None else Fo
            ldf = self._square_layout("schur_device: out [1]", m, Fb, dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        ok = self.L.cholmod_l_hip_schur_device(Lf, m, Sc.data_ptr() or 1, lds, (Fb.data_ptr() or 2) if factor else None, ldf,
                                               stream, C.byref(self.cm))
        if not ok:
            raise RuntimeError(f"cholmod_l_hip_schur_device failed, status {self.cm.status}")
        F = Fb.t() if factor else None
        if order is not None:
            idx = torch.as_tensor(order, device=dev)
            Sc = Sc.index_select(0, idx).index_select(1, idx)
            # (a symmetric permutation of L22 is not triangular: with subset, F stays in the factor's order)
        return (Sc, F) if factor else Sc

    def schur_reduce_device(self, Lf, m, B):
        """cholmod_l_hip_schur_reduce_device: the condensed right-hand side.  B: device tensor as for `solve_device`, shape
        (nrhs, n) or (n,), in A's ordering.  Returns (G, Y): G of shape (nrhs, m) (or (m,)), B_S - A_SI inv (A_II) B_I for
        S = `schur_index (Lf, m)`; Y of the shape of B, inv (L) P B in the factor's ordering, for `schur_expand_device`.
        Enqueued on torch's current stream."""
        import torch
        n, m = int(Lf.contents.n), int(m)
        if not 0 <= m <= n:
            raise ValueError(f"schur_reduce_device: m must lie in 0 .. n = {n}")
        ldb, nrhs = self._device_layout("schur_reduce_device: B", n, B)
        Y = torch.empty(B.shape, dtype=torch.float64, device=B.device)
        G = torch.empty(B.shape[:-1] + (m,), dtype=torch.float64, device=B.device)
        stream = torch.cuda.current_stream(B.device).cuda_stream
        ok = self.L.cholmod_l_hip_schur_reduce_device(Lf, m, B.data_ptr() or 1, ldb, Y.data_ptr() or 2, n, G.data_ptr() or 3,
                                                      max(m, 1), nrhs, stream, C.byref(self.cm))
        if not ok:
            raise RuntimeError(f"cholmod_l_hip_schur_reduce_device failed, status {self.cm.status}")
        return G, Y

    def schur_expand_device(self, Lf, m, Y, XS, out=None):
        """cholmod_l_hip_schur_expand_device: the solution on all variables from the solution XS on S = `schur_index (Lf,
        m)` (shape (nrhs, m) or (m,), of Sc x_S = G or of what the caller has added to both) and the Y of
        `schur_reduce_device` (read only).  Returns X of the shape of Y in A's ordering, or writes into `out` (never Y).
        m = 0: the plain solve P' inv (L') Y.  Enqueued on torch's current stream."""
        import torch
        n, m = int(Lf.contents.n), int(m)
        if not 0 <= m <= n:
            raise ValueError(f"schur_expand_device: m must lie in 0 .. n = {n}")
        ldy, nrhs = self._device_layout("schur_expand_device: Y", n, Y)
        if not (isinstance(XS, torch.Tensor) and XS.dim() == Y.dim() and XS.shape[:-1] == Y.shape[:-1]):
            raise ValueError("schur_expand_device: XS must have one right-hand side per right-hand side of Y")
        ldxs, _ = self._device_layout("schur_expand_device: XS", m, XS)
        if XS.device != Y.device:
            raise ValueError("schur_expand_device: XS must be on the device of Y")
        if out is None:
            out = torch.empty(Y.shape, dtype=torch.float64, device=Y.device)
        ldx, _ = self._device_layout("schur_expand_device: out", n, out, like=Y)
        stream = torch.cuda.current_stream(Y.device).cuda_stream
        ok = self.L.cholmod_l_hip_schur_expand_device(Lf, m, Y.data_ptr() or 2, ldy, XS.data_ptr() or 3, max(ldxs, 1),
                                                      out.data_ptr() or 1, ldx, nrhs, stream, C.byref(self.cm))
        if not ok:
            raise RuntimeError(f"cholmod_l_hip_schur_expand_device failed, status {self.cm.status}")
        return out

    @staticmethod
    def schur_perm(A, subset):
        """A permutation for `analyze` that orders `subset` (distinct variables of A) LAST, in the given order: the
        built-in fill-reducing ordering of the principal submatrix of A on the other variables (for an unsymmetric A,
        stype 0, whose A A' is factorized: of its rows), then subset.  Analyze with it on a Session with postorder=False:
        the weighted postorder may move a variable of the subset.  A pure host helper: the submatrix's pattern is analyzed
        on the host and its Perm read."""
        a = A.contents
        n = int(a.nrow)
        sub = np.asarray(subset, dtype=np.int64).reshape(-1)
        if len(sub) and (sub.min() < 0 or sub.max() >= n):
            raise ValueError("schur_perm: subset holds a variable outside 0 .. n-1")
        if len(set(sub.tolist())) != len(sub):
            raise ValueError("schur_perm: subset holds a variable twice")
        keep = np.ones(n, dtype=bool)
        keep[sub] = False
        rest = np.flatnonzero(keep).astype(np.int64)
        if len(rest) == 0:
            return sub.copy()
        ncol = int(a.ncol)
        Ap = _view(a.p, ncol + 1, C.c_int64, np.int64)
        if a.packed:
            cnt = np.diff(Ap)
        else:
            cnt = _view(a.nz, ncol, C.c_int64, np.int64)
        col = np.repeat(np.arange(ncol, dtype=np.int64), cnt)
        pos = np.concatenate([np.arange(Ap[j], Ap[j] + cnt[j], dtype=np.int64) for j in range(ncol)]) if ncol else np.zeros(0, np.int64)
        row = _view(a.i, max(int(Ap[-1]), 1), C.c_int64, np.int64)[pos] if len(pos) else np.zeros(0, np.int64)
        newid = np.full(n, -1, dtype=np.int64)
        newid[rest] = np.arange(len(rest))
        if a.stype != 0:
            ok = keep[row] & keep[col]
            r, c, nc = newid[row[ok]], newid[col[ok]], len(rest)
        else:
            ok = keep[row]
            r, c, nc = newid[row[ok]], col[ok], ncol
        o = np.lexsort((r, c))
        r, c = r[o], c[o]
        Bp = np.zeros(nc + 1, dtype=np.int64)
        np.add.at(Bp, c + 1, 1)
        Bp = np.cumsum(Bp)
        S = Session(use_gpu=0, ordering="default")
        nzb = max(int(Bp[-1]), 1)
        Bm = S.L.cholmod_l_allocate_sparse(len(rest), nc, nzb, 1, 1, int(a.stype), REAL, C.byref(S.cm))
        if not Bm:
            raise MemoryError("cholmod_l_allocate_sparse")
        _view(Bm.contents.p, nc + 1, C.c_int64, np.int64)[:] = Bp
        if len(r):
            _view(Bm.contents.i, len(r), C.c_int64, np.int64)[:] = r
            _view(Bm.contents.x, len(r), C.c_double, np.float64)[:] = 1.0
        try:
            Lf = S.analyze(Bm)
            head = _view(Lf.contents.Perm, len(rest), C.c_int64, np.int64).copy()
            S.free_factor(Lf)
        finally:
            S.free_sparse(Bm)
            S.finish()
        return np.concatenate([rest[head], sub])

    def solve_subset(self, Lf, b, bset, sys=SYS_A, handles=None):
        """cholmod_l_solve2 with a sparse right-hand side: b (length n, only its entries at the indices `bset` are
        read).  Returns (x, xset): x of length n -- defined at the indices xset only, NaN elsewhere when the handles
        are fresh -- and xset in the order the library produced it.  `handles`: a dict kept by the caller between calls
        (the X / Xset / Y workspaces of the reference's interface); free with free_subset_handles."""
        h = handles if handles is not None else {}
        n = int(Lf.contents.n)
        B = self.dense(b)
        bset = np.ascontiguousarray(bset, dtype=np.int64)
        Bs = self.L.cholmod_l_allocate_sparse(n, 1, max(len(bset), 1), 0, 1, 0, PATTERN, C.byref(self.cm))
        _view(Bs.contents.p, 2, C.c_int64, np.int64)[:] = [0, len(bset)]
        if len(bset):
            _view(Bs.contents.i, len(bset), C.c_int64, np.int64)[:] = bset
        X = h.get("X") or C.POINTER(Dense)()
        Xs = h.get("Xset") or C.POINTER(Sparse)()
        Y = h.get("Y") or C.POINTER(Dense)()
        E = C.POINTER(Dense)()
        fresh = not bool(X)
        ok = self.L.cholmod_l_solve2(sys, Lf, B, Bs, C.byref(X), C.byref(Xs), C.byref(Y), C.byref(E), C.byref(self.cm))
        self.free_dense(B)
        self.free_sparse(Bs)
        h.update(X=X, Xset=Xs, Y=Y)
        try:
            if not ok:
                raise RuntimeError(f"cholmod_l_solve2 (Bset) failed, status {self.cm.status}")
            k = int(_view(Xs.contents.p, 2, C.c_int64, np.int64)[1])
            xset = _view(Xs.contents.i, max(k, 1), C.c_int64, np.int64)[:k].copy()
            xall = self.dense_to_numpy(X)
            x = np.full(n, np.nan, dtype=xall.dtype) if fresh else xall.copy()
            x[xset] = xall[xset]
            return x, xset
        finally:
            if handles is None:
                self.free_subset_handles(h)

    def free_subset_handles(self, h):
        for k, fr in (("X", self.free_dense), ("Y", self.free_dense), ("Xset", self.free_sparse)):
            if h.get(k):
                fr(h[k])
            h.pop(k, None)

    def hip_stats(self, Lf):
        s = (C.c_double * CHOLMOD_HIP_NSTATS)()
        self.L.cholmod_l_hip_stats(Lf, C.byref(s), C.byref(self.cm))
        return np.array(list(s))

    def factor_checks(self, Lf):
        """Invariants of the device-resident factor (cholmod_hip_factor_checks):
        dict(half_logdet, upper_nonzeros, nonfinite, fro2, nonpositive_diag)."""
        out = np.zeros(5)
        rc = self.L.cholmod_hip_factor_checks(Lf.contents.hip_plan, out.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"cholmod_hip_factor_checks failed: {rc}")
        return dict(half_logdet=out[0], upper_nonzeros=int(out[1]), nonfinite=int(out[2]),
                    fro2=out[3], nonpositive_diag=int(out[4]))

    def factor_checks_local(self, Lf):
        """This rank's share of the invariants of a distributed factor (cholmod_hip_factor_checks_local):
        the five numbers as an array; their sums over the ranks are those of the complete factor."""
        out = np.zeros(5)
        f = Lf.contents
        plan = C.cast(f.cx_twin, C.POINTER(Factor)).contents.hip_plan if f.cx_twin else f.hip_plan
        rc = self.L.cholmod_hip_factor_checks_local(plan, out.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"cholmod_hip_factor_checks_local failed: {rc}")
        return out

    def launch_profile(self, Lf):
        """Per-launch (kind, grid, aux, ms, flops, bytes) of the last profiled factorization."""
        plan = Lf.contents.hip_plan
        nl = self.L.cholmod_hip_get_launch_profile(plan, 0, None, None, None, None, None, None)
        kind = np.zeros(nl, dtype=np.int32); grid = np.zeros(nl, dtype=np.int32); aux = np.zeros(nl, dtype=np.int32)
        ms = np.zeros(nl); fl = np.zeros(nl); by = np.zeros(nl)
        self.L.cholmod_hip_get_launch_profile(plan, nl, kind.ctypes.data, grid.ctypes.data, aux.ctypes.data,
                                              ms.ctypes.data, fl.ctypes.data, by.ctypes.data)
        return dict(kind=kind, grid=grid, aux=aux, ms=ms, flops=fl, bytes=by)

    def set_profiling(self, Lf, on=True):
        if Lf.contents.hip_plan:
            self.L.cholmod_hip_set_profiling(Lf.contents.hip_plan, int(on))


class FactorView:
    """numpy views of a cholmod_factor's supernodal fields."""

    def __init__(self, Lf):
        f = Lf.contents
        self.n, self.nsuper = int(f.n), int(f.nsuper)
        self.ssize, self.xsize = int(f.ssize), int(f.xsize)
        self.maxcsize, self.maxesize, self.minor = int(f.maxcsize), int(f.maxesize), int(f.minor)
        self.ordering, self.is_super, self.is_ll, self.xtype = f.ordering, f.is_super, f.is_ll, f.xtype
        self.useGPU = f.useGPU
        self.Perm = _view(f.Perm, self.n, C.c_int64, np.int64)
        self.ColCount = _view(f.ColCount, self.n, C.c_int64, np.int64)
        self.super = _view(f.super, self.nsuper + 1, C.c_int64, np.int64)
        self.pi = _view(f.pi, self.nsuper + 1, C.c_int64, np.int64)
        self.px = _view(f.px, self.nsuper + 1, C.c_int64, np.int64)
        self.s = _view(f.s, self.ssize, C.c_int64, np.int64)
        if f.x and f.xtype == COMPLEX:      # interleaved (re, im) pairs
            self.x = _view(f.x, 2 * self.xsize, C.c_double, np.float64).view(np.complex128)
        else:
            self.x = _view(f.x, self.xsize, C.c_double, np.float64) if f.x else None
        self.hip_plan = f.hip_plan
        self.cx_twin = f.cx_twin
