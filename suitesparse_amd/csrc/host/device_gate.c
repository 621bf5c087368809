/* device_gate.c -- what the entry points that work on the device-resident factor (selinv.c, grad.c, factor_grad.c, schur.c,
 * the residual and the complex trio of numeric.c) ask alike before a device is touched, once: the map from the engine's
 * status to Common->status, the rule "real, supernodal, positive definite, one rank, Common->useGPU, factorized on the
 * device", the check that a matrix of values has the pattern L was last factorized from, the permutation on the plan,
 * and a current selected inverse.  A feature passes its own texts (ssamd_device_feature, host_internal.h): what a caller
 * reads in Common->error_handler is the feature's wording, the order of the checks is the same for all. */
#include "host_internal.h"

int ssamd_device_status (int rc, cholmod_common *Common, const char *what)
{
    switch (rc)
    {
        case CHOLMOD_HIP_OK: return TRUE ;
        case CHOLMOD_HIP_OUT_OF_MEMORY: ERROR (CHOLMOD_OUT_OF_MEMORY, what) ; return FALSE ;
        case CHOLMOD_HIP_INVALID: ERROR (CHOLMOD_INVALID, what) ; return FALSE ;
        default: ERROR (CHOLMOD_GPU_PROBLEM, what) ; return FALSE ;
    }
}

/* TRUE: L->hip_plan holds L's numeric factor (need_posdef: a positive definite one), computed on the device */
int ssamd_resident_factor_ready (cholmod_factor *L, const ssamd_device_feature *feature, int need_posdef, cholmod_common *Common)
{
    if (L->xtype == CHOLMOD_COMPLEX || L->xtype == CHOLMOD_ZOMPLEX) { ERROR (CHOLMOD_NOT_INSTALLED, feature->complex_factor) ; return FALSE ; }
    if (L->xtype != CHOLMOD_REAL || !L->is_super)
    { ERROR (CHOLMOD_INVALID, "L must be a numeric supernodal factor") ; return FALSE ; }
    if (need_posdef && L->minor < L->n) { ERROR (CHOLMOD_INVALID, "L is not positive definite") ; return FALSE ; }
    /* the operands live in device memory: no fallback, whatever Common->hip_cpu_fallback says */
    if (ssamd_resolve_use_gpu (Common) != 1) { ERROR (CHOLMOD_INVALID, feature->use_gpu) ; return FALSE ; }
    if (Common->hip_world > 1) { ERROR (CHOLMOD_INVALID, feature->one_rank) ; return FALSE ; }
    if (!L->hip_plan || !L->hip_on_device)
    { ERROR (CHOLMOD_INVALID, "L was not factorized on the device") ; return FALSE ; }
    return TRUE ;
}

/* What an entry point asks of A, L and the smallest leading dimension it was passed (ld; L->n: none) when it samples on, or
 * gathers at, the entries of A: A is a packed, real or pattern, square symmetric matrix of L's size, L passes the gate
 * above, and A has the pattern L was last factorized from -- the proof that the plan's value map fits A; a mismatch
 * touches no device state.  wanted = FALSE (the caller takes no output on A's entries): A may be NULL and only its xtype is
 * looked at.  TRUE with *annz = nnz (A), 0 if it is not wanted. */
int ssamd_values_matrix_fits (cholmod_sparse *A, int wanted, cholmod_factor *L, size_t ld, int need_posdef,
    const ssamd_device_feature *feature, size_t *annz, cholmod_common *Common)
{
    *annz = 0 ;
    if (wanted)
    {
        RETURN_IF_NULL (A, FALSE) ;
        RETURN_IF_NULL (A->p, FALSE) ;
    }
    if (A && (A->xtype == CHOLMOD_COMPLEX || A->xtype == CHOLMOD_ZOMPLEX)) { ERROR (CHOLMOD_NOT_INSTALLED, feature->complex_matrix) ; return FALSE ; }
    if (L->xtype == CHOLMOD_COMPLEX || L->xtype == CHOLMOD_ZOMPLEX) { ERROR (CHOLMOD_NOT_INSTALLED, feature->complex_factor) ; return FALSE ; }
    if (wanted)
    {
        if (A->xtype != CHOLMOD_REAL && A->xtype != CHOLMOD_PATTERN) { ERROR (CHOLMOD_INVALID, "invalid xtype") ; return FALSE ; }
        /* (A*A' and column subsets: the caller's entries are then not the entries of the factorized matrix) */
        if (A->stype == 0) { ERROR (CHOLMOD_INVALID, feature->unsymmetric_matrix) ; return FALSE ; }
        if (!A->packed) { ERROR (CHOLMOD_INVALID, "A must be packed") ; return FALSE ; }
        if (A->nrow != L->n || A->nrow != A->ncol) { ERROR (CHOLMOD_INVALID, "A and L dimensions do not match") ; return FALSE ; }
        if (ld < L->n) { ERROR (CHOLMOD_INVALID, "leading dimension smaller than n") ; return FALSE ; }
        *annz = (size_t) ((Int *) A->p) [A->ncol] ;
        if (*annz > 0 && !A->i) { ERROR (CHOLMOD_INVALID, "argument missing") ; return FALSE ; }
    }
    if (!ssamd_resident_factor_ready (L, feature, need_posdef, Common)) return FALSE ;
    if (wanted)
    {
        if (!L->hip_apat_valid)
        { ERROR (CHOLMOD_INVALID, "L holds no pattern record: cholmod_l_factorize from a host matrix of this pattern first") ; return FALSE ; }
        uint64_t hash [2] ;
        hash [0] = ssamd_pattern_hash (A, &hash [1]) ;
        if (L->hip_apat_nnz != *annz || L->hip_apat_hash != hash [0] || L->hip_apat_hash2 != hash [1])
        { ERROR (CHOLMOD_INVALID, "A does not have the pattern L was last factorized from") ; return FALSE ; }
    }
    return TRUE ;
}

/* L->Perm to L's plan on first use (a new plan clears L->hip_perm_set) */
int ssamd_perm_ready (cholmod_factor *L, cholmod_common *Common)
{
    if (L->hip_perm_set) return TRUE ;
    int rc = cholmod_hip_set_perm ((cholmod_hip_plan *) L->hip_plan, (const int64_t *) L->Perm) ;
    if (rc != CHOLMOD_HIP_OK) return ssamd_device_status (rc, Common, "the permutation could not be stored on the device") ;
    L->hip_perm_set = TRUE ;
    return TRUE ;
}

/* Zx of the plan current: computed now, on `stream`, if it is stale */
int ssamd_selinv_current (cholmod_hip_plan *plan, void *stream, cholmod_common *Common)
{
    double info [8] ;
    int rc = cholmod_hip_selinv_info (plan, info) ;
    if (rc == CHOLMOD_HIP_OK && info [6] == 0) rc = cholmod_hip_selinv_device (plan, stream) ;
    return ssamd_device_status (rc, Common, "the selected inverse could not be computed on the device") ;
}
