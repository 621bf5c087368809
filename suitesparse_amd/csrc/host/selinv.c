/* selinv.c -- the selected inverse of the host layer (cholmod.h): cholmod_l_hip_selinv_device hands a PyTorch or HIP caller
 * the entries of (A + beta I)^-1 at the entries of A and its diagonal in device memory, cholmod_l_hip_selinv_to_host the
 * whole subset in the layout of L->x -- what the reference ships as MATLAB_Tools/sparseinv (there on a simplicial LDL',
 * column by column).  Both run on the engine (cholmod_hip_selinv_*, csrc/hip/selinv.hip) against the factor that is
 * resident on the device; there is no host fallback.  Every argument is checked before a device is touched. */
#include "host_internal.h"

static int si_status (int rc, cholmod_common *Common, const char *what)
{
    switch (rc)
    {
        case CHOLMOD_HIP_OK: return TRUE ;
        case CHOLMOD_HIP_OUT_OF_MEMORY: ERROR (CHOLMOD_OUT_OF_MEMORY, what) ; return FALSE ;
        case CHOLMOD_HIP_INVALID: ERROR (CHOLMOD_INVALID, what) ; return FALSE ;
        default: ERROR (CHOLMOD_GPU_PROBLEM, what) ; return FALSE ;
    }
}

/* what both entry points ask of L; TRUE: L->hip_plan holds its numeric, positive definite factor */
static int si_factor_ready (cholmod_factor *L, cholmod_common *Common)
{
    if (L->xtype == CHOLMOD_COMPLEX || L->xtype == CHOLMOD_ZOMPLEX)
    { ERROR (CHOLMOD_NOT_INSTALLED, "the selected inverse of a complex factor is not supported") ; return FALSE ; }
    if (L->xtype != CHOLMOD_REAL || !L->is_super)
    { ERROR (CHOLMOD_INVALID, "L must be a numeric supernodal factor") ; return FALSE ; }
    if (L->minor < L->n) { ERROR (CHOLMOD_INVALID, "L is not positive definite") ; return FALSE ; }
    /* the inverse is formed from the factor in device memory: no fallback, whatever Common->hip_cpu_fallback says */
    if (ssamd_resolve_use_gpu (Common) != 1) { ERROR (CHOLMOD_INVALID, "the selected inverse needs Common->useGPU") ; return FALSE ; }
    if (Common->hip_world > 1) { ERROR (CHOLMOD_INVALID, "the selected inverse runs on one rank only") ; return FALSE ; }
    if (!L->hip_plan || !L->hip_on_device)
    { ERROR (CHOLMOD_INVALID, "L was not factorized on the device") ; return FALSE ; }
    return TRUE ;
}

/* Zx of the plan current: computed now, on `stream`, if it is stale */
static int si_current (cholmod_hip_plan *plan, void *stream, cholmod_common *Common)
{
    double info [8] ;
    int rc = cholmod_hip_selinv_info (plan, info) ;
    if (rc == CHOLMOD_HIP_OK && info [6] == 0) rc = cholmod_hip_selinv_device (plan, stream) ;
    return si_status (rc, Common, "the selected inverse could not be computed on the device") ;
}

int cholmod_l_hip_selinv_device (cholmod_sparse *A, cholmod_factor *L, double *Z_dev, double *diag_dev, void *stream,
    cholmod_common *Common)
{
    RETURN_IF_NULL_COMMON (FALSE) ;
    RETURN_IF_NULL (L, FALSE) ;
    if (!Z_dev && !diag_dev) { ERROR (CHOLMOD_INVALID, "argument missing") ; return FALSE ; }
    size_t annz = 0 ;
    if (Z_dev)
    {
        RETURN_IF_NULL (A, FALSE) ;
        RETURN_IF_NULL (A->p, FALSE) ;
        if (A->xtype == CHOLMOD_COMPLEX || A->xtype == CHOLMOD_ZOMPLEX)
        { ERROR (CHOLMOD_NOT_INSTALLED, "the selected inverse of a complex matrix is not supported") ; return FALSE ; }
    }
    else if (A && (A->xtype == CHOLMOD_COMPLEX || A->xtype == CHOLMOD_ZOMPLEX))
    { ERROR (CHOLMOD_NOT_INSTALLED, "the selected inverse of a complex matrix is not supported") ; return FALSE ; }
    if (L->xtype == CHOLMOD_COMPLEX || L->xtype == CHOLMOD_ZOMPLEX)
    { ERROR (CHOLMOD_NOT_INSTALLED, "the selected inverse of a complex factor is not supported") ; return FALSE ; }
    if (Z_dev)
    {
        if (A->xtype != CHOLMOD_REAL && A->xtype != CHOLMOD_PATTERN) { ERROR (CHOLMOD_INVALID, "invalid xtype") ; return FALSE ; }
        /* (A*A' and column subsets: the caller's entries are then not the entries of the factorized matrix) */
        if (A->stype == 0) { ERROR (CHOLMOD_INVALID, "Z_dev needs a symmetric A (stype != 0)") ; return FALSE ; }
        if (!A->packed) { ERROR (CHOLMOD_INVALID, "A must be packed") ; return FALSE ; }
        if (A->nrow != L->n || A->nrow != A->ncol) { ERROR (CHOLMOD_INVALID, "A and L dimensions do not match") ; return FALSE ; }
        annz = (size_t) ((Int *) A->p) [A->ncol] ;
        if (annz > 0 && !A->i) { ERROR (CHOLMOD_INVALID, "argument missing") ; return FALSE ; }
    }
    if (!si_factor_ready (L, Common)) return FALSE ;
    if (Z_dev)
    {
        if (!L->hip_apat_valid)
        { ERROR (CHOLMOD_INVALID, "L holds no pattern record: cholmod_l_factorize from a host matrix of this pattern first") ; return FALSE ; }
        /* the proof that the plan's value map fits A, as in cholmod_l_hip_factorize_values_device: a mismatch touches no device state */
        uint64_t hash [2] ;
        hash [0] = ssamd_pattern_hash (A, &hash [1]) ;
        if (L->hip_apat_nnz != annz || L->hip_apat_hash != hash [0] || L->hip_apat_hash2 != hash [1])
        { ERROR (CHOLMOD_INVALID, "A does not have the pattern L was last factorized from") ; return FALSE ; }
    }
    Common->status = CHOLMOD_OK ;
    if (L->n == 0) return TRUE ;
    cholmod_hip_plan *plan = (cholmod_hip_plan *) L->hip_plan ;
    if (diag_dev && !L->hip_perm_set)
    {
        int rc = cholmod_hip_set_perm (plan, (const int64_t *) L->Perm) ;
        if (rc != CHOLMOD_HIP_OK) return si_status (rc, Common, "the permutation could not be stored on the device") ;
        L->hip_perm_set = TRUE ;
    }
    if (!si_current (plan, stream, Common)) return FALSE ;
    return si_status (cholmod_hip_selinv_gather_device (plan, Z_dev, (int64_t) annz, diag_dev, 1, stream), Common,
        "the plan holds no value map for this matrix") ;
}

int cholmod_l_hip_selinv_to_host (cholmod_factor *L, double *Zx, cholmod_common *Common)
{
    RETURN_IF_NULL_COMMON (FALSE) ;
    RETURN_IF_NULL (L, FALSE) ;
    RETURN_IF_NULL (Zx, FALSE) ;
    if (!si_factor_ready (L, Common)) return FALSE ;
    Common->status = CHOLMOD_OK ;
    if (L->n == 0) return TRUE ;
    cholmod_hip_plan *plan = (cholmod_hip_plan *) L->hip_plan ;
    if (!si_current (plan, NULL, Common)) return FALSE ;
    return si_status (cholmod_hip_selinv_download (plan, Zx), Common, "the selected inverse could not be copied to the host") ;
}
