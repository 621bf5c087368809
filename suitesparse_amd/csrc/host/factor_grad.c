/* factor_grad.c -- the gradient through the factor, in the host layer (cholmod.h): for a scalar f of the entries of L,
 * cholmod_l_hip_factor_grad_device turns Lbar = df/dL (an array of the caller's in the layout of L->x, in device memory) into
 * the gradient with respect to the values of A and with respect to beta, cholmod_l_hip_factor_outer_grad_device does the
 * same for Lbar = alpha P Q' sampled on the pattern of L -- the form the gradients of the two triangular solves take --, and
 * cholmod_l_hip_factor_grad_to_host hands out the whole of Gx = df/dS on the pattern of L.  All run on the engine
 * (cholmod_hip_factor_grad_*, csrc/hip/factor_grad.hip) against the factor that is resident on the device; there is no host
 * fallback.  Every argument is checked before a device is touched. */
#include "host_internal.h"

static int fg_status (int rc, cholmod_common *Common, const char *what)
{
    switch (rc)
    {
        case CHOLMOD_HIP_OK: return TRUE ;
        case CHOLMOD_HIP_OUT_OF_MEMORY: ERROR (CHOLMOD_OUT_OF_MEMORY, what) ; return FALSE ;
        case CHOLMOD_HIP_INVALID: ERROR (CHOLMOD_INVALID, what) ; return FALSE ;
        default: ERROR (CHOLMOD_GPU_PROBLEM, what) ; return FALSE ;
    }
}

/* what every entry point asks of L; TRUE: L->hip_plan holds its numeric, positive definite factor */
static int fg_factor_ready (cholmod_factor *L, cholmod_common *Common)
{
    if (L->xtype == CHOLMOD_COMPLEX || L->xtype == CHOLMOD_ZOMPLEX)
    { ERROR (CHOLMOD_NOT_INSTALLED, "the gradient through a complex factor is not supported") ; return FALSE ; }
    if (L->xtype != CHOLMOD_REAL || !L->is_super)
    { ERROR (CHOLMOD_INVALID, "L must be a numeric supernodal factor") ; return FALSE ; }
    if (L->minor < L->n) { ERROR (CHOLMOD_INVALID, "L is not positive definite") ; return FALSE ; }
    /* the sweep runs on the factor in device memory: no fallback, whatever Common->hip_cpu_fallback says */
    if (ssamd_resolve_use_gpu (Common) != 1) { ERROR (CHOLMOD_INVALID, "the factor gradient needs Common->useGPU") ; return FALSE ; }
    if (Common->hip_world > 1) { ERROR (CHOLMOD_INVALID, "the factor gradient runs on one rank only") ; return FALSE ; }
    if (!L->hip_plan || !L->hip_on_device)
    { ERROR (CHOLMOD_INVALID, "L was not factorized on the device") ; return FALSE ; }
    return TRUE ;
}

/* what both device entry points ask of A (needed with G_dev only), L and the outputs, as cholmod_l_hip_selinv_device asks
 * it for Z_dev: TRUE with *annz = nnz (A): the plan's value map fits A */
static int fg_ready (cholmod_sparse *A, cholmod_factor *L, double *G_dev, size_t *annz, cholmod_common *Common)
{
    *annz = 0 ;
    if (G_dev)
    {
        RETURN_IF_NULL (A, FALSE) ;
        RETURN_IF_NULL (A->p, FALSE) ;
    }
    if (A && (A->xtype == CHOLMOD_COMPLEX || A->xtype == CHOLMOD_ZOMPLEX))
    { ERROR (CHOLMOD_NOT_INSTALLED, "the gradient through the factor of a complex matrix is not supported") ; return FALSE ; }
    if (L->xtype == CHOLMOD_COMPLEX || L->xtype == CHOLMOD_ZOMPLEX)
    { ERROR (CHOLMOD_NOT_INSTALLED, "the gradient through a complex factor is not supported") ; return FALSE ; }
    if (G_dev)
    {
        if (A->xtype != CHOLMOD_REAL && A->xtype != CHOLMOD_PATTERN) { ERROR (CHOLMOD_INVALID, "invalid xtype") ; return FALSE ; }
        /* (A*A' and column subsets: the caller's entries are then not the entries of the factorized matrix) */
        if (A->stype == 0) { ERROR (CHOLMOD_INVALID, "G_dev needs a symmetric A (stype != 0)") ; return FALSE ; }
        if (!A->packed) { ERROR (CHOLMOD_INVALID, "A must be packed") ; return FALSE ; }
        if (A->nrow != L->n || A->nrow != A->ncol) { ERROR (CHOLMOD_INVALID, "A and L dimensions do not match") ; return FALSE ; }
        *annz = (size_t) ((Int *) A->p) [A->ncol] ;
        if (*annz > 0 && !A->i) { ERROR (CHOLMOD_INVALID, "argument missing") ; return FALSE ; }
    }
    if (!fg_factor_ready (L, Common)) return FALSE ;
    if (G_dev)
    {
        if (!L->hip_apat_valid)
        { ERROR (CHOLMOD_INVALID, "L holds no pattern record: cholmod_l_factorize from a host matrix of this pattern first") ; return FALSE ; }
        /* the proof that the plan's value map fits A, as in cholmod_l_hip_selinv_device: a mismatch touches no device state */
        uint64_t hash [2] ;
        hash [0] = ssamd_pattern_hash (A, &hash [1]) ;
        if (L->hip_apat_nnz != *annz || L->hip_apat_hash != hash [0] || L->hip_apat_hash2 != hash [1])
        { ERROR (CHOLMOD_INVALID, "A does not have the pattern L was last factorized from") ; return FALSE ; }
    }
    return TRUE ;
}

int cholmod_l_hip_factor_grad_device (cholmod_sparse *A, cholmod_factor *L, const double *Lbar_dev, double *G_dev,
    double *trace_dev, void *stream, cholmod_common *Common)
{
    RETURN_IF_NULL_COMMON (FALSE) ;
    RETURN_IF_NULL (L, FALSE) ;
    RETURN_IF_NULL (Lbar_dev, FALSE) ;
    size_t annz = 0 ;
    if (!fg_ready (A, L, G_dev, &annz, Common)) return FALSE ;
    Common->status = CHOLMOD_OK ;
    if (L->n == 0) return TRUE ;
    cholmod_hip_plan *plan = (cholmod_hip_plan *) L->hip_plan ;
    if (!fg_status (cholmod_hip_factor_grad_device (plan, Lbar_dev, stream), Common,
        "the factor gradient could not be computed on the device")) return FALSE ;
    return fg_status (cholmod_hip_factor_grad_gather_device (plan, G_dev, (int64_t) annz, trace_dev, stream), Common,
        "the plan holds no value map for this matrix") ;
}

int cholmod_l_hip_factor_outer_grad_device (cholmod_sparse *A, cholmod_factor *L, double alpha, const double *P_dev, size_t ldp,
    const double *Q_dev, size_t ldq, size_t nrhs, double *G_dev, double *trace_dev, void *stream, cholmod_common *Common)
{
    RETURN_IF_NULL_COMMON (FALSE) ;
    RETURN_IF_NULL (L, FALSE) ;
    RETURN_IF_NULL (P_dev, FALSE) ;
    RETURN_IF_NULL (Q_dev, FALSE) ;
    if (ldp < L->n || ldq < L->n) { ERROR (CHOLMOD_INVALID, "leading dimension smaller than n") ; return FALSE ; }
    size_t annz = 0 ;
    if (!fg_ready (A, L, G_dev, &annz, Common)) return FALSE ;
    Common->status = CHOLMOD_OK ;
    if (L->n == 0) return TRUE ;
    cholmod_hip_plan *plan = (cholmod_hip_plan *) L->hip_plan ;
    if (!fg_status (cholmod_hip_factor_outer_grad_device (plan, alpha, P_dev, (int64_t) ldp, Q_dev, (int64_t) ldq, (int64_t) nrhs,
        stream), Common, "the factor gradient could not be computed on the device")) return FALSE ;
    return fg_status (cholmod_hip_factor_grad_gather_device (plan, G_dev, (int64_t) annz, trace_dev, stream), Common,
        "the plan holds no value map for this matrix") ;
}

int cholmod_l_hip_factor_grad_to_host (cholmod_factor *L, double *Gx, cholmod_common *Common)
{
    RETURN_IF_NULL_COMMON (FALSE) ;
    RETURN_IF_NULL (L, FALSE) ;
    RETURN_IF_NULL (Gx, FALSE) ;
    if (!fg_factor_ready (L, Common)) return FALSE ;
    Common->status = CHOLMOD_OK ;
    if (L->n == 0) return TRUE ;
    /* (no Lbar is known here: a Gx that is stale or was never computed is refused) */
    return fg_status (cholmod_hip_factor_grad_download ((cholmod_hip_plan *) L->hip_plan, Gx), Common,
        "the plan holds no current factor gradient: cholmod_l_hip_factor_grad_device first") ;
}
