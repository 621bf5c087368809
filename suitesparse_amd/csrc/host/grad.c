/* grad.c -- what backpropagation through the device path needs, in the host layer (cholmod.h):
 * cholmod_l_hip_values_grad_device samples alpha (U V' + V U') on the entries of A the factorization reads -- the gradient of
 * a scalar with respect to A's values through a solve --, cholmod_l_hip_logdet_device leaves log det (A + beta I) of the
 * resident factor in device memory.  cholmod_l_hip_aat_values_grad_device / cholmod_l_hip_aat_logdet_grad_device are the
 * gradients with respect to the values of an UNSYMMETRIC A through L L' = A*A' + beta*I (the chain rule through the product
 * map of cholmod_l_hip_factorize_values_device).  All run on the engine (cholmod_hip_values_grad_device,
 * cholmod_hip_logdet_device, cholmod_hip_product_*_grad_device, csrc/hip/grad.hip); there is no host fallback.  Every
 * argument is checked before a device is touched. */
#include "host_internal.h"

static const ssamd_device_feature grad_feature = {
    "gradients of a complex factor are not supported", "device gradients need Common->useGPU",
    "device gradients run on one rank only",
    "gradients of a complex matrix are not supported", "the gradient needs a symmetric A (stype != 0)" } ;

int cholmod_l_hip_values_grad_device (cholmod_sparse *A, cholmod_factor *L, double alpha, const double *U_dev, size_t ldu,
    const double *V_dev, size_t ldv, size_t nrhs, double *G_dev, void *stream, cholmod_common *Common)
{
    RETURN_IF_NULL_COMMON (FALSE) ;
    RETURN_IF_NULL (A, FALSE) ;
    RETURN_IF_NULL (L, FALSE) ;
    RETURN_IF_NULL (U_dev, FALSE) ;
    RETURN_IF_NULL (V_dev, FALSE) ;
    RETURN_IF_NULL (G_dev, FALSE) ;
    RETURN_IF_NULL (A->p, FALSE) ;
    size_t annz = 0 ;
    if (!ssamd_values_matrix_fits (A, TRUE, L, ldu < ldv ? ldu : ldv, FALSE, &grad_feature, &annz, Common)) return FALSE ;
    Common->status = CHOLMOD_OK ;
    if (L->n == 0 || annz == 0) return TRUE ;
    cholmod_hip_plan *plan = (cholmod_hip_plan *) L->hip_plan ;
    if (!ssamd_perm_ready (L, Common)) return FALSE ;
    return ssamd_device_status (cholmod_hip_values_grad_device (plan, 1, alpha, U_dev, (int64_t) ldu, V_dev, (int64_t) ldv,
        (int64_t) nrhs, G_dev, (int64_t) annz, stream), Common, "the plan holds no value map for this matrix") ;
}

int cholmod_l_hip_logdet_device (cholmod_factor *L, double *out_dev, void *stream, cholmod_common *Common)
{
    RETURN_IF_NULL_COMMON (FALSE) ;
    RETURN_IF_NULL (L, FALSE) ;
    RETURN_IF_NULL (out_dev, FALSE) ;
    if (!ssamd_resident_factor_ready (L, &grad_feature, TRUE, Common)) return FALSE ;
    Common->status = CHOLMOD_OK ;
    return ssamd_device_status (cholmod_hip_logdet_device ((cholmod_hip_plan *) L->hip_plan, out_dev, stream), Common,
        "the plan holds no positive definite factor on the device") ;
}

/* ---- through A*A' + beta*I ------------------------------------------------------------------------------------------------ */

/* what both entry points ask of A and L (ld: the smallest leading dimension passed), and the product map (built here if this
 * is the first call for the pattern, by the helper cholmod_l_hip_factorize_values_device uses).  TRUE: L->hip_plan holds
 * tril (A*A') with its product map. */
static int gr_aat_ready (cholmod_sparse *A, cholmod_factor *L, int posdef, size_t ld, size_t *annz_out, cholmod_common *Common)
{
    if (A->xtype == CHOLMOD_COMPLEX || A->xtype == CHOLMOD_ZOMPLEX) { ERROR (CHOLMOD_NOT_INSTALLED, grad_feature.complex_matrix) ; return FALSE ; }
    if (L->xtype == CHOLMOD_COMPLEX || L->xtype == CHOLMOD_ZOMPLEX) { ERROR (CHOLMOD_NOT_INSTALLED, grad_feature.complex_factor) ; return FALSE ; }
    if (A->xtype != CHOLMOD_REAL && A->xtype != CHOLMOD_PATTERN) { ERROR (CHOLMOD_INVALID, "invalid xtype") ; return FALSE ; }
    if (A->stype != 0)
    { ERROR (CHOLMOD_INVALID, "the gradient through A*A' needs an unsymmetric A (stype == 0); a symmetric A: cholmod_l_hip_values_grad_device") ; return FALSE ; }
    if (!A->packed) { ERROR (CHOLMOD_INVALID, "A must be packed") ; return FALSE ; }
    if (A->nrow != L->n) { ERROR (CHOLMOD_INVALID, "A and L dimensions do not match") ; return FALSE ; }
    if (ld < L->n) { ERROR (CHOLMOD_INVALID, "leading dimension smaller than n") ; return FALSE ; }
    const size_t annz = (size_t) ((Int *) A->p) [A->ncol] ;
    if (annz > 0 && !A->i) { ERROR (CHOLMOD_INVALID, "argument missing") ; return FALSE ; }
    if (!ssamd_resident_factor_ready (L, &grad_feature, posdef, Common)) return FALSE ;
    if (!L->hip_apat_valid)
    { ERROR (CHOLMOD_INVALID, "L holds no pattern record: cholmod_l_factorize from a host matrix of this pattern first") ; return FALSE ; }
    Common->status = CHOLMOD_OK ;
    *annz_out = annz ;
    if (L->n == 0 || annz == 0) return TRUE ;
    uint64_t hash [2] ;
    hash [0] = ssamd_pattern_hash (A, &hash [1]) ;
    return ssamd_aat_product_map_ready (A, L, annz, hash, Common) ;
}

int cholmod_l_hip_aat_values_grad_device (cholmod_sparse *A, cholmod_factor *L, double alpha, const double *U_dev, size_t ldu,
    const double *V_dev, size_t ldv, size_t nrhs, const double *Avalues_dev, double *G_dev, void *stream, cholmod_common *Common)
{
    RETURN_IF_NULL_COMMON (FALSE) ;
    RETURN_IF_NULL (A, FALSE) ;
    RETURN_IF_NULL (L, FALSE) ;
    RETURN_IF_NULL (U_dev, FALSE) ;
    RETURN_IF_NULL (V_dev, FALSE) ;
    RETURN_IF_NULL (Avalues_dev, FALSE) ;
    RETURN_IF_NULL (G_dev, FALSE) ;
    RETURN_IF_NULL (A->p, FALSE) ;
    size_t annz = 0 ;
    if (!gr_aat_ready (A, L, FALSE, ldu < ldv ? ldu : ldv, &annz, Common)) return FALSE ;
    if (L->n == 0 || annz == 0) return TRUE ;
    cholmod_hip_plan *plan = (cholmod_hip_plan *) L->hip_plan ;
    if (!ssamd_perm_ready (L, Common)) return FALSE ;
    return ssamd_device_status (cholmod_hip_product_values_grad_device (plan, 1, alpha, U_dev, (int64_t) ldu, V_dev, (int64_t) ldv,
        (int64_t) nrhs, Avalues_dev, G_dev, (int64_t) annz, stream), Common, "the plan holds no product map for this matrix") ;
}

int cholmod_l_hip_aat_logdet_grad_device (cholmod_sparse *A, cholmod_factor *L, const double *Avalues_dev, double *G_dev,
    void *stream, cholmod_common *Common)
{
    RETURN_IF_NULL_COMMON (FALSE) ;
    RETURN_IF_NULL (A, FALSE) ;
    RETURN_IF_NULL (L, FALSE) ;
    RETURN_IF_NULL (Avalues_dev, FALSE) ;
    RETURN_IF_NULL (G_dev, FALSE) ;
    RETURN_IF_NULL (A->p, FALSE) ;
    size_t annz = 0 ;
    if (!gr_aat_ready (A, L, TRUE, L->n, &annz, Common)) return FALSE ;
    if (L->n == 0 || annz == 0) return TRUE ;
    cholmod_hip_plan *plan = (cholmod_hip_plan *) L->hip_plan ;
    if (!ssamd_selinv_current (plan, stream, Common)) return FALSE ;
    return ssamd_device_status (cholmod_hip_product_logdet_grad_device (plan, Avalues_dev, G_dev, (int64_t) annz, stream), Common,
        "the plan holds no product map for this matrix") ;
}
