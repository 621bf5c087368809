/* factor_grad.c -- the gradient through the factor, in the host layer (cholmod.h): for a scalar f of the entries of L,
 * cholmod_l_hip_factor_grad_device turns Lbar = df/dL (an array of the caller's in the layout of L->x, in device memory) into
 * the gradient with respect to the values of A and with respect to beta, cholmod_l_hip_factor_outer_grad_device does the
 * same for Lbar = alpha P Q' sampled on the pattern of L -- the form the gradients of the two triangular solves take --, and
 * cholmod_l_hip_factor_grad_to_host hands out the whole of Gx = df/dS on the pattern of L.  All run on the engine
 * (cholmod_hip_factor_grad_*, csrc/hip/factor_grad.hip) against the factor that is resident on the device; there is no host
 * fallback.  Every argument is checked before a device is touched. */
#include "host_internal.h"

static const ssamd_device_feature factor_grad_feature = {
    "the gradient through a complex factor is not supported", "the factor gradient needs Common->useGPU",
    "the factor gradient runs on one rank only",
    "the gradient through the factor of a complex matrix is not supported", "G_dev needs a symmetric A (stype != 0)" } ;

int cholmod_l_hip_factor_grad_device (cholmod_sparse *A, cholmod_factor *L, const double *Lbar_dev, double *G_dev,
    double *trace_dev, void *stream, cholmod_common *Common)
{
    RETURN_IF_NULL_COMMON (FALSE) ;
    RETURN_IF_NULL (L, FALSE) ;
    RETURN_IF_NULL (Lbar_dev, FALSE) ;
    size_t annz = 0 ;
    if (!ssamd_values_matrix_fits (A, G_dev != NULL, L, L->n, TRUE, &factor_grad_feature, &annz, Common)) return FALSE ;
    Common->status = CHOLMOD_OK ;
    if (L->n == 0) return TRUE ;
    cholmod_hip_plan *plan = (cholmod_hip_plan *) L->hip_plan ;
    if (!ssamd_device_status (cholmod_hip_factor_grad_device (plan, Lbar_dev, stream), Common,
        "the factor gradient could not be computed on the device")) return FALSE ;
    return ssamd_device_status (cholmod_hip_factor_grad_gather_device (plan, G_dev, (int64_t) annz, trace_dev, stream), Common,
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
    if (!ssamd_values_matrix_fits (A, G_dev != NULL, L, L->n, TRUE, &factor_grad_feature, &annz, Common)) return FALSE ;
    Common->status = CHOLMOD_OK ;
    if (L->n == 0) return TRUE ;
    cholmod_hip_plan *plan = (cholmod_hip_plan *) L->hip_plan ;
    if (!ssamd_device_status (cholmod_hip_factor_outer_grad_device (plan, alpha, P_dev, (int64_t) ldp, Q_dev, (int64_t) ldq, (int64_t) nrhs,
        stream), Common, "the factor gradient could not be computed on the device")) return FALSE ;
    return ssamd_device_status (cholmod_hip_factor_grad_gather_device (plan, G_dev, (int64_t) annz, trace_dev, stream), Common,
        "the plan holds no value map for this matrix") ;
}

int cholmod_l_hip_factor_grad_to_host (cholmod_factor *L, double *Gx, cholmod_common *Common)
{
    RETURN_IF_NULL_COMMON (FALSE) ;
    RETURN_IF_NULL (L, FALSE) ;
    RETURN_IF_NULL (Gx, FALSE) ;
    if (!ssamd_resident_factor_ready (L, &factor_grad_feature, TRUE, Common)) return FALSE ;
    Common->status = CHOLMOD_OK ;
    if (L->n == 0) return TRUE ;
    /* (no Lbar is known here: a Gx that is stale or was never computed is refused) */
    return ssamd_device_status (cholmod_hip_factor_grad_download ((cholmod_hip_plan *) L->hip_plan, Gx), Common,
        "the plan holds no current factor gradient: cholmod_l_hip_factor_grad_device first") ;
}
