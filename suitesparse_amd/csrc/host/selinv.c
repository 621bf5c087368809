/* selinv.c -- the selected inverse of the host layer (cholmod.h): cholmod_l_hip_selinv_device hands a PyTorch or HIP caller
 * the entries of (A + beta I)^-1 at the entries of A and its diagonal in device memory, cholmod_l_hip_selinv_to_host the
 * whole subset in the layout of L->x -- what the reference ships as MATLAB_Tools/sparseinv (there on a simplicial LDL',
 * column by column).  Both run on the engine (cholmod_hip_selinv_*, csrc/hip/selinv.hip) against the factor that is
 * resident on the device; there is no host fallback.  Every argument is checked before a device is touched. */
#include "host_internal.h"

static const ssamd_device_feature selinv_feature = {
    "the selected inverse of a complex factor is not supported", "the selected inverse needs Common->useGPU",
    "the selected inverse runs on one rank only",
    "the selected inverse of a complex matrix is not supported", "Z_dev needs a symmetric A (stype != 0)" } ;

int cholmod_l_hip_selinv_device (cholmod_sparse *A, cholmod_factor *L, double *Z_dev, double *diag_dev, void *stream,
    cholmod_common *Common)
{
    RETURN_IF_NULL_COMMON (FALSE) ;
    RETURN_IF_NULL (L, FALSE) ;
    if (!Z_dev && !diag_dev) { ERROR (CHOLMOD_INVALID, "argument missing") ; return FALSE ; }
    size_t annz = 0 ;
    if (!ssamd_values_matrix_fits (A, Z_dev != NULL, L, L->n, TRUE, &selinv_feature, &annz, Common)) return FALSE ;
    Common->status = CHOLMOD_OK ;
    if (L->n == 0) return TRUE ;
    cholmod_hip_plan *plan = (cholmod_hip_plan *) L->hip_plan ;
    if (diag_dev && !ssamd_perm_ready (L, Common)) return FALSE ;
    if (!ssamd_selinv_current (plan, stream, Common)) return FALSE ;
    return ssamd_device_status (cholmod_hip_selinv_gather_device (plan, Z_dev, (int64_t) annz, diag_dev, 1, stream), Common,
        "the plan holds no value map for this matrix") ;
}

int cholmod_l_hip_selinv_to_host (cholmod_factor *L, double *Zx, cholmod_common *Common)
{
    RETURN_IF_NULL_COMMON (FALSE) ;
    RETURN_IF_NULL (L, FALSE) ;
    RETURN_IF_NULL (Zx, FALSE) ;
    if (!ssamd_resident_factor_ready (L, &selinv_feature, TRUE, Common)) return FALSE ;
    Common->status = CHOLMOD_OK ;
    if (L->n == 0) return TRUE ;
    cholmod_hip_plan *plan = (cholmod_hip_plan *) L->hip_plan ;
    if (!ssamd_selinv_current (plan, NULL, Common)) return FALSE ;
    return ssamd_device_status (cholmod_hip_selinv_download (plan, Zx), Common, "the selected inverse could not be copied to the host") ;
}
