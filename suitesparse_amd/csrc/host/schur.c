/* schur.c -- the Schur complement and the condensed solves of the host layer (cholmod.h): cholmod_l_hip_schur_device hands a
 * PyTorch or HIP caller Sc = L22 L22' and L22 for the last m variables of the factor's ordering, cholmod_l_hip_schur_reduce_device
 * the condensed right-hand side, cholmod_l_hip_schur_expand_device the solution on all variables from the one on the last m.
 * All three run on the engine (cholmod_hip_schur_device, cholmod_hip_trailing_multiply_device, csrc/hip/schur.hip, and the
 * sweeps of cholmod_hip_solve_device) against the factor that is resident on the device; there is no host fallback.  Every
 * argument is checked before a device is touched. */
#include "host_internal.h"

static const ssamd_device_feature schur_feature = {
    "the Schur complement of a complex factor is not supported", "the Schur complement needs Common->useGPU",
    "the Schur complement runs on one rank only", NULL, NULL } ;

/* what the three entry points ask of L and m; TRUE: L->hip_plan holds its numeric, positive definite factor */
static int sc_ready (cholmod_factor *L, size_t m, cholmod_common *Common)
{
    /* (a wrong kind of L is reported before a wrong m, a wrong m before the rest of the gate) */
    if (L->xtype == CHOLMOD_REAL && L->is_super && m > L->n) { ERROR (CHOLMOD_INVALID, "m is larger than n") ; return FALSE ; }
    return ssamd_resident_factor_ready (L, &schur_feature, TRUE, Common) ;
}

int cholmod_l_hip_schur_device (cholmod_factor *L, size_t m, double *S_dev, size_t lds, double *F_dev, size_t ldf,
    void *stream, cholmod_common *Common)
{
    RETURN_IF_NULL_COMMON (FALSE) ;
    RETURN_IF_NULL (L, FALSE) ;
    if (!S_dev && !F_dev) { ERROR (CHOLMOD_INVALID, "argument missing") ; return FALSE ; }
    if (!sc_ready (L, m, Common)) return FALSE ;
    if ((S_dev && lds < m) || (F_dev && ldf < m)) { ERROR (CHOLMOD_INVALID, "leading dimension smaller than m") ; return FALSE ; }
    Common->status = CHOLMOD_OK ;
    if (m == 0) return TRUE ;
    return ssamd_device_status (cholmod_hip_schur_device ((cholmod_hip_plan *) L->hip_plan, (int64_t) m, S_dev, (int64_t) lds, F_dev,
        (int64_t) ldf, stream), Common, "the Schur complement could not be formed on the device") ;
}

int cholmod_l_hip_schur_reduce_device (cholmod_factor *L, size_t m, const double *B_dev, size_t ldb, double *Y_dev, size_t ldy,
    double *G_dev, size_t ldg, size_t nrhs, void *stream, cholmod_common *Common)
{
    RETURN_IF_NULL_COMMON (FALSE) ;
    RETURN_IF_NULL (L, FALSE) ;
    RETURN_IF_NULL (B_dev, FALSE) ;
    RETURN_IF_NULL (Y_dev, FALSE) ;
    RETURN_IF_NULL (G_dev, FALSE) ;
    if (!sc_ready (L, m, Common)) return FALSE ;
    if (ldb < L->n || ldy < L->n) { ERROR (CHOLMOD_INVALID, "leading dimension smaller than n") ; return FALSE ; }
    if (ldg < m) { ERROR (CHOLMOD_INVALID, "leading dimension smaller than m") ; return FALSE ; }
    Common->status = CHOLMOD_OK ;
    if (m == 0 || nrhs == 0) return TRUE ;
    if (!ssamd_perm_ready (L, Common)) return FALSE ;
    cholmod_hip_plan *plan = (cholmod_hip_plan *) L->hip_plan ;
    const int64_t n = (int64_t) L->n ;
    /* Y = inv (L) P B, in the factor's ordering */
    int rc = cholmod_hip_solve_device (plan, 1, 1, 0, B_dev, (int64_t) ldb, Y_dev, (int64_t) ldy, (int64_t) nrhs, stream) ;
    if (rc != CHOLMOD_HIP_OK) return ssamd_device_status (rc, Common, "HIP device solve failed") ;
    /* G = L22 Y_S */
    return ssamd_device_status (cholmod_hip_trailing_multiply_device (plan, (int64_t) m, 0, Y_dev + (n - (int64_t) m), (int64_t) ldy, G_dev,
        (int64_t) ldg, (int64_t) nrhs, stream), Common, "the condensed right-hand side could not be formed on the device") ;
}

int cholmod_l_hip_schur_expand_device (cholmod_factor *L, size_t m, const double *Y_dev, size_t ldy, const double *XS_dev,
    size_t ldxs, double *X_dev, size_t ldx, size_t nrhs, void *stream, cholmod_common *Common)
{
    RETURN_IF_NULL_COMMON (FALSE) ;
    RETURN_IF_NULL (L, FALSE) ;
    RETURN_IF_NULL (Y_dev, FALSE) ;
    RETURN_IF_NULL (XS_dev, FALSE) ;
    RETURN_IF_NULL (X_dev, FALSE) ;
    if (!sc_ready (L, m, Common)) return FALSE ;
    if (ldy < L->n || ldx < L->n) { ERROR (CHOLMOD_INVALID, "leading dimension smaller than n") ; return FALSE ; }
    if (ldxs < m) { ERROR (CHOLMOD_INVALID, "leading dimension smaller than m") ; return FALSE ; }
    if ((const double *) X_dev == Y_dev) { ERROR (CHOLMOD_INVALID, "X_dev and Y_dev must differ") ; return FALSE ; }
    Common->status = CHOLMOD_OK ;
    if (nrhs == 0 || L->n == 0) return TRUE ;
    if (!ssamd_perm_ready (L, Common)) return FALSE ;
    cholmod_hip_plan *plan = (cholmod_hip_plan *) L->hip_plan ;
    const int64_t n = (int64_t) L->n ;
    /* W = [Y_I ; L22' XS], built in X_dev: all of Y first (a plain copy), then its last m rows overwritten ... */
    int rc = cholmod_hip_solve_device (plan, 3, 0, 0, Y_dev, (int64_t) ldy, X_dev, (int64_t) ldx, (int64_t) nrhs, stream) ;
    if (rc != CHOLMOD_HIP_OK) return ssamd_device_status (rc, Common, "HIP device copy failed") ;
    if (m > 0)
    {
        rc = cholmod_hip_trailing_multiply_device (plan, (int64_t) m, 1, XS_dev, (int64_t) ldxs, X_dev + (n - (int64_t) m),
            (int64_t) ldx, (int64_t) nrhs, stream) ;
        if (rc != CHOLMOD_HIP_OK) return ssamd_device_status (rc, Common, "the interface solution could not be applied on the device") ;
    }
    /* ... X = P' inv (L') W, in place (the sweeps run on the engine's own panel).  m == 0: the plain L' solve of Y. */
    return ssamd_device_status (cholmod_hip_solve_device (plan, 2, 0, 1, X_dev, (int64_t) ldx, X_dev, (int64_t) ldx, (int64_t) nrhs, stream),
        Common, "HIP device solve failed") ;
}
