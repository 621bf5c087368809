// sweep_device.hip.h -- what the device code of the two sweeps that run the factorization backwards shares
// (selinv_kernels.hip.h: the selected inverse; factor_grad_kernels.hip.h: reverse-mode Cholesky): the block sizes and LDS
// layouts, the slot and task descriptors of the launch program, the search for an entry in the panel of an ancestor, and
// the two triangular solves against a diagonal block.  Inline device functions only: no kernel lives here.
#pragma once
#include "descriptors.hip.h"

namespace sship {

#define SI_NB 64            /* column block of the recurrence */
#define SI_KC 64            /* k-chunk of L [R, b] staged in LDS by k_si_block */
#define SI_BLD 68           /* ... its leading dimension (k-major, column fastest) */
#define SI_TLD 65           /* leading dimension of the 64 x 64 LDS tiles that lanes walk by column */
#define SI_PTILE (SI_NB * SI_NB)    /* doubles of one partial of L [R, b]' T (one per 64-row slice of R) */
#define SI_BLOCK_LDS ((SI_NB * SI_TLD + SI_KC * SI_BLD) * sizeof (double))    /* k_si_block, k_si_diag: two tiles */
#define SI_THIN_LDS_MAX (160 * 1024)  /* k_si_thin: a front of SM_MAX rows needs at most 18 366 doubles */

// a generic front in flight: its square in the scratch buffer
struct SiSlot { i32 front ; i32 pad ; i64 moff ; } ;
// one unit of a launch; the workgroups [wg0, wg0 of the next task) belong to it.  k_si_fill: one workgroup per column of
// Z [I, I]; k_si_block: one per 64-row slice of R (nslices of them, partials at poff); k_si_diag: one; k_si_store: one per
// panel column
struct SiTask { i32 slot ; i32 b0 ; i32 nb ; i32 wg0 ; i32 nslices ; i32 pad ; i64 poff ; } ;

typedef double si_d4 __attribute__ ((ext_vector_type (4))) ;

// the task workgroup `bid` belongs to (tasks sorted by wg0, tasks [0].wg0 == 0)
__device__ __forceinline__ int si_find (const SiTask *t, int nt, int bid)
{
    int lo = 0, hi = nt - 1 ;
    while (lo < hi)
    {
        const int mid = (lo + hi + 1) >> 1 ;
        if (t [mid].wg0 <= bid) lo = mid ; else hi = mid - 1 ;
    }
    return lo ;
}

// Where Z (r, c), r >= c (the factor's ordering), lives in Zx: column c belongs to supernode supermap [c], row r is found
// in that supernode's row list -- its own columns first, a binary search below them.  -1: not in the pattern of L.
__device__ __forceinline__ i64 si_locate (const FrontD &t, const i64 *Ls, i64 r, i64 c)
{
    const i64 base = t.psx + (c - t.k1) * (i64) t.nsrow ;
    if (r < (i64) t.k1 + t.nscol) return base + (r - t.k1) ;
    const i64 *rows = Ls + t.psi ;
    int lo = t.nscol, hi = t.nsrow ;
    while (lo < hi) { const int mid = (lo + hi) >> 1 ; if (rows [mid] < r) lo = mid + 1 ; else hi = mid ; }
    return (lo < t.nsrow && rows [lo] == r) ? base + lo : -1 ;
}

__device__ __forceinline__ double si_nan () { return __longlong_as_double (0x7ff8000000000000LL) ; }

// X L_bb = B by rows, in place: row i of the nb columns of X (X [i + c ldx]); Lb = entry (0, 0) of L_bb, ld = ldl
__device__ __forceinline__ void si_row_solve (double *X, int ldx, int i, const double *Lb, i64 ldl, int nb)
{
    for (int c = nb - 1 ; c >= 0 ; c--)
    {
        const double *Lc = Lb + (i64) c * ldl ;
        double s = X [i + c * ldx] ;
        for (int k = c + 1 ; k < nb ; k++) s -= X [i + k * ldx] * Lc [k] ;
        X [i + c * ldx] = s / Lc [c] ;
    }
}

// L_bb' X = B by columns, in place: column c of X
__device__ __forceinline__ void si_col_solve (double *X, int ldx, int c, const double *Lb, i64 ldl, int nb)
{
    for (int a = nb - 1 ; a >= 0 ; a--)
    {
        const double *La = Lb + (i64) a * ldl ;
        double s = X [a + c * ldx] ;
        for (int k = a + 1 ; k < nb ; k++) s -= La [k] * X [k + c * ldx] ;
        X [a + c * ldx] = s / La [a] ;
    }
}

// The hot product of both sweeps, by the 256 threads of a workgroup: T = M [slice, R] L [R, b] for the 64 rows of R from
// row0 on, on the matrix cores -- MR = entry (0, 0) of the square M [R, R] (ld), read once, straight from the scratch; Lb =
// column 0 of the block in the panel (column c at Lb + c ld, L [R, b] from row b1 on), through Bs in k-chunks.  Rows past
// nR = |R| are clamped on the way in (the caller masks them on the way out); k past |R| and columns past nb contribute
// zeros.  T is left in Ts [i + SI_TLD c]; the caller synchronizes before it reads Ts or writes Bs again.
__device__ __forceinline__ void si_slice_product (const double *MR, const double *Lb, i64 ld, int b1, int nb, int nR, int row0,
    double *Ts, double *Bs)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lk = lane >> 4 ;
    si_d4 acc [4] ;
#pragma unroll
    for (int t = 0 ; t < 4 ; t++) acc [t] = (si_d4) {0.0, 0.0, 0.0, 0.0} ;
    const int ia = min (row0 + 16 * wave + lr, nR - 1) ;
    for (int kc = 0 ; kc < nR ; kc += SI_KC)
    {
        // the chunk's operands of this lane straight from the square, all loads in flight beside the staging of L [R, b]
        double av [SI_KC / 4] ;
#pragma unroll
        for (int u = 0 ; u < SI_KC / 4 ; u++)
        {
            const int kk = kc + 4 * u + lk ;
            av [u] = MR [ia + (i64) min (kk, nR - 1) * ld] ;
            if (kk >= nR) av [u] = 0.0 ;
        }
        __syncthreads () ;
#pragma unroll
        for (int q = 0 ; q < SI_KC * 64 / 256 ; q++)
        {
            const int k = tid & (SI_KC - 1), c = tid / SI_KC + (256 / SI_KC) * q ;
            Bs [k * SI_BLD + c] = (kc + k < nR && c < nb) ? Lb [(i64) c * ld + b1 + kc + k] : 0.0 ;
        }
        __syncthreads () ;
#pragma unroll
        for (int u = 0 ; u < SI_KC / 4 ; u++)
        {
            if (kc + 4 * u >= nR) break ;
#pragma unroll
            for (int t = 0 ; t < 4 ; t++)
                acc [t] = __builtin_amdgcn_mfma_f64_16x16x4f64 (av [u], Bs [(4 * u + lk) * SI_BLD + 16 * t + lr], acc [t], 0, 0, 0) ;
        }
    }
    __syncthreads () ;
    // acc [t][r] of lane (lr, lk) is T (row 16 wave + lk + 4 r, column 16 t + lr)
#pragma unroll
    for (int t = 0 ; t < 4 ; t++)
#pragma unroll
        for (int r = 0 ; r < 4 ; r++) Ts [16 * wave + lk + 4 * r + SI_TLD * (16 * t + lr)] = acc [t][r] ;
}

// doubles of LDS a thin front needs: M (ncb x ncb), T (ncb x nb), Q (nb x nb), odd leading dimensions
__host__ __device__ __forceinline__ int si_thin_lds (int nscol, int nsrow)
{
    const int ncb = nsrow - nscol ;
    return (ncb | 1) * (ncb + nscol) + (nscol | 1) * nscol ;
}

} // namespace sship
