// solve_kernels.hip.h -- gfx950 kernels of the triangular solves (solve.hip launches them): first the ones that
// sweep L once per right-hand side (k_lsolve ... k_perm), then the ones that take a panel of 16 right-hand sides
// (k_sd_*, cholmod_hip_solve_device).
#pragma once
#include "device_util.hip.h"

namespace sship {

// ---- triangular solves with the device-resident factor (nrhs columns) -------
// Level-scheduled restatement of cholmod_l_super_lsolve / _ltsolve
// (t_cholmod_super_solve.c:14-220, :222-411).  One workgroup per supernode of
// the level.  Forward: x1 = L1 \ x1 ; X[Ls2] -= L2 * x1 (children of one parent
// may hit the same rows, hence the atomic add).  Backward: x1 = L1' \ (x1 -
// L2' * X[Ls2]) needs no atomics.

template <bool CX>
__global__ void __launch_bounds__(256) k_lsolve (const SolveTask *tasks,
    const FrontD *fr, const i64 *Ls, const double *Lx, double *X, i64 ldx, int nrhs)
{
    __shared__ double xb [64] ;
    __shared__ double Dl [64 * 65] ;
    SolveTask T = tasks [blockIdx.x] ;
    const FrontD &f = fr [T.front] ;
    int nscol = f.nscol, nsrow = f.nsrow, k1 = f.k1, tid = threadIdx.x ;
    int lane = tid & 63, wave = tid >> 6 ;
    int c0 = T.c0, c1 = T.c1 ;
    const double *L = Lx + f.psx ;
    const i64 *rows = Ls + f.psi ;
    for (int r = 0 ; r < nrhs ; r++)
    {
        double *x = X + (i64) r * ldx ;
        for (int jb = c0 ; jb < c1 ; jb += 64)
        {
            int nb = c1 - jb < 64 ? c1 - jb : 64 ;
            // stage the diagonal block in LDS (coalesced), so the sequential
            // substitution below never waits on HBM
            for (int e = tid ; e < 64 * 64 ; e += 256)
            {
                int i = e & 63, j = e >> 6 ;
                Dl [i * 65 + j] = (i < nb && j < nb && j <= i) ? ldcx<CX> (L, jb + i, jb + j, nsrow) : (i == j ? 1.0 : 0.0) ;
            }
            __syncthreads () ;
            if (wave == 0)
            {
                // dtrsv("L","N","N") on the 64-wide diagonal block, one wave
                // (reciprocal diagonal once per lane and v_readlane broadcasts: a
                // division or a ds_bpermute on the 64-step chain costs 5x the rest)
                double xv = (lane < nb) ? x [k1 + jb + lane] : 0.0 ;
                double rdi = 1.0 / Dl [lane * 65 + lane] ;
                for (int j = 0 ; j < nb ; j++)
                {
                    double xj = readlane_f64 (xv, j) * readlane_f64 (rdi, j) ;
                    if (lane == j) xv = xj ;
                    else if (lane > j) xv = __builtin_fma (-Dl [lane * 65 + j], xj, xv) ;
                }
                xb [lane] = xv ;
                if (lane < nb) x [k1 + jb + lane] = xv ;
            }
            __syncthreads () ;
            for (int i = jb + nb + tid ; i < c1 ; i += 256)
            {
                double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0 ;
                int j = 0 ;
                for ( ; j + 4 <= nb ; j += 4)
                {
                    double l0 = ldcx<CX> (L, i, jb + j, nsrow), l1 = ldcx<CX> (L, i, jb + j + 1, nsrow) ;
                    double l2 = ldcx<CX> (L, i, jb + j + 2, nsrow), l3 = ldcx<CX> (L, i, jb + j + 3, nsrow) ;
                    a0 += l0 * xb [j] ; a1 += l1 * xb [j + 1] ; a2 += l2 * xb [j + 2] ; a3 += l3 * xb [j + 3] ;
                }
                for ( ; j < nb ; j++) a0 += ldcx<CX> (L, i, jb + j, nsrow) * xb [j] ;
                x [k1 + i] -= (a0 + a1) + (a2 + a3) ;
            }
            __syncthreads () ;
        }
        if (T.below)
        {
            // dgemv: X[rows2] -= L2 * x1 ; siblings share ancestor rows -> atomic
            for (int i = nscol + tid ; i < nsrow ; i += 256)
            {
                double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0 ;
                int j = 0 ;
                for ( ; j + 4 <= nscol ; j += 4)
                {
                    double l0 = ldcx<CX> (L, i, j, nsrow), l1 = ldcx<CX> (L, i, j + 1, nsrow) ;
                    double l2 = ldcx<CX> (L, i, j + 2, nsrow), l3 = ldcx<CX> (L, i, j + 3, nsrow) ;
                    a0 += l0 * x [k1 + j] ; a1 += l1 * x [k1 + j + 1] ;
                    a2 += l2 * x [k1 + j + 2] ; a3 += l3 * x [k1 + j + 3] ;
                }
                for ( ; j < nscol ; j++) a0 += ldcx<CX> (L, i, j, nsrow) * x [k1 + j] ;
                atomicAdd (&x [rows [i]], -((a0 + a1) + (a2 + a3))) ;
            }
        }
        __syncthreads () ;
    }
}

// column block of the big-supernode walk (k_solve_fwd_blk / k_solve_bwd_blk below)

template <bool CX>
__global__ void __launch_bounds__(256) k_ltsolve (const SolveTask *tasks,
    const FrontD *fr, const i64 *Ls, const double *Lx, double *X, i64 ldx, int nrhs)
{
    __shared__ double xb [64] ;
    __shared__ double ych [512] ;
    __shared__ double Dl [64 * 65] ;
    SolveTask T = tasks [blockIdx.x] ;
    const FrontD &f = fr [T.front] ;
    int nscol = f.nscol, nsrow = f.nsrow, k1 = f.k1, tid = threadIdx.x ;
    int lane = tid & 63, wave = tid >> 6 ;
    int c0 = T.c0, c1 = T.c1 ;
    const double *L = Lx + f.psx ;
    const i64 *rows = Ls + f.psi ;
    for (int r = 0 ; r < nrhs ; r++)
    {
        double *x = X + (i64) r * ldx ;
        if (T.below)
        {
            // dgemv("C"): x1 -= L2' * X[rows2].  The gathered X[rows2] is staged in
            // LDS in chunks of 512 rows (one gather per row instead of one per row
            // and column); a wave walks the columns, 8 independent loads per lane
            for (int i0 = nscol ; i0 < nsrow ; i0 += 512)
            {
                int nr = nsrow - i0 < 512 ? nsrow - i0 : 512 ;
                for (int q = tid ; q < 512 ; q += 256) ych [q] = (q < nr) ? x [rows [i0 + q]] : 0.0 ;
                __syncthreads () ;
                for (int j = wave ; j < nscol ; j += 4)
                {
                    double v [8] ;
#pragma unroll
                    for (int u = 0 ; u < 8 ; u++) { int q = lane + 64 * u ; v [u] = (q < nr) ? ldcx<CX> (L, i0 + q, j, nsrow) : 0.0 ; }
                    double acc = 0.0 ;
#pragma unroll
                    for (int u = 0 ; u < 8 ; u++) acc += v [u] * ych [lane + 64 * u] ;
                    for (int o = 32 ; o > 0 ; o >>= 1) acc += __shfl_down (acc, o) ;
                    if (lane == 0) x [k1 + j] -= acc ;
                }
                __syncthreads () ;
            }
        }
        // dtrsv("L","C","N") by 64-wide blocks from the bottom of [c0,c1)
        int last = c0 + ((c1 - c0 - 1) / 64) * 64 ;
        for (int jb = last ; jb >= c0 ; jb -= 64)
        {
            int nb = c1 - jb < 64 ? c1 - jb : 64 ;
            for (int e = tid ; e < 64 * 64 ; e += 256)
            {
                int i = e & 63, j = e >> 6 ;
                Dl [i * 65 + j] = (i < nb && j < nb && j <= i) ? ldcx<CX> (L, jb + i, jb + j, nsrow) : (i == j ? 1.0 : 0.0) ;
            }
            for (int jj = wave ; jj < nb ; jj += 4)
            {
                int j = jb + jj ;
                double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0 ;
                int i = jb + nb + lane ;
                for ( ; i + 192 < c1 ; i += 256)
                {
                    double l0 = ldcx<CX> (L, i, j, nsrow), l1 = ldcx<CX> (L, i + 64, j, nsrow), l2 = ldcx<CX> (L, i + 128, j, nsrow), l3 = ldcx<CX> (L, i + 192, j, nsrow) ;
                    a0 += l0 * x [k1 + i] ; a1 += l1 * x [k1 + i + 64] ;
                    a2 += l2 * x [k1 + i + 128] ; a3 += l3 * x [k1 + i + 192] ;
                }
                for ( ; i < c1 ; i += 64) a0 += ldcx<CX> (L, i, j, nsrow) * x [k1 + i] ;
                double acc = (a0 + a1) + (a2 + a3) ;
                for (int o = 32 ; o > 0 ; o >>= 1) acc += __shfl_down (acc, o) ;
                if (lane == 0) xb [jj] = x [k1 + j] - acc ;
            }
            __syncthreads () ;
            if (wave == 0)
            {
                double xv = (lane < nb) ? xb [lane] : 0.0 ;
                double rdi = 1.0 / Dl [lane * 65 + lane] ;
                for (int j = nb - 1 ; j >= 0 ; j--)
                {
                    double xj = readlane_f64 (xv, j) * readlane_f64 (rdi, j) ;
                    if (lane == j) xv = xj ;
                    else if (lane < j) xv = __builtin_fma (-Dl [j * 65 + lane], xj, xv) ;
                }
                if (lane < nb) x [k1 + jb + lane] = xv ;
            }
            __syncthreads () ;
        }
    }
}


// ---- big supernodes: a batched walk in 256-column blocks -----------------------
// The 64x64 diagonal blocks of the big supernodes are inverted once per
// factorization (k_diag_inv64, every block independent).  The solve walks a big
// supernode in blocks of SOLVE_SB = 256 columns, and one launch carries the same
// step of EVERY big supernode of the etree level (they are independent), so the
// number of dependent launches is the block count of the level's widest
// supernode, not the sum over its supernodes (Poisson 100^3: 1680 -> 130 per
// direction):
//   forward  k_solve_fwd_diag (one workgroup per task) forms x_b = inv(L_bb) x_b, four
//            64-column sub-blocks with the explicit inverses on the diagonal, into a
//            side vector; k_solve_fwd_apply (256-row x 64-column workgroups) subtracts
//            L[rows, b] x_b from the rows below; k_solve_commit copies x_b back per level;
//   backward k_solve_bwd_apply adds L[rows, b]' x[rows] into the task's accumulator,
//            k_solve_bwd_diag forms x_b = inv(L_bb)' (x_b - acc).
// Inverse layout (per 64-block, 2 x 4096 doubles): Wm [k*64 + r] = W(r,k) and
// WmT [k*64 + c] = W(k,c), both zero outside the lower triangle and
// identity-padded past the supernode's last column.

template <bool CX>
__global__ void __launch_bounds__(64) k_diag_inv64 (const InvTask *tasks, const FrontD *fr,
    const double *Lx, double *Winv)
{
    __shared__ double Lm [64 * 64] ;        // Lm [e*64 + r] = L(r,e)
    __shared__ double Wl [64 * 65] ;        // Wl [k*65 + q] = W(k,q)
    __shared__ double rdl [64] ;
    InvTask T = tasks [blockIdx.x] ;
    const FrontD &f = fr [T.front] ;
    int nsrow = f.nsrow, q = threadIdx.x ;
    int nb = f.nscol - T.jb < 64 ? f.nscol - T.jb : 64 ;
    const double *L = Lx + f.psx + T.jb + colx<CX> (T.jb, nsrow) ;
    for (int e = 0 ; e < 64 ; e++)
        Lm [e * 64 + q] = (q < nb && e < nb && e <= q) ? ldcx<CX> (L, q, e, nsrow) : (q == e ? 1.0 : 0.0) ;
    __syncthreads () ;
    rdl [q] = 1.0 / Lm [q * 64 + q] ;
    __syncthreads () ;
    // lane q = column q of the inverse, rows in blocks of 16
    for (int R = 0 ; R < 4 ; R++)
    {
        double acc [16] ;
#pragma unroll
        for (int r = 0 ; r < 16 ; r++) acc [r] = (16 * R + r == q) ? 1.0 : 0.0 ;
        for (int k = 0 ; k < 16 * R ; k++)
        {
            double wk = Wl [k * 65 + q] ;
#pragma unroll
            for (int r = 0 ; r < 16 ; r++) acc [r] = __builtin_fma (-Lm [k * 64 + 16 * R + r], wk, acc [r]) ;
        }
#pragma unroll
        for (int e = 0 ; e < 16 ; e++)
        {
            double y = acc [e] * rdl [16 * R + e] ;
            Wl [(16 * R + e) * 65 + q] = y ;
#pragma unroll
            for (int r = e + 1 ; r < 16 ; r++) acc [r] = __builtin_fma (-Lm [(16 * R + e) * 64 + 16 * R + r], y, acc [r]) ;
        }
    }
    __syncthreads () ;
    double *Wm = Winv + T.w_off, *WmT = Wm + 4096 ;
    for (int k = 0 ; k < 64 ; k++)
    {
        Wm [k * 64 + q] = Wl [q * 65 + k] ;     // W(r = q, k)
        WmT [k * 64 + q] = Wl [k * 65 + q] ;    // W(k, c = q)
    }
}

// One step of the walk for every big supernode of a level at once: task t = block
// [jb, jb+w) of one supernode, workgroups wg_start .. of the launch belong to it.

__device__ __forceinline__ int find_solve_task (const SolveBlk *t, int nt, int b)
{
    int lo = 0, hi = nt - 1 ;
    while (lo < hi) { int mid = (lo + hi + 1) >> 1 ; if (t [mid].wg_start <= b) lo = mid ; else hi = mid - 1 ; }
    return lo ;
}

// forward, step 1 (one workgroup per task): x_b = inv(L_bb) x_b by 64-column
// sub-blocks -- explicit inverses on the diagonal, matrix-vector products below it.
// The solved x_b goes to the side vector Y (k_solve_commit copies it back per level).
template <bool CX>
__global__ void __launch_bounds__(256) k_solve_fwd_diag (const SolveBlk *tasks,
    const FrontD *fr, const double *Lx, const double *Winv, const double *X, i64 ldx, int nrhs, double *Y)
{
    __shared__ double xs [SOLVE_SB], t [64], part [4][64] ;
    const SolveBlk T = tasks [blockIdx.x] ;
    const FrontD &f = fr [T.front] ;
    const int nsrow = f.nsrow, k1 = f.k1, tid = threadIdx.x ;
    const int jb = T.jb, w = T.w, nsub = (w + 63) >> 6 ;
    const int r = tid & 63, p = tid >> 6 ;
    const double *L = Lx + f.psx ;
    // everything this thread will ever need of L_bb leaves for the registers at once
    // (sub-step k: row 64 k + r, columns == p (mod 4) before the sub-block: 16 k values;
    // 96 in all, one HBM latency instead of one per sub-step); the chain below then
    // only waits for LDS and for the 64 x 64 inverses (L2)
    double l1 [16], l2 [32], l3 [48] ;
    {
#pragma unroll
        for (int u = 0 ; u < 16 ; u++) l1 [u] = (64 + r < w) ? ldcx<CX> (L, jb + 64 + r, jb + p + 4 * u, nsrow) : 0.0 ;
#pragma unroll
        for (int u = 0 ; u < 32 ; u++) l2 [u] = (128 + r < w) ? ldcx<CX> (L, jb + 128 + r, jb + p + 4 * u, nsrow) : 0.0 ;
#pragma unroll
        for (int u = 0 ; u < 48 ; u++) l3 [u] = (192 + r < w) ? ldcx<CX> (L, jb + 192 + r, jb + p + 4 * u, nsrow) : 0.0 ;
    }
    // ... and so do the four 64 x 64 inverses (16 values per thread and sub-step): fetched
    // inside the chain they cost one L2 / HBM latency per sub-step, four per launch
    double w0 [16], w1 [16], w2 [16], w3 [16] ;
    {
        const double *Wm = Winv + (i64) T.inv * 8192 + r ;
#pragma unroll
        for (int u = 0 ; u < 16 ; u++)
        {
            const int o = (p + 4 * u) * 64 ;
            w0 [u] = Wm [o] ;
            w1 [u] = (nsub > 1) ? Wm [8192 + o] : 0.0 ;
            w2 [u] = (nsub > 2) ? Wm [2 * 8192 + o] : 0.0 ;
            w3 [u] = (nsub > 3) ? Wm [3 * 8192 + o] : 0.0 ;
        }
    }
    for (int rhs = 0 ; rhs < nrhs ; rhs++)
    {
        const double *x = X + (i64) rhs * ldx ;
        xs [tid] = (tid < w) ? x [k1 + jb + tid] : 0.0 ;
        __syncthreads () ;
        for (int k = 0 ; k < nsub ; k++)
        {
            // t = x_k - L[k-th row block, columns before it] * (solved part)
            double a0 = 0.0, a1 = 0.0 ;
            if (k == 1)
            {
#pragma unroll
                for (int u = 0 ; u < 16 ; u += 2) { a0 = __builtin_fma (l1 [u], xs [p + 4 * u], a0) ; a1 = __builtin_fma (l1 [u + 1], xs [p + 4 * u + 4], a1) ; }
            }
            else if (k == 2)
            {
#pragma unroll
                for (int u = 0 ; u < 32 ; u += 2) { a0 = __builtin_fma (l2 [u], xs [p + 4 * u], a0) ; a1 = __builtin_fma (l2 [u + 1], xs [p + 4 * u + 4], a1) ; }
            }
            else if (k == 3)
            {
#pragma unroll
                for (int u = 0 ; u < 48 ; u += 2) { a0 = __builtin_fma (l3 [u], xs [p + 4 * u], a0) ; a1 = __builtin_fma (l3 [u + 1], xs [p + 4 * u + 4], a1) ; }
            }
            part [p][r] = a0 + a1 ;
            __syncthreads () ;
            if (tid < 64) t [tid] = xs [64 * k + tid] - ((part [0][tid] + part [1][tid]) + (part [2][tid] + part [3][tid])) ;
            __syncthreads () ;
            double a = 0.0 ;                                            // W(r, kk), kk == p (mod 4)
            if (k == 0)
            {
#pragma unroll
                for (int u = 0 ; u < 16 ; u++) a = __builtin_fma (w0 [u], t [p + 4 * u], a) ;
            }
            else if (k == 1)
            {
#pragma unroll
                for (int u = 0 ; u < 16 ; u++) a = __builtin_fma (w1 [u], t [p + 4 * u], a) ;
            }
            else if (k == 2)
            {
#pragma unroll
                for (int u = 0 ; u < 16 ; u++) a = __builtin_fma (w2 [u], t [p + 4 * u], a) ;
            }
            else
            {
#pragma unroll
                for (int u = 0 ; u < 16 ; u++) a = __builtin_fma (w3 [u], t [p + 4 * u], a) ;
            }
            part [p][r] = a ;
            __syncthreads () ;
            if (tid < 64) xs [64 * k + tid] = (part [0][tid] + part [1][tid]) + (part [2][tid] + part [3][tid]) ;
            __syncthreads () ;
        }
        if (tid < w) Y [(i64) rhs * ldx + k1 + jb + tid] = xs [tid] ;
        __syncthreads () ;
    }
}

// forward, step 2: X[rows below] -= L[rows, b] x_b ; workgroup = (256-row chunk) x
// (64-column sub-block), so that a single supernode fills the chip
template <bool CX>
__global__ void __launch_bounds__(256) k_solve_fwd_apply (const SolveBlk *tasks, int ntasks,
    const FrontD *fr, const i64 *Ls, const double *Lx, double *X, i64 ldx, int nrhs, const double *Y)
{
    __shared__ double xs [64] ;
    const SolveBlk T = tasks [find_solve_task (tasks, ntasks, (int) blockIdx.x)] ;
    const FrontD &f = fr [T.front] ;
    const int nscol = f.nscol, nsrow = f.nsrow, k1 = f.k1, tid = threadIdx.x ;
    const int jb = T.jb, w = T.w, nsub = (w + 63) >> 6 ;
    const int wgl = (int) blockIdx.x - T.wg_start ;
    const int q = wgl % nsub, chunk = wgl / nsub ;
    const int c0 = 64 * q, cw = (w - c0 < 64) ? w - c0 : 64 ;
    const double *L = Lx + f.psx ;
    const i64 *rows = Ls + f.psi ;
    const int i = jb + w + chunk * 256 + tid ;
    for (int rhs = 0 ; rhs < nrhs ; rhs++)
    {
        double *x = X + (i64) rhs * ldx ;
        if (tid < 64) xs [tid] = (tid < cw) ? Y [(i64) rhs * ldx + k1 + jb + c0 + tid] : 0.0 ;
        __syncthreads () ;
        if (i < nsrow)
        {
            double acc [4] = {0.0, 0.0, 0.0, 0.0} ;
            int c = 0 ;
            for ( ; c + 16 <= cw ; c += 16)
            {
                double l [16] ;
#pragma unroll
                for (int u = 0 ; u < 16 ; u++) l [u] = ldcx<CX> (L, i, jb + c0 + c + u, nsrow) ;
#pragma unroll
                for (int u = 0 ; u < 16 ; u++) acc [u & 3] = __builtin_fma (l [u], xs [c + u], acc [u & 3]) ;
            }
            for ( ; c < cw ; c++) acc [0] = __builtin_fma (ldcx<CX> (L, i, jb + c0 + c, nsrow), xs [c], acc [0]) ;
            double sm = (acc [0] + acc [1]) + (acc [2] + acc [3]) ;
            // (several column sub-blocks, and siblings of the level, add into the same row)
            atomicAdd (i < nscol ? &x [k1 + i] : &x [rows [i]], -sm) ;
        }
        __syncthreads () ;
    }
}

// solved values of the big supernodes of a level back into X (one task per supernode)
__global__ void __launch_bounds__(256) k_solve_commit (const SolveBlk *tasks, int ntasks, const FrontD *fr,
    double *X, i64 ldx, int nrhs, const double *Y)
{
    const SolveBlk T = tasks [find_solve_task (tasks, ntasks, (int) blockIdx.x)] ;
    const FrontD &f = fr [T.front] ;
    int j = ((int) blockIdx.x - T.wg_start) * 256 + threadIdx.x ;
    if (j >= f.nscol) return ;
    for (int rhs = 0 ; rhs < nrhs ; rhs++) X [(i64) rhs * ldx + f.k1 + j] = Y [(i64) rhs * ldx + f.k1 + j] ;
}

// backward, step 1: acc (task) += L[rows, b]' x[rows] ; workgroup = (256-row chunk) x
// (64-column sub-block); thread = row, the column sums of a wave go through an LDS
// transpose, one atomic add per column and wave
template <bool CX>
__global__ void __launch_bounds__(256) k_solve_bwd_apply (const SolveBlk *tasks, int ntasks,
    const FrontD *fr, const i64 *Ls, const double *Lx, const double *X, i64 ldx, int nrhs, double *accbuf)
{
    __shared__ double Tw [4][64 * 17] ;      // per wave: 64 rows x 16 columns of products
    const SolveBlk T = tasks [find_solve_task (tasks, ntasks, (int) blockIdx.x)] ;
    const FrontD &f = fr [T.front] ;
    const int nscol = f.nscol, nsrow = f.nsrow, k1 = f.k1, tid = threadIdx.x ;
    const int lane = tid & 63, wave = tid >> 6 ;
    const int jb = T.jb, w = T.w, nsub = (w + 63) >> 6 ;
    const int wgl = (int) blockIdx.x - T.wg_start ;
    const int qsub = wgl % nsub, chunk = wgl / nsub ;
    const double *L = Lx + f.psx ;
    const i64 *rows = Ls + f.psi ;
    double *acc = accbuf + (i64) T.slot * nrhs * SOLVE_SB ;
    const int r0 = jb + w + chunk * 256 ;
    const int nr = nsrow - r0 < 256 ? nsrow - r0 : 256 ;
    if (nr <= 0) return ;
    const int i = r0 + tid ;
    const bool ok = tid < nr ;
    const int c16 = lane & 15, seg = lane >> 4 ;
    for (int rhs = 0 ; rhs < nrhs ; rhs++)
    {
        const double *x = X + (i64) rhs * ldx ;
        double y = ok ? ((i < nscol) ? x [k1 + i] : x [rows [i]]) : 0.0 ;
        for (int q = 4 * qsub ; q < 4 * qsub + 4 ; q++)
        {
            double l [16] ;
#pragma unroll
            for (int c = 0 ; c < 16 ; c++) l [c] = ldcx<CX> (L, ok ? i : r0, jb + 16 * q + (16 * q + c < w ? c : 0), nsrow) ;
#pragma unroll
            for (int c = 0 ; c < 16 ; c++) Tw [wave][lane * 17 + c] = (16 * q + c < w) ? l [c] * y : 0.0 ;
            __builtin_amdgcn_s_waitcnt (0xc07f) ;      // lgkmcnt(0): own wave's LDS writes landed
            __builtin_amdgcn_wave_barrier () ;
            double sum = 0.0 ;
#pragma unroll
            for (int rr = 0 ; rr < 16 ; rr++) sum += Tw [wave][(seg * 16 + rr) * 17 + c16] ;
            sum += __shfl_xor (sum, 16) ;
            sum += __shfl_xor (sum, 32) ;
            if (seg == 0 && 16 * q + c16 < w) atomicAdd (&acc [rhs * SOLVE_SB + 16 * q + c16], sum) ;
            __builtin_amdgcn_wave_barrier () ;
        }
    }
}

// backward, step 2 (one workgroup per task): x_b = inv(L_bb)' (x_b - acc) by
// sub-blocks from the bottom; the accumulator is cleared for the next step
template <bool CX>
__global__ void __launch_bounds__(256) k_solve_bwd_diag (const SolveBlk *tasks,
    const FrontD *fr, const double *Lx, const double *Winv, double *X, i64 ldx, int nrhs, double *accbuf)
{
    __shared__ double xs [SOLVE_SB], t [64], part [4][64] ;
    __shared__ double Tw [4][64 * 17] ;
    const SolveBlk T = tasks [blockIdx.x] ;
    const FrontD &f = fr [T.front] ;
    const int nsrow = f.nsrow, k1 = f.k1, tid = threadIdx.x ;
    const int jb = T.jb, w = T.w, nsub = (w + 63) >> 6 ;
    const double *L = Lx + f.psx ;
    double *acc = accbuf + (i64) T.slot * nrhs * SOLVE_SB ;
    const int r = tid & 63, p = tid >> 6 ;
    const int lane = tid & 63, wave = tid >> 6, c16 = lane & 15, seg = lane >> 4 ;
    // sub-step k needs L(rows below sub-block k inside the block, its 64 columns):
    // wave = 16 of the columns, lane = row (coalesced), all 96 values per thread
    // requested at once
    double m2 [16], m1 [32], m0 [48] ;
    {
#pragma unroll
        for (int c = 0 ; c < 16 ; c++)
        {
            m2 [c] = (192 + lane < w) ? ldcx<CX> (L, jb + 192 + lane, jb + 128 + 16 * wave + c, nsrow) : 0.0 ;
#pragma unroll
            for (int j = 0 ; j < 2 ; j++) m1 [2 * c + j] = (128 + 64 * j + lane < w) ? ldcx<CX> (L, jb + 128 + 64 * j + lane, jb + 64 + 16 * wave + c, nsrow) : 0.0 ;
#pragma unroll
            for (int j = 0 ; j < 3 ; j++) m0 [3 * c + j] = (64 + 64 * j + lane < w) ? ldcx<CX> (L, jb + 64 + 64 * j + lane, jb + 16 * wave + c, nsrow) : 0.0 ;
        }
    }
    // the transposed 64 x 64 inverses as well (see k_solve_fwd_diag)
    double w0 [16], w1 [16], w2 [16], w3 [16] ;
    {
        const double *WmT = Winv + (i64) T.inv * 8192 + 4096 + r ;
#pragma unroll
        for (int u = 0 ; u < 16 ; u++)
        {
            const int o = (p + 4 * u) * 64 ;
            w0 [u] = WmT [o] ;
            w1 [u] = (nsub > 1) ? WmT [8192 + o] : 0.0 ;
            w2 [u] = (nsub > 2) ? WmT [2 * 8192 + o] : 0.0 ;
            w3 [u] = (nsub > 3) ? WmT [3 * 8192 + o] : 0.0 ;
        }
    }
    for (int rhs = 0 ; rhs < nrhs ; rhs++)
    {
        double *x = X + (i64) rhs * ldx ;
        xs [tid] = (tid < w) ? x [k1 + jb + tid] - acc [rhs * SOLVE_SB + tid] : 0.0 ;
        acc [rhs * SOLVE_SB + tid] = 0.0 ;
        __syncthreads () ;
        for (int k = nsub - 1 ; k >= 0 ; k--)
        {
            // t[c] = xs[64k + c] - sum over the solved rows below (inside the block) of L(row, 64k + c) xs[row]
            double sm [16] ;
#pragma unroll
            for (int c = 0 ; c < 16 ; c++) sm [c] = 0.0 ;
            if (k == 2)
            {
                double y = xs [192 + lane] ;
#pragma unroll
                for (int c = 0 ; c < 16 ; c++) sm [c] = m2 [c] * y ;
            }
            else if (k == 1)
            {
                double y0 = xs [128 + lane], y1 = xs [192 + lane] ;
#pragma unroll
                for (int c = 0 ; c < 16 ; c++) sm [c] = __builtin_fma (m1 [2 * c + 1], y1, m1 [2 * c] * y0) ;
            }
            else if (k == 0)
            {
                double y0 = xs [64 + lane], y1 = xs [128 + lane], y2 = xs [192 + lane] ;
#pragma unroll
                for (int c = 0 ; c < 16 ; c++) sm [c] = __builtin_fma (m0 [3 * c + 2], y2, __builtin_fma (m0 [3 * c + 1], y1, m0 [3 * c] * y0)) ;
            }
            // column sums over the wave's 64 rows through an LDS transpose
#pragma unroll
            for (int c = 0 ; c < 16 ; c++) Tw [wave][lane * 17 + c] = sm [c] ;
            __builtin_amdgcn_s_waitcnt (0xc07f) ;
            __builtin_amdgcn_wave_barrier () ;
            double sum = 0.0 ;
#pragma unroll
            for (int rr = 0 ; rr < 16 ; rr++) sum += Tw [wave][(seg * 16 + rr) * 17 + c16] ;
            sum += __shfl_xor (sum, 16) ;
            sum += __shfl_xor (sum, 32) ;
            if (seg == 0) t [16 * wave + c16] = xs [64 * k + 16 * wave + c16] - sum ;
            __syncthreads () ;
            double a = 0.0 ;                                            // W(kk, c), kk == p (mod 4)
            if (k == 0)
            {
#pragma unroll
                for (int u = 0 ; u < 16 ; u++) a = __builtin_fma (w0 [u], t [p + 4 * u], a) ;
            }
            else if (k == 1)
            {
#pragma unroll
                for (int u = 0 ; u < 16 ; u++) a = __builtin_fma (w1 [u], t [p + 4 * u], a) ;
            }
            else if (k == 2)
            {
#pragma unroll
                for (int u = 0 ; u < 16 ; u++) a = __builtin_fma (w2 [u], t [p + 4 * u], a) ;
            }
            else
            {
#pragma unroll
                for (int u = 0 ; u < 16 ; u++) a = __builtin_fma (w3 [u], t [p + 4 * u], a) ;
            }
            part [p][r] = a ;
            __syncthreads () ;
            if (tid < 64) xs [64 * k + tid] = (part [0][tid] + part [1][tid]) + (part [2][tid] + part [3][tid]) ;
            __syncthreads () ;
        }
        if (tid < w) x [k1 + jb + tid] = xs [tid] ;
        __syncthreads () ;
    }
}

// gather / scatter by the fill-reducing permutation (cholmod_solve.c:105,:322)
__global__ void k_perm (i64 n, const i64 *perm, const double *src, double *dst,
    int inverse)
{
    i64 k = blockIdx.x * (i64) 256 + threadIdx.x ;
    if (k >= n) return ;
    if (inverse) dst [perm [k]] = src [k] ; else dst [k] = src [perm [k]] ;
}

// ---- triangular solves with a panel of 16 right-hand sides (cholmod_hip_solve_device) ------------------------------
// The kernels above sweep L once per right-hand side.  Here the right-hand sides travel 16 at a time
// in a panel workspace W [n][16], the right-hand side index fastest: row k of the permuted system is one 128-byte
// line, so a gather or scatter by Ls [i] touches one line per row, and every product with L is a sequence of
// v_mfma_f64_16x16x4 tiles -- L is read once per panel (the reference's dtrsm / dgemm branch,
// t_cholmod_super_solve.c:164-173, :368-379).  A panel narrower than 16 has zero columns: they stay zero.
//
// Lane maps of v_mfma_f64_16x16x4 (lr = lane & 15, lk = lane >> 4): first operand A [row lr][k lk], second operand
// B [k lk][column lr], result register r = D [row lk + 4 r][column lr].  The column is always the right-hand side,
// so the four result registers of a lane group are 16 lanes x 8 bytes of one row of W.
//
// The schedule is the plan's: the whole-supernode tasks of a level (SolveTask, one workgroup each) and the
// 256-column blocks of the big supernodes (SolveBlk, the launches of sb_launch) with their explicit 64 x 64
// inverses (k_diag_inv64).
//
// CX = a complex factor in its own storage (device_util.hip.h): every read of L goes through ldcx<CX>, every block
// base is formed with colx<CX> (twin column c lives at column c >> 1 of the nsrow-leading-dimension panel), and the
// <false> forms are the real kernels unchanged.  ldcx touches row r ^ 1 of an in-range row r: every row and column
// bound of a twin is even (plan_build.hip checks it where the task lists are built), so the partner row is in range.
// W, the accumulators, the explicit inverses (full real 64 x 64 blocks) and the schedule are the twin's: real.
#define SD_NP 16        /* right-hand sides per panel */

__device__ __forceinline__ d4 sd_zero () { d4 z = {0.0, 0.0, 0.0, 0.0} ; return z ; }

// acc (rows i0 .. i0+15, 16 right-hand sides) += M [i0 .., 0 .. K) * Xs [0 .. K)[.]
// M: column-major, leading dimension ld (16 consecutive rows of a column per lane group: coalesced), rows >= ilim
// read as zero; Xs: LDS, [K][16].  CX: M addresses an even row and an even column of the twin, i0, ilim and K are even.
template <bool CX>
__device__ __forceinline__ d4 sd_mul_nx (const double *M, int ld, int i0, int ilim, int K, const double *Xs,
    d4 acc, int lr, int lk)
{
    const int i = i0 + lr ;
    const bool rok = i < ilim ;
    const double *Mi = M + (rok ? i : 0) ;
    for (int k0 = 0 ; k0 < K ; k0 += 4)
    {
        const int k = k0 + lk ;
        const bool ok = k < K ;
        const double a = (rok && ok) ? (CX ? ldcx<CX> (M, i, k, ld) : Mi [(i64) k * ld]) : 0.0 ;
        const double b = ok ? Xs [k * SD_NP + lr] : 0.0 ;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64 (a, b, acc, 0, 0, 0) ;
    }
    return acc ;
}

// acc (columns j0 .. j0+15 of M, 16 right-hand sides) += sum over rows i = ia, ia + 1, .. (16 at a time, then
// istep further on) below ib of M [i, j0 ..]' y (i)[.]
// A lane reads four consecutive rows of its column (lk-th quarter of the 16): a lane group covers 128 contiguous
// bytes of each of its 16 columns, and the four values feed four k-steps.  Columns >= jlim read as zero.  CX: M
// addresses an even row and an even column of the twin, ia, ib and jlim are even (a lane of an odd column reads its
// four rows pairwise swapped: the same 32 bytes).
template <bool CX, class YF>
__device__ __forceinline__ d4 sd_mul_ty (const double *M, int ld, int j0, int jlim, int ia, int ib, int istep,
    YF y, d4 acc, int lr, int lk)
{
    const int j = j0 + lr ;
    const bool cok = j < jlim ;
    const double *Mc = M + (i64) (cok ? j : j0) * ld ;
    for (int ibase = ia ; ibase < ib ; ibase += istep)
    {
        double a [4], b [4] ;
#pragma unroll
        for (int s = 0 ; s < 4 ; s++)
        {
            const int i = ibase + 4 * lk + s ;
            const bool ok = i < ib ;
            a [s] = (ok && cok) ? (CX ? ldcx<CX> (M, i, j, ld) : Mc [i]) : 0.0 ;
            b [s] = ok ? y (i, lr) : 0.0 ;
        }
#pragma unroll
        for (int s = 0 ; s < 4 ; s++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64 (a [s], b [s], acc, 0, 0, 0) ;
    }
    return acc ;
}

// ---- pack / unpack: B (column-major, ldb) through Perm into W, W through Perm into X ------------------------------
// One workgroup = 256 rows of the permuted system, transposed through LDS: a right-hand side is read / written
// along its column, W along its lines.  pw = width of this panel (<= 16): the missing columns of W are zero and
// are never written to X.
__global__ void __launch_bounds__(256) k_sd_pack (i64 n, const i64 *perm, const double *B, i64 ldb, int pw, double *W)
{
    __shared__ double tile [256 * 17] ;
    const int tid = threadIdx.x ;
    const i64 k0 = blockIdx.x * (i64) 256, k = k0 + tid ;
    if (k < n)
    {
        const i64 src = perm ? perm [k] : k ;
        for (int r = 0 ; r < SD_NP ; r++) tile [tid * 17 + r] = (r < pw) ? B [src + (i64) r * ldb] : 0.0 ;
    }
    __syncthreads () ;
    for (int e = tid ; e < 256 * SD_NP ; e += 256)
        if (k0 + (e >> 4) < n) W [k0 * SD_NP + e] = tile [(e >> 4) * 17 + (e & 15)] ;
}

__global__ void __launch_bounds__(256) k_sd_unpack (i64 n, const i64 *perm, const double *W, int pw, double *X, i64 ldx)
{
    __shared__ double tile [256 * 17] ;
    const int tid = threadIdx.x ;
    const i64 k0 = blockIdx.x * (i64) 256, k = k0 + tid ;
    for (int e = tid ; e < 256 * SD_NP ; e += 256)
        if (k0 + (e >> 4) < n) tile [(e >> 4) * 17 + (e & 15)] = W [k0 * SD_NP + e] ;
    __syncthreads () ;
    if (k < n)
    {
        const i64 dst = perm ? perm [k] : k ;
        for (int r = 0 ; r < pw ; r++) X [dst + (i64) r * ldx] = tile [tid * 17 + r] ;
    }
}

// ---- whole supernodes (at most 256 columns, one workgroup each) ----------------------------------------------------
// the 16 x 16 diagonal block at column jb into LDS, identity-padded past the supernode's last column
template <bool CX>
__device__ __forceinline__ void sd_stage_diag (const double *L, int nsrow, int jb, int nb, double *Dl, int tid)
{
    const int i = tid & 15, j = tid >> 4 ;
    Dl [i * 17 + j] = (i < nb && j < nb && j <= i) ? ldcx<CX> (L, jb + i, jb + j, nsrow) : (i == j ? 1.0 : 0.0) ;
}

// forward: x1 = L1 \ x1 by 16-column blocks (substitution on 16 right-hand sides at once, one lane each, then the
// rows below inside the supernode as tiles), W [Ls2] -= L2 x1 as tiles (siblings share ancestor rows: atomic)
template <bool CX>
__global__ void __launch_bounds__(256) k_sd_lsolve (const SolveTask *tasks, const FrontD *fr, const i64 *Ls,
    const double *Lx, double *W)
{
    __shared__ double x1 [256 * SD_NP] ;
    __shared__ double Dl [16 * 17] ;
    const SolveTask T = tasks [blockIdx.x] ;
    const FrontD &f = fr [T.front] ;
    const int nscol = f.nscol, nsrow = f.nsrow, tid = threadIdx.x ;
    const int lane = tid & 63, wave = tid >> 6, lr = lane & 15, lk = lane >> 4 ;
    const double *L = Lx + f.psx ;
    const i64 *rows = Ls + f.psi ;
    double *Wk = W + (i64) f.k1 * SD_NP ;
    for (int e = tid ; e < nscol * SD_NP ; e += 256) x1 [e] = Wk [e] ;
    __syncthreads () ;
    for (int jb = 0 ; jb < nscol ; jb += 16)
    {
        const int nb = nscol - jb < 16 ? nscol - jb : 16 ;
        sd_stage_diag<CX> (L, nsrow, jb, nb, Dl, tid) ;
        __syncthreads () ;
        if (tid < 16)
        {
            double v [16] ;
#pragma unroll
            for (int i = 0 ; i < 16 ; i++) v [i] = (i < nb) ? x1 [(jb + i) * SD_NP + tid] : 0.0 ;
#pragma unroll
            for (int j = 0 ; j < 16 ; j++)
            {
                v [j] = v [j] / Dl [j * 17 + j] ;
#pragma unroll
                for (int i = j + 1 ; i < 16 ; i++) v [i] = __builtin_fma (-Dl [i * 17 + j], v [j], v [i]) ;
            }
#pragma unroll
            for (int i = 0 ; i < 16 ; i++) if (i < nb) x1 [(jb + i) * SD_NP + tid] = v [i] ;
        }
        __syncthreads () ;
        for (int i0 = jb + 16 + 16 * wave ; i0 < nscol ; i0 += 64)
        {
            const d4 p = sd_mul_nx<CX> (L + colx<CX> (jb, nsrow), nsrow, i0, nscol, nb, x1 + jb * SD_NP, sd_zero (), lr, lk) ;
#pragma unroll
            for (int r = 0 ; r < 4 ; r++)
            {
                const int i = i0 + lk + 4 * r ;
                if (i < nscol) x1 [i * SD_NP + lr] -= p [r] ;
            }
        }
        __syncthreads () ;
    }
    for (int e = tid ; e < nscol * SD_NP ; e += 256) Wk [e] = x1 [e] ;
    if (T.below)
        for (int i0 = nscol + 16 * wave ; i0 < nsrow ; i0 += 64)
        {
            const d4 p = sd_mul_nx<CX> (L, nsrow, i0, nsrow, nscol, x1, sd_zero (), lr, lk) ;
#pragma unroll
            for (int r = 0 ; r < 4 ; r++)
            {
                const int i = i0 + lk + 4 * r ;
                if (i < nsrow) atomicAdd (&W [rows [i] * SD_NP + lr], -p [r]) ;
            }
        }
}

// backward: x1 -= L2' W [Ls2] (the rows split over the four waves, their partial tiles summed in a fixed order: no
// atomics), then x1 = L1' \ x1 by 16-column blocks from the bottom
template <bool CX>
__global__ void __launch_bounds__(256) k_sd_ltsolve (const SolveTask *tasks, const FrontD *fr, const i64 *Ls,
    const double *Lx, double *W)
{
    __shared__ double x1 [256 * SD_NP] ;
    __shared__ double red [4][256] ;
    __shared__ double Dl [16 * 17] ;
    const SolveTask T = tasks [blockIdx.x] ;
    const FrontD &f = fr [T.front] ;
    const int nscol = f.nscol, nsrow = f.nsrow, tid = threadIdx.x ;
    const int lane = tid & 63, wave = tid >> 6, lr = lane & 15, lk = lane >> 4 ;
    const double *L = Lx + f.psx ;
    const i64 *rows = Ls + f.psi ;
    double *Wk = W + (i64) f.k1 * SD_NP ;
    for (int e = tid ; e < nscol * SD_NP ; e += 256) x1 [e] = Wk [e] ;
    __syncthreads () ;
    if (T.below && nsrow > nscol)
    {
        auto yg = [&] (int i, int c) { return W [rows [i] * SD_NP + c] ; } ;
        for (int j0 = 0 ; j0 < nscol ; j0 += 16)
        {
            const d4 p = sd_mul_ty<CX> (L, nsrow, j0, nscol, nscol + 16 * wave, nsrow, 64, yg, sd_zero (), lr, lk) ;
#pragma unroll
            for (int r = 0 ; r < 4 ; r++) red [wave][(lk + 4 * r) * SD_NP + lr] = p [r] ;
            __syncthreads () ;
            if (j0 + (tid >> 4) < nscol)
                x1 [j0 * SD_NP + tid] -= (red [0][tid] + red [1][tid]) + (red [2][tid] + red [3][tid]) ;
            __syncthreads () ;
        }
    }
    auto ys = [&] (int i, int c) { return x1 [i * SD_NP + c] ; } ;
    for (int jb = ((nscol - 1) / 16) * 16 ; jb >= 0 ; jb -= 16)
    {
        const int nb = nscol - jb < 16 ? nscol - jb : 16 ;
        sd_stage_diag<CX> (L, nsrow, jb, nb, Dl, tid) ;
        __syncthreads () ;
        if (tid < 16)
        {
            double v [16] ;
#pragma unroll
            for (int i = 0 ; i < 16 ; i++) v [i] = (i < nb) ? x1 [(jb + i) * SD_NP + tid] : 0.0 ;
#pragma unroll
            for (int j = 15 ; j >= 0 ; j--)
            {
                v [j] = v [j] / Dl [j * 17 + j] ;
#pragma unroll
                for (int i = 0 ; i < j ; i++) v [i] = __builtin_fma (-Dl [j * 17 + i], v [j], v [i]) ;
            }
#pragma unroll
            for (int i = 0 ; i < 16 ; i++) if (i < nb) x1 [(jb + i) * SD_NP + tid] = v [i] ;
        }
        __syncthreads () ;
        // the columns before the block: x1 [0, jb) -= L [jb .. jb+nb, 0 .. jb)' x1 [jb .. jb+nb)
        for (int j0 = 16 * wave ; j0 < jb ; j0 += 64)
        {
            const d4 p = sd_mul_ty<CX> (L, nsrow, j0, jb, jb, jb + nb, 16, ys, sd_zero (), lr, lk) ;
#pragma unroll
            for (int r = 0 ; r < 4 ; r++) x1 [(j0 + lk + 4 * r) * SD_NP + lr] -= p [r] ;
        }
        __syncthreads () ;
    }
    for (int e = tid ; e < nscol * SD_NP ; e += 256) Wk [e] = x1 [e] ;
}

// ---- big supernodes: the walk in 256-column blocks of kernels.hip.h, 16 right-hand sides wide --------------------------
// forward, step 1 (one workgroup per task): x_b = inv (L_bb) x_b by 64-column sub-blocks, in place in W.  Wave =
// 16 rows of the sub-block: t = x_k - L [sub-block k, columns before it] x (solved), then x_k = W_k t with the
// explicit inverse, both as tiles.
template <bool CX>
__global__ void __launch_bounds__(256) k_sd_fwd_diag (const SolveBlk *tasks, const FrontD *fr, const double *Lx,
    const double *Winv, double *W)
{
    __shared__ double xs [SOLVE_SB * SD_NP] ;
    __shared__ double ts [64 * SD_NP] ;
    const SolveBlk T = tasks [blockIdx.x] ;
    const FrontD &f = fr [T.front] ;
    const int nsrow = f.nsrow, tid = threadIdx.x ;
    const int jb = T.jb, w = T.w, nsub = (w + 63) >> 6 ;
    const int lane = tid & 63, wave = tid >> 6, lr = lane & 15, lk = lane >> 4 ;
    const double *Lbb = Lx + f.psx + jb + colx<CX> (jb, nsrow) ;
    double *Wk = W + (i64) (f.k1 + jb) * SD_NP ;
    for (int e = tid ; e < SOLVE_SB * SD_NP ; e += 256) xs [e] = (e < w * SD_NP) ? Wk [e] : 0.0 ;
    __syncthreads () ;
    for (int k = 0 ; k < nsub ; k++)
    {
        const int i0 = 64 * k + 16 * wave ;
        const d4 p = sd_mul_nx<CX> (Lbb, nsrow, i0, w, 64 * k, xs, sd_zero (), lr, lk) ;
#pragma unroll
        for (int r = 0 ; r < 4 ; r++) ts [(16 * wave + lk + 4 * r) * SD_NP + lr] = xs [(i0 + lk + 4 * r) * SD_NP + lr] - p [r] ;
        __syncthreads () ;
        const d4 q = sd_mul_nx<false> (Winv + (i64) (T.inv + k) * 8192, 64, 16 * wave, 64, 64, ts, sd_zero (), lr, lk) ;
#pragma unroll
        for (int r = 0 ; r < 4 ; r++) xs [(i0 + lk + 4 * r) * SD_NP + lr] = q [r] ;
        __syncthreads () ;
    }
    for (int e = tid ; e < w * SD_NP ; e += 256) Wk [e] = xs [e] ;
}

// forward, step 2: W [rows below the block] -= L [rows, b] x_b ; workgroup = (256-row chunk) x (64-column
// sub-block), wave = 64 of the rows as four tiles that share the x_b operand
template <bool CX>
__global__ void __launch_bounds__(256) k_sd_fwd_apply (const SolveBlk *tasks, int ntasks, const FrontD *fr,
    const i64 *Ls, const double *Lx, double *W)
{
    __shared__ double xs [64 * SD_NP] ;
    const SolveBlk T = tasks [find_solve_task (tasks, ntasks, (int) blockIdx.x)] ;
    const FrontD &f = fr [T.front] ;
    const int nscol = f.nscol, nsrow = f.nsrow, k1 = f.k1, tid = threadIdx.x ;
    const int jb = T.jb, w = T.w, nsub = (w + 63) >> 6 ;
    const int lane = tid & 63, wave = tid >> 6, lr = lane & 15, lk = lane >> 4 ;
    const int wgl = (int) blockIdx.x - T.wg_start ;
    const int q = wgl % nsub, chunk = wgl / nsub ;
    const int c0 = 64 * q, cw = (w - c0 < 64) ? w - c0 : 64 ;
    const double *L = Lx + f.psx + colx<CX> (jb + c0, nsrow) ;
    const i64 *rows = Ls + f.psi ;
    const double *Wb = W + (i64) (k1 + jb + c0) * SD_NP ;
    for (int e = tid ; e < 64 * SD_NP ; e += 256) xs [e] = (e < cw * SD_NP) ? Wb [e] : 0.0 ;
    __syncthreads () ;
    const int rb = jb + w + chunk * 256 + 64 * wave ;
    if (rb >= nsrow) return ;
    d4 acc [4] = {sd_zero (), sd_zero (), sd_zero (), sd_zero ()} ;
    bool rok [4] ;
    int ri [4] ;
    const double *Li [4] ;
#pragma unroll
    for (int t = 0 ; t < 4 ; t++)
    {
        const int i = rb + 16 * t + lr ;
        rok [t] = i < nsrow ;
        ri [t] = rok [t] ? i : rb ;
        Li [t] = L + ri [t] ;
    }
    for (int k0 = 0 ; k0 < cw ; k0 += 4)
    {
        const int k = k0 + lk ;
        const bool ok = k < cw ;
        const double b = ok ? xs [k * SD_NP + lr] : 0.0 ;
        double a [4] ;
#pragma unroll
        for (int t = 0 ; t < 4 ; t++) a [t] = (ok && rok [t]) ? (CX ? ldcx<CX> (L, ri [t], k, nsrow) : Li [t][(i64) k * nsrow]) : 0.0 ;
#pragma unroll
        for (int t = 0 ; t < 4 ; t++) acc [t] = __builtin_amdgcn_mfma_f64_16x16x4f64 (a [t], b, acc [t], 0, 0, 0) ;
    }
#pragma unroll
    for (int t = 0 ; t < 4 ; t++)
#pragma unroll
        for (int r = 0 ; r < 4 ; r++)
        {
            const int i = rb + 16 * t + lk + 4 * r ;
            // (several column sub-blocks, and siblings of the level, add into the same row)
            if (i < nsrow) atomicAdd (&W [(i < nscol ? (i64) k1 + i : rows [i]) * SD_NP + lr], -acc [t][r]) ;
        }
}

// backward, step 1: acc (task) += L [rows, b]' W [rows] ; workgroup = (256-row chunk) x (64-column sub-block);
// the gathered rows are staged in LDS once, wave = 16 of the columns, one atomic add per column, right-hand side
// and workgroup.  acc: [slot][256][16].
template <bool CX>
__global__ void __launch_bounds__(256) k_sd_bwd_apply (const SolveBlk *tasks, int ntasks, const FrontD *fr,
    const i64 *Ls, const double *Lx, const double *W, double *accbuf)
{
    __shared__ double ys [256 * SD_NP] ;
    const SolveBlk T = tasks [find_solve_task (tasks, ntasks, (int) blockIdx.x)] ;
    const FrontD &f = fr [T.front] ;
    const int nscol = f.nscol, nsrow = f.nsrow, k1 = f.k1, tid = threadIdx.x ;
    const int jb = T.jb, w = T.w, nsub = (w + 63) >> 6 ;
    const int lane = tid & 63, wave = tid >> 6, lr = lane & 15, lk = lane >> 4 ;
    const int wgl = (int) blockIdx.x - T.wg_start ;
    const int qsub = wgl % nsub, chunk = wgl / nsub ;
    const double *L = Lx + f.psx ;
    const i64 *rows = Ls + f.psi ;
    double *acc = accbuf + (i64) T.slot * SOLVE_SB * SD_NP ;
    const int r0 = jb + w + chunk * 256 ;
    const int nr = nsrow - r0 < 256 ? nsrow - r0 : 256 ;
    if (nr <= 0) return ;
    for (int e = tid ; e < 256 * SD_NP ; e += 256)
    {
        const int i = r0 + (e >> 4) ;
        ys [e] = (i < nsrow) ? W [(i < nscol ? (i64) k1 + i : rows [i]) * SD_NP + (e & 15)] : 0.0 ;
    }
    __syncthreads () ;
    const int c0 = 64 * qsub + 16 * wave ;
    if (c0 >= w) return ;
    auto yl = [&] (int i, int c) { return ys [(i - r0) * SD_NP + c] ; } ;
    const d4 p = sd_mul_ty<CX> (L, nsrow, jb + c0, jb + w, r0, r0 + nr, 16, yl, sd_zero (), lr, lk) ;
#pragma unroll
    for (int r = 0 ; r < 4 ; r++)
    {
        const int c = c0 + lk + 4 * r ;
        if (c < w) atomicAdd (&acc [c * SD_NP + lr], p [r]) ;
    }
}

// backward, step 2 (one workgroup per task): x_b = inv (L_bb)' (x_b - acc) by sub-blocks from the bottom; the
// accumulator is cleared for the next step
template <bool CX>
__global__ void __launch_bounds__(256) k_sd_bwd_diag (const SolveBlk *tasks, const FrontD *fr, const double *Lx,
    const double *Winv, double *W, double *accbuf)
{
    __shared__ double xs [SOLVE_SB * SD_NP] ;
    __shared__ double ts [64 * SD_NP] ;
    const SolveBlk T = tasks [blockIdx.x] ;
    const FrontD &f = fr [T.front] ;
    const int nsrow = f.nsrow, tid = threadIdx.x ;
    const int jb = T.jb, w = T.w, nsub = (w + 63) >> 6 ;
    const int lane = tid & 63, wave = tid >> 6, lr = lane & 15, lk = lane >> 4 ;
    const double *Lbb = Lx + f.psx + jb + colx<CX> (jb, nsrow) ;
    double *acc = accbuf + (i64) T.slot * SOLVE_SB * SD_NP ;
    double *Wk = W + (i64) (f.k1 + jb) * SD_NP ;
    for (int e = tid ; e < SOLVE_SB * SD_NP ; e += 256)
    {
        xs [e] = (e < w * SD_NP) ? Wk [e] - acc [e] : 0.0 ;
        acc [e] = 0.0 ;
    }
    __syncthreads () ;
    auto yl = [&] (int i, int c) { return xs [i * SD_NP + c] ; } ;
    for (int k = nsub - 1 ; k >= 0 ; k--)
    {
        const int c0 = 64 * k + 16 * wave ;
        // t = x_k - sum over the solved rows below sub-block k (inside the block) of L (row, column)' x (row)
        const d4 p = sd_mul_ty<CX> (Lbb, nsrow, c0, w, 64 * (k + 1), w, 16, yl, sd_zero (), lr, lk) ;
#pragma unroll
        for (int r = 0 ; r < 4 ; r++) ts [(16 * wave + lk + 4 * r) * SD_NP + lr] = xs [(c0 + lk + 4 * r) * SD_NP + lr] - p [r] ;
        __syncthreads () ;
        const d4 q = sd_mul_nx<false> (Winv + (i64) (T.inv + k) * 8192 + 4096, 64, 16 * wave, 64, 64, ts, sd_zero (), lr, lk) ;
#pragma unroll
        for (int r = 0 ; r < 4 ; r++) xs [(c0 + lk + 4 * r) * SD_NP + lr] = q [r] ;
        __syncthreads () ;
    }
    for (int e = tid ; e < w * SD_NP ; e += 256) Wk [e] = xs [e] ;
}

} // namespace sship
