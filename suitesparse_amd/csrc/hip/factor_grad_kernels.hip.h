// factor_grad_kernels.hip.h -- device code of the factor gradient (factor_grad.hip): reverse-mode Cholesky on the pattern
// of L, front by front from the roots down.  Given Lbar = df/dL it produces Gbar = df/dS, S = L L' LOWER-STORED (an
// off-diagonal entry stands for two entries of the symmetric matrix).  For a column block b = [b0, b1) of a front (at
// most SI_NB wide) and R = the front's rows after b1 (its later columns, then its below-rows), with W = Gbar [R, R] known:
//     M           = W + W'                                 (full square, the diagonal doubled)
//     Y           = Lbar [R, b] - M L [R, b]               (the hot product: v_mfma_f64_16x16x4, K = |R|)
//     Gbar [R, b] = Y inv (L_bb)                           (a row-wise solve against L_bb: no explicit inverse)
//     Q           = tril (Lbar [b, b]) - tril (sum over the 64-row slices s of R of Gbar [s, b]' L [s, b])
//     P           = inv (L_bb)' Phi (L_bb' Q) inv (L_bb),  Phi = the lower triangle with the diagonal halved
//     Gbar [b, b] = tril (P + P') - diag (P)
// The selected inverse is the special case Lbar = diag (2 / L_jj), and the sweep has its shape (selinv_kernels.hip.h): a
// generic front lives in flight as a full square (ld = nsrow) in the scratch buffer, here holding M -- both triangles,
// the diagonal doubled --; a thin front (one block, nsrow <= SM_MAX) is done whole by one workgroup in LDS.  Gx holds
// Lbar when the sweep begins and is overwritten panel by panel: a panel holds Lbar until its front is done and Gbar
// afterwards, the dead upper triangles of the diagonal blocks exact +0.0 (what stood there in Lbar is never read).
// Every entry of Gx has one owner and one summation order: no atomics, the same inputs give the same bits.
#pragma once
#include "sweep_device.hip.h"

namespace sship {

// M [I, I] of every front of the launch, both triangles, the diagonal doubled, from the finished panels of its
// ancestors: a gather by the reader (one workgroup per column of I), as k_si_fill's.
__global__ void __launch_bounds__(256) k_fg_fill (const SiTask *tasks, int nt, const SiSlot *slots, const FrontD *fr,
    const i32 *supermap, const i64 *Ls, const double *Gx, double *M)
{
    const SiTask T = tasks [si_find (tasks, nt, blockIdx.x)] ;
    const SiSlot S = slots [T.slot] ;
    const FrontD &f = fr [S.front] ;
    const int j = blockIdx.x - T.wg0, ld = f.nsrow, nscol = f.nscol, ncb = f.nsrow - f.nscol ;
    if (j >= ncb) return ;
    const i64 *I = Ls + f.psi + nscol ;
    const i64 c = I [j] ;
    const FrontD &t = fr [supermap [c]] ;
    double *Mf = M + S.moff ;
    for (int i = j + threadIdx.x ; i < ncb ; i += 256)
    {
        const i64 q = si_locate (t, Ls, I [i], c) ;
        double v = q >= 0 ? Gx [q] : si_nan () ;
        if (i == j) v += v ;
        Mf [(i64) (nscol + i) + (i64) (nscol + j) * ld] = v ;
        Mf [(i64) (nscol + j) + (i64) (nscol + i) * ld] = v ;
    }
}

// One 64-row slice of R of one block: T = M [slice, R] L [R, b] on the matrix cores (M read once, straight from the
// scratch; L [R, b] through LDS in k-chunks, as in k_si_block), Y = Lbar [slice, b] - T with Lbar from the panel in Gx,
// Gbar [slice, b] = Y inv (L_bb), the slice's partial of Gbar [s, b]' L [s, b], and Gbar [slice, b] into the square,
// mirrored.  Rows past |R| are clamped on the way in, zero in the tile and masked on the way out; k past |R| and columns
// past nb contribute zeros.
__global__ void __launch_bounds__(256) k_fg_block (const SiTask *tasks, int nt, const SiSlot *slots, const FrontD *fr,
    const double *Lx, const double *Gx, double *M, double *Pbuf)
{
    extern __shared__ __attribute__ ((aligned (16))) double si_lds [] ;
    double *Ts = si_lds ;                           // T, then Y, then Gbar [slice, b]: [i + SI_TLD c]
    double *Bs = si_lds + SI_NB * SI_TLD ;          // chunk of L [R, b]: [k SI_BLD + c]; then L_bb: [k + 64 c]; then L [slice, b]: [i + 64 a]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6 ;
    const SiTask T = tasks [si_find (tasks, nt, blockIdx.x)] ;
    const SiSlot S = slots [T.slot] ;
    const FrontD &f = fr [S.front] ;
    const i64 ld = f.nsrow ;
    const int b0 = T.b0, nb = T.nb, b1 = b0 + nb, nR = f.nsrow - b1 ;
    const int row0 = (blockIdx.x - T.wg0) * 64 ;
    if (row0 >= nR) return ;
    double *Mf = M + S.moff ;
    const double *MR = Mf + b1 + (i64) b1 * ld ;            // M [R, R]
    const double *Lb = Lx + f.psx + (i64) b0 * ld ;         // column c of the block: Lb + c ld; L_bb at row b0, L [R, b] at row b1
    const double *Gb = Gx + f.psx + (i64) b0 * ld ;         // ... and of Lbar
    si_slice_product (MR, Lb, ld, b1, nb, nR, row0, Ts, Bs) ;
    for (int e = tid ; e < 64 * nb ; e += 256) Bs [e] = Lb [(i64) (e >> 6) * ld + b0 + min (e & 63, nb - 1)] ;       // L_bb: [k + 64 c]
    __syncthreads () ;
    // Y = Lbar [slice, b] - T; zero in the rows past |R| and the columns past nb
    for (int e = tid ; e < 64 * 64 ; e += 256)
    {
        const int i = e & 63, c = e >> 6 ;
        Ts [i + SI_TLD * c] = (row0 + i < nR && c < nb) ? Gb [(i64) c * ld + b1 + row0 + i] - Ts [i + SI_TLD * c] : 0.0 ;
    }
    __syncthreads () ;
    if (tid < 64) si_row_solve (Ts, SI_TLD, tid, Bs, 64, nb) ;
    __syncthreads () ;
    for (int e = tid ; e < 64 * 64 ; e += 256)
    {
        const int i = e & 63, a = e >> 6 ;
        Bs [e] = (row0 + i < nR && a < nb) ? Lb [(i64) a * ld + b1 + row0 + i] : 0.0 ;
    }
    __syncthreads () ;
    // the slice's partial P (a, c) = sum_i Gbar (i, a) L (i, c), i ascending; stored [a + 64 c]
    double *Pt = Pbuf + (T.poff + (blockIdx.x - T.wg0)) * (i64) SI_PTILE ;
    for (int q = 0 ; q < 16 ; q++)
    {
        const int c = wave + 4 * q, a = lane ;
        double s = 0 ;
        for (int i = 0 ; i < 64 ; i++) s += Ts [i + SI_TLD * a] * Bs [i + 64 * c] ;
        Pt [a + 64 * c] = s ;
    }
    for (int e = tid ; e < 64 * nb ; e += 256)
    {
        const int i = e & 63, c = e >> 6 ;
        if (row0 + i < nR) Mf [(i64) (b1 + row0 + i) + (i64) (b0 + c) * ld] = Ts [i + SI_TLD * c] ;
    }
    for (int e = tid ; e < 64 * 64 ; e += 256)
    {
        const int c = e & 63, i = e >> 6 ;
        if (c < nb && row0 + i < nR) Mf [(i64) (b0 + c) + (i64) (b1 + row0 + i) * ld] = Ts [i + SI_TLD * c] ;
    }
}

// Phi (L_bb' Q) in place, column c of Q (X [a + c ldx]) by one thread: a ascending, so that entry (a, c) is overwritten
// after its last use (the sum over k >= a); the rows above the diagonal are cleared, the diagonal is halved
__device__ __forceinline__ void fg_phi_column (double *X, int ldx, int c, const double *Lb, i64 ldl, int nb)
{
    for (int a = 0 ; a < nb ; a++)
    {
        const double *La = Lb + (i64) a * ldl ;
        double s = 0.0 ;
        if (a >= c) for (int k = a ; k < nb ; k++) s += La [k] * X [k + c * ldx] ;
        X [a + c * ldx] = (a == c) ? 0.5 * s : s ;
    }
}

// Gbar [b, b] of one block: Q = tril (Lbar [b, b]) - the partials of its slices (added in slice order), Phi (L_bb' Q) by
// columns, then the two triangular solves of k_si_diag; P + P' goes into the square, both triangles (its diagonal is the
// doubled one).
__global__ void __launch_bounds__(256) k_fg_diag (const SiTask *tasks, const SiSlot *slots, const FrontD *fr,
    const double *Lx, const double *Gx, double *M, const double *Pbuf)
{
    extern __shared__ __attribute__ ((aligned (16))) double si_lds [] ;
    double *Qs = si_lds ;                           // Q (a, c) at [a + SI_TLD c]
    double *Lbs = si_lds + SI_NB * SI_TLD ;         // L_bb: [k + 64 c]
    const int tid = threadIdx.x ;
    const SiTask T = tasks [blockIdx.x] ;
    const SiSlot S = slots [T.slot] ;
    const FrontD &f = fr [S.front] ;
    const i64 ld = f.nsrow ;
    const int b0 = T.b0, nb = T.nb ;
    const double *Lbb = Lx + f.psx + (i64) b0 * ld + b0 ;
    const double *Gbb = Gx + f.psx + (i64) b0 * ld + b0 ;
    for (int e = tid ; e < SI_PTILE ; e += 256)
    {
        const int a = e & 63, c = e >> 6 ;
        double v = 0.0 ;
        if (a < nb && c <= a)
        {
            double s = 0.0 ;
            for (int q = 0 ; q < T.nslices ; q++) s += Pbuf [(T.poff + q) * (i64) SI_PTILE + e] ;
            v = Gbb [(i64) c * ld + a] - s ;
        }
        Qs [a + SI_TLD * c] = v ;
    }
    for (int e = tid ; e < 64 * nb ; e += 256) Lbs [e] = Lbb [(i64) (e >> 6) * ld + min (e & 63, nb - 1)] ;
    __syncthreads () ;
    if (tid < nb) fg_phi_column (Qs, SI_TLD, tid, Lbs, 64, nb) ;
    __syncthreads () ;
    if (tid < nb) si_row_solve (Qs, SI_TLD, tid, Lbs, 64, nb) ;
    __syncthreads () ;
    if (tid < nb) si_col_solve (Qs, SI_TLD, tid, Lbs, 64, nb) ;
    __syncthreads () ;
    double *Mf = M + S.moff ;
    for (int e = tid ; e < SI_PTILE ; e += 256)
    {
        const int a = e & 63, c = e >> 6 ;
        if (a >= nb || c > a) continue ;
        const double v = Qs [a + SI_TLD * c] + Qs [c + SI_TLD * a] ;
        Mf [(i64) (b0 + a) + (i64) (b0 + c) * ld] = v ;
        Mf [(i64) (b0 + c) + (i64) (b0 + a) * ld] = v ;
    }
}

// the finished panel columns of a front from its square into Gx (the layout of Lx): lower-stored, so the doubled
// diagonal is halved again (exactly); the dead upper triangle of the diagonal block cleared
__global__ void __launch_bounds__(256) k_fg_store (const SiTask *tasks, int nt, const SiSlot *slots, const FrontD *fr,
    const double *M, double *Gx)
{
    const SiTask T = tasks [si_find (tasks, nt, blockIdx.x)] ;
    const SiSlot S = slots [T.slot] ;
    const FrontD &f = fr [S.front] ;
    const int c = blockIdx.x - T.wg0, ld = f.nsrow ;
    if (c >= f.nscol) return ;
    const double *Mc = M + S.moff + (i64) c * ld ;
    double *Gc = Gx + f.psx + (i64) c * ld ;
    for (int i = threadIdx.x ; i < ld ; i += 256) Gc [i] = i < c ? 0.0 : i == c ? 0.5 * Mc [i] : Mc [i] ;
}

// A thin front (nscol <= SI_NB, nsrow <= SM_MAX) whole: one workgroup, the recurrence above with b = all its columns
// and R = its below-rows, everything in LDS (the layout and the size of k_si_thin: si_thin_lds), L read from the (cached)
// panel, Lbar from the front's panel in Gx, which is overwritten at the end.
__global__ void __launch_bounds__(256) k_fg_thin (const i32 *fronts, const FrontD *fr, const i32 *supermap, const i64 *Ls,
    const double *Lx, double *Gx)
{
    extern __shared__ __attribute__ ((aligned (16))) double si_lds [] ;
    const int tid = threadIdx.x ;
    const FrontD &f = fr [fronts [blockIdx.x]] ;
    const int nb = f.nscol, ld = f.nsrow, ncb = ld - nb, ldm = ncb | 1, ldq = nb | 1 ;
    double *Ms = si_lds, *Ts = Ms + ldm * ncb, *Qs = Ts + ldm * nb ;
    const i64 *I = Ls + f.psi + nb ;
    const double *Lp = Lx + f.psx ;             // L_bb at row 0, L [R, b] at row nb
    double *Gp = Gx + f.psx ;                   // Lbar likewise, then Gbar
    for (int e = tid ; e < ncb * ncb ; e += 256)
    {
        const int j = e / ncb, i = e - j * ncb ;
        if (i < j) continue ;
        const i64 c = I [j] ;
        const i64 q = si_locate (fr [supermap [c]], Ls, I [i], c) ;
        double v = q >= 0 ? Gx [q] : si_nan () ;
        if (i == j) v += v ;
        Ms [i + ldm * j] = v ; Ms [j + ldm * i] = v ;
    }
    __syncthreads () ;
    for (int e = tid ; e < ncb * nb ; e += 256)
    {
        const int c = e / ncb, i = e - c * ncb ;
        const double *Lc = Lp + (i64) c * ld + nb ;
        double s = 0 ;
        for (int k = 0 ; k < ncb ; k++) s += Ms [i + ldm * k] * Lc [k] ;
        Ts [i + ldm * c] = Gp [(i64) c * ld + nb + i] - s ;
    }
    __syncthreads () ;
    if (tid < ncb) si_row_solve (Ts, ldm, tid, Lp, ld, nb) ;
    __syncthreads () ;
    for (int e = tid ; e < nb * nb ; e += 256)
    {
        const int c = e / nb, a = e - c * nb ;
        double v = 0.0 ;
        if (a >= c)
        {
            const double *Lc = Lp + (i64) c * ld + nb ;
            double s = 0 ;
            for (int i = 0 ; i < ncb ; i++) s += Ts [i + ldm * a] * Lc [i] ;
            v = Gp [(i64) c * ld + a] - s ;
        }
        Qs [a + ldq * c] = v ;
    }
    __syncthreads () ;
    if (tid < nb) fg_phi_column (Qs, ldq, tid, Lp, ld, nb) ;
    __syncthreads () ;
    if (tid < nb) si_row_solve (Qs, ldq, tid, Lp, ld, nb) ;
    __syncthreads () ;
    if (tid < nb) si_col_solve (Qs, ldq, tid, Lp, ld, nb) ;
    __syncthreads () ;
    for (int e = tid ; e < ld * nb ; e += 256)
    {
        const int c = e / ld, i = e - c * ld ;
        Gp [e] = i < c ? 0.0 : i == c ? Qs [c + ldq * c] : i < nb ? Qs [i + ldq * c] + Qs [c + ldq * i] : Ts [(i - nb) + ldm * c] ;
    }
}

// ---- Lbar of cholmod_hip_factor_outer_grad_device ---------------------------------------------------------------------------

// Lbar (i, j) = alpha sum_r P (i, r) Q (j, r) over the lower trapezoid of column j of L straight into Gx, r in index order;
// +0.0 in the dead triangle, and everywhere when there is no right-hand side.  One workgroup per column of L.
__global__ void __launch_bounds__(256) k_fg_outer (const i32 *supermap, const FrontD *fr, const i64 *Ls, double alpha,
    const double *Pm, i64 ldp, const double *Qm, i64 ldq, int nrhs, double *Gx)
{
    const i64 j = blockIdx.x ;
    const FrontD &f = fr [supermap [j]] ;
    const int jc = (int) (j - f.k1), ld = f.nsrow ;
    const i64 *rows = Ls + f.psi ;
    double *Gc = Gx + f.psx + (i64) jc * ld ;
    for (int i = threadIdx.x ; i < ld ; i += 256)
    {
        double s = 0.0 ;
        if (i >= jc && nrhs > 0)
        {
            const i64 r = rows [i] ;
            for (int k = 0 ; k < nrhs ; k++) s += Pm [r + k * ldp] * Qm [j + k * ldq] ;
            s *= alpha ;
        }
        Gc [i] = s ;
    }
}

// ---- the gather of cholmod_hip_factor_grad_gather_device ------------------------------------------------------------------------

__global__ void __launch_bounds__(256) k_fg_zero_fill (i64 n, double *out)
{
    const i64 k = blockIdx.x * (i64) 256 + threadIdx.x ;
    if (k < n) out [k] = 0.0 ;
}

// out [src [p]] = Gbar at the position of entry p of the resident packed S, for the entries S is read at (the rule of
// k_si_gather_values: on or below the diagonal, the last of equal neighbours), into an array filled with +0.0.  One
// thread per column of S.
__global__ void __launch_bounds__(256) k_fg_gather_values (i64 n, const i64 *Sp, const i64 *Si, const i64 *src,
    const i32 *supermap, const FrontD *fr, const i64 *Ls, const double *Gx, double *out)
{
    const i64 k = blockIdx.x * (i64) 256 + threadIdx.x ;
    if (k >= n) return ;
    const FrontD &t = fr [supermap [k]] ;
    const i64 pend = Sp [k + 1] ;
    for (i64 p = Sp [k] ; p < pend ; p++)
    {
        const i64 i = Si [p] ;
        if (i < k || i >= n || (p + 1 < pend && Si [p + 1] == i)) continue ;
        const i64 q = si_locate (t, Ls, i, k) ;
        if (q >= 0) out [src [p]] = Gx [q] ;
    }
}

// the 256 values of a workgroup added in a fixed tree; the sum in red [0]
__device__ __forceinline__ void fg_block_sum (double *red, double v)
{
    red [threadIdx.x] = v ;
    __syncthreads () ;
    for (int o = 128 ; o > 0 ; o >>= 1)
    {
        if ((int) threadIdx.x < o) red [threadIdx.x] += red [threadIdx.x + o] ;
        __syncthreads () ;
    }
}

// part [b] = sum of Gbar (j, j) over the 256 columns of workgroup b
__global__ void __launch_bounds__(256) k_fg_trace_partial (i64 n, const i32 *supermap, const FrontD *fr, const double *Gx, double *part)
{
    __shared__ double red [256] ;
    const i64 k = blockIdx.x * (i64) 256 + threadIdx.x ;
    double v = 0.0 ;
    if (k < n)
    {
        const FrontD &f = fr [supermap [k]] ;
        const i64 jj = k - f.k1 ;
        v = Gx [f.psx + jj + jj * (i64) f.nsrow] ;
    }
    fg_block_sum (red, v) ;
    if (threadIdx.x == 0) part [blockIdx.x] = red [0] ;
}

// out [0] = the sum of the partials: one workgroup, thread t adds the partials t, t + 256, ... in index order, then the tree
__global__ void __launch_bounds__(256) k_fg_trace_final (i64 nparts, const double *part, double *out)
{
    __shared__ double red [256] ;
    double v = 0.0 ;
    for (i64 q = threadIdx.x ; q < nparts ; q += 256) v += part [q] ;
    fg_block_sum (red, v) ;
    if (threadIdx.x == 0) out [0] = red [0] ;
}

} // namespace sship
