// selinv_kernels.hip.h -- device code of the selected inverse (selinv.hip): Z = (L L')^-1 on the pattern of L, front by
// front from the roots down.  For a column block b = [b0, b1) of a front (at most SI_NB wide) and R = the front's rows
// after b1 (its later columns, then its below-rows), with M = Z [R, R] known:
//     T        = M L [R, b]                                   (the hot product: v_mfma_f64_16x16x4, K = |R|)
//     Z [R, b] = -T inv (L [b, b])                            (a row-wise solve against L_bb: no explicit inverse)
//     Z [b, b] = inv (L_bb)' (I + L [R, b]' T) inv (L_bb)     (two triangular solves)
// which is Takahashi's  Z_Rb = -Z_RR G,  Z_bb = inv (L_bb)' inv (L_bb) - G' Z_Rb  with G = L_Rb inv (L_bb), written so that
// G never exists in memory.  A generic front lives in flight as a full symmetric square (ld = nsrow, both triangles
// filled) in the scratch buffer; a thin front (one block, nsrow <= SM_MAX) is done whole by one workgroup in LDS.
// Every entry of Zx has one owner and one summation order: no atomics, the same factor gives the same bits.
#pragma once
#include "sweep_device.hip.h"

namespace sship {

// M [I, I] of every front of the launch, both triangles, from the finished panels of its ancestors: a gather by the
// reader (one workgroup per column of I), never a scatter by several writers.
__global__ void __launch_bounds__(256) k_si_fill (const SiTask *tasks, int nt, const SiSlot *slots, const FrontD *fr,
    const i32 *supermap, const i64 *Ls, const double *Zx, double *M)
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
        const double v = q >= 0 ? Zx [q] : si_nan () ;
        Mf [(i64) (nscol + i) + (i64) (nscol + j) * ld] = v ;
        Mf [(i64) (nscol + j) + (i64) (nscol + i) * ld] = v ;
    }
}

// One 64-row slice of R of one block: T = M [slice, R] L [R, b] on the matrix cores (M read once, straight from the
// scratch; L [R, b] through LDS in k-chunks), the slice's partial of L [R, b]' T, then Z [slice, b] = -T inv (L_bb) into the
// square, mirrored.  Rows past |R| are clamped on the way in and masked on the way out; k past |R| and columns past nb
// contribute zeros.
__global__ void __launch_bounds__(256) k_si_block (const SiTask *tasks, int nt, const SiSlot *slots, const FrontD *fr,
    const double *Lx, double *M, double *Pbuf)
{
    extern __shared__ __attribute__ ((aligned (16))) double si_lds [] ;
    double *Ts = si_lds ;                           // T, then W: [i + SI_TLD c]
    double *Bs = si_lds + SI_NB * SI_TLD ;          // chunk of L [R, b]: [k SI_BLD + c]; then L [slice, b]: [i + 64 a]; then L_bb
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6 ;
    const SiTask T = tasks [si_find (tasks, nt, blockIdx.x)] ;
    const SiSlot S = slots [T.slot] ;
    const FrontD &f = fr [S.front] ;
    const i64 ld = f.nsrow ;
    const int b0 = T.b0, nb = T.nb, b1 = b0 + nb, nR = f.nsrow - b1 ;
    const int row0 = (blockIdx.x - T.wg0) * 64 ;
    if (row0 >= nR) return ;
    double *Mf = M + S.moff ;
    const double *MR = Mf + b1 + (i64) b1 * ld ;            // Z [R, R]
    const double *Lb = Lx + f.psx + (i64) b0 * ld ;         // column c of the block: Lb + c ld; L_bb at row b0, L [R, b] at row b1
    si_slice_product (MR, Lb, ld, b1, nb, nR, row0, Ts, Bs) ;
    for (int e = tid ; e < 64 * 64 ; e += 256)
    {
        const int i = e & 63, a = e >> 6 ;
        Bs [e] = (row0 + i < nR && a < nb) ? Lb [(i64) a * ld + b1 + row0 + i] : 0.0 ;
    }
    __syncthreads () ;
    // the slice's partial P (a, c) = sum_i L (i, a) T (i, c), i ascending; stored [c + 64 a]
    double *Pt = Pbuf + (T.poff + (blockIdx.x - T.wg0)) * (i64) SI_PTILE ;
    for (int q = 0 ; q < 16 ; q++)
    {
        const int a = wave + 4 * q, c = lane ;
        double s = 0 ;
        for (int i = 0 ; i < 64 ; i++) s += Bs [i + 64 * a] * Ts [i + SI_TLD * c] ;
        Pt [c + 64 * a] = s ;
    }
    __syncthreads () ;
    for (int e = tid ; e < 64 * nb ; e += 256) Bs [e] = Lb [(i64) (e >> 6) * ld + b0 + min (e & 63, nb - 1)] ;       // L_bb: [k + 64 c]
    __syncthreads () ;
    if (tid < 64)
    {
        for (int c = 0 ; c < nb ; c++) Ts [tid + SI_TLD * c] = -Ts [tid + SI_TLD * c] ;
        si_row_solve (Ts, SI_TLD, tid, Bs, 64, nb) ;
    }
    __syncthreads () ;
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

// Z [b, b] of one block: Q = I + the partials of its slices (added in slice order), Y = Q inv (L_bb) by rows,
// Z = inv (L_bb)' Y by columns; the lower triangle goes into the square and is mirrored into the upper one.
__global__ void __launch_bounds__(256) k_si_diag (const SiTask *tasks, const SiSlot *slots, const FrontD *fr,
    const double *Lx, double *M, const double *Pbuf)
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
    for (int e = tid ; e < SI_PTILE ; e += 256)
    {
        const int c = e & 63, a = e >> 6 ;
        double s = (a == c) ? 1.0 : 0.0 ;
        for (int q = 0 ; q < T.nslices ; q++) s += Pbuf [(T.poff + q) * (i64) SI_PTILE + e] ;
        Qs [a + SI_TLD * c] = s ;
    }
    for (int e = tid ; e < 64 * nb ; e += 256) Lbs [e] = Lbb [(i64) (e >> 6) * ld + min (e & 63, nb - 1)] ;
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
        const double v = Qs [a + SI_TLD * c] ;
        Mf [(i64) (b0 + a) + (i64) (b0 + c) * ld] = v ;
        Mf [(i64) (b0 + c) + (i64) (b0 + a) * ld] = v ;
    }
}

// the finished panel columns of a front from its square into Zx (the layout of Lx), the dead upper triangle of the
// diagonal block cleared
__global__ void __launch_bounds__(256) k_si_store (const SiTask *tasks, int nt, const SiSlot *slots, const FrontD *fr,
    const double *M, double *Zx)
{
    const SiTask T = tasks [si_find (tasks, nt, blockIdx.x)] ;
    const SiSlot S = slots [T.slot] ;
    const FrontD &f = fr [S.front] ;
    const int c = blockIdx.x - T.wg0, ld = f.nsrow ;
    if (c >= f.nscol) return ;
    const double *Mc = M + S.moff + (i64) c * ld ;
    double *Zc = Zx + f.psx + (i64) c * ld ;
    for (int i = threadIdx.x ; i < ld ; i += 256) Zc [i] = i < c ? 0.0 : Mc [i] ;
}

// A thin front (nscol <= SI_NB, nsrow <= SM_MAX) whole: one workgroup, the recurrence above with b = all its columns
// and R = its below-rows, everything in LDS, L read from the (cached) panel.
__global__ void __launch_bounds__(256) k_si_thin (const i32 *fronts, const FrontD *fr, const i32 *supermap, const i64 *Ls,
    const double *Lx, double *Zx)
{
    extern __shared__ __attribute__ ((aligned (16))) double si_lds [] ;
    const int tid = threadIdx.x ;
    const FrontD &f = fr [fronts [blockIdx.x]] ;
    const int nb = f.nscol, ld = f.nsrow, ncb = ld - nb, ldm = ncb | 1, ldq = nb | 1 ;
    double *Ms = si_lds, *Ts = Ms + ldm * ncb, *Qs = Ts + ldm * nb ;
    const i64 *I = Ls + f.psi + nb ;
    const double *Lp = Lx + f.psx ;             // L_bb at row 0, L [R, b] at row nb
    for (int e = tid ; e < ncb * ncb ; e += 256)
    {
        const int j = e / ncb, i = e - j * ncb ;
        if (i < j) continue ;
        const i64 c = I [j] ;
        const i64 q = si_locate (fr [supermap [c]], Ls, I [i], c) ;
        const double v = q >= 0 ? Zx [q] : si_nan () ;
        Ms [i + ldm * j] = v ; Ms [j + ldm * i] = v ;
    }
    __syncthreads () ;
    for (int e = tid ; e < ncb * nb ; e += 256)
    {
        const int c = e / ncb, i = e - c * ncb ;
        const double *Lc = Lp + (i64) c * ld + nb ;
        double s = 0 ;
        for (int k = 0 ; k < ncb ; k++) s += Ms [i + ldm * k] * Lc [k] ;
        Ts [i + ldm * c] = s ;
    }
    __syncthreads () ;
    for (int e = tid ; e < nb * nb ; e += 256)
    {
        const int c = e / nb, a = e - c * nb ;
        const double *La = Lp + (i64) a * ld + nb ;
        double s = (a == c) ? 1.0 : 0.0 ;
        for (int i = 0 ; i < ncb ; i++) s += La [i] * Ts [i + ldm * c] ;
        Qs [a + ldq * c] = s ;
    }
    __syncthreads () ;
    if (tid < ncb)
    {
        for (int c = 0 ; c < nb ; c++) Ts [tid + ldm * c] = -Ts [tid + ldm * c] ;
        si_row_solve (Ts, ldm, tid, Lp, ld, nb) ;
    }
    else if (tid < ncb + nb) si_row_solve (Qs, ldq, tid - ncb, Lp, ld, nb) ;
    __syncthreads () ;
    if (tid < nb) si_col_solve (Qs, ldq, tid, Lp, ld, nb) ;
    __syncthreads () ;
    double *Zp = Zx + f.psx ;
    for (int e = tid ; e < ld * nb ; e += 256)
    {
        const int c = e / ld, i = e - c * ld ;
        Zp [e] = i < c ? 0.0 : i < nb ? Qs [i + ldq * c] : Ts [(i - nb) + ldm * c] ;
    }
}

// ---- the gather of cholmod_hip_selinv_gather_device ------------------------------------------------------------------------

__global__ void __launch_bounds__(256) k_si_nan_fill (i64 n, double *out)
{
    const i64 k = blockIdx.x * (i64) 256 + threadIdx.x ;
    if (k < n) out [k] = si_nan () ;
}

// out [src [p]] = Z at the position of entry p of the resident packed S, for the entries S is read at (on or below the
// diagonal, the last of equal neighbours); the position comes from the supernode map and a search in the row list
// (d_amap knows the generic fronts only).  One thread per column of S.
__global__ void __launch_bounds__(256) k_si_gather_values (i64 n, const i64 *Sp, const i64 *Si, const i64 *src,
    const i32 *supermap, const FrontD *fr, const i64 *Ls, const double *Zx, double *out)
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
        if (q >= 0) out [src [p]] = Zx [q] ;
    }
}

// The variant of grad.hip (cholmod_hip_product_logdet_grad_device): the gradient of log det with respect to the value of
// entry p -- Z once on the diagonal, twice off it -- into an array the caller has filled with +0.0: where the gather above
// leaves the NaN of its fill, this one leaves the zero, so that no NaN enters a sum.  Work is divided by ENTRIES of S, as
// in grad_kernels.hip.h, with the column of an entry from grad.hip's column-of-entry array: S = tril (A A') has columns of
// hundreds of entries next to columns of one (one thread per column took 1.05 ms where this takes 26 us: a grid
// least-squares problem with eight dense rows, profiles/aat_grad_times.json).
__global__ void __launch_bounds__(256) k_si_gather_logdet_grad (i64 n, i64 nz, const i64 *Sp, const i64 *Si, const i32 *colof,
    const i64 *src, const i32 *supermap, const FrontD *fr, const i64 *Ls, const double *Zx, double *out)
{
    const i64 p = blockIdx.x * (i64) 256 + threadIdx.x ;
    if (p >= nz) return ;
    const i64 k = colof [p], i = Si [p] ;
    if (i < k || i >= n || (p + 1 < Sp [k + 1] && Si [p + 1] == i)) return ;
    const i64 q = si_locate (fr [supermap [k]], Ls, i, k) ;
    if (q >= 0) out [src [p]] = i != k ? 2.0 * Zx [q] : Zx [q] ;
}

// out [perm ? perm [k] : k] = Z (k, k)
__global__ void __launch_bounds__(256) k_si_gather_diag (i64 n, const i64 *perm, const i32 *supermap, const FrontD *fr,
    const double *Zx, double *out)
{
    const i64 k = blockIdx.x * (i64) 256 + threadIdx.x ;
    if (k >= n) return ;
    const FrontD &t = fr [supermap [k]] ;
    const i64 jc = k - t.k1 ;
    out [perm ? perm [k] : k] = Zx [t.psx + jc * (i64) t.nsrow + jc] ;
}

} // namespace sship
