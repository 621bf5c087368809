// solve_internal.hip.h -- what solve.hip shares with residual.hip: the workspaces of a device-resident solve and the
// sweeps over the plan's level schedule on a workspace that is already packed and permuted.  The kernels themselves
// (solve_kernels.hip.h) stay in solve.hip's translation unit; these are the host-side launchers.
#pragma once
#include "plan.hip.h"

#ifndef SD_NP
#define SD_NP 16        /* right-hand sides per panel */
#endif

// first nrhs that takes the 16-wide kernels.  A panel costs what about 3.5 sweeps of the one-column kernels cost
// (Poisson 100^3: 31 ms against 9.2 ms; its walk over the big supernodes is as latency-bound as theirs), and they
// take about 4.6 ms per further column: the panel wins from 6 - 8 right-hand sides on the 3D problems, from 4 on
// the 2D one (profiles/solve_device_times.json).  Below it the right-hand sides run column by column.
#define SD_BLOCK_MIN_NRHS 8

namespace sship {

// workspaces of a device-resident solve (its two timed events, W [n][16]; with_factor: those of the sweeps, for fewer than
// SD_BLOCK_MIN_NRHS right-hand sides if `columns`, for panels otherwise); nothing is allocated once they exist
int sd_ensure (cholmod_hip_plan *P, bool with_factor, bool columns) ;
// the explicit inverses of the diagonal blocks of the big supernodes, recomputed on the engine stream if the factor
// changed since they were
void refresh_inverses (cholmod_hip_plan *P, const FrontD *frw, const double *Lw, bool cxs) ;
// the columns src [nrhs][lds] into dst [nrhs][ldd], through the permutation if there is one (inverse: scattered by it)
int sd_move_columns (hipStream_t st, i64 n, i64 nrhs, const i64 *perm, int inverse, const double *src, i64 lds, double *dst, i64 ldd) ;
// pw (<= 16) columns of B (column-major, ldb) through perm into the panel W [n][16] / of W through perm into X
void sd_pack (hipStream_t st, i64 n, const i64 *perm, const double *B, i64 ldb, int pw, double *W) ;
void sd_unpack (hipStream_t st, i64 n, const i64 *perm, const double *W, int pw, double *X, i64 ldx) ;
// solve_sweeps (which: 0 = L then L', 1 = L, 2 = L') with the one-column kernels on x [nrhs][ldx], with the 16-wide
// ones on W [n][16]; cxs: Lw is a complex factor in its own storage (CHOLMOD_HIP_CX_STORAGE)
void sd_sweeps_columns (const cholmod_hip_plan *P, int which, const FrontD *frw, const double *Lw, bool cxs, hipStream_t st, double *x, i64 ldx, int nrhs) ;
void sd_sweeps_panel (const cholmod_hip_plan *P, int which, const FrontD *frw, const double *Lw, bool cxs, hipStream_t st, double *W) ;

} // namespace sship
