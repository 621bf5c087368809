// selinv_internal.hip.h -- what the two sweeps that run the factorization backwards share (selinv.hip: the selected
// inverse; factor_grad.hip: reverse-mode Cholesky): the launch program -- the plan's batches from the last to the first, cut
// into chunks under CHOLMOD_HIP_SELINV_BUDGET_MB, with their slots, tasks and partial offsets --, the scratch squares and
// partials.  Both sweeps run on the engine stream, behind the caller's (stream_enter, stream_leave: plan.hip.h), so the
// scratch is never live in two of them.  Zx and Gx are separate arrays with separate staleness (P->si_valid,
// P->fg_valid).  The program is built by selinv.hip (sweep_ensure); the kernels differ, the steps do not.
#pragma once
#include "sweep_device.hip.h"
#include "plan.hip.h"

// device time and launches of the last run of one sweep (two events on the engine stream, read by its _info)
struct SweepClock {
    hipEvent_t ev0 = nullptr, ev1 = nullptr ;
    bool pending = false ;
    double seconds = 0 ;
    long launches = 0 ;
} ;

struct SelInv {
    enum { THIN, FILL, BLOCK, DIAG, STORE } ;
    struct Step { int kind ; i64 first ; int ntasks ; unsigned grid ; size_t lds ; } ;
    std::vector<Step> steps ;
    std::vector<SiTask> tasks ;
    std::vector<SiSlot> slots ;
    std::vector<i32> thin ;
    i64 m_len = 0, p_len = 0 ;              // doubles of the square scratch and of the partials
    double hot_flops = 0, all_flops = 0 ;
    bool built = false ;
    SiTask *d_tasks = nullptr ; SiSlot *d_slots = nullptr ; i32 *d_thin = nullptr ;
    double *d_Zx = nullptr, *d_M = nullptr, *d_P = nullptr ;
    SweepClock si_clock ;
    // factor_grad.hip: Gx, the partial sums of its trace (one per 256 columns), its clock; fg_ready: its kernels'
    // attributes are set
    double *d_Gx = nullptr, *d_tr = nullptr ;
    SweepClock fg_clock ;
    bool fg_ready = false ;
} ;

// what every entry point of both sweeps refuses, before any device call
static inline bool sweep_bad_plan (const cholmod_hip_plan *P)
{
    if (!real_device_plan (P)) return true ;
    return P->factor_state != 1 || !P->d_Lx ;       // no numeric factor on the device, or one that is not positive definite
}

// selinv.hip: the program (once per plan), the clocks, the scratch and the sweep's own array (xsize doubles) behind
// `result`: &SelInv::d_Zx or &SelInv::d_Gx; nothing is allocated once they exist.  A failure frees what the call allocated.
int sweep_ensure (cholmod_hip_plan *P, double *SelInv::*result) ;
// frees the sweep's own array, and the scratch if the other sweep holds no array either (the program stays)
void sweep_release (cholmod_hip_plan *P, double *SelInv::*result) ;
// seconds and launches of a clock into out8 [0], [1] (may wait for the run), the program's flops into [2], [3]
void sweep_info (SelInv *S, SweepClock &c, double *out8) ;
