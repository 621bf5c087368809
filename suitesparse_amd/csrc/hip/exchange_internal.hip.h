// exchange_internal.hip.h -- what engine.hip needs of exchange.hip: the runner of an exchange launch, the agreement at
// the end of a factorization on several ranks, the statistics of the exchange and the release of the communicators.
// The kernels (exchange_kernels.hip.h) stay in exchange.hip's translation unit.  Internal to the library: not exported.
#pragma once
#include "plan.hip.h"

namespace sship {
#pragma GCC visibility push(hidden)

// one K_XCHG_RS / K_XCHG_AG launch of the schedule; run_launch does the cross-stream wait and the event record around it
int run_exchange (cholmod_hip_plan *P, const Launch &L, hipStream_t st, bool serial) ;
// every rank's first failing supernode and failed launches, agreed on: *sbad / *binfo become those of the first failing
// supernode of all ranks; an error (this rank's own `poisoned`, if it has one) when a launch failed anywhere
int agree_first_fail (cholmod_hip_plan *P, int poisoned, i64 *sbad, i64 *binfo) ;
// what the plan exchanges per factorization (stats [17], [18], [25], [39])
void exchange_volume (const cholmod_hip_plan *P, double *S) ;
// destroys the communicators of the native exchange, if any
void exchange_release (cholmod_hip_plan *P) ;
// the kernels of the exchange stream as one-wave workgroups (CHOLMOD_HIP_NARROW_EXCHANGE_KERNELS; K_WIN and K_EA ask, too)
bool narrow_xs () ;

#pragma GCC visibility pop
} // namespace sship
