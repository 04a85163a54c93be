// Host side of zm_tracedcon_t (traced_con.hip) that ilqr_solve.hip calls: the descriptor check and the expansion with the solve's
// per-trajectory iteration counter.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/zopt_amd.h"

namespace zm {

// sizes, counts and pointers of a recorded constraint over a model of (n, m); `arrays`: lam, lam_terminal and mu are needed too.
// ZM_OK or an error set with set_error under the name `who`.  Host code only.
int tracedcon_check(const zm_tracedcon_t* con, int n, int m, bool arrays, const char* who);

// zm_traced_con_expand_list_f64 behind its checks; visits (batch, optional) += 1 per listed active trajectory
int traced_con_expand(const zm_tracedcon_t* con, const double* xTraj, const double* uTraj, const int32_t* list, int64_t count,
                      const int32_t* active, const double* sc_xx, const double* sc_ux, const double* sc_uu, const double* sv_xx,
                      double* c_x, double* c_u, double* v_x, double* c_xx, double* c_ux, double* c_uu, double* v_xx, int32_t* visits,
                      int64_t batch, int T, hipStream_t st);

}  // namespace zm
