// Host-side dispatch of ZM_MODEL_TRACED (traced.hip): what the entry points of rollout.hip, linearize.hip and mpc.hip call once they
// have seen the kind.  `md` has passed traced_check; sizes and the other operands are the caller's to check.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/zopt_amd.h"

namespace zm {

// counts, pointers and mask of a ZM_MODEL_TRACED descriptor; ZM_OK or an error set with set_error under the name `who`
int traced_check(const zm_model_t* model, const char* who);

int traced_rollout(const zm_model_t& md, const zm_quadcost_t* cost, const double* x0, const double* l, const double* L,
                   const double* xPrev, const double* uPrev, const double* alphas, int n_alpha, const int* active, const int* list,
                   long count, double* xTraj, double* uTraj, double* J, int* alpha_idx, long batch, int T, hipStream_t st);
int traced_step(const zm_model_t& md, const double* x, const double* u, double* xNext, long batch, hipStream_t st);
int traced_linearize(const zm_model_t& md, const double* xTraj, const double* uTraj, const int* active, double* f, double* f_x,
                     double* f_u, long batch, int T, const int* list, long count, hipStream_t st);
int traced_quadratic(const zm_model_t& md, const double* xTraj, const double* uTraj, const int* active, double* f_xx, double* f_ux,
                     double* f_uu, long batch, int T, const int* list, long count, hipStream_t st);

// the structural mask of any model kind on the host (model_nonlinear_mask of models.h is also device code and stays as it is)
inline unsigned traced_or_registered_mask(const zm_model_t& md, unsigned registered_mask) {
    return md.kind == ZM_MODEL_TRACED ? (unsigned)md.reserved : registered_mask;
}

}  // namespace zm
