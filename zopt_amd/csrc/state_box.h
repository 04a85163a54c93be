// State box (zm_statebox_t): what the kernels of the augmented-Lagrangian loop share.  Extension; the reference has no counterpart.
//
//   s_ub = lam_ub + mu (x_i - ub_i),  s_lb = lam_lb + mu (lb_i - x_i),  pos(s) = s > 0 ? s : 0  (a NaN gives 0)
//   psi  = (pos(s_ub)^2 - lam_ub^2 + pos(s_lb)^2 - lam_lb^2) / (2 mu)       penalty of component i of row k >= 1
//   g_i  = pos(s_ub) - pos(s_lb),   h_i = mu ((s_ub > 0) + (s_lb > 0))      its gradient and (Gauss-Newton) Hessian entry
#pragma once
#include "zm_common.h"

namespace zm {

// device view of a zm_statebox_t: the bounds of trajectory t are the n doubles at lb + t * stride, ub + t * stride (stride 0: shared);
// the multipliers of its row k the n doubles at lam_* + (t * (T + 1) + k) * n; its penalty mu[t]
struct PenRef {
    const double* lb;
    const double* ub;
    long stride;
    const double* lam_lb;
    const double* lam_ub;
    const double* mu;
};

inline PenRef pen_ref(const zm_statebox_t& b) { return PenRef{b.lb, b.ub, (long)b.stride, b.lam_lb, b.lam_ub, b.mu}; }

// argument check shared by the state-box entry points (before any launch)
inline int statebox_check(const zm_statebox_t* b, const int n, const char* who) {
    if (!b || !b->lb || !b->ub || !b->lam_lb || !b->lam_ub || !b->mu) return set_error(ZM_EINVAL, "%s: the state box needs lb, ub, lam_lb, lam_ub and mu", who);
    if (b->stride != 0 && b->stride != n)
        return set_error(ZM_EINVAL, "%s: state box stride %lld (0: shared bounds, n = %d: per trajectory)", who, (long long)b->stride, n);
    return ZM_OK;
}

__device__ __forceinline__ double pen_pos(const double s) { return s > 0.0 ? s : 0.0; }   // NaN -> 0

// psi of one component; the products are written as they are summed (no contraction across the differences would change a 0.0)
__device__ __forceinline__ double pen_psi(const double x, const double lb, const double ub, const double ll, const double lu, const double mu) {
    const double pu = pen_pos(lu + mu * (x - ub)), pl = pen_pos(ll + mu * (lb - x));
    return (((pu * pu - lu * lu) + pl * pl) - ll * ll) / (2.0 * mu);
}

}  // namespace zm
