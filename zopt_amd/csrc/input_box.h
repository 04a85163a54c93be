// Input box (zm_inputbox_t): what the kernels share.  Extension; the reference has no counterpart.
#pragma once
#include "zm_common.h"

namespace zm {

// device view of a zm_inputbox_t: the bounds of trajectory t at step k are the m doubles at lb + t * stride + k * step, ub + t * stride
// + k * step (stride 0: shared by the trajectories; step 0: one box for the whole horizon -- the constant form, whose kernels never
// read `step`)
struct BoxRef {
    const double* lb;
    const double* ub;
    long stride;
    long step;
};

inline BoxRef box_ref(const zm_inputbox_t& b) { return BoxRef{b.lb, b.ub, (long)b.stride, (long)b.step_stride}; }

// argument check shared by the box entry points (before any launch); T: the horizon of the call (the stage form's rows per trajectory)
inline int box_check(const zm_inputbox_t* b, const int m, const int T, const char* who) {
    if (!b || !b->lb || !b->ub) return set_error(ZM_EINVAL, "%s: the box needs lb and ub", who);
    if (b->step_stride == 0) {
        if (b->stride != 0 && b->stride != m)
            return set_error(ZM_EINVAL, "%s: box stride %lld (0: shared bounds, m = %d: per trajectory)", who, (long long)b->stride, m);
    } else if (b->step_stride == m) {
        if (b->stride != 0 && b->stride != (int64_t)T * m)
            return set_error(ZM_EINVAL, "%s: box stride %lld with step_stride %d (0: one schedule for every trajectory, T * m = %lld: per "
                                        "trajectory)", who, (long long)b->stride, m, (long long)T * m);
    } else {
        return set_error(ZM_EINVAL, "%s: box step_stride %lld (0: one box for the horizon, m = %d: a row per step)", who,
                         (long long)b->step_stride, m);
    }
    return ZM_OK;
}

// the input box inside a state box: the penalty kernels take the constant form only
inline int box_check_constant(const zm_inputbox_t* b, const int m, const int T, const char* who) {
    if (const int rc = box_check(b, m, T, who)) return rc;
    if (b->step_stride != 0)
        return set_error(ZM_EUNSUPPORTED, "%s: stage-varying input bounds (step_stride != 0) next to a state box are not built", who);
    return ZM_OK;
}

// clip that lets a NaN through (fmin / fmax would return the bound): the line search's "NaN wins the argmin" rule relies on it
__device__ __forceinline__ double clip_nan(const double u, const double lb, const double ub) { return u < lb ? lb : (u > ub ? ub : u); }

}  // namespace zm
