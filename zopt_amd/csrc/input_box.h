// Input box (zm_inputbox_t): what the kernels share.  Extension; the reference has no counterpart.
#pragma once
#include "zm_common.h"

namespace zm {

// device view of a zm_inputbox_t: the bounds of trajectory t are the m doubles at lb + t * stride, ub + t * stride (stride 0: shared)
struct BoxRef {
    const double* lb;
    const double* ub;
    long stride;
};

inline BoxRef box_ref(const zm_inputbox_t& b) { return BoxRef{b.lb, b.ub, (long)b.stride}; }

// argument check shared by the box entry points (before any launch)
inline int box_check(const zm_inputbox_t* b, const int m, const char* who) {
    if (!b || !b->lb || !b->ub) return set_error(ZM_EINVAL, "%s: the box needs lb and ub", who);
    if (b->stride != 0 && b->stride != m)
        return set_error(ZM_EINVAL, "%s: box stride %lld (0: shared bounds, m = %d: per trajectory)", who, (long long)b->stride, m);
    return ZM_OK;
}

// clip that lets a NaN through (fmin / fmax would return the bound): the line search's "NaN wins the argmin" rule relies on it
__device__ __forceinline__ double clip_nan(const double u, const double lb, const double ub) { return u < lb ? lb : (u > ub ? ub : u); }

}  // namespace zm
