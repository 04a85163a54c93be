// Tracking cost (zm_trackcost_t): what the kernels share.
//
//   c(x,u) = (x - xr_k)^T Q (x - xr_k) + (u - ur_k)^T R (u - ur_k),   c_f(x) = (x - xr_T)^T Qf (x - xr_T)
//
// The reference's drivers take cost callables (zopt/ilqrUtils.py:260-269); its demo's cost is the one about the origin
// (demos/iterativeLqr.py:12-13,37).  Every kernel forms the difference d = z - ref first and then runs the operation sequence of
// its zm_quadcost_t sibling on d: with a zero reference d == z bit for bit (z - 0.0 and fma(0.0, -1.0, z) return z, also for -0.0,
// infinities and NaN), hence so is every result.
#pragma once
#include "models.h"
#include "zm_common.h"

namespace zm {

// device view of the reference of a zm_trackcost_t: row k of trajectory t of xRef starts at x + t * xt + k * xk (doubles; a stride
// may be 0), nullptr = zeros
struct TrackRef {
    const double* x;
    const double* u;
    long xt, xk, ut, uk;
};

inline TrackRef track_ref(const zm_trackcost_t& c) {
    return TrackRef{c.xRef, c.uRef, (long)c.xref_traj_stride, (long)c.xref_step_stride, (long)c.uref_traj_stride,
                    (long)c.uref_step_stride};
}
inline zm_quadcost_t track_weights(const zm_trackcost_t& c) { return zm_quadcost_t{c.Q, c.R, c.Qf, c.diagonal, 0}; }

// argument check shared by the tracking entry points (before any launch)
inline int track_check(const zm_trackcost_t* c, const char* who) {
    if (!c || !c->Q || !c->R || !c->Qf) return set_error(ZM_EINVAL, "%s: tracking cost needs Q, R, Qf", who);
    if (c->xref_traj_stride < 0 || c->xref_step_stride < 0 || c->uref_traj_stride < 0 || c->uref_step_stride < 0)
        return set_error(ZM_EINVAL, "%s: negative reference stride", who);
    return ZM_OK;
}

// The cost argument(s) of an entry, resolved (host): the weights (the Hessians, the conditioning and the kernels' cost arithmetic read
// only these) and, for a zm_trackcost_t, the reference that cost values and gradients are taken about.  `track` == nullptr is the
// zm_quadcost_t path with exactly its launches.
struct CostRef {
    bool given = false;
    zm_quadcost_t w = zm_quadcost_t{nullptr, nullptr, nullptr, 0, 0};
    const zm_trackcost_t* track = nullptr;
    TrackRef ref = TrackRef{};
    const zm_quadcost_t* weights() const { return given ? &w : nullptr; }
    const TrackRef* ref_ptr() const { return track ? &ref : nullptr; }
};
// what an entry's parameter list takes: a zm_quadcost_t (may be missing: the entry's own null check answers), a zm_trackcost_t, or
// the pair (cost, track) with at most / exactly one of the two given
enum class CostArg { quad, track, at_most_one, exactly_one };
inline int cost_resolve(const zm_quadcost_t* cost, const zm_trackcost_t* track, const CostArg form, const char* who, CostRef* out) {
    if (form == CostArg::at_most_one && cost && track) return set_error(ZM_EINVAL, "%s: pass cost or track, not both", who);
    if (form == CostArg::exactly_one && (cost != nullptr) == (track != nullptr))
        return set_error(ZM_EINVAL, "%s: pass exactly one of cost and track", who);
    if (track || form == CostArg::track) {
        if (const int rc = track_check(track, who)) return rc;
        out->given = true, out->w = track_weights(*track), out->track = track, out->ref = track_ref(*track);
    } else if (cost) {
        out->given = true, out->w = *cost;
    }
    return ZM_OK;
}

__device__ __forceinline__ const double* track_xrow(const TrackRef& r, const long t, const long k) {
    return r.x ? r.x + t * r.xt + k * r.xk : nullptr;
}
__device__ __forceinline__ const double* track_urow(const TrackRef& r, const long t, const long k) {
    return r.u ? r.u + t * r.ut + k * r.uk : nullptr;
}

// d[i] = z[i] - ref[i] for i < cnt (ref == nullptr: zeros); entries past cnt are copied
template <int K>
__device__ __forceinline__ void track_diff(double (&d)[K], const double (&z)[K], const double* __restrict__ ref, const int cnt) {
#pragma unroll
    for (int i = 0; i < K; ++i) d[i] = (ref && i < cnt) ? z[i] - ref[i] : z[i];
}

}  // namespace zm
