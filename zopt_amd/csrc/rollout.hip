// K6  rollout_linesearch -- batched policy rollout + parallel line search over step sizes, fp64, gfx950.
//
// Replaces zopt/ilqrUtils.py:33-66 (trajectoryRollout), :116-150 (forwardPass2), pytrees.py:215-220 (AffinePolicy call)
// and pytrees.py:49-52 (CostFunction call) for registered device models (models.h).
//
// Mapping: ONE LANE per (trajectory, step size).  With 16 step sizes a wave64 carries 4 trajectories; the 16 lanes of a
// trajectory read the same l_k, L_k, xPrev_k, uPrev_k addresses (one memory transaction each) and keep x, u in
// registers.  Pass 1 accumulates J for every step size; a 16-lane argmin (NaN wins, first index on ties, as
// jnp.argmin) picks the step; pass 2 re-rolls that step size (bit-identical arithmetic) and its first lane stores the
// trajectory -- the other 15 rollouts never touch HBM.  This chain is latency/ALU-bound, not HBM-bound: it reads
// 8(mn + 2m + n) = 544 B per trajectory step.
#include "input_box.h"
#include "models.h"
#include "state_box.h"
#include "track_cost.h"
#include "traced.h"
#include "zm_common.h"

#include <cstdlib>

namespace zm {

// one rollout; STORE: write xTraj/uTraj; returns J (0 when cost == nullptr)
// TRK: tracking cost -- the cost of step k is that of (x_k - xr_k, u_k - ur_k), rows of trajectory `t` of `tr`
// BOX: u_k is clipped into [lb, ub], the bounds of trajectory `t` of `bx` (the clip lets a NaN through); the cost may then be absent
// (cs == nullptr) also in the TRK form
// STG (with BOX): the bounds change along the horizon -- step k clips into row k of the trajectory's schedule (bx.step doubles apart),
// read inside the step loop with the step's policy data; the constant form loads its one row before the loop
// PEN: the augmented-Lagrangian penalty of the state box `pr` on the rows k = 1..T goes into an accumulator of its own (k ascending,
// i ascending) and joins the cost once, at the end; *jcost (optional) <- the cost without it
template <bool STORE, bool TRK = false, bool BOX = false, bool PEN = false, bool STG = false>
__device__ __forceinline__ double rollout_one(const zm_model_t& md, const zm_quadcost_t* cs, const double alpha,
                                              const double* __restrict__ x0, const double* __restrict__ l,
                                              const double* __restrict__ L, const double* __restrict__ xPrev,
                                              const double* __restrict__ uPrev, double* __restrict__ xTraj,
                                              double* __restrict__ uTraj, const int T, const TrackRef& tr = TrackRef{},
                                              const long t = 0, const BoxRef& bx = BoxRef{}, const PenRef& pr = PenRef{},
                                              double* jcost = nullptr) {
    const int n = md.n, m = md.m;
    double x[MAXN], u[MAXM], xn[MAXN];
    double plo[PEN ? MAXN : 1], phi[PEN ? MAXN : 1];
    double P = 0.0, pmu = 1.0;
    if constexpr (PEN) {
        pmu = pr.mu[t];
#pragma unroll
        for (int i = 0; i < MAXN; ++i) {
            plo[i] = (i < n) ? pr.lb[t * pr.stride + i] : -__builtin_inf();
            phi[i] = (i < n) ? pr.ub[t * pr.stride + i] : __builtin_inf();
        }
    }
    double blo[BOX ? MAXM : 1], bhi[BOX ? MAXM : 1];
    static_assert(!STG || (BOX && !PEN), "stage-varying bounds: the box form without a state-box penalty");
    if constexpr (BOX && !STG) {
#pragma unroll
        for (int i = 0; i < MAXM; ++i) {
            blo[i] = (i < m) ? bx.lb[t * bx.stride + i] : -__builtin_inf();
            bhi[i] = (i < m) ? bx.ub[t * bx.stride + i] : __builtin_inf();
        }
    }
#pragma unroll
    for (int i = 0; i < MAXN; ++i) x[i] = (i < n) ? x0[i] : 0.0;
    if (STORE) {
#pragma unroll
        for (int i = 0; i < MAXN; ++i)
            if (i < n) xTraj[i] = x[i];
    }
    double J = 0.0;
    for (int k = 0; k < T; ++k) {
        const double* Lk = L + (long)k * m * n;
        const double* xp = xPrev + (long)k * n;
        if constexpr (STG) {   // row k of the schedule: independent of x, in flight under the policy product
#pragma unroll
            for (int i = 0; i < MAXM; ++i) {
                blo[i] = (i < m) ? bx.lb[t * bx.stride + (long)k * bx.step + i] : -__builtin_inf();
                bhi[i] = (i < m) ? bx.ub[t * bx.stride + (long)k * bx.step + i] : __builtin_inf();
            }
        }
        double dx[MAXN];
#pragma unroll
        for (int j = 0; j < MAXN; ++j) dx[j] = (j < n) ? (x[j] - xp[j]) : 0.0;
#pragma unroll
        for (int i = 0; i < MAXM; ++i) {
            if (i < m) {
                double s = 0.0;  // L_k @ dx
#pragma unroll
                for (int j = 0; j < MAXN; ++j)
                    if (j < n) s = __builtin_fma(Lk[i * n + j], dx[j], s);
                u[i] = (alpha * l[(long)k * m + i] + s) + uPrev[(long)k * m + i];   // pytrees.py:220, ilqrUtils.py:60
                if constexpr (BOX) u[i] = clip_nan(u[i], blo[i], bhi[i]);
            } else {
                u[i] = 0.0;
            }
        }
        if constexpr (TRK) {
            if (!BOX || cs) {
                double ex[MAXN], eu[MAXM];
                track_diff(ex, x, track_xrow(tr, t, k), n);
                track_diff(eu, u, track_urow(tr, t, k), m);
                J += running_cost(*cs, n, m, ex, eu);
            }
        } else {
            if (cs) J += running_cost(*cs, n, m, x, u);
        }
        if constexpr (PEN) {
            if (k >= 1) {
                const double* ll = pr.lam_lb + (t * (T + 1) + k) * n;
                const double* lu = pr.lam_ub + (t * (T + 1) + k) * n;
#pragma unroll
                for (int i = 0; i < MAXN; ++i)
                    if (i < n) P += pen_psi(x[i], plo[i], phi[i], ll[i], lu[i], pmu);
            }
        }
        model_step<double>(md, x, u, xn);
#pragma unroll
        for (int i = 0; i < MAXN; ++i) x[i] = xn[i];
        if (STORE) {
#pragma unroll
            for (int i = 0; i < MAXM; ++i)
                if (i < m) uTraj[(long)k * m + i] = u[i];
#pragma unroll
            for (int i = 0; i < MAXN; ++i)
                if (i < n) xTraj[(long)(k + 1) * n + i] = x[i];
        }
    }
    if constexpr (TRK) {
        if (!BOX || cs) {
            double ex[MAXN];
            track_diff(ex, x, track_xrow(tr, t, T), n);
            J += terminal_cost(*cs, n, ex);
        }
    } else {
        if (cs) J += terminal_cost(*cs, n, x);
    }
    if constexpr (PEN) {
        const double* ll = pr.lam_lb + (t * (T + 1) + T) * n;
        const double* lu = pr.lam_ub + (t * (T + 1) + T) * n;
#pragma unroll
        for (int i = 0; i < MAXN; ++i)
            if (i < n) P += pen_psi(x[i], plo[i], phi[i], ll[i], lu[i], pmu);
        if (jcost) *jcost = J;
        J += P;
    }
    return J;
}

// NA = lanes per trajectory (power of two <= 16 that holds n_alpha)
#define ZM_TRK_FLAG
#define ZM_TRK_ARGS
#define ZM_PEN_STORE_ARGS
template <int NA>
__global__ __launch_bounds__(64) void rollout_linesearch_kernel(const zm_model_t md, const zm_quadcost_t cost,
                                                                const bool has_cost, const double* __restrict__ x0,
                                                                const double* __restrict__ l, const double* __restrict__ L,
                                                                const double* __restrict__ xPrev,
                                                                const double* __restrict__ uPrev,
                                                                const double* __restrict__ alphas, const int n_alpha,
                                                                const int* __restrict__ active, const int* __restrict__ list,
                                                                const long count, double* __restrict__ xTraj,
                                                                double* __restrict__ uTraj, double* __restrict__ Jout,
                                                                int* __restrict__ idx_out, const long batch, const int T) {
#include "rollout_linesearch_body.h"
}
#undef ZM_TRK_FLAG
#undef ZM_TRK_ARGS
#undef ZM_PEN_STORE_ARGS
// the same line search on the tracking cost (zm_trackcost_t): `cost` holds its weights, `tr` its reference
#define ZM_TRK_FLAG , true
#define ZM_TRK_ARGS , tr, t
#define ZM_PEN_STORE_ARGS
template <int NA>
__global__ __launch_bounds__(64) void rollout_linesearch_track_kernel(const zm_model_t md, const zm_quadcost_t cost, const TrackRef tr,
                                                                      const double* __restrict__ x0, const double* __restrict__ l,
                                                                      const double* __restrict__ L, const double* __restrict__ xPrev,
                                                                      const double* __restrict__ uPrev,
                                                                      const double* __restrict__ alphas, const int n_alpha,
                                                                      const int* __restrict__ active, const int* __restrict__ list,
                                                                      const long count, double* __restrict__ xTraj,
                                                                      double* __restrict__ uTraj, double* __restrict__ Jout,
                                                                      int* __restrict__ idx_out, const long batch, const int T) {
    constexpr bool has_cost = true;
#include "rollout_linesearch_body.h"
}
#undef ZM_TRK_FLAG
#undef ZM_TRK_ARGS
#undef ZM_PEN_STORE_ARGS
// the same line search with input bounds (zm_inputbox_t), on either cost: the tracking form, whose reference is null for a
// zm_quadcost_t (the differences are then the values themselves, bit for bit)
// STG: the bounds are a row per step (zm_inputbox_t.step_stride == m); the constant form is the kernel's other instantiation
#define ZM_TRK_FLAG , true, true, false, STG
#define ZM_TRK_ARGS , tr, t, bx
#define ZM_PEN_STORE_ARGS
template <int NA, bool STG>
__global__ __launch_bounds__(64) void rollout_linesearch_box_kernel(const zm_model_t md, const zm_quadcost_t cost, const bool has_cost,
                                                                    const TrackRef tr, const BoxRef bx, const double* __restrict__ x0,
                                                                    const double* __restrict__ l, const double* __restrict__ L,
                                                                    const double* __restrict__ xPrev, const double* __restrict__ uPrev,
                                                                    const double* __restrict__ alphas, const int n_alpha,
                                                                    const int* __restrict__ active, const int* __restrict__ list,
                                                                    const long count, double* __restrict__ xTraj,
                                                                    double* __restrict__ uTraj, double* __restrict__ Jout,
                                                                    int* __restrict__ idx_out, const long batch, const int T) {
#include "rollout_linesearch_body.h"
}
#undef ZM_TRK_FLAG
#undef ZM_TRK_ARGS
#undef ZM_PEN_STORE_ARGS
// the same line search on the augmented-Lagrangian cost of a state box (zm_statebox_t), without (BOXED = false: infinite input bounds
// are never read) or with input bounds; the store pass also writes the cost without the penalty (Jc_out, optional)
#define ZM_TRK_FLAG , true, BOXED, true
#define ZM_TRK_ARGS , tr, t, bx, pr
#define ZM_PEN_STORE_ARGS , (Jc_out ? Jc_out + t : nullptr)
template <int NA, bool BOXED>
__global__ __launch_bounds__(64) void rollout_linesearch_pen_kernel(const zm_model_t md, const zm_quadcost_t cost, const TrackRef tr,
                                                                    const BoxRef bx, const PenRef pr, const double* __restrict__ x0,
                                                                    const double* __restrict__ l, const double* __restrict__ L,
                                                                    const double* __restrict__ xPrev, const double* __restrict__ uPrev,
                                                                    const double* __restrict__ alphas, const int n_alpha,
                                                                    const int* __restrict__ active, const int* __restrict__ list,
                                                                    const long count, double* __restrict__ xTraj,
                                                                    double* __restrict__ uTraj, double* __restrict__ Jout,
                                                                    double* __restrict__ Jc_out, int* __restrict__ idx_out,
                                                                    const long batch, const int T) {
    constexpr bool has_cost = true;
#include "rollout_linesearch_body.h"
}
#undef ZM_TRK_FLAG
#undef ZM_TRK_ARGS
#undef ZM_PEN_STORE_ARGS

// rollout_fast.hip: compile-time (n, m) = (12, 4), 16 step sizes
int rollout_fast_dispatch(const zm_model_t& md, const double* Q, const double* R, const double* Qf, int diagonal, const double* x0,
                          const double* l, const double* L, const double* xPrev, const double* uPrev,
                          const double* alphas, int n_alpha, const int* active, const int* list, int64_t count, double* xTraj,
                          double* uTraj, double* J, int* idx, int64_t batch, int T, hipStream_t st, double* scratch,
                          const TrackRef* track, const BoxRef* box = nullptr);

}  // namespace zm

namespace zm {
int rollout_wide_dispatch(const zm_model_t& md, const zm_quadcost_t* cost, const double* x0, const double* l, const double* L,
                          const double* xPrev, const double* uPrev, const double* alphas, int n_alpha, const int* active,
                          const int* list, long count, double* xTraj, double* uTraj, double* J, int* idx, long batch, int T,
                          hipStream_t st);   // rollout_wide.hip
}
// the penalty form (the *_state_* entry points): the state box, its optional input box and the cost-without-penalty output
struct PenArgs {
    const zm_statebox_t* sbox;
    const zm_inputbox_t* box;
    double* J_cost;
};
static const char* const ROLLOUT = "zm_rollout_linesearch_f64";   // the name the entries without a penalty report under
static int rollout_impl(const char* who, const zm_model_t* model, const zm_quadcost_t* cost, const double* x0,
                                         const double* l, const double* L, const double* xPrev, const double* uPrev,
                                         const double* alphas, int n_alpha, const int32_t* active, const int32_t* list,
                                         int64_t count, double* xTraj, double* uTraj, double* J, int32_t* alpha_idx,
                                         int64_t batch, int T, void* stream, double* scratch = nullptr,
                                         const zm::TrackRef* track = nullptr, const zm::BoxRef* box = nullptr,
                                         const PenArgs* pen = nullptr) {
    // box != nullptr: the inputs are clipped into it (the *_box_* entry points); one lane per rollout, two passes
    // track != nullptr: `cost` holds the weights of a zm_trackcost_t and *track its reference (the *_tracking_* entry points)
    // pen != nullptr: the cost is the augmented-Lagrangian one of pen->sbox, with pen->box clipping the inputs (generic kernel only)
    if (!model || !x0 || !l || !L || !xPrev || !uPrev || !alphas || !xTraj || !uTraj || (pen && !J))
        return zm::set_error(ZM_EINVAL, "%s: null pointer", who);
    if (batch < 0 || T < (pen ? 1 : 0) || n_alpha < 1 || n_alpha > 16)
        return zm::set_error(ZM_EINVAL, "%s: bad size batch=%lld T=%d n_alpha=%d", who, (long long)batch, T, n_alpha);
    if (n_alpha > 1 && !cost) return zm::set_error(ZM_EINVAL, "%s: a line search needs a cost", who);
    zm_model_t md;
    if (const int rc = zm::model_check(model, who, &md)) return rc;
    if (md.kind == ZM_MODEL_TRACED) {   // the interpreter's kernels (traced.hip): plain cost, no bounds
        if (track || box || pen || scratch)
            return zm::set_error(ZM_EUNSUPPORTED, "%s: a traced model takes a zm_quadcost_t and no bounds (tracking cost, input box and "
                                                  "state box on the tape interpreter are not built)", who);
        if (cost && (!cost->Q || !cost->R || !cost->Qf)) return zm::set_error(ZM_EINVAL, "%s: cost needs Q, R, Qf", who);
        if (batch == 0 || (list && count == 0)) return ZM_OK;
        if (count < 0 || count > batch) return zm::set_error(ZM_EINVAL, "zm_rollout_linesearch: bad list length");
        return zm::traced_rollout(md, cost, x0, l, L, xPrev, uPrev, alphas, n_alpha, (const int*)active, (const int*)list, (long)count,
                                  xTraj, uTraj, J, (int*)alpha_idx, (long)batch, T, (hipStream_t)stream);
    }
    const bool wide = !pen && md.kind == ZM_MODEL_LINEAR && (md.n > zm::MAXN || md.m > zm::MAXM) && md.n >= 1 && md.m >= 1 &&
                      md.n <= 64 && md.m <= 16;   // large linear models: one wave per rollout (rollout_wide.hip)
    if (!wide && (md.n < 1 || md.n > zm::MAXN || md.m < 1 || md.m > zm::MAXM))
        return zm::set_error(ZM_EUNSUPPORTED, "%s: (n=%d, m=%d) not covered (%s)", who, md.n, md.m,
                             pen ? "state box: n<=12, m<=4" : "n<=12, m<=4; linear models n<=64, m<=16");
    if (cost && (!cost->Q || !cost->R || !cost->Qf)) return zm::set_error(ZM_EINVAL, "%s: cost needs Q, R, Qf", who);
    if (pen) {
        if (pen->box)
            if (const int rc = zm::box_check_constant(pen->box, md.m, T, who)) return rc;
        if (const int rc = zm::statebox_check(pen->sbox, md.n, who)) return rc;
        if (list && (count < 0 || count > batch)) return zm::set_error(ZM_EINVAL, "%s: bad list length", who);
    }
    if (batch == 0 || (list && count == 0)) return ZM_OK;
    if (count < 0 || count > batch) return zm::set_error(ZM_EINVAL, "zm_rollout_linesearch: bad list length");
    if (wide && track)
        return zm::set_error(ZM_EUNSUPPORTED, "zm_rollout_linesearch_tracking_f64: (n=%d, m=%d) not covered (tracking cost: n<=12, m<=4)",
                             md.n, md.m);
    if (wide && box)
        return zm::set_error(ZM_EUNSUPPORTED, "zm_rollout_linesearch_box_f64: (n=%d, m=%d) not covered (input box: n<=12, m<=4)", md.n, md.m);
    if (box && scratch) return zm::set_error(ZM_EUNSUPPORTED, "rollout: the input box has no all-store form");
    if (wide) {
        if (scratch) return zm::set_error(ZM_EUNSUPPORTED, "rollout: all-store mode needs the fast path");
        return zm::rollout_wide_dispatch(md, cost, x0, l, L, xPrev, uPrev, alphas, n_alpha, (const int*)active, (const int*)list,
                                         (long)count, xTraj, uTraj, J, (int*)alpha_idx, (long)batch, T, (hipStream_t)stream);
    }
    if (scratch && !(n_alpha == 16 && list && alpha_idx && J)) return zm::set_error(ZM_EINVAL, "rollout: all-store mode needs 16 step sizes, a list, J and alpha_idx");
    const int64_t nslot = list ? count : batch;
    hipStream_t st = (hipStream_t)stream;
    zm_quadcost_t cs = cost ? *cost : zm_quadcost_t{nullptr, nullptr, nullptr, 0, 0};
    const bool hc = cost != nullptr;
    const int* act = (const int*)active;
    static const bool force_generic = [] {
        const char* e = zm::fallback_env("ZOPT_AMD_ROLLOUT_PATH");
        return e && e[0] == 'g';
    }();
    const bool windy = md.wind_ned[0] != 0.0 || md.wind_ned[1] != 0.0 || md.wind_ned[2] != 0.0;   // fast path: still air only
    // (one step size -- the solvers' initial rollout -- runs the same kernel with all 16 lanes of a group on that step size: 16x
    //  redundant, and still several times faster than the generic lane-per-trajectory kernel with its uncoalesced policy reads)
    if (!pen && !force_generic && !windy && (n_alpha == 16 || n_alpha == 1) && md.n == 12 && md.m == 4 && cost && T >= 1)
        return zm::rollout_fast_dispatch(md, cs.Q, cs.R, cs.Qf, cs.diagonal, x0, l, L, xPrev, uPrev, alphas, n_alpha, act, (const int*)list, count, xTraj,
                                         uTraj, J, (int*)alpha_idx, batch, T, st, scratch, track, box);
    if (scratch) return zm::set_error(ZM_EUNSUPPORTED, "rollout: all-store mode needs the fast path");
    const zm::TrackRef tr = track ? *track : zm::TrackRef{};
    if (pen) {
        const zm::BoxRef bx = pen->box ? zm::box_ref(*pen->box) : zm::BoxRef{};
        const zm::PenRef pr = zm::pen_ref(*pen->sbox);
#define ZM_LAUNCH_PEN(NA_, BOXED_, BLOCKS_)                                                                                               \
    hipLaunchKernelGGL((zm::rollout_linesearch_pen_kernel<NA_, BOXED_>), dim3((unsigned)(BLOCKS_)), dim3(64), 0, st, md, cs, tr, bx, pr, x0, \
                       l, L, xPrev, uPrev, alphas, n_alpha, act, (const int*)list, (long)count, xTraj, uTraj, J, pen->J_cost,             \
                       (int*)alpha_idx, (long)batch, T)
        if (n_alpha == 1) {
            if (pen->box) ZM_LAUNCH_PEN(1, true, (nslot + 63) / 64);
            else ZM_LAUNCH_PEN(1, false, (nslot + 63) / 64);
        } else {
            if (pen->box) ZM_LAUNCH_PEN(16, true, (nslot + 3) / 4);
            else ZM_LAUNCH_PEN(16, false, (nslot + 3) / 4);
        }
#undef ZM_LAUNCH_PEN
        ZM_HIP_CHECK(hipGetLastError());
        return ZM_OK;
    }
    if (box) {
#define ZM_LAUNCH_BOX(NA_, STG_, BLOCKS_)                                                                                                 \
    hipLaunchKernelGGL((zm::rollout_linesearch_box_kernel<NA_, STG_>), dim3((unsigned)(BLOCKS_)), dim3(64), 0, st, md, cs, hc, tr, *box, x0, \
                       l, L, xPrev, uPrev, alphas, n_alpha, act, (const int*)list, (long)count, xTraj, uTraj, J, (int*)alpha_idx,          \
                       (long)batch, T)
        const bool stg = box->step != 0;
        if (n_alpha == 1) {
            if (stg) ZM_LAUNCH_BOX(1, true, (nslot + 63) / 64);
            else ZM_LAUNCH_BOX(1, false, (nslot + 63) / 64);
        } else {
            if (stg) ZM_LAUNCH_BOX(16, true, (nslot + 3) / 4);
            else ZM_LAUNCH_BOX(16, false, (nslot + 3) / 4);
        }
#undef ZM_LAUNCH_BOX
        ZM_HIP_CHECK(hipGetLastError());
        return ZM_OK;
    }
    if (track && n_alpha == 1) {
        const unsigned blocks = (unsigned)((nslot + 63) / 64);
        hipLaunchKernelGGL((zm::rollout_linesearch_track_kernel<1>), dim3(blocks), dim3(64), 0, st, md, cs, *track, x0, l, L, xPrev,
                           uPrev, alphas, n_alpha, act, (const int*)list, (long)count, xTraj, uTraj, J, (int*)alpha_idx, (long)batch, T);
    } else if (track) {
        const unsigned blocks = (unsigned)((nslot + 3) / 4);
        hipLaunchKernelGGL((zm::rollout_linesearch_track_kernel<16>), dim3(blocks), dim3(64), 0, st, md, cs, *track, x0, l, L, xPrev,
                           uPrev, alphas, n_alpha, act, (const int*)list, (long)count, xTraj, uTraj, J, (int*)alpha_idx, (long)batch, T);
    } else if (n_alpha == 1) {
        const unsigned blocks = (unsigned)((nslot + 63) / 64);
        hipLaunchKernelGGL((zm::rollout_linesearch_kernel<1>), dim3(blocks), dim3(64), 0, st, md, cs, hc, x0, l, L, xPrev,
                           uPrev, alphas, n_alpha, act, (const int*)list, (long)count, xTraj, uTraj, J, (int*)alpha_idx, (long)batch, T);
    } else {
        const unsigned blocks = (unsigned)((nslot + 3) / 4);
        hipLaunchKernelGGL((zm::rollout_linesearch_kernel<16>), dim3(blocks), dim3(64), 0, st, md, cs, hc, x0, l, L, xPrev,
                           uPrev, alphas, n_alpha, act, (const int*)list, (long)count, xTraj, uTraj, J, (int*)alpha_idx, (long)batch, T);
    }
    ZM_HIP_CHECK(hipGetLastError());
    return ZM_OK;
}

// The entries: each resolves its cost argument(s) (track_cost.h) and hands the line search to rollout_impl; the dense forms are the
// list forms without a list.
extern "C" int zm_rollout_linesearch_f64(const zm_model_t* model, const zm_quadcost_t* cost, const double* x0, const double* l,
                                         const double* L, const double* xPrev, const double* uPrev, const double* alphas,
                                         int n_alpha, const int32_t* active, double* xTraj, double* uTraj, double* J,
                                         int32_t* alpha_idx, int64_t batch, int T, void* stream) {
    if (batch == 0) return ZM_OK;   /* empty batch: nothing to do (pointers of empty arrays may be NULL) */
    return rollout_impl(ROLLOUT, model, cost, x0, l, L, xPrev, uPrev, alphas, n_alpha, active, nullptr, 0, xTraj, uTraj, J, alpha_idx,
                        batch, T, stream);
}

extern "C" int zm_rollout_linesearch_list_f64(const zm_model_t* model, const zm_quadcost_t* cost, const double* x0,
                                              const double* l, const double* L, const double* xPrev, const double* uPrev,
                                              const double* alphas, int n_alpha, const int32_t* list, int64_t count,
                                              const int32_t* active, double* xTraj, double* uTraj, double* J, int32_t* alpha_idx,
                                              int64_t batch, int T, void* stream) {
    if (batch == 0) return ZM_OK;   /* empty batch: nothing to do (pointers of empty arrays may be NULL) */
    if (!list) return zm::set_error(ZM_EINVAL, "zm_rollout_linesearch_list_f64: null list");
    return rollout_impl(ROLLOUT, model, cost, x0, l, L, xPrev, uPrev, alphas, n_alpha, active, list, count, xTraj, uTraj, J, alpha_idx,
                        batch, T, stream);
}

extern "C" int zm_rollout_linesearch_tracking_list_f64(const zm_model_t* model, const zm_trackcost_t* cost, const double* x0,
                                                       const double* l, const double* L, const double* xPrev, const double* uPrev,
                                                       const double* alphas, int n_alpha, const int32_t* list, int64_t count,
                                                       const int32_t* active, double* xTraj, double* uTraj, double* J,
                                                       int32_t* alpha_idx, int64_t batch, int T, void* stream) {
    zm::CostRef ck;
    if (const int rc = zm::cost_resolve(nullptr, cost, zm::CostArg::track, "zm_rollout_linesearch_tracking_f64", &ck)) return rc;
    if (batch == 0) return ZM_OK;
    return rollout_impl(ROLLOUT, model, &ck.w, x0, l, L, xPrev, uPrev, alphas, n_alpha, active, list, count, xTraj, uTraj, J, alpha_idx,
                        batch, T, stream, nullptr, &ck.ref);
}

extern "C" int zm_rollout_linesearch_tracking_f64(const zm_model_t* model, const zm_trackcost_t* cost, const double* x0, const double* l,
                                                  const double* L, const double* xPrev, const double* uPrev, const double* alphas,
                                                  int n_alpha, const int32_t* active, double* xTraj, double* uTraj, double* J,
                                                  int32_t* alpha_idx, int64_t batch, int T, void* stream) {
    return zm_rollout_linesearch_tracking_list_f64(model, cost, x0, l, L, xPrev, uPrev, alphas, n_alpha, nullptr, 0, active, xTraj, uTraj,
                                                   J, alpha_idx, batch, T, stream);
}

// Extension; the reference has no counterpart: the line search with input bounds, on a zm_quadcost_t or a zm_trackcost_t.
extern "C" int zm_rollout_linesearch_box_list_f64(const zm_model_t* model, const zm_quadcost_t* cost, const zm_trackcost_t* track,
                                                  const zm_inputbox_t* box, const double* x0, const double* l, const double* L,
                                                  const double* xPrev, const double* uPrev, const double* alphas, int n_alpha,
                                                  const int32_t* list, int64_t count, const int32_t* active, double* xTraj,
                                                  double* uTraj, double* J, int32_t* alpha_idx, int64_t batch, int T, void* stream) {
    const char* who = "zm_rollout_linesearch_box_f64";
    zm::CostRef ck;
    if (const int rc = zm::cost_resolve(cost, track, zm::CostArg::at_most_one, who, &ck)) return rc;
    if (!model) return zm::set_error(ZM_EINVAL, "%s: null pointer", who);
    if (const int rc = zm::box_check(box, zm::model_sized(*model).m, T, who)) return rc;
    if (batch == 0) return ZM_OK;
    const zm::BoxRef bx = zm::box_ref(*box);
    return rollout_impl(ROLLOUT, model, ck.weights(), x0, l, L, xPrev, uPrev, alphas, n_alpha, active, list, count, xTraj, uTraj, J,
                        alpha_idx, batch, T, stream, nullptr, ck.ref_ptr(), &bx);
}

extern "C" int zm_rollout_linesearch_box_f64(const zm_model_t* model, const zm_quadcost_t* cost, const zm_trackcost_t* track,
                                             const zm_inputbox_t* box, const double* x0, const double* l, const double* L,
                                             const double* xPrev, const double* uPrev, const double* alphas, int n_alpha,
                                             const int32_t* active, double* xTraj, double* uTraj, double* J, int32_t* alpha_idx,
                                             int64_t batch, int T, void* stream) {
    return zm_rollout_linesearch_box_list_f64(model, cost, track, box, x0, l, L, xPrev, uPrev, alphas, n_alpha, nullptr, 0, active, xTraj,
                                              uTraj, J, alpha_idx, batch, T, stream);
}

// Extension; the reference has no counterpart: the line search on the augmented-Lagrangian cost of a state box, on a zm_quadcost_t or
// a zm_trackcost_t, with or without input bounds.  One lane per rollout, two passes (the generic kernel's penalty form only).
extern "C" int zm_rollout_linesearch_state_list_f64(const zm_model_t* model, const zm_quadcost_t* cost, const zm_trackcost_t* track,
                                                    const zm_inputbox_t* box, const zm_statebox_t* sbox, const double* x0, const double* l,
                                                    const double* L, const double* xPrev, const double* uPrev, const double* alphas,
                                                    int n_alpha, const int32_t* list, int64_t count, const int32_t* active, double* xTraj,
                                                    double* uTraj, double* J, double* J_cost, int32_t* alpha_idx, int64_t batch, int T,
                                                    void* stream) {
    const char* who = "zm_rollout_linesearch_state_f64";
    zm::CostRef ck;
    if (const int rc = zm::cost_resolve(cost, track, zm::CostArg::exactly_one, who, &ck)) return rc;
    const PenArgs pen{sbox, box, J_cost};
    return rollout_impl(who, model, &ck.w, x0, l, L, xPrev, uPrev, alphas, n_alpha, active, list, count, xTraj, uTraj, J, alpha_idx, batch,
                        T, stream, nullptr, ck.ref_ptr(), nullptr, &pen);
}

extern "C" int zm_rollout_linesearch_state_f64(const zm_model_t* model, const zm_quadcost_t* cost, const zm_trackcost_t* track,
                                               const zm_inputbox_t* box, const zm_statebox_t* sbox, const double* x0, const double* l,
                                               const double* L, const double* xPrev, const double* uPrev, const double* alphas,
                                               int n_alpha, const int32_t* active, double* xTraj, double* uTraj, double* J, double* J_cost,
                                               int32_t* alpha_idx, int64_t batch, int T, void* stream) {
    return zm_rollout_linesearch_state_list_f64(model, cost, track, box, sbox, x0, l, L, xPrev, uPrev, alphas, n_alpha, nullptr, 0, active,
                                                xTraj, uTraj, J, J_cost, alpha_idx, batch, T, stream);
}

// Solver-internal (ilqr_solve.hip): the 16-way line search in all-store mode -- every step size's rollout goes to the scratch blocks
// of its slot ((T+1) * 256 doubles per slot, layout in rollout_fast.hip), alpha_idx[t] names the winner, nothing is written to
// xTraj / uTraj.
namespace zm {
// the part of the predicate below that is known when the workspace is sized (model kind, dimensions, wind, the fallback switch)
bool rollout_all_store_model_ok(const zm_model_t* model) {
    if (!model) return false;
    static const bool force_generic = [] {
        const char* e = zm::fallback_env("ZOPT_AMD_ROLLOUT_PATH");
        return e && e[0] == 'g';
    }();
    const bool windy = model->wind_ned[0] != 0.0 || model->wind_ned[1] != 0.0 || model->wind_ned[2] != 0.0;
    const bool dims = model->kind == ZM_MODEL_QUADCOPTER || (model->kind == ZM_MODEL_LINEAR && model->n == 12 && model->m == 4);
    return !force_generic && !windy && dims;
}
bool rollout_all_store_supported(const zm_model_t* model, const zm_quadcost_t* cost, int T) {
    return model && cost && T >= 1 && rollout_all_store_model_ok(model);
}
int rollout_linesearch_all_store(const zm_model_t* model, const zm_quadcost_t* cost, const double* x0, const double* l, const double* L,
                                 const double* xPrev, const double* uPrev, const double* alphas, const int32_t* list, int64_t count,
                                 const int32_t* active, double* scratch, double* J, int32_t* alpha_idx, int64_t batch, int T,
                                 void* stream, const TrackRef* track) {
    // (xTraj / uTraj are not written in this mode; the non-null placeholders only pass the argument check)
    return rollout_impl(ROLLOUT, model, cost, x0, l, L, xPrev, uPrev, alphas, 16, active, list, count, scratch, scratch, J, alpha_idx, batch,
                        T, stream, scratch, track);
}
}  // namespace zm

// ---------------------------------------------------------------------------------------------------------------------
// Acceptance step of the iLQR / DDP loop for the trajectories of a compacted id list: take the line search's result
// (trajectory, cost), test convergence and retire converged trajectories.  Replaces zopt/ilqrUtils.py:316-320
//     converged = abs(J - J_new) <= tol;  traj, J = traj_new, J_new
// One block per listed trajectory; only those rows are touched (a masked whole-array update would move the entire batch
// every iteration although most of it has converged).
namespace zm {
__global__ __launch_bounds__(256) void ilqr_accept_kernel(const int* __restrict__ list, const long count,
                                                          double* __restrict__ J, const double* __restrict__ Jn,
                                                          double* __restrict__ xT, const double* __restrict__ xT2,
                                                          double* __restrict__ uT, const double* __restrict__ uT2,
                                                          int* __restrict__ converged, int* __restrict__ active,
                                                          const double tol, const long xrow, const long urow,
                                                          const double* __restrict__ scratch, const int* __restrict__ idx,
                                                          int* __restrict__ where, const int where_val) {
    const long slot = blockIdx.x;
    if (slot >= count) return;
    const long t = list[slot];
    // The mask is read ONCE per block and shared: thread 0 clears active[t] at the end of this same block, and a wave that
    // is scheduled late must not see that store and skip its stripe of the copy (a torn trajectory).
    __shared__ int act;
    // (everything that depends on t alone leaves together with the mask's load: one memory round trip instead of three)
    const int win = scratch ? idx[t] : 0;
    double jn = 0.0, jo = 0.0;
    if (threadIdx.x == 0) {
        act = active[t];   // the list may be older than the mask (it is rebuilt only every few iterations)
        jn = Jn[t];
        jo = J[t];
    }
    __syncthreads();
    if (act == 0) return;
    // the new trajectory: row t of (xT2, uT2), or -- after an all-store line search (n = 12, m = 4) -- the winner's 16-byte pieces
    // of this slot's scratch blocks (layout: rollout_fast.hip, allstore)
    if (scratch) {
        // 16-byte pieces: (T + 1) * 6 of x, T * 2 of u
        constexpr int n = 12, m = 4, PB = (n + m) / 2;
        typedef double d2 __attribute__((ext_vector_type(2)));
        const double* sb = scratch + slot * (xrow / n) * (PB * 32) + win * 2;
        const long nxp = xrow / 2, nup = urow / 2;
        for (long e = threadIdx.x; e < nxp; e += blockDim.x) {
            const long k = e / (n / 2), p = e % (n / 2);
            *(d2*)(xT + t * xrow + 2 * e) = *(const d2*)(sb + (k * PB + p) * 32);
        }
        for (long e = threadIdx.x; e < nup; e += blockDim.x) {
            const long k = e / (m / 2), p = e % (m / 2);
            *(d2*)(uT + t * urow + 2 * e) = *(const d2*)(sb + ((k + 1) * PB + n / 2 + p) * 32);
        }
    } else if (xT2) {
        for (long e = threadIdx.x; e < xrow; e += blockDim.x) xT[t * xrow + e] = xT2[t * xrow + e];
        for (long e = threadIdx.x; e < urow; e += blockDim.x) uT[t * urow + e] = uT2[t * urow + e];
    }   // (else: the line search wrote the new rows where the caller wants them -- the solvers' alternating buffers)
    if (threadIdx.x == 0) {
        if (where) where[t] = where_val;   // which of the solver's two buffers holds this trajectory's newest rows
        const int cv = (__builtin_fabs(jo - jn) <= tol) ? 1 : 0;   // NaN compares false: never "converged"
        J[t] = jn;
        converged[t] = cv;
        active[t] = cv ? 0 : 1;
    }
}
}  // namespace zm

namespace zm {
int ilqr_accept(const int32_t* list, int64_t count, double* J, const double* Jn, double* xTraj, const double* xTrajNew, double* uTraj,
                const double* uTrajNew, int32_t* converged, int32_t* active, double tol, int64_t batch, int T, int n, int m,
                void* stream, const double* scratch, const int32_t* idx, int32_t* where, int where_val) {
    if (batch == 0 || count == 0) return ZM_OK;
    // (where != nullptr and no scratch: xTrajNew / uTrajNew may be nullptr -- nothing to copy, the new rows are in place)
    if (!list || !J || !Jn || !xTraj || !uTraj || !converged || !active || (scratch ? !idx : (!where && (!xTrajNew || !uTrajNew))))
        return set_error(ZM_EINVAL, "zm_ilqr_accept_f64: null pointer");
    if (count < 0 || count > batch || T < 1 || n < 1 || m < 1) return set_error(ZM_EINVAL, "zm_ilqr_accept_f64: bad size");
    if (scratch && (n != 12 || m != 4)) return set_error(ZM_EUNSUPPORTED, "ilqr_accept: all-store scratch is laid out for n = 12, m = 4");
    hipLaunchKernelGGL(ilqr_accept_kernel, dim3((unsigned)count), dim3(256), 0, (hipStream_t)stream, (const int*)list,
                       (long)count, J, Jn, xTraj, xTrajNew, uTraj, uTrajNew, (int*)converged, (int*)active, tol,
                       (long)(T + 1) * n, (long)T * m, scratch, (const int*)idx, (int*)where, where_val);
    ZM_HIP_CHECK(hipGetLastError());
    return ZM_OK;
}

// End of a solve on alternating buffers: the rows of every trajectory whose newest state sits in the workspace buffer (where[t] != 0)
// move to the caller's arrays.  One block per trajectory.
__global__ __launch_bounds__(256) void ilqr_collect_kernel(const int* __restrict__ where, double* __restrict__ xT,
                                                           const double* __restrict__ xAlt, double* __restrict__ uT,
                                                           const double* __restrict__ uAlt, const long xrow, const long urow) {
    const long t = blockIdx.x;
    if (where[t] == 0) return;
    for (long e = threadIdx.x; e < xrow; e += blockDim.x) xT[t * xrow + e] = xAlt[t * xrow + e];
    for (long e = threadIdx.x; e < urow; e += blockDim.x) uT[t * urow + e] = uAlt[t * urow + e];
}
int ilqr_collect(const int32_t* where, double* xTraj, const double* xAlt, double* uTraj, const double* uAlt, int64_t batch, int T, int n,
                 int m, void* stream) {
    if (batch == 0) return ZM_OK;
    hipLaunchKernelGGL(ilqr_collect_kernel, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream, (const int*)where, xTraj, xAlt,
                       uTraj, uAlt, (long)(T + 1) * n, (long)T * m);
    ZM_HIP_CHECK(hipGetLastError());
    return ZM_OK;
}
}  // namespace zm

extern "C" int zm_ilqr_accept_f64(const int32_t* list, int64_t count, double* J, const double* Jn, double* xTraj,
                                  const double* xTrajNew, double* uTraj, const double* uTrajNew, int32_t* converged,
                                  int32_t* active, double tol, int64_t batch, int T, int n, int m, void* stream) {
    return zm::ilqr_accept(list, count, J, Jn, xTraj, xTrajNew, uTraj, uTrajNew, converged, active, tol, batch, T, n, m, stream,
                           nullptr, nullptr, nullptr, 0);
}
