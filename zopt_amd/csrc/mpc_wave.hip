// K9-W  mpc_solve_wave -- the ADMM of mpc.hip with 16 LANES PER INSTANCE (4 instances per wave64), iterates in LDS.
//
// Same algorithm, same termination and certificate as mpc_solve_kernel (mpc.hip; problem: zopt/mpcUtils.py:48-59): only
// the mapping differs.  One lane per instance leaves an MI355X nearly idle at the batch sizes MPC is used with (1024
// instances = 16 waves) and makes every ADMM iteration a chain of 60 x ~500 dependent FMAs in one lane.  Here the 16 lanes of a
// group carry the STACKED index [x ; u]: lane i < n holds state component i, lane n + j control component j, each with its row / column
// of A, B, K_k, Suu_k^-1; a mat-vec is NL broadcasts (DPP row_newbcast, no LDS) + NL FMAs per lane, and it serves both blocks at once:
//     backward stage:  p = p' - rho z_x;  [A^T p ; Qu = -rho z_u + B^T p] in one pass over p;  [K^T Qu ; kf] in one pass over Qu
//     forward  stage:  [A x ; K x] in one pass over x;  + B u;  clip / dual update once, on the stacked iterate
// ~75 vector instructions per stage pair.  The iterates y, lam, kf (and the certificate's r) live in LDS, one private
// slot per lane and stage: no cross-lane LDS traffic, hence no barrier anywhere in the loop; HBM is touched only for the
// tables K_k, Suu_k^-1 (L2-resident, fetched three stages ahead) and at entry / exit (warm start, results).
#include "mpc_common.h"

#include <hip/hip_runtime.h>

namespace zm {

// acc += c * (value of lane L of this lane's 16-lane row of v): ONE instruction.  gfx90a+ accept a DPP source operand on
// 64-bit ALU instructions for exactly one control, row_newbcast -- the one a mat-vec needs -- so the broadcast costs no
// instruction of its own (two v_mov_b32_dpp + the FMA before: a third of the kernel's vector instructions were broadcasts).
// hipcc pads nothing inside asm: the two wait states a DPP read needs after a VALU write of its source come from dpp_src(),
// which every mat-vec passes its vector through once (the broadcasts then depend on that statement, hence follow it).
template <int L>
__device__ __forceinline__ void fma_bc(double& acc, const double c, const double v) {
    asm("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(v), "v"(c), "i"(L));
}
__device__ __forceinline__ double dpp_src(double v) {
    asm("s_nop 1" : "+v"(v));
    return v;
}
// acc += sum_l c[l] v_(OFF + l): the vector's components sit in lanes OFF .. OFF + NL - 1 of the row.  The sums run as PS interleaved
// partial chains (term l goes to chain l % PS; chain 0 starts from acc): a single chain of 12 dependent FMAs would be the longest
// dependency of a stage.
template <int NL, int PS, int OFF, int L = 0>
__device__ __forceinline__ void mv_acc(const double (&c)[NL], const double v, double (&s)[PS]) {
    if constexpr (L < NL) {
        fma_bc<OFF + L>(s[L % PS], c[L], v);
        mv_acc<NL, PS, OFF, L + 1>(c, v, s);
    }
}
template <int NL, int OFF = 0>
__device__ __forceinline__ void mv(const double (&c)[NL], const double v, double& a) {
    constexpr int PS = NL >= 9 ? 3 : (NL >= 4 ? 2 : 1);
    double s[PS];
    s[0] = a;
#pragma unroll
    for (int i = 1; i < PS; ++i) s[i] = 0.0;
    mv_acc<NL, PS, OFF>(c, dpp_src(v), s);
    if constexpr (PS == 3)
        a = (s[0] + s[1]) + s[2];
    else if constexpr (PS == 2)
        a = s[0] + s[1];
    else
        a = s[0];
}
// the same as ONE chain (the short products onto an accumulator that is itself the end of a chain)
template <int NL, int OFF, int L = 0>
__device__ __forceinline__ void mv_seq_acc(const double (&c)[NL], const double v, double& a) {
    if constexpr (L < NL) {
        fma_bc<OFF + L>(a, c[L], v);
        mv_seq_acc<NL, OFF, L + 1>(c, v, a);
    }
}
template <int NL, int OFF>
__device__ __forceinline__ void mv_seq(const double (&c)[NL], const double v, double& a) {
    mv_seq_acc<NL, OFF>(c, dpp_src(v), a);
}
// acc = max(acc, |v|) in ONE instruction.  __builtin_fmax(acc, __builtin_fabs(v)) compiles to three (both operands are first passed
// through a canonicalising v_max with themselves, which only matters for signalling NaNs); five norms per forward stage made that a sixth
// of the stage.  Same result for every input the solve can produce (a quiet NaN is ignored by both forms).
__device__ __forceinline__ void amax(double& acc, const double v) {
    asm("v_max_f64 %0, %0, |%1|" : "+v"(acc) : "v"(v));
}
// (DPP butterflies: the __shfl_xor ladders they replace were eight ds_bpermute round trips per reduction, five reductions per iteration)
__device__ __forceinline__ double row_max(double v) { return row16_max(v); }
__device__ __forceinline__ double row_sum(double v) { return row16_sum_from8(v); }

// LDS per group and stage (doubles): y[16] lam[16] r[16] kf[16], one slot per lane
constexpr int WS_STAGE = 64;

// The hooks of the body (mpc_solve_wave_body.h) for the reference-tracking variant: nothing in the kernels without a reference, so
// those compile from the tokens they always had.
#define ZM_TRK_TAB
#define ZM_TRK_SETUP
#define ZM_TRK_G(t)
#define ZM_TRK_LOAD(k, t)
#define ZM_TRK_ED(ed, dual)
#define ZM_TRK_LEVEL(nl)
// The hooks of the soft-box variant (below, after the tracking kernels): nothing, or the tokens the body had before it had them.
#define ZM_SOFT_SETUP
#define ZM_SOFT_X0
#define ZM_SOFT_RHO
#define ZM_SOFT_GUARD
#define ZM_SOFT_PROJECT(yn) yn = yn < lo ? lo : (yn > hi ? hi : yn);
#define ZM_SOFT_SUP_LO lo
#define ZM_SOFT_SUP_HI hi

// Lane roles (round 3): the STACKED index [x ; u] on the 16 lanes of a group -- lane i < NS owns state component i, lane NS + j owns
// control component j (NS + MC <= 16 for every compiled shape).  A mat-vec over the state lanes then serves both blocks of its result in
// ONE FMA per broadcast, each lane with its own coefficients ([A^T p ; B^T p], [A x ; K x]), and the projection / dual update runs once
// for the stacked iterate -- rounds 1-2 kept the control components in lanes 0 .. MC-1 next to the states, which cost two FMAs per
// broadcast and a second, four-lane copy of the update (~120 vector instructions per stage pair instead of ~75).  Same sums in the same
// order: the iterates are bit for bit those of the older mapping.
template <int NS, int MC>
__global__ __launch_bounds__(64) void mpc_solve_wave_kernel(const double* __restrict__ A, const double* __restrict__ B,
                                                            const double* __restrict__ Ktab, const double* __restrict__ Mtab,
                                                            const double* __restrict__ x_lb, const double* __restrict__ x_ub,
                                                            const double* __restrict__ u_lb, const double* __restrict__ u_ub,
                                                            const MpcArgs g) {
#include "mpc_solve_wave_body.h"
}

// Per-problem data (zm_mpc_solve_batched_f64): the group reads its problem index once at entry -- uniform over the 16-lane group, not
// over the wave (a wave holds 4 instances, possibly of 4 problems) -- and offsets A, B, the bounds and the tables by it, and takes the
// problem's penalty as g.rho; the body is that of mpc_solve_wave_kernel.  The table offset thereby enters the per-lane bases that
// set_level_bases() forms: the stage loops are the shared-problem kernel's, and the levels' penalties are rho_p * rho_step^(l - level0).
// Idle groups of the last block shadow the last instance, as in the body.
template <int NS, int MC>
__global__ __launch_bounds__(64) void mpc_solve_wave_batched_kernel(const double* __restrict__ A, const double* __restrict__ B,
                                                                    const double* __restrict__ Ktab, const double* __restrict__ Mtab,
                                                                    const double* __restrict__ x_lb, const double* __restrict__ x_ub,
                                                                    const double* __restrict__ u_lb, const double* __restrict__ u_ub,
                                                                    const MpcArgs g_all, const MpcProb pb) {
    MpcArgs g = g_all;
    {
        const long inst_raw = (long)blockIdx.x * 4 + (threadIdx.x >> 4);
        ZM_MPC_ENTER_PROBLEM(inst_raw < g.batch ? inst_raw : g.batch - 1)
    }
#include "mpc_solve_wave_body.h"
}
// Closed-loop run (zm_mpc_closed_loop_f64): the receding-horizon loop of demos/lqrMpc.py:40-47 INSIDE the kernel, around the same body --
// per step s: the state (already clipped into the box) is solved from, the group's state lanes form x_{s+1} = clip(xTraj_s[1] + w_s) and
// store it, the control lanes store u_s = uTraj_s[0]; the body sees a local MpcArgs whose x0, outputs and warm point at step s.  One
// launch for the whole run: no launch, allocation or host round trip per step, and a wave whose four instances finish a step early goes on
// to the next one at once instead of waiting for the slowest instance of the batch (the step loop is wave-uniform: the gain is per wave,
// not per instance).
// Across a step boundary the body reads what the previous step wrote to global memory: the warm-start blocks and the state (each lane
// its own words) and the `ok` flag / level (lane 0 of the group writes, all 16 lanes read; an idle group reads the last instance's, which
// another group of the same wave writes).  Every reader sits in the same single-wave workgroup, so a workgroup-scope release / acquire
// fence between the steps orders them (a wait for the outstanding stores, no cache maintenance); none of these words is reached through a
// `const __restrict__` parameter.  Idle groups of the last block shadow the last instance and store nothing here either; they keep
// looping with their wave.  PB: per-problem data, the entry block of mpc_solve_wave_batched_kernel.
// (mpc_closed_loop_wave_soft_kernel, below, is a COPY of this frame with a per-lane clip: a fix here belongs there too.)
template <int NS, int MC, bool PB>
__global__ __launch_bounds__(64) void mpc_closed_loop_wave_kernel(const double* __restrict__ A, const double* __restrict__ B,
                                                                  const double* __restrict__ Ktab, const double* __restrict__ Mtab,
                                                                  const double* __restrict__ x_lb, const double* __restrict__ x_ub,
                                                                  const double* __restrict__ u_lb, const double* __restrict__ u_ub,
                                                                  const MpcArgs g_all, const MpcProb pb, const MpcLoop lp) {
    MpcArgs g_run = g_all;
    const long o_batch = g_all.batch;
    const int o_li = threadIdx.x & 15;
    const long o_raw = (long)blockIdx.x * 4 + (threadIdx.x >> 4);
    const bool o_live = o_raw < o_batch;
    const long o_inst = o_live ? o_raw : o_batch - 1;
    if constexpr (PB) {
        MpcArgs& g = g_run;
        ZM_MPC_ENTER_PROBLEM(o_inst)
    }
    const bool o_sx = o_li < NS, o_su = (o_li >= NS) && (o_li < NS + MC);
    const int o_ix = o_sx ? o_li : 0, o_iu = o_su ? o_li - NS : 0;
    const bool o_clip = lp.clip_tol >= 0.0;
    const double c_lo = x_lb[o_ix] + lp.clip_tol, c_hi = x_ub[o_ix] - lp.clip_tol;
    const auto into_box = [&](double v) {   // min(max(v, lo), hi): np.clip's order, a NaN passes through
        if (o_clip) {
            v = v < c_lo ? c_lo : v;
            v = v > c_hi ? c_hi : v;
        }
        return v;
    };
    const long slab_x = o_batch * NS, slab_u = o_batch * MC;
    if (o_live && o_sx) lp.states[o_inst * NS + o_ix] = into_box(lp.x0[o_inst * NS + o_ix]);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#pragma unroll 1
    for (int s = 0; s < lp.steps; ++s) {
        MpcArgs g = g_run;
        g.x0 = lp.states + s * slab_x;
        g.xTraj = lp.xPred + s * lp.xpred_step;
        g.uTraj = lp.uPred + s * lp.upred_step;
        g.status = lp.status + s * o_batch;
        g.iters = lp.iters + s * o_batch;
        g.resid = nullptr;
        g.warm = s ? lp.warm : 0;
        {
#include "mpc_solve_wave_body.h"
        }
        if (o_live) {
            if (o_sx) {
                double xn = g.xTraj[(o_inst * (g.N + 1) + 1) * NS + o_ix];
                if (lp.dist) xn += lp.dist[s * slab_x + o_inst * NS + o_ix];
                lp.states[(s + 1) * slab_x + o_inst * NS + o_ix] = into_box(xn);
            }
            if (o_su) lp.inputs[s * slab_u + o_inst * MC + o_iu] = g.uTraj[(o_inst * g.N) * MC + o_iu];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
}

// Reference tracking (zm_mpc_solve_tracking_f64): the same body with a second linear term, -rho (y - lam) + g_k, at the top of each
// backward stage.  g (mpc.hip: mpc_track_linear_kernel) is constant over the iterations and read-only, so it is NOT a fifth LDS slot:
// the lane's component of stage k is fetched from L2 three stages ahead, together with the table slices of that stage (one more
// coalesced 128-byte line per group and stage, in flight behind the same ~500 cycles), and only in the backward sweep.  The LDS stage
// stays WS_STAGE doubles: the horizon cap and the occupancy are those of the kernels without a reference.  The scale of the dual
// tolerance becomes max(rho |lam|_inf, |g|_inf) (OSQP's ||q|| term); |g|_inf is taken once at entry.  PB: per-problem data, the entry
// block of mpc_solve_wave_batched_kernel.
#undef ZM_TRK_TAB
#undef ZM_TRK_SETUP
#undef ZM_TRK_G
#undef ZM_TRK_LOAD
#undef ZM_TRK_ED
#undef ZM_TRK_LEVEL
#define ZM_TRK_TAB double g;
#define ZM_TRK_SETUP                                                                          \
    const double* gw = trk.g + inst * ((long)N * W) + iw; /* + k * W */                       \
    double gnorm = 0.0;                                                                       \
    for (int k = 0; k < N; ++k) {                                                             \
        const double gk = gw[(long)k * W];                                                    \
        if (sw) amax(gnorm, gk);                                                              \
    }                                                                                         \
    gnorm = row_max(gnorm);                                                                   \
    int trk_last = 0, trk_rev = 0; /* the last level move; consecutive reversals of it */     \
    bool trk_locked = false;                                                                  \
    auto load_g = [&](int k, Tab& t) {                                                        \
        k = k < 0 ? 0 : (k >= N ? N - 1 : k);                                                 \
        t.g = gw[(long)k * W];                                                                \
    };
// (added to the costate and to Qu, not to z: the sums without a reference keep their roundings, so a zero reference gives their bits)
#define ZM_TRK_G(t) +t.g
#define ZM_TRK_LOAD(k, t) load_g(k, t);
#define ZM_TRK_ED(ed, dual) \
    if (gnorm > dual) ed = g.eps_abs + g.eps_rel * gnorm;
// Cycle guard of the adaptive penalty.  The level rule reads the residual ratio one check (ZM_MPC_CHK iterations) after a move, while
// the move's transient still dominates it; from a cold start far from a reference outside the box two adjacent levels can each ask
// for the other at every check, for ever (seen: levels 5 <-> 6, ratio ~5.5 / ~0.34, "user_limit" where a fixed penalty needs 95
// iterations).  A move that undoes the move of the check before is a reversal; the third reversal in a row is refused and the
// penalty stays where it is for the rest of the solve (ADMM converges at any fixed penalty).  Anything short of that pattern -- in
// particular every solve whose level sequence does not ping-pong four times running -- takes the moves of the kernels without a
// reference, which have no such guard (their code is pinned).  With a zero reference (g = 0) the guard is off: that solve IS the
// regulator's, move for move, as zm_mpc_solve_tracking_f64 promises.
constexpr int ZM_TRK_REVERSALS = 3;
#define ZM_TRK_LEVEL(nl)                                                                  \
    if (gnorm > 0.0 ZM_SOFT_GUARD) {                                                      \
        const int mv = nl - lvl;                                                          \
        if (trk_locked) {                                                                 \
            nl = lvl;                                                                     \
        } else if (mv != 0 && trk_last != 0 && ((mv > 0) != (trk_last > 0))) {            \
            if (++trk_rev >= ZM_TRK_REVERSALS) {                                          \
                trk_locked = true;                                                        \
                nl = lvl;                                                                 \
            }                                                                             \
        } else {                                                                          \
            trk_rev = 0;                                                                  \
        }                                                                                 \
        trk_last = nl - lvl;                                                              \
    }
template <int NS, int MC, bool PB>
__global__ __launch_bounds__(64) void mpc_solve_wave_track_kernel(const double* __restrict__ A, const double* __restrict__ B,
                                                                  const double* __restrict__ Ktab, const double* __restrict__ Mtab,
                                                                  const double* __restrict__ x_lb, const double* __restrict__ x_ub,
                                                                  const double* __restrict__ u_lb, const double* __restrict__ u_ub,
                                                                  const MpcArgs g_all, const MpcProb pb, const MpcTrack trk) {
    MpcArgs g = g_all;
    if constexpr (PB) {
        const long inst_raw = (long)blockIdx.x * 4 + (threadIdx.x >> 4);
        ZM_MPC_ENTER_PROBLEM(inst_raw < g.batch ? inst_raw : g.batch - 1)
    }
#include "mpc_solve_wave_body.h"
}

// Soft box constraints (zm_mpc_solve_soft_f64, zm_mpc_closed_loop_soft_f64): the same body with the penalty weights of the lane's
// component, sf.l1, sf.l2 (P,n+m) in the stacked layout [x ; u] (one row without per-problem data; l2 may be NULL: zeros).  A component
// with a finite l1 pays l1 d + l2 d^2 for its distance d from its box instead of being held inside it; l1 = +inf is a hard component, and
// a lane outside every role carries l1 = +inf, l2 = 0.  What differs from the tracking kernel, each through a ZM_SOFT_* hook:
//     x0 test:     a soft state component of x0 is not tested against the box
//     projection:  the proximal map of the penalty with t = l1 / rho, a = rho / (rho + 2 l2) at the penalty the iteration runs at (set at
//                  entry, after a warm start has restored a level, and after every level move).  The branches are tested in the order of
//                  the clip (lo first) and written with selects, as ZM_LTV_PROJECT is: l1 = +inf gives t = +inf, e = -inf and y = the
//                  bound bit for bit, a bound of -0.0 included
//     certificate: the support term takes -inf / +inf for a soft component, whose y ranges over the whole line
//     cycle guard: on when the reference term is nonzero or any component of the instance's problem is soft (uniform over the 16-lane
//                  group, not over the wave)
// ONE kernel for shared and per-problem data (pb.prob NULL or not: a group-uniform pointer offset at entry) and for solves with and without
// a reference (trk.g NULL or not).  Without a reference the lane's g is -0.0, the one value with x + g == x for every x, zeros of either
// sign included: the sums keep the bits of the kernels without a reference.  With every l1 = +inf the solve is the pinned kernels' own.
#undef ZM_TRK_SETUP
#undef ZM_SOFT_SETUP
#undef ZM_SOFT_X0
#undef ZM_SOFT_RHO
#undef ZM_SOFT_GUARD
#undef ZM_SOFT_PROJECT
#undef ZM_SOFT_SUP_LO
#undef ZM_SOFT_SUP_HI
#define ZM_TRK_SETUP                                                                                      \
    const double* gw = trk.g ? trk.g + inst * ((long)N * W) + iw : nullptr; /* + k * W */                 \
    double gnorm = 0.0;                                                                                   \
    if (gw) {                                                                                             \
        for (int k = 0; k < N; ++k) {                                                                     \
            const double gk = gw[(long)k * W];                                                            \
            if (sw) amax(gnorm, gk);                                                                      \
        }                                                                                                 \
    }                                                                                                     \
    gnorm = row_max(gnorm);                                                                               \
    int trk_last = 0, trk_rev = 0; /* the last level move; consecutive reversals of it */                 \
    bool trk_locked = false;                                                                              \
    auto load_g = [&](int k, Tab& t) {                                                                    \
        k = k < 0 ? 0 : (k >= N ? N - 1 : k);                                                             \
        t.g = gw ? gw[(long)k * W] : -0.0;                                                                \
    };
#define ZM_SOFT_SETUP                                                                                     \
    const double l1 = sw ? soft_l1[iw] : inf, l2 = (sw && soft_l2) ? soft_l2[iw] : 0.0;                   \
    const bool soft = l1 < inf;                                                                           \
    const bool any_soft = row_max(soft ? 1.0 : 0.0) > 0.0; /* uniform over the group: its problem's */    \
    double prox_t = inf, prox_a = 1.0;                     /* t = l1 / rho, a = rho / (rho + 2 l2) */
#define ZM_SOFT_X0 &&!soft
#define ZM_SOFT_RHO      \
    prox_t = l1 / rho;   \
    prox_a = rho / (rho + 2.0 * l2);
#define ZM_SOFT_GUARD || any_soft
#define ZM_SOFT_PROJECT(yn)                                \
    if (yn < lo) {                                         \
        const double e = prox_a * ((lo - yn) - prox_t);    \
        yn = (e > 0.0) ? lo - e : lo;                      \
    } else if (yn > hi) {                                  \
        const double e = prox_a * ((yn - hi) - prox_t);    \
        yn = (e > 0.0) ? hi + e : hi;                      \
    }
#define ZM_SOFT_SUP_LO (soft ? -inf : lo)
#define ZM_SOFT_SUP_HI (soft ? inf : hi)
// the group's problem: the entry block of the per-problem kernels, and its row of the weights
#define ZM_SOFT_ENTER_PROBLEM(inst)                    \
    const double *soft_l1 = sf.l1, *soft_l2 = sf.l2;   \
    if (pb.prob) {                                     \
        ZM_MPC_ENTER_PROBLEM(inst)                     \
        soft_l1 += p * (NS + MC);                      \
        if (soft_l2) soft_l2 += p * (NS + MC);         \
    }
template <int NS, int MC>
__global__ __launch_bounds__(64) void mpc_solve_wave_soft_kernel(const double* __restrict__ A, const double* __restrict__ B,
                                                                 const double* __restrict__ Ktab, const double* __restrict__ Mtab,
                                                                 const double* __restrict__ x_lb, const double* __restrict__ x_ub,
                                                                 const double* __restrict__ u_lb, const double* __restrict__ u_ub,
                                                                 const MpcArgs g_all, const MpcProb pb, const MpcTrack trk, const MpcSoft sf) {
    MpcArgs g = g_all;
    const long inst_raw_ = (long)blockIdx.x * 4 + (threadIdx.x >> 4);
    ZM_SOFT_ENTER_PROBLEM(inst_raw_ < g.batch ? inst_raw_ : g.batch - 1)
#include "mpc_solve_wave_body.h"
}

// The closed-loop run of a softened regulator (zm_mpc_closed_loop_soft_f64): the frame of mpc_closed_loop_wave_kernel -- see there for the
// step loop, the fences between the steps and the idle groups -- around the body with the soft hooks, without a reference (trk.g NULL: the
// cycle guard rests on the soft components alone).  One thing differs in the frame: the clip into [x_lb + clip_tol, x_ub - clip_tol]
// applies to the HARD state components only.  A soft component of the state is never moved, so states[s + 1] is the plant's own state
// xTraj_s[1] + w_s there, and the solve from it pays for its distance from the box.
template <int NS, int MC>
__global__ __launch_bounds__(64) void mpc_closed_loop_wave_soft_kernel(const double* __restrict__ A, const double* __restrict__ B,
                                                                       const double* __restrict__ Ktab, const double* __restrict__ Mtab,
                                                                       const double* __restrict__ x_lb, const double* __restrict__ x_ub,
                                                                       const double* __restrict__ u_lb, const double* __restrict__ u_ub,
                                                                       const MpcArgs g_all, const MpcProb pb, const MpcLoop lp,
                                                                       const MpcSoft sf) {
    MpcArgs g_run = g_all;
    const MpcTrack trk{nullptr};
    const long o_batch = g_all.batch;
    const int o_li = threadIdx.x & 15;
    const long o_raw = (long)blockIdx.x * 4 + (threadIdx.x >> 4);
    const bool o_live = o_raw < o_batch;
    const long o_inst = o_live ? o_raw : o_batch - 1;
    MpcArgs& g = g_run;
    ZM_SOFT_ENTER_PROBLEM(o_inst)
    const bool o_sx = o_li < NS, o_su = (o_li >= NS) && (o_li < NS + MC);
    const int o_ix = o_sx ? o_li : 0, o_iu = o_su ? o_li - NS : 0;
    const bool o_clip = lp.clip_tol >= 0.0 && !(o_sx && soft_l1[o_ix] < __builtin_inf());   // (per lane: a soft component is not clipped)
    const double c_lo = x_lb[o_ix] + lp.clip_tol, c_hi = x_ub[o_ix] - lp.clip_tol;
    const auto into_box = [&](double v) {   // min(max(v, lo), hi): np.clip's order, a NaN passes through
        if (o_clip) {
            v = v < c_lo ? c_lo : v;
            v = v > c_hi ? c_hi : v;
        }
        return v;
    };
    const long slab_x = o_batch * NS, slab_u = o_batch * MC;
    if (o_live && o_sx) lp.states[o_inst * NS + o_ix] = into_box(lp.x0[o_inst * NS + o_ix]);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#pragma unroll 1
    for (int s = 0; s < lp.steps; ++s) {
        MpcArgs g = g_run;
        g.x0 = lp.states + s * slab_x;
        g.xTraj = lp.xPred + s * lp.xpred_step;
        g.uTraj = lp.uPred + s * lp.upred_step;
        g.status = lp.status + s * o_batch;
        g.iters = lp.iters + s * o_batch;
        g.resid = nullptr;
        g.warm = s ? lp.warm : 0;
        {
#include "mpc_solve_wave_body.h"
        }
        if (o_live) {
            if (o_sx) {
                double xn = g.xTraj[(o_inst * (g.N + 1) + 1) * NS + o_ix];
                if (lp.dist) xn += lp.dist[s * slab_x + o_inst * NS + o_ix];
                lp.states[(s + 1) * slab_x + o_inst * NS + o_ix] = into_box(xn);
            }
            if (o_su) lp.inputs[s * slab_u + o_inst * MC + o_iu] = g.uTraj[(o_inst * g.N) * MC + o_iu];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
}
// (the ltv kernels below take none of these hooks)
#undef ZM_SOFT_ENTER_PROBLEM

// stage-varying dynamics (zm_mpc_solve_ltv_f64): mpc_solve_wave_ltv_kernel, in this translation unit with the kernels it borrows from.
// The hooks of mpc_solve_wave_ltv.h for one box per problem: the lane's bounds are read once and stay in lo / hi.
#define ZM_LTV_KERNEL mpc_solve_wave_ltv_kernel
#define ZM_LTV_BOX \
    const double lo = sx ? x_lb[p * NS + ix] : (su ? u_lb[p * MC + iu] : -inf), hi = sx ? x_ub[p * NS + ix] : (su ? u_ub[p * MC + iu] : inf);
#define ZM_LTV_X0_LO lo
#define ZM_LTV_X0_HI hi
#define ZM_LTV_TABF
#define ZM_LTV_LOAD_BOX(k, t)
#define ZM_LTV_LO(t) lo
#define ZM_LTV_HI(t) hi
// (the hooks of the soft-constrained variant below: nothing, or the tokens the file had before it had them)
#define ZM_LTV_ARGS
#define ZM_LTV_RHO
#define ZM_LTV_GUARD
#define ZM_LTV_PROJECT(yn, t) yn = yn < ZM_LTV_LO(t) ? ZM_LTV_LO(t) : (yn > ZM_LTV_HI(t) ? ZM_LTV_HI(t) : yn);
#define ZM_LTV_SUP_LO(t) ZM_LTV_LO(t)
#define ZM_LTV_SUP_HI(t) ZM_LTV_HI(t)
#include "mpc_solve_wave_ltv.h"

// stage-varying weights and bounds (zm_mpc_solve_ltv_stage_f64): mpc_solve_wave_ltv_stage_kernel, the same file with the stage's box in
// the forward prefetch set.  x_lb, x_ub: the box of x_0 (P,n); u_lb, u_ub: lo, hi (P,N,n+m), row k = [bound of x_{k+1} ; bound of u_k].
// The load is outside the lane-role branches of load_f and a select, so every lane writes both members (see the header's note).
#undef ZM_LTV_KERNEL
#undef ZM_LTV_BOX
#undef ZM_LTV_X0_LO
#undef ZM_LTV_X0_HI
#undef ZM_LTV_TABF
#undef ZM_LTV_LOAD_BOX
#undef ZM_LTV_LO
#undef ZM_LTV_HI
#define ZM_LTV_KERNEL mpc_solve_wave_ltv_stage_kernel
#define ZM_LTV_BOX                                                                                            \
    const double lo0 = sx ? x_lb[p * NS + ix] : -inf, hi0 = sx ? x_ub[p * NS + ix] : inf;                     \
    const double *lo_base = u_lb + (p * N * W + iw), *hi_base = u_ub + (p * N * W + iw); /* + k * W */
#define ZM_LTV_X0_LO lo0
#define ZM_LTV_X0_HI hi0
#define ZM_LTV_TABF double lo, hi;
#define ZM_LTV_LOAD_BOX(k, t)                   \
    t.lo = sw ? lo_base[(long)k * W] : -inf;    \
    t.hi = sw ? hi_base[(long)k * W] : inf;
#define ZM_LTV_LO(t) t.lo
#define ZM_LTV_HI(t) t.hi
#include "mpc_solve_wave_ltv.h"

// soft box constraints (zm_mpc_solve_ltv_soft_f64): mpc_solve_wave_ltv_soft_kernel, the stage form once more with the penalty weights of
// the lane's component, sf.l1, sf.l2 (P,n+m) in the stacked layout [x ; u] (l2 may be NULL: zeros).  Lanes outside every role carry
// l1 = +inf, l2 = 0, as the padded components of an embedded shape do in the caller's arrays.  The branches of the proximal map are
// tested in the order of the stage kernel's clip (lo first) and written with selects: l1 = +inf gives t = +inf, e = -inf and y = the
// bound bit for bit, where bound + max(0, e) would turn a bound of -0.0 into +0.0.
#undef ZM_LTV_KERNEL
#undef ZM_LTV_BOX
#undef ZM_LTV_ARGS
#undef ZM_LTV_RHO
#undef ZM_LTV_GUARD
#undef ZM_LTV_PROJECT
#undef ZM_LTV_SUP_LO
#undef ZM_LTV_SUP_HI
#define ZM_LTV_KERNEL mpc_solve_wave_ltv_soft_kernel
#define ZM_LTV_ARGS , const MpcSoft sf
#define ZM_LTV_BOX                                                                                            \
    const double l1 = sw ? sf.l1[p * W + iw] : inf, l2 = (sw && sf.l2) ? sf.l2[p * W + iw] : 0.0;            \
    const bool soft = l1 < inf;                                                                               \
    const bool any_soft = row_max(soft ? 1.0 : 0.0) > 0.0; /* uniform over the group: its problem's */        \
    double prox_t = inf, prox_a = 1.0;                             /* t = l1 / rho, a = rho / (rho + 2 l2) */         \
    const double lo0 = (sx && !soft) ? x_lb[p * NS + ix] : -inf, hi0 = (sx && !soft) ? x_ub[p * NS + ix] : inf; \
    const double *lo_base = u_lb + (p * N * W + iw), *hi_base = u_ub + (p * N * W + iw); /* + k * W */
#define ZM_LTV_RHO       \
    prox_t = l1 / rho;       \
    prox_a = rho / (rho + 2.0 * l2);
#define ZM_LTV_GUARD || any_soft
#define ZM_LTV_PROJECT(yn, t)                              \
    if (yn < t.lo) {                                       \
        const double e = prox_a * ((t.lo - yn) - prox_t);          \
        yn = (e > 0.0) ? t.lo - e : t.lo;                  \
    } else if (yn > t.hi) {                                \
        const double e = prox_a * ((yn - t.hi) - prox_t);          \
        yn = (e > 0.0) ? t.hi + e : t.hi;                  \
    }
#define ZM_LTV_SUP_LO(t) (soft ? -inf : t.lo)
#define ZM_LTV_SUP_HI(t) (soft ? inf : t.hi)
#include "mpc_solve_wave_ltv.h"

// for_mpc_shape() without (24, 8): f(Int<NS>, Int<MC>) for the compiled shape (n, m) with NS + MC <= 16, ZM_EUNSUPPORTED for any other,
// and no kernel of this file is instantiated beyond the 16 lanes
template <typename F>
static int for_wave_shape(int n, int m, F f) {
    return for_mpc_shape(n, m, [&](auto ns, auto mc) -> int {
        if constexpr (ns.value + mc.value <= 16)
            return f(ns, mc);
        else
            return ZM_EUNSUPPORTED;
    });
}

// One launch of a kernel of this file: 4 instances per one-wave block, their iterates in dynamic LDS; `more`: the kernel's arguments after
// MpcArgs.  ZM_EUNSUPPORTED if the horizon is too long for LDS: the lane-per-instance kernels take it, where there are any.
template <typename Kernel, typename... More>
static int launch_wave(Kernel kernel, const MpcTabs& t, const MpcArgs& g, hipStream_t st, const More&... more) {
    if (!mpc_iterates_fit_lds(g.N)) return ZM_EUNSUPPORTED;
    // per launch (cheap): the attribute is per device, and several devices may be driven from one process
    ZM_HIP_CHECK(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, MPC_LDS_MAX));
    hipLaunchKernelGGL(kernel, dim3((unsigned)((g.batch + 3) / 4)), dim3(64), mpc_iterate_bytes(g.N), st, t.A, t.B, t.K, t.Minv, t.x_lb,
                       t.x_ub, t.u_lb, t.u_ub, g, more...);
    ZM_HIP_CHECK(hipGetLastError());
    return ZM_OK;
}

// pb != nullptr: per-problem data; trk != nullptr: the tracking variants
int mpc_wave_dispatch(const MpcTabs& t, const MpcArgs& g, const MpcProb* pb, const MpcTrack* trk, int n, int m, hipStream_t st) {
    return for_wave_shape(n, m, [&](auto ns, auto mc) {
        constexpr int NS = ns.value, MC = mc.value;
        if (trk && pb) return launch_wave(mpc_solve_wave_track_kernel<NS, MC, true>, t, g, st, *pb, *trk);
        if (trk) return launch_wave(mpc_solve_wave_track_kernel<NS, MC, false>, t, g, st, MpcProb{}, *trk);
        if (pb) return launch_wave(mpc_solve_wave_batched_kernel<NS, MC>, t, g, st, *pb);
        return launch_wave(mpc_solve_wave_kernel<NS, MC>, t, g, st);
    });
}

int mpc_wave_ltv_dispatch(const MpcTabs& t, const MpcArgs& g, const MpcProb& pb, const MpcTrack& trk, const MpcLtv& lv, bool stage_box,
                          int n, int m, hipStream_t st) {
    return for_wave_shape(n, m, [&](auto ns, auto mc) {
        return stage_box ? launch_wave(mpc_solve_wave_ltv_stage_kernel<ns.value, mc.value>, t, g, st, pb, trk, lv)
                         : launch_wave(mpc_solve_wave_ltv_kernel<ns.value, mc.value>, t, g, st, pb, trk, lv);
    });
}

int mpc_wave_ltv_soft_dispatch(const MpcTabs& t, const MpcArgs& g, const MpcProb& pb, const MpcTrack& trk, const MpcLtv& lv,
                               const MpcSoft& sf, int n, int m, hipStream_t st) {
    return for_wave_shape(n, m, [&](auto ns, auto mc) {
        return launch_wave(mpc_solve_wave_ltv_soft_kernel<ns.value, mc.value>, t, g, st, pb, trk, lv, sf);
    });
}

// pb, trk: either may be nullptr (shared data; no reference) -- the one kernel takes both as possibly-NULL arrays
int mpc_wave_soft_dispatch(const MpcTabs& t, const MpcArgs& g, const MpcProb* pb, const MpcTrack* trk, const MpcSoft& sf, int n, int m,
                           hipStream_t st) {
    return for_wave_shape(n, m, [&](auto ns, auto mc) {
        return launch_wave(mpc_solve_wave_soft_kernel<ns.value, mc.value>, t, g, st, pb ? *pb : MpcProb{}, trk ? *trk : MpcTrack{}, sf);
    });
}

int mpc_wave_closed_loop_soft_dispatch(const MpcTabs& t, const MpcArgs& g, const MpcProb* pb, const MpcLoop& lp, const MpcSoft& sf, int n,
                                       int m, hipStream_t st) {
    return for_wave_shape(n, m, [&](auto ns, auto mc) {
        return launch_wave(mpc_closed_loop_wave_soft_kernel<ns.value, mc.value>, t, g, st, pb ? *pb : MpcProb{}, lp, sf);
    });
}

int mpc_wave_closed_loop_dispatch(const MpcTabs& t, const MpcArgs& g, const MpcProb* pb, const MpcLoop& lp, int n, int m, hipStream_t st) {
    return for_wave_shape(n, m, [&](auto ns, auto mc) {
        return pb ? launch_wave(mpc_closed_loop_wave_kernel<ns.value, mc.value, true>, t, g, st, *pb, lp)
                  : launch_wave(mpc_closed_loop_wave_kernel<ns.value, mc.value, false>, t, g, st, MpcProb{}, lp);
    });
}

}  // namespace zm
