// Shared argument blocks of the MPC solve kernels (mpc.hip: one lane per instance; mpc_wave.hip: 16 lanes per instance).
#pragma once
#include "zm_common.h"

#include <type_traits>

// Every ZM_MPC_CHK-th ADMM iteration checks the primal-infeasibility certificate and lets the adaptive penalty move (OSQP's
// `check_termination` / `adaptive_rho_interval`, both tunables of the solver, not of the problem).  8 with moves to the NEAREST
// tabulated level: measured on BASELINE configs[2] (profiles/r03_mpc_check_interval_ab.txt) 106 -> 60 worst-case iterations.
// CHECK_EVERY of the reference ADMM solver under oracle/ replays this schedule and must stay equal to it.
constexpr int ZM_MPC_CHK = 8;

namespace zm {

struct MpcArgs {
    const double* x0;
    double rho, eps_abs, eps_rel, eps_pinf;
    int max_iter;
    int warm;   // 1: the workspace holds the iterates (y, lam) of a previous solve of the same problem family; 2: same, shifted by one step
    double *ws, *xTraj, *uTraj;
    int *status, *iters;
    double* resid;
    long batch;
    int N;
    // adaptive penalty (OSQP's adaptive_rho): tables for n_levels penalties rho * rho_step^(l - level0), level-major in K / Minv
    int n_levels, level0;
    double rho_step;
    // over-relaxation (OSQP's alpha; 1 = plain ADMM): w_hat = alpha w + (1 - alpha) y_prev enters the projection and the dual update
    double alpha;
};

struct MpcTabs {
    const double *A, *B, *K, *Minv, *x_lb, *x_ub, *u_lb, *u_ub;
};

// per-problem data (zm_mpc_solve_batched_f64): instance i solves problem prob[i] in [0, P), whose A, B, bounds and tables sit at
// p x their single-problem size in the MpcTabs arrays (tables: p x n_levels levels), with the penalty rho[p]
struct MpcProb {
    const int* prob;
    const double* rho;
};

// reference tracking (zm_mpc_solve_tracking_f64): the linear term of the cost, g (batch, N, n + m) in the stacked stage layout
// [x_{k+1} ; u_k], formed once per solve by mpc_track_linear_kernel (mpc.hip) and constant over the ADMM iterations.  Its own kernel
// argument, after MpcArgs / MpcProb: the argument blocks of the kernels without a reference keep their layout.
struct MpcTrack {
    const double* g;
};

// stage-varying dynamics (zm_mpc_solve_ltv_f64): with A (P,N,n,n) and B (P,N,n,m) in MpcTabs, the offsets c (P,N,n), their share of the costate D (P,n_levels,N,n) and ABt (P,N,n+m,n), the columns of [A_k | B_k] as contiguous rows, the last two
// written by mpc_setup_ltv_kernel (mpc.hip)
struct MpcLtv {
    const double *c, *D, *ABt;
};

// soft box constraints (zm_mpc_solve_ltv_soft_f64): the penalty weights l1, l2 (P,n+m) of every problem's stacked component [x ; u];
// l1 = +inf is a hard component, l2 may be nullptr (zeros).  Its own kernel argument, after MpcLtv: the kernels without it keep theirs.
// zm_mpc_solve_soft_f64, zm_mpc_closed_loop_soft_f64: the same rows for lqrMpc's kernels, (1,n+m) without per-problem data.
struct MpcSoft {
    const double *l1, *l2;
};

// closed-loop run (zm_mpc_closed_loop_f64): `steps` receding-horizon solves in a row, step-major arrays -- step s of an array is one
// batch-sized slab further on, so a step's solve sees the layouts of a single solve through offset pointers.
struct MpcLoop {
    int steps;
    int warm;                 // MpcArgs::warm of the steps after the first (the first is always a cold start)
    double clip_tol;          // every state is clipped into [x_lb + clip_tol, x_ub - clip_tol] before it is solved from; < 0: no clip
    const double* x0;         // (batch, n)         the initial states
    const double* dist;       // (steps, batch, n)  added to the successor state; may be nullptr
    double* states;           // (steps + 1, batch, n)
    double* inputs;           // (steps, batch, m)
    int *status, *iters;      // (steps, batch)
    double *xPred, *uPred;    // the rollout of every step, (batch, N + 1, n) / (batch, N, m) each ...
    long xpred_step, upred_step;   // ... this many doubles apart: one rollout when predictions are kept, 0 when every step reuses one scratch
};

// Entry block of the per-problem kernels: instance `inst` reads its problem index, offsets A, B, the bounds and the tables by it and takes
// the problem's penalty.  A macro, not a function: the kernels' `__restrict__` parameters do not survive being passed by reference
// (other code, more scratch).  Expands inside a kernel with the parameters of mpc_solve_batched_kernel and a local MpcArgs g.
#define ZM_MPC_ENTER_PROBLEM(inst)              \
    const long p = pb.prob[inst];               \
    A += p * NS * NS;                           \
    B += p * NS * MC;                           \
    Ktab += p * g.n_levels * g.N * MC * NS;     \
    Mtab += p * g.n_levels * g.N * MC * MC;     \
    x_lb += p * NS;                             \
    x_ub += p * NS;                             \
    u_lb += p * MC;                             \
    u_ub += p * MC;                             \
    g.rho = pb.rho[p];

// the (n, m) of a compiled kernel as a value: what for_mpc_shape() hands to its callback
template <int V>
using Int = std::integral_constant<int, V>;

// f(Int<NS>, Int<MC>) for the compiled shape (n, m); ZM_EUNSUPPORTED for any other.  (24, 8) is beyond the 16-index tile: only the
// lane-per-instance kernels have it (registers + scratch); mpc_wave.hip keeps to NS + MC <= 16.
template <typename F>
static int for_mpc_shape(int n, int m, F f) {
    if (n == 24 && m == 8) return f(Int<24>{}, Int<8>{});
    if (n == 12 && m == 4) return f(Int<12>{}, Int<4>{});
    if (n == 8 && m == 4) return f(Int<8>{}, Int<4>{});
    if (n == 4 && m == 2) return f(Int<4>{}, Int<2>{});
    if (n == 4 && m == 1) return f(Int<4>{}, Int<1>{});
    if (n == 2 && m == 2) return f(Int<2>{}, Int<2>{});
    if (n == 2 && m == 1) return f(Int<2>{}, Int<1>{});
    if (n == 1 && m == 1) return f(Int<1>{}, Int<1>{});
    return ZM_EUNSUPPORTED;
}

// The 16-lanes-per-instance kernels keep the iterates of a block's 4 instances in LDS, 64 doubles per instance and stage (mpc_wave.hip:
// WS_STAGE), and may ask for 150 KiB of it: horizons up to N = 75.  The refusals of mpc.hip (mpc_ltv_check_shape) and ltvMpc.N_MAX
// (mpcUtils.py) spell that "N <= 75" out as text: a change here changes them.
constexpr int MPC_LDS_MAX = 150 * 1024;
inline size_t mpc_iterate_bytes(int N) { return (size_t)4 * N * 64 * sizeof(double); }
inline bool mpc_iterates_fit_lds(int N) { return mpc_iterate_bytes(N) <= (size_t)MPC_LDS_MAX; }

// mpc_wave.hip: 16 lanes per instance, iterates in LDS.  ZM_EUNSUPPORTED if the shape / horizon does not fit.  pb: per-problem data,
// trk: reference tracking; either may be nullptr.
int mpc_wave_dispatch(const MpcTabs& t, const MpcArgs& g, const MpcProb* pb, const MpcTrack* trk, int n, int m, hipStream_t st);
// mpc_wave.hip: the whole closed-loop run of a regulator as ONE launch of the same kernels with the step loop inside.  `g` carries the
// options and the workspace of every step (its x0, outputs and warm are set per step from `lp`).  ZM_EUNSUPPORTED as above.
int mpc_wave_closed_loop_dispatch(const MpcTabs& t, const MpcArgs& g, const MpcProb* pb, const MpcLoop& lp, int n, int m, hipStream_t st);
// mpc_wave.hip: stage-varying dynamics, always per-problem and with a linear term (mpc_solve_wave_ltv.h).  ZM_EUNSUPPORTED as above; there
// is no other kernel to take what does not fit.  stage_box (zm_mpc_solve_ltv_stage_f64): the box varies by stage -- t.x_lb, t.x_ub are
// the box of x_0 (P,n) and t.u_lb, t.u_ub the stacked lo, hi (P,N,n+m), row k = [bound of x_{k+1} ; bound of u_k].
int mpc_wave_ltv_dispatch(const MpcTabs& t, const MpcArgs& g, const MpcProb& pb, const MpcTrack& trk, const MpcLtv& lv, bool stage_box,
                          int n, int m, hipStream_t st);
// mpc_wave.hip: the stage form of the above (stage_box) with soft box constraints, weights sf (mpc_solve_wave_ltv_soft_kernel)
int mpc_wave_ltv_soft_dispatch(const MpcTabs& t, const MpcArgs& g, const MpcProb& pb, const MpcTrack& trk, const MpcLtv& lv,
                               const MpcSoft& sf, int n, int m, hipStream_t st);
// mpc_wave.hip: lqrMpc's solve with soft box constraints, weights sf (P,n+m), one row without per-problem data
// (mpc_solve_wave_soft_kernel); pb, trk: either may be nullptr.  ZM_EUNSUPPORTED as above; there is no other kernel to take what does not fit.
int mpc_wave_soft_dispatch(const MpcTabs& t, const MpcArgs& g, const MpcProb* pb, const MpcTrack* trk, const MpcSoft& sf, int n, int m,
                           hipStream_t st);
// mpc_wave.hip: the closed-loop run of a softened regulator as ONE launch (mpc_closed_loop_wave_soft_kernel): mpc_wave_closed_loop_dispatch
// with the weights; the clip between the steps leaves the soft state components alone
int mpc_wave_closed_loop_soft_dispatch(const MpcTabs& t, const MpcArgs& g, const MpcProb* pb, const MpcLoop& lp, const MpcSoft& sf, int n,
                                       int m, hipStream_t st);

// linearize.hip (where the model expansions live): the argument check of the entry points that take a registered model, and the launch
// of mpc_rti_relinearize_kernel -- the expansion of `md` about every stage of the plans xPlan (batch,N+1,n), uPlan (batch,N,m), written
// into A (batch,N,ns,ns), B (batch,N,ns,mc), c (batch,N,ns) (n = md.n <= ns, m = md.m <= mc).
int check_model(const zm_model_t* model, zm_model_t& md, const char* who);
int mpc_relinearize_enqueue(const zm_model_t& md, const double* xPlan, const double* uPlan, double* A, double* B, double* c, long batch,
                            int N, int ns, int mc, hipStream_t st);

}  // namespace zm
