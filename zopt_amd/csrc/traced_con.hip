// zm_tracedcon_t: the kernels that run recorded inequality constraints (tape_con.h) -- the hot path of the augmented-Lagrangian iLQR
// whose constraints are user-written.  Extension; the reference has no counterpart (its iLQR is unconstrained, ilqrUtils.py:260-327).
//
//   traced_con_rollout_kernel   the line search on cost + penalty (sibling of traced_cost_rollout_kernel and of rollout_one's PEN
//                               form): one lane per (trajectory, step size), two passes, the shared argmin; per step the policy, the
//                               cost, the stage tape with psi into an accumulator of its own, the model step; S = double
//   traced_con_expand_kernel    16 lanes per point, lane j seeds variable j and owns entry j of the gradient addend and row j of the
//                               per-point Hessian = shared conditioned set + mu G^T diag(s > 0) G; S = Dual
//   traced_con_update_kernel    one wave per trajectory between two inner solves: violation, done test, lam, mu, masks; S = double
//   traced_con_values_kernel    g along given trajectories, one lane per point; S = double
//
// A wave runs ONE tape at a time (fetch and decode are on the scalar unit: tape_model.h), so the expansion and values kernels give the
// stage points and the terminal points to different workgroups.  Slot file: LDS, sized per launch by the largest slot count the
// launch runs; a wave's file fits 64 KiB for double and Dual at the interpreter's 64 slots.
#include "tape_con.h"
#include "track_cost.h"
#include "traced_con.h"
#include "zm_common.h"

namespace zm {

extern __shared__ __attribute__((aligned(16))) double zm_con_lds[];

template <typename S>
struct ConFile {
    LdsSlots<S> f;
    __device__ __forceinline__ ConFile() : f{zm_con_lds + threadIdx.x, (int)blockDim.x} {}
};

// device view of the arrays of a zm_tracedcon_t: the multipliers of stage k of trajectory t are the n_con doubles at
// lam + (t * T + k) * n_con, its terminal ones the n_con_terminal doubles at lam_terminal + t * n_con_terminal; its penalty mu[t]

// one rollout of trajectory t under step size alpha on cost + penalty; *jcost (optional) <- the cost without the penalty
template <bool STORE, bool TRACED, bool TRK, typename SLOTS>
__device__ __forceinline__ double traced_con_rollout_one(const zm_model_t& md, const zm_quadcost_t& cs, const TrackRef& tr,
                                                         const zm_tracedcon_t& con, SLOTS& f, const long t, const double alpha,
                                                         const double* __restrict__ x0, const double* __restrict__ l,
                                                         const double* __restrict__ L, const double* __restrict__ xPrev,
                                                         const double* __restrict__ uPrev, double* __restrict__ xTraj,
                                                         double* __restrict__ uTraj, const int T, double* jcost) {
    const int n = md.n, m = md.m, nc = con.n_con, nct = con.n_con_terminal;
    const double* prow = TRACED ? tape_con_params(traced_of(md), t) : nullptr;
    const double* grow = tape_con_params(con.stage, t);
    const double* trow = tape_con_params(con.terminal, t);
    const double mu = con.mu[t];
    double x[MAXN], u[MAXM], xn[MAXN], g[MAXC];
#pragma unroll
    for (int i = 0; i < MAXN; ++i) x[i] = (i < n) ? x0[i] : 0.0;
    if (STORE) {
#pragma unroll
        for (int i = 0; i < MAXN; ++i)
            if (i < n) xTraj[i] = x[i];
    }
    double J = 0.0, P = 0.0;
    for (int k = 0; k < T; ++k) {
        const double* Lk = L + (long)k * m * n;
        const double* xp = xPrev + (long)k * n;
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
            } else {
                u[i] = 0.0;
            }
        }
        if constexpr (TRK) {
            double ex[MAXN], eu[MAXM];
            track_diff(ex, x, track_xrow(tr, t, k), n);
            track_diff(eu, u, track_urow(tr, t, k), m);
            J += running_cost(cs, n, m, ex, eu);
        } else {
            J += running_cost(cs, n, m, x, u);
        }
        if (nc > 0) {   // (uniform over the wave)
            tape_con<double, true, SLOTS>(con.stage, n, m, nc, f, x, u, grow, g);
            const double* lam = con.lam + (t * T + k) * nc;
#pragma unroll
            for (int i = 0; i < MAXC; ++i)
                if (i < nc) P += con_psi(g[i], lam[i], mu);
        }
        if constexpr (TRACED) tape_step<double, SLOTS>(md, f, x, u, prow, xn);
        else model_step<double>(md, x, u, xn);
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
        double ex[MAXN];
        track_diff(ex, x, track_xrow(tr, t, T), n);
        J += terminal_cost(cs, n, ex);
    } else {
        J += terminal_cost(cs, n, x);
    }
    if (nct > 0) {
        tape_con<double, false, SLOTS>(con.terminal, n, m, nct, f, x, u, trow, g);
        const double* lam = con.lam_terminal + t * nct;
#pragma unroll
        for (int i = 0; i < MAXC; ++i)
            if (i < nct) P += con_psi(g[i], lam[i], mu);
    }
    if (jcost) *jcost = J;
    return J + P;
}

// NA = lanes per trajectory (1 or 16); the frame is traced_cost_rollout_kernel's
template <int NA, bool TRACED, bool TRK>
__global__ __launch_bounds__(64) void traced_con_rollout_kernel(const zm_model_t md, const zm_quadcost_t cost, const TrackRef tr,
                                                                const zm_tracedcon_t con, const double* __restrict__ x0,
                                                                const double* __restrict__ l, const double* __restrict__ L,
                                                                const double* __restrict__ xPrev, const double* __restrict__ uPrev,
                                                                const double* __restrict__ alphas, const int n_alpha,
                                                                const int* __restrict__ active, const int* __restrict__ list,
                                                                const long count, double* __restrict__ xTraj,
                                                                double* __restrict__ uTraj, double* __restrict__ Jout,
                                                                double* __restrict__ Jc_out, int* __restrict__ idx_out,
                                                                const long batch, const int T) {
    constexpr int TPW = 64 / NA;  // trajectories per wave
    const int lane = threadIdx.x;
    const int a = lane % NA;
    const long slot = (long)blockIdx.x * TPW + lane / NA;   // slot -> trajectory id (through `list` when given)
    const long nslot = list ? count : batch;
    const long traj = (slot < nslot) ? (list ? (long)list[slot] : slot) : 0;
    const bool live = (slot < nslot) && (a < n_alpha) && (active == nullptr || active[traj] != 0);
    const long t = live ? traj : 0;
    const int n = md.n, m = md.m;
    const double alpha = alphas[a < n_alpha ? a : 0];
    const double* x0t = x0 + t * n;
    const double* lt = l + t * T * m;
    const double* Lt = L + t * T * m * n;
    const double* xpt = xPrev + t * (T + 1) * n;
    const double* upt = uPrev + t * T * m;
    double* xo = xTraj + t * (T + 1) * n;
    double* uo = uTraj + t * T * m;
    ConFile<double> cf;

    double J = 0.0;
    int best = 0;
    if (NA > 1) {
        if (live)
            J = traced_con_rollout_one<false, TRACED, TRK>(md, cost, tr, con, cf.f, t, alpha, x0t, lt, Lt, xpt, upt, nullptr, nullptr, T,
                                                           nullptr);
        // dead lanes carry (+inf, index NA)
        const int who = argmin_nan_first<NA>(live ? J : __builtin_inf(), live ? a : NA);
        best = who < NA ? who : 0;
    }
    // lane 0 of the group re-rolls the winning step size (the same arithmetic) and stores
    const double abest = alphas[best];
    if (live) {
        if (a == 0) {
            const double Jb = traced_con_rollout_one<true, TRACED, TRK>(md, cost, tr, con, cf.f, t, abest, x0t, lt, Lt, xpt, upt, xo, uo, T,
                                                                        Jc_out ? Jc_out + t : nullptr);
            if (Jout) Jout[t] = Jb;
            if (idx_out) idx_out[t] = best;
        }
    }
}

// Expansion of the penalty: 16 lanes per point (n + m <= 16 variables), 4 points per wave.  Lane j evaluates the tape on dual numbers
// seeded e_j: it then holds g and column j of G.  Every lane of a group stays in the kernel to the end (a dead group computes on
// point 0 and stores nothing), so that the cross-lane reads below always find their source lane running.  Blocks past
// `blocks_stage` take the terminal points: the targets are v_x and v_xx.
__global__ __launch_bounds__(64) void traced_con_expand_kernel(const zm_tracedcon_t con, const double* __restrict__ xTraj,
                                                               const double* __restrict__ uTraj, const int* __restrict__ active,
                                                               const double* __restrict__ sc_xx, const double* __restrict__ sc_ux,
                                                               const double* __restrict__ sc_uu, const double* __restrict__ sv_xx,
                                                               double* __restrict__ c_x, double* __restrict__ c_u,
                                                               double* __restrict__ v_x, double* __restrict__ c_xx,
                                                               double* __restrict__ c_ux, double* __restrict__ c_uu,
                                                               double* __restrict__ v_xx, int* __restrict__ visits, const long batch,
                                                               const int T, const int* __restrict__ list, const long count,
                                                               const unsigned blocks_stage) {
    const int lane = threadIdx.x;
    const int j = lane & 15;
    const bool terminal = blockIdx.x >= blocks_stage;   // uniform over the workgroup
    const long nslot = list ? count : batch;
    const int n = con.n, m = con.m;
    const long gi = (long)(terminal ? blockIdx.x - blocks_stage : blockIdx.x) * 4 + (lane >> 4);   // slot * T + k, or slot
    const bool inside = gi < (terminal ? nslot : nslot * T);
    const long slot = inside ? (terminal ? gi : gi / T) : 0;
    const int k = terminal ? T : (inside ? (int)(gi - slot * T) : 0);
    const long traj = inside ? (list ? (long)list[slot] : slot) : 0;
    const bool live = inside && (active == nullptr || active[traj] != 0);
    const long tt = live ? traj : 0;
    const int kk = live ? k : (terminal ? T : 0);
    const long pt = tt * T + kk;   // (stage points only)
    const int nc = terminal ? con.n_con_terminal : con.n_con;
    const zm_traced_t& tp = terminal ? con.terminal : con.stage;
    const double* xk = xTraj + (tt * (T + 1) + kk) * n;
    Dual x[MAXN], u[MAXM], g[MAXC];
#pragma unroll
    for (int i = 0; i < MAXN; ++i) x[i] = Dual{(i < n) ? xk[i] : 0.0, (i == j) ? 1.0 : 0.0};
#pragma unroll
    for (int i = 0; i < MAXM; ++i) u[i] = Dual{(!terminal && i < m) ? uTraj[pt * m + i] : 0.0, (n + i == j) ? 1.0 : 0.0};
    ConFile<Dual> cf;
#pragma unroll
    for (int i = 0; i < MAXC; ++i) g[i] = Dual{0.0, 0.0};
    // (one call for both tapes: the terminal tape's control slots receive zeros that it never reads; an absent tape is not run)
    if (nc > 0) tape_con<Dual, true>(tp, n, m, nc, cf.f, x, u, tape_con_params(tp, tt), g);
    const double mu = con.mu[tt];
    const double* lam = terminal ? con.lam_terminal + tt * nc : con.lam + pt * nc;
    double w[MAXC];   // a_i G_ij: this lane's column, the rows that are not active zeroed
    double grad = 0.0;
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
        const double s = (i < nc) ? con_slack(g[i].v, lam[i], mu) : 0.0;
        w[i] = (s > 0.0) ? g[i].d : 0.0;
        grad = (s > 0.0) ? __builtin_fma(s, g[i].d, grad) : grad;
    }
    // row j of mu G^T diag(s > 0) G: entry j' needs column j' of G, held by lane j' of this 16-lane group
    double row[16];
#pragma unroll
    for (int jp = 0; jp < 16; ++jp) {
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < MAXC; ++i) acc = __builtin_fma(w[i], __shfl(w[i], jp, 16), acc);
        row[jp] = mu * acc;
    }
    if (!live) return;
    if (terminal) {
        if (j < n) {
            v_x[tt * n + j] += grad;
#pragma unroll
            for (int jp = 0; jp < MAXN; ++jp)
                if (jp < n) v_xx[(tt * n + j) * n + jp] = sv_xx[j * n + jp] + row[jp];
        }
        return;
    }
    if (visits && kk == 0 && j == 0) visits[tt] += 1;   // one visit per iteration of the loop over this trajectory
    if (j < n) {
        c_x[pt * n + j] += grad;
#pragma unroll
        for (int jp = 0; jp < MAXN; ++jp)
            if (jp < n) c_xx[(pt * n + j) * n + jp] = sc_xx[j * n + jp] + row[jp];
    } else if (j < n + m) {
        const int ju = j - n;
        c_u[pt * m + ju] += grad;
#pragma unroll
        for (int jp = 0; jp < 16; ++jp) {
            if (jp < n) c_ux[(pt * m + ju) * n + jp] = sc_ux[ju * n + jp] + row[jp];
            else if (jp < n + m) c_uu[(pt * m + ju) * m + (jp - n)] = sc_uu[ju * m + (jp - n)] + row[jp];
        }
    }
}

// one wave per trajectory; the lanes stride the stage rows, then every lane runs the terminal tape on x_T
template <bool UPDATE>
__device__ __forceinline__ void traced_con_rows(const zm_tracedcon_t& con, LdsSlots<double>& f, const double* __restrict__ xTraj,
                                                const double* __restrict__ uTraj, const long t, const int T, const double mu,
                                                double& v, int& isnan_) {
    const int lane = threadIdx.x;
    const int n = con.n, m = con.m, nc = con.n_con, nct = con.n_con_terminal;
    double x[MAXN], u[MAXM], g[MAXC];
    if (nc > 0) {
        const double* grow = tape_con_params(con.stage, t);
        for (int k0 = 0; k0 < T; k0 += 64) {   // (a uniform trip count: the tape runs with every lane of the wave)
            const bool has = k0 + lane < T;
            const int k = has ? k0 + lane : T - 1;
#pragma unroll
            for (int i = 0; i < MAXN; ++i) x[i] = (i < n) ? xTraj[(t * (T + 1) + k) * n + i] : 0.0;
#pragma unroll
            for (int i = 0; i < MAXM; ++i) u[i] = (i < m) ? uTraj[(t * T + k) * m + i] : 0.0;
            tape_con<double, true>(con.stage, n, m, nc, f, x, u, grow, g);
            if (has) {
                double* lam = con.lam + (t * T + k) * nc;
#pragma unroll
                for (int i = 0; i < MAXC; ++i) {
                    if (i < nc) {
                        if (UPDATE) {
                            lam[i] = con_pos(con_slack(g[i], lam[i], mu));
                        } else {
                            isnan_ |= (g[i] != g[i]) ? 1 : 0;
                            v = g[i] > v ? g[i] : v;
                        }
                    }
                }
            }
        }
    }
    if (nct > 0) {
#pragma unroll
        for (int i = 0; i < MAXN; ++i) x[i] = (i < n) ? xTraj[(t * (T + 1) + T) * n + i] : 0.0;
#pragma unroll
        for (int i = 0; i < MAXM; ++i) u[i] = 0.0;
        tape_con<double, false>(con.terminal, n, m, nct, f, x, u, tape_con_params(con.terminal, t), g);
        double* lam = con.lam_terminal + t * nct;
#pragma unroll
        for (int i = 0; i < MAXC; ++i) {
            if (i < nct) {
                if (UPDATE) {
                    if (lane == 0) lam[i] = con_pos(con_slack(g[i], lam[i], mu));
                } else {
                    isnan_ |= (g[i] != g[i]) ? 1 : 0;
                    v = g[i] > v ? g[i] : v;
                }
            }
        }
    }
}

__global__ __launch_bounds__(64) void traced_con_update_kernel(const zm_tracedcon_t con, const double* __restrict__ xTraj,
                                                               const double* __restrict__ uTraj, int* __restrict__ active,
                                                               int* __restrict__ converged, double* __restrict__ violation,
                                                               int* __restrict__ outer_count, int* __restrict__ remaining,
                                                               const double ctol, const double growth, const double mu_max,
                                                               const int update, const int T) {
    const long t = blockIdx.x;
    const int lane = threadIdx.x;
    if (active[t] == 0) return;   // done earlier: nothing of it is touched (the whole wave leaves: the mask is written below by lane 0
                                  // only after every lane has read it -- one wave, in order)
    ConFile<double> cf;
    const double m0 = con.mu[t];
    double v = 0.0;
    int isnan_ = 0;
    traced_con_rows<false>(con, cf.f, xTraj, uTraj, t, T, m0, v, isnan_);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double o = __shfl_xor(v, off, 64);
        isnan_ |= __shfl_xor(isnan_, off, 64);
        v = o > v ? o : v;
    }
    const double viol = isnan_ ? __builtin_nan("") : v;
    const bool done = converged[t] != 0 && viol <= ctol;   // a NaN is never <= ctol
    __builtin_amdgcn_wave_barrier();
    if (!done && update) traced_con_rows<true>(con, cf.f, xTraj, uTraj, t, T, m0, v, isnan_);
    if (lane == 0) {
        violation[t] = viol;
        if (outer_count) outer_count[t] += 1;
        converged[t] = done ? 1 : 0;
        active[t] = done ? 0 : 1;
        if (!done) {
            if (update) {
                const double gm = m0 * growth;
                con.mu[t] = gm < mu_max ? gm : mu_max;
            }
            if (remaining) atomicAdd(remaining, 1);
        }
    }
}

// g along the trajectories: one lane per point; blocks past `blocks_stage` take the terminal points
__global__ __launch_bounds__(64) void traced_con_values_kernel(const zm_tracedcon_t con, const double* __restrict__ xTraj,
                                                               const double* __restrict__ uTraj, double* __restrict__ gout,
                                                               double* __restrict__ gtout, const long batch, const int T,
                                                               const unsigned blocks_stage) {
    const bool terminal = blockIdx.x >= blocks_stage;   // uniform over the workgroup
    const long gi = (long)(terminal ? blockIdx.x - blocks_stage : blockIdx.x) * 64 + threadIdx.x;
    const bool has = gi < (terminal ? batch : batch * T);
    const long p = has ? gi : 0;
    const long t = terminal ? p : p / T;
    const int k = terminal ? T : (int)(p - t * T);
    const int n = con.n, m = con.m;
    const int nc = terminal ? con.n_con_terminal : con.n_con;
    const zm_traced_t& tp = terminal ? con.terminal : con.stage;
    double x[MAXN], u[MAXM], g[MAXC];
#pragma unroll
    for (int i = 0; i < MAXN; ++i) x[i] = (i < n) ? xTraj[(t * (T + 1) + k) * n + i] : 0.0;
#pragma unroll
    for (int i = 0; i < MAXM; ++i) u[i] = (!terminal && i < m) ? uTraj[p * m + i] : 0.0;
    ConFile<double> cf;
    tape_con<double, true>(tp, n, m, nc, cf.f, x, u, tape_con_params(tp, t), g);
    if (!has) return;
    double* o = terminal ? gtout + p * nc : gout + p * nc;
#pragma unroll
    for (int i = 0; i < MAXC; ++i)
        if (i < nc) o[i] = g[i];
}

// ---- host side ----------------------------------------------------------------------------------------------------------------

static int con_tape_check(const zm_traced_t& t, int n, int m, int nc, const char* which, const char* who) {
    if (nc == 0) return ZM_OK;   // absent
    if (t.n_params < 0 || t.n_params > ZM_TRACED_MAX_PARAMS || t.n_instr < 0 || t.n_instr > ZM_TRACED_MAX_INSTR || t.n_const < 0 ||
        t.n_const > ZM_TRACED_MAX_CONSTS || t.n_slots < n + m + t.n_params || t.n_slots > ZM_TRACED_MAX_SLOTS)
        return set_error(ZM_EUNSUPPORTED, "%s: %s tape outside the interpreter's caps (instructions %d <= %d, slots %d <= %d, constants "
                         "%d <= %d, parameters %d <= %d)", who, which, t.n_instr, ZM_TRACED_MAX_INSTR, t.n_slots, ZM_TRACED_MAX_SLOTS,
                         t.n_const, ZM_TRACED_MAX_CONSTS, t.n_params, ZM_TRACED_MAX_PARAMS);
    if (!t.tape || ((uintptr_t)t.tape & 7)) return set_error(ZM_EINVAL, "%s: the %s constraint needs an 8-byte aligned tape", who, which);
    if (t.n_params > 0 && (!t.params || t.param_stride < 0))
        return set_error(ZM_EINVAL, "%s: %s constraint with %d parameters needs params and a non-negative stride", who, which, t.n_params);
    return ZM_OK;
}

int tracedcon_check(const zm_tracedcon_t* con, int n, int m, bool arrays, const char* who) {
    if (!con) return set_error(ZM_EINVAL, "%s: null constraint descriptor", who);
    if (con->n < 1 || con->n > MAXN || con->m < 1 || con->m > MAXM)
        return set_error(ZM_EUNSUPPORTED, "%s: traced constraint with (n=%d, m=%d): need 1 <= n <= 12, 1 <= m <= 4", who, con->n, con->m);
    if (con->n_con < 0 || con->n_con > MAXC || con->n_con_terminal < 0 || con->n_con_terminal > MAXC)
        return set_error(ZM_EUNSUPPORTED, "%s: n_con = %d, n_con_terminal = %d: each between 0 and %d", who, con->n_con,
                         con->n_con_terminal, MAXC);
    if (con->n_con == 0 && con->n_con_terminal == 0) return set_error(ZM_EINVAL, "%s: a constraint with no rows at all", who);
    if (n >= 0 && (con->n != n || con->m != m))
        return set_error(ZM_EINVAL, "%s: the constraint is (n=%d, m=%d), the model (n=%d, m=%d)", who, con->n, con->m, n, m);
    if (const int rc = con_tape_check(con->stage, con->n, con->m, con->n_con, "stage", who)) return rc;
    if (const int rc = con_tape_check(con->terminal, con->n, con->m, con->n_con_terminal, "terminal", who)) return rc;
    if (arrays && (!con->mu || (con->n_con > 0 && !con->lam) || (con->n_con_terminal > 0 && !con->lam_terminal)))
        return set_error(ZM_EINVAL, "%s: the constraint needs lam, lam_terminal and mu", who);
    return ZM_OK;
}

static int con_slots(const zm_tracedcon_t& c) {
    const int a = c.n_con > 0 ? c.stage.n_slots : 0, b = c.n_con_terminal > 0 ? c.terminal.n_slots : 0;
    return a > b ? a : b;
}

static int con_sizes(const char* who, int64_t batch, int T, int n) {
    if (batch < 0 || T < 1) return set_error(ZM_EINVAL, "%s: bad size batch=%lld T=%d", who, (long long)batch, T);
    if ((int64_t)T * n * n >= (int64_t)1 << 31 || batch >= ((int64_t)1 << 31))
        return set_error(ZM_EUNSUPPORTED, "%s: T*n*n or batch too large", who);
    return ZM_OK;
}

int traced_con_expand(const zm_tracedcon_t* con, const double* xTraj, const double* uTraj, const int32_t* list, int64_t count,
                      const int32_t* active, const double* sc_xx, const double* sc_ux, const double* sc_uu, const double* sv_xx,
                      double* c_x, double* c_u, double* v_x, double* c_xx, double* c_ux, double* c_uu, double* v_xx, int32_t* visits,
                      int64_t batch, int T, hipStream_t st) {
    const long nslot = list ? (long)count : (long)batch;
    // (an absent tape still gets its blocks: its points' Hessians are the shared set, and stage 0 counts the visit)
    const unsigned bs = (unsigned)((nslot * T + 3) / 4), bt = (unsigned)((nslot + 3) / 4);
    hipLaunchKernelGGL(traced_con_expand_kernel, dim3(bs + bt), dim3(64), (size_t)LdsSlots<Dual>::bytes(con_slots(*con), 64), st, *con,
                       xTraj, uTraj, (const int*)active, sc_xx, sc_ux, sc_uu, sv_xx, c_x, c_u, v_x, c_xx, c_ux, c_uu, v_xx, (int*)visits,
                       (long)batch, T, (const int*)list, (long)count, bs);
    ZM_HIP_CHECK(hipGetLastError());
    return ZM_OK;
}

}  // namespace zm

extern "C" int zm_traced_con_values_f64(const zm_tracedcon_t* con, const double* xTraj, const double* uTraj, double* g, double* g_terminal,
                                        int64_t batch, int T, void* stream) {
    const char* who = "zm_traced_con_values_f64";
    if (const int rc = zm::tracedcon_check(con, -1, -1, false, who)) return rc;
    if (!xTraj || !uTraj) return zm::set_error(ZM_EINVAL, "%s: null pointer", who);
    if (const int rc = zm::con_sizes(who, batch, T, con->n)) return rc;
    if (batch == 0) return ZM_OK;
    const unsigned bs = (g && con->n_con > 0) ? (unsigned)((batch * T + 63) / 64) : 0u;
    const unsigned bt = (g_terminal && con->n_con_terminal > 0) ? (unsigned)((batch + 63) / 64) : 0u;
    if (bs + bt == 0) return ZM_OK;
    hipLaunchKernelGGL(zm::traced_con_values_kernel, dim3(bs + bt), dim3(64), (size_t)zm::LdsSlots<double>::bytes(zm::con_slots(*con), 64),
                       (hipStream_t)stream, *con, xTraj, uTraj, g, g_terminal, (long)batch, T, bs);
    ZM_HIP_CHECK(hipGetLastError());
    return ZM_OK;
}

extern "C" int zm_traced_con_linesearch_list_f64(const zm_model_t* model, const zm_quadcost_t* cost, const zm_trackcost_t* track,
                                                 const zm_tracedcon_t* con, const double* x0, const double* l, const double* L,
                                                 const double* xPrev, const double* uPrev, const double* alphas, int n_alpha,
                                                 const int32_t* list, int64_t count, const int32_t* active, double* xTraj,
                                                 double* uTraj, double* J, double* J_cost, int32_t* alpha_idx, int64_t batch, int T,
                                                 void* stream) {
    const char* who = "zm_traced_con_linesearch_list_f64";
    if (!model || !x0 || !l || !L || !xPrev || !uPrev || !alphas || !xTraj || !uTraj || !J) return zm::set_error(ZM_EINVAL, "%s: null pointer", who);
    if (batch < 0 || T < 1 || (n_alpha != 1 && n_alpha != 16))
        return zm::set_error(ZM_EINVAL, "%s: bad size batch=%lld T=%d n_alpha=%d (1 or 16)", who, (long long)batch, T, n_alpha);
    zm::CostRef cr;
    if (const int rc = zm::cost_resolve(cost, track, zm::CostArg::exactly_one, who, &cr)) return rc;
    if (cost && (!cost->Q || !cost->R || !cost->Qf)) return zm::set_error(ZM_EINVAL, "%s: cost needs Q, R, Qf", who);
    zm_model_t md;
    if (const int rc = zm::model_check(model, who, &md)) return rc;
    if (md.n < 1 || md.n > zm::MAXN || md.m < 1 || md.m > zm::MAXM)
        return zm::set_error(ZM_EUNSUPPORTED, "%s: (n=%d, m=%d) not covered (traced constraint: n<=12, m<=4)", who, md.n, md.m);
    const bool traced = md.kind == ZM_MODEL_TRACED;
    if (traced && track)
        return zm::set_error(ZM_EUNSUPPORTED, "%s: a traced model takes a zm_quadcost_t (the tracking cost on the tape interpreter is not "
                                              "built)", who);
    if (const int rc = zm::tracedcon_check(con, md.n, md.m, true, who)) return rc;
    if (list && (count < 0 || count > batch)) return zm::set_error(ZM_EINVAL, "%s: bad list length", who);
    if (const int rc = zm::con_sizes(who, batch, T, md.n)) return rc;
    if (batch == 0 || (list && count == 0)) return ZM_OK;
    const long nslot = list ? count : batch;
    const int cslots = zm::con_slots(*con), mslots = traced ? zm::traced_of(md).n_slots : 0;
    const size_t lds = (size_t)zm::LdsSlots<double>::bytes(cslots > mslots ? cslots : mslots, 64);
    hipStream_t st = (hipStream_t)stream;
#define ZM_LAUNCH_CON(NA_, TR_, TRK_, BLOCKS_)                                                                                         \
    hipLaunchKernelGGL((zm::traced_con_rollout_kernel<NA_, TR_, TRK_>), dim3((unsigned)(BLOCKS_)), dim3(64), lds, st, md, cr.w, cr.ref,   \
                       *con, x0, l, L, xPrev, uPrev, alphas, n_alpha, (const int*)active, (const int*)list, (long)count, xTraj, uTraj, \
                       J, J_cost, (int*)alpha_idx, (long)batch, T)
#define ZM_LAUNCH_CON_NA(TR_, TRK_)                                       \
    do {                                                                  \
        if (n_alpha == 1) ZM_LAUNCH_CON(1, TR_, TRK_, (nslot + 63) / 64); \
        else ZM_LAUNCH_CON(16, TR_, TRK_, (nslot + 3) / 4);               \
    } while (0)
    if (traced) ZM_LAUNCH_CON_NA(true, false);
    else if (track) ZM_LAUNCH_CON_NA(false, true);
    else ZM_LAUNCH_CON_NA(false, false);
#undef ZM_LAUNCH_CON_NA
#undef ZM_LAUNCH_CON
    ZM_HIP_CHECK(hipGetLastError());
    return ZM_OK;
}

extern "C" int zm_traced_con_expand_list_f64(const zm_tracedcon_t* con, const double* xTraj, const double* uTraj, const int32_t* list,
                                             int64_t count, const int32_t* active, const double* sc_xx, const double* sc_ux,
                                             const double* sc_uu, const double* sv_xx, double* c_x, double* c_u, double* v_x,
                                             double* c_xx, double* c_ux, double* c_uu, double* v_xx, int64_t batch, int T, void* stream) {
    const char* who = "zm_traced_con_expand_list_f64";
    if (const int rc = zm::tracedcon_check(con, -1, -1, true, who)) return rc;
    if (!xTraj || !uTraj || !sc_xx || !sc_ux || !sc_uu || !sv_xx || !c_x || !c_u || !v_x || !c_xx || !c_ux || !c_uu || !v_xx)
        return zm::set_error(ZM_EINVAL, "%s: null pointer", who);
    if (const int rc = zm::con_sizes(who, batch, T, con->n)) return rc;
    if (list && (count < 0 || count > batch)) return zm::set_error(ZM_EINVAL, "%s: bad list length", who);
    if (batch == 0 || (list && count == 0)) return ZM_OK;
    return zm::traced_con_expand(con, xTraj, uTraj, list, count, active, sc_xx, sc_ux, sc_uu, sv_xx, c_x, c_u, v_x, c_xx, c_ux, c_uu, v_xx,
                                 nullptr, batch, T, (hipStream_t)stream);
}

extern "C" int zm_traced_con_multiplier_update_f64(const zm_tracedcon_t* con, const double* xTraj, const double* uTraj, int32_t* active,
                                                   int32_t* converged, double* violation, int32_t* outer_count, int32_t* remaining,
                                                   double ctol, double growth, double mu_max, int update, int64_t batch, int T,
                                                   void* stream) {
    const char* who = "zm_traced_con_multiplier_update_f64";
    if (const int rc = zm::tracedcon_check(con, -1, -1, true, who)) return rc;
    if (!xTraj || !uTraj || !active || !converged || !violation) return zm::set_error(ZM_EINVAL, "%s: null pointer", who);
    if (const int rc = zm::con_sizes(who, batch, T, con->n)) return rc;
    if (!(growth >= 1.0) || !(mu_max > 0.0) || !(ctol >= 0.0)) return zm::set_error(ZM_EINVAL, "%s: need growth >= 1, mu_max > 0, ctol >= 0", who);
    if (batch == 0) return ZM_OK;
    hipLaunchKernelGGL(zm::traced_con_update_kernel, dim3((unsigned)batch), dim3(64),
                       (size_t)zm::LdsSlots<double>::bytes(zm::con_slots(*con), 64), (hipStream_t)stream, *con, xTraj, uTraj, (int*)active,
                       (int*)converged, violation, (int*)outer_count, (int*)remaining, ctol, growth, mu_max, update ? 1 : 0, T);
    ZM_HIP_CHECK(hipGetLastError());
    return ZM_OK;
}
