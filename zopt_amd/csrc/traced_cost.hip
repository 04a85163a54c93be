// zm_tracedcost_t: the kernels that run a recorded cost function (tape_cost.h) -- the hot path of a solve whose cost is user-written.
//
//   traced_cost_rollout_kernel   zopt/ilqrUtils.py:33-66, :116-150 -- the line search: one lane per (trajectory, step size), two passes,
//                                the shared argmin (zm_common.h: argmin_nan_first); per step the policy, the cost tape, the model step
//                                (model_step of a registered model or tape_step of a traced one), then the terminal tape; S = double
//   traced_cost_gradient_kernel  zopt/pytrees.py:100-115, :72-81 -- 16 lanes per point, lane j seeds variable j; S = Dual
//   traced_cost_hessian_kernel   the same expansions' second derivatives -- the unordered pairs of the tape's structural mask over the
//                                lanes of a point; S = Hyper
//
// A wave runs ONE tape at a time (fetch and decode are on the scalar unit: tape_model.h), so the expansion kernels give the running
// points (k < T) and the terminal points (k = T) to different workgroups: the first `blocks_running` blocks run the running tape.
//
// Slot file: LDS, sized per launch by the largest slot count the launch runs (both cost tapes, and the model's tape in the line search
// of a traced model), wherever a wave's file fits 64 KiB: always for double and Dual, for Hyper up to 32 slots; a Hyper file beyond that
// is private scratch.
#include "tape_cost.h"
#include "traced_cost.h"
#include "zm_common.h"

namespace zm {

extern __shared__ __attribute__((aligned(16))) double zm_cost_lds[];

template <typename S, bool LDS>
struct CostFile;
template <typename S>
struct CostFile<S, true> {
    LdsSlots<S> f;
    __device__ __forceinline__ CostFile() : f{zm_cost_lds + threadIdx.x, (int)blockDim.x} {}
};
template <typename S>
struct CostFile<S, false> {
    ArraySlots<S> f;
};

// one rollout of trajectory t under step size alpha with the recorded cost (traced.hip: traced_rollout_one; rollout.hip: rollout_one)
template <bool STORE, bool TRACED, typename SLOTS>
__device__ __forceinline__ double traced_cost_rollout_one(const zm_model_t& md, const zm_tracedcost_t& tc, SLOTS& f,
                                                          const double* __restrict__ prow, const double* __restrict__ crow,
                                                          const double* __restrict__ vrow, const double alpha,
                                                          const double* __restrict__ x0, const double* __restrict__ l,
                                                          const double* __restrict__ L, const double* __restrict__ xPrev,
                                                          const double* __restrict__ uPrev, double* __restrict__ xTraj,
                                                          double* __restrict__ uTraj, const int T) {
    const int n = md.n, m = md.m;
    double x[MAXN], u[MAXM], xn[MAXN];
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
        J += tape_cost<double, true, SLOTS>(tc.running, n, m, f, x, u, crow);
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
    J += tape_cost<double, false, SLOTS>(tc.terminal, n, m, f, x, u, vrow);
    return J;
}

// NA = lanes per trajectory (1 or 16); the frame is traced_rollout_kernel's
template <int NA, bool TRACED, bool LDS>
__global__ __launch_bounds__(64) void traced_cost_rollout_kernel(const zm_model_t md, const zm_tracedcost_t tc,
                                                                 const double* __restrict__ x0, const double* __restrict__ l,
                                                                 const double* __restrict__ L, const double* __restrict__ xPrev,
                                                                 const double* __restrict__ uPrev, const double* __restrict__ alphas,
                                                                 const int n_alpha, const int* __restrict__ active,
                                                                 const int* __restrict__ list, const long count,
                                                                 double* __restrict__ xTraj, double* __restrict__ uTraj,
                                                                 double* __restrict__ Jout, int* __restrict__ idx_out, const long batch,
                                                                 const int T) {
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
    const double* prow = TRACED ? tape_cost_params(traced_of(md), t) : nullptr;
    const double* crow = tape_cost_params(tc.running, t);
    const double* vrow = tape_cost_params(tc.terminal, t);
    CostFile<double, LDS> cf;

    double J = 0.0;
    int best = 0;
    if (NA > 1) {
        if (live)
            J = traced_cost_rollout_one<false, TRACED>(md, tc, cf.f, prow, crow, vrow, alpha, x0t, lt, Lt, xpt, upt, nullptr, nullptr, T);
        // dead lanes carry (+inf, index NA)
        const int who = argmin_nan_first<NA>(live ? J : __builtin_inf(), live ? a : NA);
        best = who < NA ? who : 0;
    }
    // lane 0 of the group re-rolls the winning step size (the same arithmetic) and stores
    const double abest = alphas[best];
    if (live) {
        if (a == 0) {
            const double Jb = traced_cost_rollout_one<true, TRACED>(md, tc, cf.f, prow, crow, vrow, abest, x0t, lt, Lt, xpt, upt, xo, uo, T);
            if (Jout) Jout[t] = Jb;
            if (idx_out) idx_out[t] = best;
        }
    }
}

// Values and gradients: 16 lanes per point (n + m <= 16 directions), lane j evaluates the tape on dual numbers seeded e_j and owns
// entry j of [c_x | c_u]; lane 0 also writes c.  Blocks past `blocks_running` take the terminal points: lanes j < n write v_x, lane 0 v.
__global__ __launch_bounds__(64) void traced_cost_gradient_kernel(const zm_tracedcost_t tc, const double* __restrict__ xTraj,
                                                                  const double* __restrict__ uTraj, const int* __restrict__ active,
                                                                  double* __restrict__ c, double* __restrict__ c_x,
                                                                  double* __restrict__ c_u, double* __restrict__ v,
                                                                  double* __restrict__ v_x, const long batch, const int T,
                                                                  const int* __restrict__ list, const long count,
                                                                  const unsigned blocks_running) {
    const int lane = threadIdx.x;
    const int j = lane & 15;
    const bool terminal = blockIdx.x >= blocks_running;   // uniform over the workgroup
    const long nslot = list ? count : batch;
    const int n = tc.n, m = tc.m;
    CostFile<Dual, true> cf;
    if (!terminal) {
        const long gi = (long)blockIdx.x * 4 + (lane >> 4);   // slot * T + k
        if (gi >= nslot * T) return;
        const long slot = gi / T;
        const int k = (int)(gi - slot * T);
        const long traj = list ? (long)list[slot] : slot;
        if (active && active[traj] == 0) return;
        const long pt = traj * T + k;
        const double* xk = xTraj + (traj * (T + 1) + k) * n;
        const double* uk = uTraj + pt * m;
        Dual x[MAXN], u[MAXM];
#pragma unroll
        for (int i = 0; i < MAXN; ++i) x[i] = Dual{(i < n) ? xk[i] : 0.0, (i == j) ? 1.0 : 0.0};
#pragma unroll
        for (int i = 0; i < MAXM; ++i) u[i] = Dual{(i < m) ? uk[i] : 0.0, (n + i == j) ? 1.0 : 0.0};
        const Dual r = tape_cost<Dual, true>(tc.running, n, m, cf.f, x, u, tape_cost_params(tc.running, traj));
        if (c && j == 0) c[pt] = r.v;
        if (j < n) {
            if (c_x) c_x[pt * n + j] = r.d;
        } else if (j < n + m) {
            if (c_u) c_u[pt * m + (j - n)] = r.d;
        }
    } else {
        const long slot = (long)(blockIdx.x - blocks_running) * 4 + (lane >> 4);
        if (slot >= nslot) return;
        const long traj = list ? (long)list[slot] : slot;
        if (active && active[traj] == 0) return;
        const double* xk = xTraj + (traj * (T + 1) + T) * n;
        Dual x[MAXN], u[MAXM];
#pragma unroll
        for (int i = 0; i < MAXN; ++i) x[i] = Dual{(i < n) ? xk[i] : 0.0, (i == j) ? 1.0 : 0.0};
#pragma unroll
        for (int i = 0; i < MAXM; ++i) u[i] = Dual{0.0, 0.0};
        const Dual r = tape_cost<Dual, false>(tc.terminal, n, m, cf.f, x, u, tape_cost_params(tc.terminal, traj));
        if (v && j == 0) v[traj] = r.v;
        if (v_x && j < n) v_x[traj * n + j] = r.d;
    }
}

// index of the k-th set bit of mask (k < popcount)
__device__ __forceinline__ int traced_cost_nth_bit(unsigned mask, int k) {
    for (; k > 0; --k) mask &= mask - 1u;
    return __builtin_ctz(mask);
}

// Hessians (traced.hip: traced_quadratic_kernel): the unordered pairs (a <= b) of the variables of the tape's structural mask are spread
// over the `lpp` lanes of a point (a power of two, 16 .. 64), each evaluated once on hyper-dual numbers seeded e_a, e_b; every other
// entry is zero.  Blocks past `blocks_running` take the terminal points with `lpp_terminal` lanes each.
template <bool LDS>
__global__ __launch_bounds__(64) void traced_cost_hessian_kernel(const zm_tracedcost_t tc, const double* __restrict__ xTraj,
                                                                 const double* __restrict__ uTraj, const int* __restrict__ active,
                                                                 double* __restrict__ c_xx, double* __restrict__ c_ux,
                                                                 double* __restrict__ c_uu, double* __restrict__ v_xx, const long batch,
                                                                 const int T, const int* __restrict__ list, const long count,
                                                                 const unsigned blocks_running, const int lpp_running,
                                                                 const int lpp_terminal) {
    const bool terminal = blockIdx.x >= blocks_running;   // uniform over the workgroup
    const int lpp = terminal ? lpp_terminal : lpp_running;
    const int sub = threadIdx.x / lpp, lp = threadIdx.x % lpp;
    const long nslot = list ? count : batch;
    const long sp = (long)(terminal ? blockIdx.x - blocks_running : blockIdx.x) * (64 / lpp) + sub;   // slot * T + k, or slot
    if (sp >= (terminal ? nslot : nslot * T)) return;
    const long slot = terminal ? sp : sp / T;
    const int k = terminal ? T : (int)(sp - slot * T);
    const long traj = list ? (long)list[slot] : slot;
    if (active && active[traj] == 0) return;
    const long pt = traj * T + k;   // (running points only)
    const int n = tc.n, m = tc.m;
    const double* xk = xTraj + (traj * (T + 1) + k) * n;
    const double* uk = terminal ? nullptr : uTraj + pt * m;
    double* oxx = terminal ? v_xx + traj * n * n : c_xx + pt * n * n;
    double* oux = terminal ? nullptr : c_ux + pt * m * n;
    double* ouu = terminal ? nullptr : c_uu + pt * m * m;
    {   // zero fill with coalesced stores, then the pairs
        for (int e = lp; e < n * n; e += lpp) oxx[e] = 0.0;
        if (!terminal) {
            for (int e = lp; e < m * n; e += lpp) oux[e] = 0.0;
            for (int e = lp; e < m * m; e += lpp) ouu[e] = 0.0;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");   // the zeros land before the entries written below
        __builtin_amdgcn_s_waitcnt(0);
    }
    const zm_traced_t& tp = terminal ? tc.terminal : tc.running;
    const unsigned mask = terminal ? tc.terminal_mask : tc.running_mask;
    const int V = __builtin_popcount(mask);
    const int npairs = V * (V + 1) / 2;
    CostFile<Hyper, LDS> cf;
    const double* prow = tape_cost_params(tp, traj);
    for (int p = lp; p < npairs; p += lpp) {
        int ia = 0, rem = p;
        while (rem >= V - ia) {  // row ia of the upper triangle holds V - ia pairs (ia, ia..V-1)
            rem -= V - ia;
            ++ia;
        }
        const int a = traced_cost_nth_bit(mask, ia), b = traced_cost_nth_bit(mask, ia + rem);
        Hyper x[MAXN], u[MAXM];
#pragma unroll
        for (int i = 0; i < MAXN; ++i) x[i] = Hyper{(i < n) ? xk[i] : 0.0, (i == a) ? 1.0 : 0.0, (i == b) ? 1.0 : 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < MAXM; ++i)
            u[i] = Hyper{(!terminal && i < m) ? uk[i] : 0.0, (n + i == a) ? 1.0 : 0.0, (n + i == b) ? 1.0 : 0.0, 0.0};
        // (one call for both tapes: the terminal tape's control slots receive zeros that it never reads)
        const double h = tape_cost<Hyper, true>(tp, n, m, cf.f, x, u, prow).d12;
        if (b < n) {                 // both states: c_xx[a][b] = c_xx[b][a]
            oxx[a * n + b] = h;
            oxx[b * n + a] = h;
        } else if (!terminal) {
            if (a < n) {             // a state, b control: c_ux[b-n][a]
                oux[(b - n) * n + a] = h;
            } else {                 // both controls
                ouu[(a - n) * m + (b - n)] = h;
                ouu[(b - n) * m + (a - n)] = h;
            }
        }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------

static int tape_check(const zm_traced_t& t, int n, int m, const char* which, const char* who) {
    if (t.n_params < 0 || t.n_params > ZM_TRACED_MAX_PARAMS || t.n_instr < 0 || t.n_instr > ZM_TRACED_MAX_INSTR || t.n_const < 0 ||
        t.n_const > ZM_TRACED_MAX_CONSTS || t.n_slots < n + m + t.n_params || t.n_slots > ZM_TRACED_MAX_SLOTS)
        return set_error(ZM_EUNSUPPORTED, "%s: %s tape outside the interpreter's caps (instructions %d <= %d, slots %d <= %d, constants "
                         "%d <= %d, parameters %d <= %d)", who, which, t.n_instr, ZM_TRACED_MAX_INSTR, t.n_slots, ZM_TRACED_MAX_SLOTS,
                         t.n_const, ZM_TRACED_MAX_CONSTS, t.n_params, ZM_TRACED_MAX_PARAMS);
    if (!t.tape || ((uintptr_t)t.tape & 7)) return set_error(ZM_EINVAL, "%s: the %s cost needs an 8-byte aligned tape", who, which);
    if (t.n_params > 0 && (!t.params || t.param_stride < 0))
        return set_error(ZM_EINVAL, "%s: %s cost with %d parameters needs params and a non-negative stride", who, which, t.n_params);
    return ZM_OK;
}

int tracedcost_check(const zm_tracedcost_t* tc, const char* who) {
    if (!tc) return set_error(ZM_EINVAL, "%s: null cost descriptor", who);
    if (tc->n < 1 || tc->n > MAXN || tc->m < 1 || tc->m > MAXM)
        return set_error(ZM_EUNSUPPORTED, "%s: traced cost with (n=%d, m=%d): need 1 <= n <= 12, 1 <= m <= 4", who, tc->n, tc->m);
    if (const int rc = tape_check(tc->running, tc->n, tc->m, "running", who)) return rc;
    if (const int rc = tape_check(tc->terminal, tc->n, tc->m, "terminal", who)) return rc;
    if ((tc->running_mask >> (tc->n + tc->m)) || (tc->terminal_mask >> tc->n))
        return set_error(ZM_EINVAL, "%s: a mask of the traced cost names a variable beyond n + m (the terminal mask: beyond n)", who);
    return ZM_OK;
}

// The line search's slot file: LDS, the traced model's choice (traced.hip: traced_scratch_linesearch has the measurement that decided
// it; profiles/traced_cost_bench.txt has the one with two tapes sharing the file).  -DZM_LAB: ZOPT_AMD_TRACED_SLOTS=scratch selects the
// scratch file here as it does there.
static bool traced_cost_scratch_linesearch() {
    const char* e = lab_env("ZOPT_AMD_TRACED_SLOTS");
    return e && e[0] == 's';
}

static int max3(int a, int b, int c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }

}  // namespace zm

extern "C" int zm_traced_cost_linesearch_list_f64(const zm_model_t* model, const zm_tracedcost_t* tcost, const double* x0,
                                                  const double* l, const double* L, const double* xPrev, const double* uPrev,
                                                  const double* alphas, int n_alpha, const int32_t* list, int64_t count,
                                                  const int32_t* active, double* xTraj, double* uTraj, double* J, int32_t* alpha_idx,
                                                  int64_t batch, int T, void* stream) {
    const char* who = "zm_traced_cost_linesearch_list_f64";
    if (!model || !x0 || !l || !L || !xPrev || !uPrev || !alphas || !xTraj || !uTraj) return zm::set_error(ZM_EINVAL, "%s: null pointer", who);
    if (batch < 0 || T < 1 || n_alpha < 1 || n_alpha > 16)
        return zm::set_error(ZM_EINVAL, "%s: bad size batch=%lld T=%d n_alpha=%d", who, (long long)batch, T, n_alpha);
    if (const int rc = zm::tracedcost_check(tcost, who)) return rc;
    zm_model_t md;
    if (const int rc = zm::model_check(model, who, &md)) return rc;
    if (md.n != tcost->n || md.m != tcost->m)
        return zm::set_error(ZM_EINVAL, "%s: the cost is (n=%d, m=%d), the model (n=%d, m=%d)", who, tcost->n, tcost->m, md.n, md.m);
    if (list && (count < 0 || count > batch)) return zm::set_error(ZM_EINVAL, "%s: bad list length", who);
    if (batch == 0 || (list && count == 0)) return ZM_OK;
    if ((int64_t)T * md.n * md.n >= (int64_t)1 << 31 || batch >= ((int64_t)1 << 31))
        return zm::set_error(ZM_EUNSUPPORTED, "%s: T*n*n or batch too large", who);
    const bool traced = md.kind == ZM_MODEL_TRACED;
    const long nslot = list ? count : batch;
    const int slots = zm::max3(tcost->running.n_slots, tcost->terminal.n_slots, traced ? zm::traced_of(md).n_slots : 0);
    const size_t lds = (size_t)zm::LdsSlots<double>::bytes(slots, 64);
    const bool scratch = zm::traced_cost_scratch_linesearch();
    hipStream_t st = (hipStream_t)stream;
#define ZM_LAUNCH_TC(NA_, TR_, LDS_, BLOCKS_)                                                                                           \
    hipLaunchKernelGGL((zm::traced_cost_rollout_kernel<NA_, TR_, LDS_>), dim3((unsigned)(BLOCKS_)), dim3(64), (LDS_) ? lds : 0, st, md,   \
                       *tcost, x0, l, L, xPrev, uPrev, alphas, n_alpha, (const int*)active, (const int*)list, (long)count, xTraj, uTraj, \
                       J, (int*)alpha_idx, (long)batch, T)
#define ZM_LAUNCH_TC_NA(TR_, LDS_)                                  \
    do {                                                            \
        if (n_alpha == 1) ZM_LAUNCH_TC(1, TR_, LDS_, (nslot + 63) / 64); \
        else ZM_LAUNCH_TC(16, TR_, LDS_, (nslot + 3) / 4);          \
    } while (0)
    if (traced) {
        if (scratch) ZM_LAUNCH_TC_NA(true, false);
        else ZM_LAUNCH_TC_NA(true, true);
    } else {
        if (scratch) ZM_LAUNCH_TC_NA(false, false);
        else ZM_LAUNCH_TC_NA(false, true);
    }
#undef ZM_LAUNCH_TC_NA
#undef ZM_LAUNCH_TC
    ZM_HIP_CHECK(hipGetLastError());
    return ZM_OK;
}

extern "C" int zm_traced_cost_expand_list_f64(const zm_tracedcost_t* tcost, const double* xTraj, const double* uTraj, const int32_t* list,
                                              int64_t count, const int32_t* active, double* c, double* c_x, double* c_u, double* c_xx,
                                              double* c_ux, double* c_uu, double* v, double* v_x, double* v_xx, int64_t batch, int T,
                                              void* stream) {
    const char* who = "zm_traced_cost_expand_list_f64";
    if (const int rc = zm::tracedcost_check(tcost, who)) return rc;
    if (!xTraj || !uTraj) return zm::set_error(ZM_EINVAL, "%s: null pointer", who);
    if ((c_xx != nullptr) != (c_ux != nullptr) || (c_xx != nullptr) != (c_uu != nullptr))
        return zm::set_error(ZM_EINVAL, "%s: c_xx, c_ux, c_uu: all or none", who);
    if (batch < 0 || T < 1) return zm::set_error(ZM_EINVAL, "%s: bad size", who);
    if (list && (count < 0 || count > batch)) return zm::set_error(ZM_EINVAL, "%s: bad list length", who);
    if (batch == 0 || (list && count == 0)) return ZM_OK;
    const int n = tcost->n;
    if ((int64_t)T * n * n >= (int64_t)1 << 31 || batch >= ((int64_t)1 << 31))
        return zm::set_error(ZM_EUNSUPPORTED, "%s: T*n*n or batch too large", who);
    hipStream_t st = (hipStream_t)stream;
    const long nslot = list ? count : batch;
    const int slots = tcost->running.n_slots > tcost->terminal.n_slots ? tcost->running.n_slots : tcost->terminal.n_slots;
    const bool grad_running = c || c_x || c_u, grad_terminal = v || v_x;
    if (grad_running || grad_terminal) {
        const unsigned br = grad_running ? (unsigned)((nslot * T + 3) / 4) : 0u, bt = grad_terminal ? (unsigned)((nslot + 3) / 4) : 0u;
        hipLaunchKernelGGL(zm::traced_cost_gradient_kernel, dim3(br + bt), dim3(64), (size_t)zm::LdsSlots<zm::Dual>::bytes(slots, 64), st,
                           *tcost, xTraj, uTraj, (const int*)active, c, c_x, c_u, v, v_x, (long)batch, T, (const int*)list, (long)count, br);
    }
    if (c_xx || v_xx) {
        auto lanes = [](unsigned mask) {
            const int V = __builtin_popcount(mask), npairs = V * (V + 1) / 2;
            int lpp = 16;
            while (lpp < 64 && lpp < npairs) lpp *= 2;
            return lpp;
        };
        const int lr = lanes(tcost->running_mask), lt = lanes(tcost->terminal_mask);
        const long pr = 64 / lr, pt = 64 / lt;
        const unsigned br = c_xx ? (unsigned)((nslot * T + pr - 1) / pr) : 0u, bt = v_xx ? (unsigned)((nslot + pt - 1) / pt) : 0u;
        const long lds = zm::LdsSlots<zm::Hyper>::bytes(slots, 64);
        if (lds <= 64 * 1024)
            hipLaunchKernelGGL(zm::traced_cost_hessian_kernel<true>, dim3(br + bt), dim3(64), (size_t)lds, st, *tcost, xTraj, uTraj,
                               (const int*)active, c_xx, c_ux, c_uu, v_xx, (long)batch, T, (const int*)list, (long)count, br, lr, lt);
        else
            hipLaunchKernelGGL(zm::traced_cost_hessian_kernel<false>, dim3(br + bt), dim3(64), 0, st, *tcost, xTraj, uTraj,
                               (const int*)active, c_xx, c_ux, c_uu, v_xx, (long)batch, T, (const int*)list, (long)count, br, lr, lt);
    }
    ZM_HIP_CHECK(hipGetLastError());
    return ZM_OK;
}
