// ZM_MODEL_TRACED: the kernels that run a recorded dynamics function (tape_model.h) -- siblings of the registered models' generic
// kernels, launched by the same entry points when the model's kind is ZM_MODEL_TRACED (rollout.hip, linearize.hip, mpc.hip dispatch
// here; ilqr_solve.hip reaches them through those entries).  No existing kernel includes the interpreter: their device code is what
// it was.
//
//   traced_rollout_kernel     zopt/ilqrUtils.py:33-66, :116-150 -- one lane per (trajectory, step size), two passes, the line search's
//                             argmin (zm_common.h: argmin_nan_first); S = double
//   traced_linearize_kernel   zopt/pytrees.py:139-153 -- 16 lanes per point, lane j seeds direction j; S = Dual
//   traced_quadratic_kernel   zopt/pytrees.py:180-194 -- the pairs of the structural mask over the lanes of a point; S = Hyper
//   traced_step_kernel        the plant step of mpcUtils.modelStep -- one lane per instance; S = double
//
// Slot file (tape_model.h): LDS, sized per launch by the model's own slot count, wherever a wave's file fits the 64 KiB a launch gets
// without raising the kernel's limit -- always for double (<= 32 KiB) and Dual (<= 64 KiB), for Hyper up to 32 slots; a Hyper file
// beyond that is private scratch (2 KiB per lane).  The line search was measured both ways (below, traced_scratch_linesearch).
#include "tape_model.h"
#include "traced.h"
#include "zm_common.h"

namespace zm {

extern __shared__ __attribute__((aligned(16))) double zm_tape_lds[];

template <typename S, bool LDS>
struct TapeFile;
template <typename S>
struct TapeFile<S, true> {
    LdsSlots<S> f;
    __device__ __forceinline__ TapeFile() : f{zm_tape_lds + threadIdx.x, (int)blockDim.x} {}
};
template <typename S>
struct TapeFile<S, false> {
    ArraySlots<S> f;
};

__device__ __forceinline__ const double* traced_params(const zm_model_t& md, const long t) {
    const zm_traced_t d = traced_of(md);
    return d.params ? d.params + t * d.param_stride : nullptr;
}

// one rollout of trajectory t under step size alpha (rollout.hip: rollout_one without tracking, box and penalty)
template <bool STORE, typename SLOTS>
__device__ __forceinline__ double traced_rollout_one(const zm_model_t& md, SLOTS& f, const double* __restrict__ prow,
                                                     const zm_quadcost_t* cs, const double alpha, const double* __restrict__ x0,
                                                     const double* __restrict__ l, const double* __restrict__ L,
                                                     const double* __restrict__ xPrev, const double* __restrict__ uPrev,
                                                     double* __restrict__ xTraj, double* __restrict__ uTraj, const int T) {
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
        if (cs) J += running_cost(*cs, n, m, x, u);
        tape_step<double, SLOTS>(md, f, x, u, prow, xn);
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
    if (cs) J += terminal_cost(*cs, n, x);
    return J;
}

// NA = lanes per trajectory (1 or 16); the frame is rollout_linesearch_body.h's, the argmin the shared one (zm_common.h)
template <int NA, bool LDS>
__global__ __launch_bounds__(64) void traced_rollout_kernel(const zm_model_t md, const zm_quadcost_t cost, const bool has_cost,
                                                            const double* __restrict__ x0, const double* __restrict__ l,
                                                            const double* __restrict__ L, const double* __restrict__ xPrev,
                                                            const double* __restrict__ uPrev, const double* __restrict__ alphas,
                                                            const int n_alpha, const int* __restrict__ active,
                                                            const int* __restrict__ list, const long count, double* __restrict__ xTraj,
                                                            double* __restrict__ uTraj, double* __restrict__ Jout,
                                                            int* __restrict__ idx_out, const long batch, const int T) {
    constexpr int TPW = 64 / NA;  // trajectories per wave
    const int lane = threadIdx.x;
    const int a = lane % NA;
    const long slot = (long)blockIdx.x * TPW + lane / NA;   // slot -> trajectory id (through `list` when given)
    const long nslot = list ? count : batch;
    const long traj = (slot < nslot) ? (list ? (long)list[slot] : slot) : 0;
    const bool live = (slot < nslot) && (a < n_alpha) && (active == nullptr || active[traj] != 0);
    const long t = live ? traj : 0;
    const int n = md.n, m = md.m;
    const zm_quadcost_t* cs = has_cost ? &cost : nullptr;
    const double alpha = alphas[a < n_alpha ? a : 0];
    const double* x0t = x0 + t * n;
    const double* lt = l + t * T * m;
    const double* Lt = L + t * T * m * n;
    const double* xpt = xPrev + t * (T + 1) * n;
    const double* upt = uPrev + t * T * m;
    double* xo = xTraj + t * (T + 1) * n;
    double* uo = uTraj + t * T * m;
    const double* prow = traced_params(md, t);
    TapeFile<double, LDS> tf;

    double J = 0.0;
    int best = 0;
    if (NA > 1) {
        if (live) J = traced_rollout_one<false>(md, tf.f, prow, cs, alpha, x0t, lt, Lt, xpt, upt, nullptr, nullptr, T);
        // dead lanes carry (+inf, index NA)
        const int who = argmin_nan_first<NA>(live ? J : __builtin_inf(), live ? a : NA);
        best = who < NA ? who : 0;
    }
    // lane 0 of the group re-rolls the winning step size (the same arithmetic) and stores
    const double abest = alphas[best];
    if (live) {
        if (a == 0) {
            const double Jb = traced_rollout_one<true>(md, tf.f, prow, cs, abest, x0t, lt, Lt, xpt, upt, xo, uo, T);
            if (Jout) Jout[t] = Jb;
            if (idx_out) idx_out[t] = best;
        }
    }
}

// One step per lane: xNext[b] = f(x[b], u[b], p[b])
__global__ __launch_bounds__(64) void traced_step_kernel(const zm_model_t md, const double* __restrict__ x, const double* __restrict__ u,
                                                         double* __restrict__ xNext, const long batch) {
    const long b = (long)blockIdx.x * 64 + threadIdx.x;
    if (b >= batch) return;
    const int n = md.n, m = md.m;
    double xv[MAXN], uv[MAXM], xn[MAXN];
#pragma unroll
    for (int i = 0; i < MAXN; ++i) xv[i] = (i < n) ? x[b * n + i] : 0.0;
#pragma unroll
    for (int i = 0; i < MAXM; ++i) uv[i] = (i < m) ? u[b * m + i] : 0.0;
    TapeFile<double, true> tf;
    tape_step<double>(md, tf.f, xv, uv, traced_params(md, b), xn);
#pragma unroll
    for (int i = 0; i < MAXN; ++i)
        if (i < n) xNext[b * n + i] = xn[i];
}

// First-order expansion: 16 lanes per point (n + m <= 16 directions), lane j evaluates the tape on dual numbers seeded e_j and owns
// column j of [f_x | f_u]; lane 0 also writes f.
__global__ __launch_bounds__(64) void traced_linearize_kernel(const zm_model_t md, const double* __restrict__ xTraj,
                                                              const double* __restrict__ uTraj, const int* __restrict__ active,
                                                              double* __restrict__ f, double* __restrict__ f_x, double* __restrict__ f_u,
                                                              const long batch, const int T, const int* __restrict__ list,
                                                              const long count) {
    const int lane = threadIdx.x;
    const int j = lane & 15;
    const long gi = (long)blockIdx.x * 4 + (lane >> 4);   // slot * T + k
    const long nslot = list ? count : batch;
    if (gi >= nslot * T) return;
    const long slot = gi / T;
    const int k = (int)(gi - slot * T);
    const long traj = list ? (long)list[slot] : slot;
    if (active && active[traj] == 0) return;
    const int n = md.n, m = md.m;
    const long pt = traj * T + k;
    const double* xk = xTraj + (traj * (T + 1) + k) * n;
    const double* uk = uTraj + pt * m;
    Dual x[MAXN], u[MAXM], xn[MAXN];
#pragma unroll
    for (int i = 0; i < MAXN; ++i) x[i] = Dual{(i < n) ? xk[i] : 0.0, (i == j) ? 1.0 : 0.0};
#pragma unroll
    for (int i = 0; i < MAXM; ++i) u[i] = Dual{(i < m) ? uk[i] : 0.0, (n + i == j) ? 1.0 : 0.0};
    TapeFile<Dual, true> tf;
    tape_step<Dual>(md, tf.f, x, u, traced_params(md, traj), xn);
    if (f && j == 0) {
#pragma unroll
        for (int i = 0; i < MAXN; ++i)
            if (i < n) f[pt * n + i] = xn[i].v;
    }
    if (j < n) {
#pragma unroll
        for (int i = 0; i < MAXN; ++i)
            if (i < n) f_x[(pt * n + i) * n + j] = xn[i].d;
    } else if (j < n + m) {
#pragma unroll
        for (int i = 0; i < MAXN; ++i)
            if (i < n) f_u[(pt * n + i) * m + (j - n)] = xn[i].d;
    }
}

// index of the k-th set bit of mask (k < popcount)
__device__ __forceinline__ int traced_nth_bit(unsigned mask, int k) {
    for (; k > 0; --k) mask &= mask - 1u;
    return __builtin_ctz(mask);
}

// Second-order expansion with full tensors (linearize.hip: quadratic_dynamics_kernel): the unordered pairs (a <= b) of the variables
// of the structural mask are spread over the `lpp` lanes of a point (a power of two, 16 .. 64), each evaluated once on hyper-dual
// numbers seeded e_a, e_b; every other entry is zero.
template <bool LDS>
__global__ __launch_bounds__(64) void traced_quadratic_kernel(const zm_model_t md, const double* __restrict__ xTraj,
                                                              const double* __restrict__ uTraj, const int* __restrict__ active,
                                                              double* __restrict__ f_xx, double* __restrict__ f_ux,
                                                              double* __restrict__ f_uu, const long batch, const int T,
                                                              const int* __restrict__ list, const long count, const int lpp) {
    const int sub = threadIdx.x / lpp, lp = threadIdx.x % lpp;
    const long nslot = list ? count : batch;
    const long sp = (long)blockIdx.x * (64 / lpp) + sub;       // slot * T + k
    if (sp >= nslot * T) return;
    const long slot = sp / T;
    const int k = (int)(sp - slot * T);
    const long traj = list ? (long)list[slot] : slot;
    if (active && active[traj] == 0) return;
    const long pt = traj * T + k;
    const int n = md.n, m = md.m;
    const double* xk = xTraj + (traj * (T + 1) + k) * n;
    const double* uk = uTraj + pt * m;
    double* oxx = f_xx + pt * n * n * n;
    double* oux = f_ux + pt * n * m * n;
    double* ouu = f_uu + pt * n * m * m;
    {   // zero fill with coalesced stores, then the pairs
        const int nxx = n * n * n, nux = n * m * n, nuu = n * m * m;
        for (int e = lp; e < nxx; e += lpp) oxx[e] = 0.0;
        if (f_ux) {
            for (int e = lp; e < nux; e += lpp) oux[e] = 0.0;
            for (int e = lp; e < nuu; e += lpp) ouu[e] = 0.0;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");   // the zeros land before the entries written below
        __builtin_amdgcn_s_waitcnt(0);
    }
    const unsigned mask = (unsigned)md.reserved;
    const int V = __builtin_popcount(mask);
    const int npairs = V * (V + 1) / 2;
    TapeFile<Hyper, LDS> tf;
    const double* prow = traced_params(md, traj);
    for (int p = lp; p < npairs; p += lpp) {
        int ia = 0, rem = p;
        while (rem >= V - ia) {  // row ia of the upper triangle holds V - ia pairs (ia, ia..V-1)
            rem -= V - ia;
            ++ia;
        }
        const int a = traced_nth_bit(mask, ia), b = traced_nth_bit(mask, ia + rem);
        Hyper x[MAXN], u[MAXM], xn[MAXN];
#pragma unroll
        for (int i = 0; i < MAXN; ++i) x[i] = Hyper{(i < n) ? xk[i] : 0.0, (i == a) ? 1.0 : 0.0, (i == b) ? 1.0 : 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < MAXM; ++i)
            u[i] = Hyper{(i < m) ? uk[i] : 0.0, (n + i == a) ? 1.0 : 0.0, (n + i == b) ? 1.0 : 0.0, 0.0};
        tape_step<Hyper>(md, tf.f, x, u, prow, xn);
#pragma unroll
        for (int i = 0; i < MAXN; ++i) {
            if (i < n) {
                const double h = xn[i].d12;  // d2 f_i / dz_a dz_b,  a <= b
                if (b < n) {                 // both states: f_xx[i][a][b] = f_xx[i][b][a]
                    oxx[(i * n + a) * n + b] = h;
                    oxx[(i * n + b) * n + a] = h;
                } else if (a < n) {          // a state, b control: f_ux[i][b-n][a]
                    oux[(i * m + (b - n)) * n + a] = h;
                } else {                     // both controls
                    ouu[(i * m + (a - n)) * m + (b - n)] = h;
                    ouu[(i * m + (b - n)) * m + (a - n)] = h;
                }
            }
        }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------

int traced_check(const zm_model_t* model, const char* who) {
    const zm_traced_t t = traced_of(*model);
    if (model->n < 1 || model->n > MAXN || model->m < 1 || model->m > MAXM)
        return set_error(ZM_EUNSUPPORTED, "%s: traced model with (n=%d, m=%d): need 1 <= n <= 12, 1 <= m <= 4", who, model->n, model->m);
    if (t.n_params < 0 || t.n_params > ZM_TRACED_MAX_PARAMS || t.n_instr < 0 || t.n_instr > ZM_TRACED_MAX_INSTR || t.n_const < 0 ||
        t.n_const > ZM_TRACED_MAX_CONSTS || t.n_slots < model->n + model->m + t.n_params || t.n_slots > ZM_TRACED_MAX_SLOTS)
        return set_error(ZM_EUNSUPPORTED, "%s: traced model outside the interpreter's caps (instructions %d <= %d, slots %d <= %d, "
                         "constants %d <= %d, parameters %d <= %d)", who, t.n_instr, ZM_TRACED_MAX_INSTR, t.n_slots, ZM_TRACED_MAX_SLOTS,
                         t.n_const, ZM_TRACED_MAX_CONSTS, t.n_params, ZM_TRACED_MAX_PARAMS);
    if (!t.tape || ((uintptr_t)t.tape & 7)) return set_error(ZM_EINVAL, "%s: traced model needs an 8-byte aligned tape", who);
    if (t.n_params > 0 && (!t.params || t.param_stride < 0))
        return set_error(ZM_EINVAL, "%s: traced model with %d parameters needs params and a non-negative stride", who, t.n_params);
    if ((unsigned)model->reserved >> (model->n + model->m))
        return set_error(ZM_EINVAL, "%s: traced model's mask names a variable beyond n + m", who);
    return ZM_OK;
}

// The line search's slot file: LDS.  Measured on 8192 traced quadcopters, T = 100 (tools/bench_traced_model.py,
// profiles/traced_model_bench.txt): the 16-way line search ALONE at the full batch is 5 % faster on scratch (22.14 ms against 23.24 ms,
// alternated in one process, the same bits), but the whole solve -- most of whose iterations run over a short list of stragglers, a few
// waves whose latency nothing hides -- is 13 % faster on LDS (iLQR 1505 ms against 1706 ms, DDP 3964 against 4153 ms; cart-pole and car
// alike).  The solver is what the kernel is for.  -DZM_LAB: ZOPT_AMD_TRACED_SLOTS=scratch selects the scratch file (read per call: the
// A/B flips it between launches of one process; the product's lab_env is the constant nullptr).
static bool traced_scratch_linesearch() {
    const char* e = lab_env("ZOPT_AMD_TRACED_SLOTS");
    return e && e[0] == 's';
}

int traced_rollout(const zm_model_t& md, const zm_quadcost_t* cost, const double* x0, const double* l, const double* L,
                   const double* xPrev, const double* uPrev, const double* alphas, int n_alpha, const int* active, const int* list,
                   long count, double* xTraj, double* uTraj, double* J, int* alpha_idx, long batch, int T, hipStream_t st) {
    const long nslot = list ? count : batch;
    const zm_quadcost_t cs = cost ? *cost : zm_quadcost_t{nullptr, nullptr, nullptr, 0, 0};
    const bool hc = cost != nullptr;
    const size_t lds = (size_t)LdsSlots<double>::bytes(traced_of(md).n_slots, 64);
    const bool scratch = traced_scratch_linesearch();
#define ZM_LAUNCH_TRACED(NA_, LDS_, BLOCKS_)                                                                                          \
    hipLaunchKernelGGL((traced_rollout_kernel<NA_, LDS_>), dim3((unsigned)(BLOCKS_)), dim3(64), (LDS_) ? lds : 0, st, md, cs, hc, x0, l, \
                       L, xPrev, uPrev, alphas, n_alpha, active, list, count, xTraj, uTraj, J, alpha_idx, batch, T)
    if (n_alpha == 1) {
        if (scratch) ZM_LAUNCH_TRACED(1, false, (nslot + 63) / 64);
        else ZM_LAUNCH_TRACED(1, true, (nslot + 63) / 64);
    } else {
        if (scratch) ZM_LAUNCH_TRACED(16, false, (nslot + 3) / 4);
        else ZM_LAUNCH_TRACED(16, true, (nslot + 3) / 4);
    }
#undef ZM_LAUNCH_TRACED
    ZM_HIP_CHECK(hipGetLastError());
    return ZM_OK;
}

int traced_step(const zm_model_t& md, const double* x, const double* u, double* xNext, long batch, hipStream_t st) {
    hipLaunchKernelGGL(traced_step_kernel, dim3((unsigned)((batch + 63) / 64)), dim3(64),
                       (size_t)LdsSlots<double>::bytes(traced_of(md).n_slots, 64), st, md, x, u, xNext, batch);
    ZM_HIP_CHECK(hipGetLastError());
    return ZM_OK;
}

int traced_linearize(const zm_model_t& md, const double* xTraj, const double* uTraj, const int* active, double* f, double* f_x,
                     double* f_u, long batch, int T, const int* list, long count, hipStream_t st) {
    const long ngrp = (list ? count : batch) * T;
    hipLaunchKernelGGL(traced_linearize_kernel, dim3((unsigned)((ngrp + 3) / 4)), dim3(64),
                       (size_t)LdsSlots<Dual>::bytes(traced_of(md).n_slots, 64), st, md, xTraj, uTraj, active, f, f_x, f_u, batch, T, list,
                       count);
    ZM_HIP_CHECK(hipGetLastError());
    return ZM_OK;
}

int traced_quadratic(const zm_model_t& md, const double* xTraj, const double* uTraj, const int* active, double* f_xx, double* f_ux,
                     double* f_uu, long batch, int T, const int* list, long count, hipStream_t st) {
    const int V = __builtin_popcount((unsigned)md.reserved), npairs = V * (V + 1) / 2;
    int lpp = 16;
    while (lpp < 64 && lpp < npairs) lpp *= 2;
    const long npts = (list ? count : batch) * T;
    const long ppw = 64 / lpp;
    const dim3 grid((unsigned)((npts + ppw - 1) / ppw));
    const long lds = LdsSlots<Hyper>::bytes(traced_of(md).n_slots, 64);
    if (lds <= 64 * 1024)
        hipLaunchKernelGGL(traced_quadratic_kernel<true>, grid, dim3(64), (size_t)lds, st, md, xTraj, uTraj, active, f_xx, f_ux, f_uu,
                           batch, T, list, count, lpp);
    else
        hipLaunchKernelGGL(traced_quadratic_kernel<false>, grid, dim3(64), 0, st, md, xTraj, uTraj, active, f_xx, f_ux, f_uu, batch, T,
                           list, count, lpp);
    ZM_HIP_CHECK(hipGetLastError());
    return ZM_OK;
}

}  // namespace zm
