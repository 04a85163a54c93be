// K9  state box -- the two small kernels of the augmented-Lagrangian loop around the fused iLQR (ilqr_solve.hip) that are neither a
// line search (rollout.hip: rollout_linesearch_pen_kernel) nor a sweep (ilqr_backward.hip: ilqr_backward_pen_t16_f64):
//   state_penalty_expand   after the expansions: c_x[k] += g_k (1 <= k < T), v_x += g_T, h (batch, T+1, n) <- the diagonal addend
//   state_multiplier_update   between two inner solves: violation, done test, lam <- pos(s), mu <- min(mu * growth, mu_max), masks
// Extension; the reference has no counterpart (its iLQR is unconstrained, ilqrUtils.py:260-327).
#include "state_box.h"
#include "zm_common.h"

namespace zm {

// lane-parallel over (slot, k, i): one thread per entry of the listed trajectories' (T+1, n) rows
__global__ __launch_bounds__(256) void state_penalty_expand_kernel(const PenRef pr, const double* __restrict__ xTraj,
                                                                   const int* __restrict__ list, const long nslot,
                                                                   const int* __restrict__ active, double* __restrict__ c_x,
                                                                   double* __restrict__ v_x, double* __restrict__ h,
                                                                   int* __restrict__ visits, const int T, const int n) {
    const long row = (long)(T + 1) * n;
    const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (e >= nslot * row) return;
    const long slot = e / row, r = e % row;
    const long t = list ? (long)list[slot] : slot;
    if (active && active[t] == 0) return;
    const int k = (int)(r / n), i = (int)(r % n);
    if (k == 0) {
        h[t * row + r] = 0.0;   // x_0 is given: never constrained
        if (i == 0 && visits) visits[t] += 1;   // one visit per iteration of the loop over this trajectory
        return;
    }
    const double x = xTraj[t * row + r], mu = pr.mu[t];
    const double su = pr.lam_ub[t * row + r] + mu * (x - pr.ub[t * pr.stride + i]);
    const double sl = pr.lam_lb[t * row + r] + mu * (pr.lb[t * pr.stride + i] - x);
    const double g = pen_pos(su) - pen_pos(sl);
    h[t * row + r] = mu * ((su > 0.0 ? 1.0 : 0.0) + (sl > 0.0 ? 1.0 : 0.0));
    if (k < T) c_x[(t * T + k) * n + i] += g;
    else v_x[t * n + i] += g;
}

// one wave per trajectory
__global__ __launch_bounds__(64) void state_multiplier_update_kernel(const double* __restrict__ lb, const double* __restrict__ ub,
                                                                     const long stride, double* __restrict__ lam_lb,
                                                                     double* __restrict__ lam_ub, double* __restrict__ mu,
                                                                     const double* __restrict__ xTraj, int* __restrict__ active,
                                                                     int* __restrict__ converged, double* __restrict__ violation,
                                                                     int* __restrict__ outer_count, int* __restrict__ remaining,
                                                                     const double ctol, const double growth, const double mu_max,
                                                                     const int update, const int T, const int n) {
    const long t = blockIdx.x;
    const int lane = threadIdx.x;
    if (active[t] == 0) return;   // done earlier: nothing of it is touched (the whole wave leaves: the mask is written below by lane 0 only
                                  // after every lane has read it -- one wave, in order)
    const long row = (long)(T + 1) * n;
    double v = 0.0;
    int isnan_ = 0;
    for (long r = n + lane; r < row; r += 64) {
        const int i = (int)(r % n);
        const double x = xTraj[t * row + r];
        const double a = x - ub[t * stride + i], b = lb[t * stride + i] - x;
        isnan_ |= (x != x) ? 1 : 0;
        v = a > v ? a : v;
        v = b > v ? b : v;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double o = __shfl_xor(v, off, 64);
        isnan_ |= __shfl_xor(isnan_, off, 64);
        v = o > v ? o : v;
    }
    const double viol = isnan_ ? __builtin_nan("") : v;
    const bool done = converged[t] != 0 && viol <= ctol;   // a NaN is never <= ctol
    __builtin_amdgcn_wave_barrier();
    if (!done && update) {
        const double m0 = mu[t];
        for (long r = n + lane; r < row; r += 64) {
            const int i = (int)(r % n);
            const double x = xTraj[t * row + r];
            lam_ub[t * row + r] = pen_pos(lam_ub[t * row + r] + m0 * (x - ub[t * stride + i]));
            lam_lb[t * row + r] = pen_pos(lam_lb[t * row + r] + m0 * (lb[t * stride + i] - x));
        }
    }
    if (lane == 0) {
        violation[t] = viol;
        if (outer_count) outer_count[t] += 1;
        converged[t] = done ? 1 : 0;
        active[t] = done ? 0 : 1;
        if (!done) {
            if (update) {
                const double g = mu[t] * growth;
                mu[t] = g < mu_max ? g : mu_max;
            }
            if (remaining) atomicAdd(remaining, 1);
        }
    }
}

// the masked start of an inner solve (ilqr_init_kernel of ilqr_solve.hip for the trajectories of `mask` only): l <- uStart, L <- 0,
// previous trajectory <- 0, converged <- 0 on the masked rows; active <- mask, where <- 0 and the step sizes for everyone
__global__ __launch_bounds__(256) void ilqr_init_masked_kernel(const int* mask, double* __restrict__ l,
                                                               const double* __restrict__ uStart, const long urow, double* __restrict__ L,
                                                               const long Lrow, double* __restrict__ xT2, const long xrow,
                                                               double* __restrict__ uT2, double* __restrict__ alphas,
                                                               int* active, int* __restrict__ converged,
                                                               int* __restrict__ where) {
    const long t = blockIdx.x;
    const int on = mask[t];
    if (t == 0 && threadIdx.x < 16) alphas[threadIdx.x] = 1.0 / (double)(1u << threadIdx.x);   // exact powers of two
    __syncthreads();   // (active may be the mask itself)
    if (threadIdx.x == 0) {
        active[t] = on ? 1 : 0;
        if (where) where[t] = 0;
        if (on) converged[t] = 0;
    }
    if (!on) return;
    for (long i = threadIdx.x; i < Lrow; i += blockDim.x) L[t * Lrow + i] = 0.0;
    for (long i = threadIdx.x; i < xrow; i += blockDim.x) xT2[t * xrow + i] = 0.0;
    for (long i = threadIdx.x; i < urow; i += blockDim.x) {
        l[t * urow + i] = uStart[t * urow + i];
        uT2[t * urow + i] = 0.0;
    }
}

int ilqr_init_masked(const int32_t* mask, double* l, const double* uStart, double* L, double* xT2, double* uT2, double* alphas,
                     int32_t* active, int32_t* converged, int32_t* where, int64_t batch, int T, int n, int m, hipStream_t st) {
    hipLaunchKernelGGL(ilqr_init_masked_kernel, dim3((unsigned)batch), dim3(256), 0, st, (const int*)mask, l, uStart, (long)T * m, L,
                       (long)T * m * n, xT2, (long)(T + 1) * n, uT2, alphas, (int*)active, (int*)converged, (int*)where);
    ZM_HIP_CHECK(hipGetLastError());
    return ZM_OK;
}

int state_penalty_expand(const zm_statebox_t* sbox, const double* xTraj, const int32_t* list, int64_t count, const int32_t* active,
                         double* c_x, double* v_x, double* h, int32_t* visits, int64_t batch, int T, int n, hipStream_t st) {
    const long nslot = list ? (long)count : (long)batch;
    const long work = nslot * (long)(T + 1) * n;
    hipLaunchKernelGGL(state_penalty_expand_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, st, pen_ref(*sbox), xTraj,
                       (const int*)list, nslot, (const int*)active, c_x, v_x, h, (int*)visits, T, n);
    ZM_HIP_CHECK(hipGetLastError());
    return ZM_OK;
}

}  // namespace zm

static int state_sizes(const char* who, int64_t batch, int T, int n) {
    if (batch < 0 || T < 1 || n < 1) return zm::set_error(ZM_EINVAL, "%s: bad size batch=%lld T=%d n=%d", who, (long long)batch, T, n);
    if (n > 12) return zm::set_error(ZM_EUNSUPPORTED, "%s: n=%d not covered (state box: n<=12, m<=4)", who, n);
    if (batch >= ((int64_t)1 << 31) || (int64_t)(T + 1) * n >= ((int64_t)1 << 31)) return zm::set_error(ZM_EUNSUPPORTED, "%s: batch or (T+1)*n too large", who);
    return ZM_OK;
}

extern "C" int zm_state_penalty_expand_list_f64(const zm_statebox_t* sbox, const double* xTraj, const int32_t* list, int64_t count,
                                                const int32_t* active, double* c_x, double* v_x, double* h, int64_t batch, int T, int n,
                                                void* stream) {
    const char* who = "zm_state_penalty_expand_list_f64";
    if (const int rc = state_sizes(who, batch, T, n)) return rc;
    if (const int rc = zm::statebox_check(sbox, n, who)) return rc;
    if (!xTraj || !c_x || !v_x || !h) return zm::set_error(ZM_EINVAL, "%s: null pointer", who);
    if (list && (count < 0 || count > batch)) return zm::set_error(ZM_EINVAL, "%s: bad list length", who);
    if (batch == 0 || (list && count == 0)) return ZM_OK;
    return zm::state_penalty_expand(sbox, xTraj, list, count, active, c_x, v_x, h, nullptr, batch, T, n, (hipStream_t)stream);
}

extern "C" int zm_state_multiplier_update_f64(const zm_statebox_t* sbox, const double* xTraj, int32_t* active, int32_t* converged,
                                              double* violation, int32_t* outer_count, int32_t* remaining, double ctol, double growth,
                                              double mu_max, int update, int64_t batch, int T, int n, void* stream) {
    const char* who = "zm_state_multiplier_update_f64";
    if (const int rc = state_sizes(who, batch, T, n)) return rc;
    if (const int rc = zm::statebox_check(sbox, n, who)) return rc;
    if (!xTraj || !active || !converged || !violation) return zm::set_error(ZM_EINVAL, "%s: null pointer", who);
    if (!(growth >= 1.0) || !(mu_max > 0.0) || !(ctol >= 0.0)) return zm::set_error(ZM_EINVAL, "%s: need growth >= 1, mu_max > 0, ctol >= 0", who);
    if (batch == 0) return ZM_OK;
    hipLaunchKernelGGL(zm::state_multiplier_update_kernel, dim3((unsigned)batch), dim3(64), 0, (hipStream_t)stream, sbox->lb, sbox->ub,
                       (long)sbox->stride, sbox->lam_lb, sbox->lam_ub, sbox->mu, xTraj, (int*)active, (int*)converged, violation,
                       (int*)outer_count, (int*)remaining, ctol, growth, mu_max, update ? 1 : 0, T, n);
    ZM_HIP_CHECK(hipGetLastError());
    return ZM_OK;
}
