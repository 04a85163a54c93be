// K9  mpc_box_qp -- batched box-constrained LQ-MPC, fp64, gfx950.
//
// Problem statement: zopt/mpcUtils.py:48-59 (class lqrMpc).  The reference solves it with cvxpy -> OSQP (ADMM on a
// sparse KKT system), code that is not part of the reference tree; this is an MI355X-first ADMM for the same QP:
//
//   split   w = (x_1..x_N, u_0..u_{N-1})  consistent with x_{k+1} = A x_k + B u_k, x_0 = x0      (dynamics, exact)
//           y = copy of w inside the box [lb, ub]                                                  (bounds, exact)
//   iterate w <- argmin cost(w) + rho/2 |w - (y - lam)|^2  s.t. dynamics     (LQ tracking problem)
//           y <- clip(w + lam, lb, ub);   lam <- lam + w - y
//
// The w-update's Riccati matrices depend on (A, B, Q, R, Qf, rho) only -- not on x0, y, lam -- so they are factored
// ONCE (mpc_setup_kernel: K_k, Suu_k^-1), shared by every instance and every iteration.  One ADMM iteration is then
//   backward:  p <- -rho z_N;  k = N-1..0:  Qu = -rho zu_k + B^T p;  kf_k = Suu_k^-1 Qu;  p <- hx_k + A^T p - K_k^T Qu
//   forward :  x <- x0;        k = 0..N-1:  u = -K_k x - kf_k;  x <- A x + B u;  y, lam update, residuals
// = ~500 FMAs per stage, no factorisation, no branching on data.
//
// Mapping: ONE LANE per MPC instance (instances are independent: mpcUtils.py:76-81); the shared tables are read at
// wave-uniform addresses (scalar loads), x and p live in registers, the iterates y, lam, kf in a batch-minor
// workspace (lane i <-> consecutive addresses: coalesced).  Each lane runs its own ADMM to convergence
// (OSQP-style criteria); a wave retires when all its lanes have.
//
// Termination (as OSQP): r_prim = |w - y|_inf <= eps_abs + eps_rel max(|w|,|y|),  r_dual = rho |y - y_prev|_inf <=
// eps_abs + eps_rel rho |lam|.  Infeasibility: x0 outside its bounds; or, every ZM_MPC_CHK (8) iterations, OSQP's primal
// infeasibility certificate on the dual step v = w - y:  |G^T v|_inf <= eps_pinf |v|_inf  (G = the linear map u -> w;
// computed by an adjoint sweep) and  v^T w(u=0) - support_box(v) > eps_pinf |v|_inf,  i.e. v separates the dynamics
// subspace from the box.  The certificate is sound but can need thousands of iterations; an infeasible instance that
// is not certified within max_iter reports "user_limit".
#include "mpc_common.h"
#include "models.h"

#include <cstdlib>
#include <vector>

namespace zm {

// ----------------------------------------------------------------------------------------------------------------
// setup: single workgroup, matrices in LDS, threads spread over matrix elements
// ----------------------------------------------------------------------------------------------------------------
constexpr int SN = 12, SM = 4;      // the shapes of the 16-lanes-per-instance kernel (mpc_wave.hip) and of the small lane kernels
constexpr int SNL = 24, SML = 8;    // larger problems: the lane-per-instance kernel only (fixed penalty), see zm_mpc_solve_relaxed_f64

__device__ __forceinline__ void mm_nn(double* C, const double* A, const double* B, int p, int q, int r) {  // C = A(p,q) B(q,r)
    for (int e = threadIdx.x; e < p * r; e += blockDim.x) {
        const int i = e / r, j = e % r;
        double s = 0.0;
        for (int k = 0; k < q; ++k) s = __builtin_fma(A[i * q + k], B[k * r + j], s);
        C[e] = s;
    }
    __syncthreads();
}
__device__ __forceinline__ void mm_tn(double* C, const double* A, const double* B, int q, int p, int r) {  // C = A(q,p)^T B(q,r)
    for (int e = threadIdx.x; e < p * r; e += blockDim.x) {
        const int i = e / r, j = e % r;
        double s = 0.0;
        for (int k = 0; k < q; ++k) s = __builtin_fma(A[k * p + i], B[k * r + j], s);
        C[e] = s;
    }
    __syncthreads();
}

template <int SN, int SM>
__global__ __launch_bounds__(256) void mpc_setup_kernel(const double* __restrict__ A, const double* __restrict__ B,
                                                        const double* __restrict__ Q, const double* __restrict__ R,
                                                        const double* __restrict__ Qf, const double rho, const int N,
                                                        const int n, const int m, double* __restrict__ Kout,
                                                        double* __restrict__ Minvout) {
#include "mpc_setup_body.h"
}

// P problems x L penalty levels in ONE launch: workgroup b = p * L + l factors problem p (its A, B, Q, R, Qf at p x their size) at the
// penalty rho_tab[b] into its own slice of the problem-major tables K (P, L, N, m, n), Minv (P, L, N, m, m).  The body is that of
// mpc_setup_kernel, so every (p, l) slice is bit for bit what zm_mpc_setup_f64 writes for that problem and penalty.
template <int SN, int SM>
__global__ __launch_bounds__(256) void mpc_setup_batched_kernel(const double* __restrict__ A, const double* __restrict__ B,
                                                                const double* __restrict__ Q, const double* __restrict__ R,
                                                                const double* __restrict__ Qf, const double* __restrict__ rho_tab,
                                                                const int L, const int N, const int n, const int m,
                                                                double* __restrict__ Kout, double* __restrict__ Minvout) {
    const long b = blockIdx.x, p = b / L;
    A += p * n * n;
    B += p * n * m;
    Q += p * n * n;
    R += p * m * m;
    Qf += p * n * n;
    Kout += b * N * m * n;
    Minvout += b * N * m * m;
    const double rho = rho_tab[b];
#include "mpc_setup_body.h"
}

// Stage-varying dynamics (zm_mpc_setup_ltv_f64): the recursion of mpc_setup_body.h with the stage's own A_k, B_k, reloaded into LDS at
// the top of every stage; workgroup b = p * L + l as in mpc_setup_batched_kernel.  The same products in the same order (the body is
// restated here, not included: its A and B are loaded once, before its stage loop), so constant A_k, B_k give that kernel's tables bit
// for bit.  Two more outputs: D_k = P_{k+1} c_k (P,L,N,n), formed from the value matrix before the stage updates it -- the offset's share
// of the costate in the solve's backward sweep -- and, by the workgroup of level 0 alone (it does not depend on the penalty), ABt
// (P,N,n+m,n): row i < n is column i of A_k, row n + j column j of B_k, the contiguous form the lanes of mpc_solve_wave_ltv_kernel read
// their column of [A_k | B_k] in.  c may be nullptr (D = 0).
template <int SN, int SM>
__global__ __launch_bounds__(256) void mpc_setup_ltv_kernel(const double* __restrict__ A, const double* __restrict__ B,
                                                            const double* __restrict__ c, const double* __restrict__ Q,
                                                            const double* __restrict__ R, const double* __restrict__ Qf,
                                                            const double* __restrict__ rho_tab, const int L, const int N, const int n,
                                                            const int m, double* __restrict__ Kout, double* __restrict__ Minvout,
                                                            double* __restrict__ Dout, double* __restrict__ ABt) {
    const long b = blockIdx.x, p = b / L;
    const bool pack = (b % L) == 0;
    A += p * N * n * n;
    B += p * N * n * m;
    if (c) c += p * N * n;
    Q += p * n * n;
    R += p * m * m;
    Qf += p * n * n;
    Kout += b * N * m * n;
    Minvout += b * N * m * m;
    Dout += b * N * n;
    ABt += p * N * (n + m) * n;
    const double rho = rho_tab[b];
    __shared__ double As[SN * SN], Bs[SN * SM], P[SN * SN], PA[SN * SN], PB[SN * SM], Sux[SM * SN], Suu[SM * SM], Mi[SM * SM], K[SM * SN],
        T1[SN * SN], T2[SN * SN];
    const int t = threadIdx.x;
    for (int e = t; e < n * n; e += blockDim.x) P[e] = 2.0 * Qf[e] + ((e / n == e % n) ? rho : 0.0);  // P_N = 2 Qf + rho I
    __syncthreads();
    for (int k = N - 1; k >= 0; --k) {
        // (As, Bs of the stage above were last read before the barrier that ends it; P holds P_{k+1})
        for (int e = t; e < n * n; e += blockDim.x) As[e] = A[(long)k * n * n + e];
        for (int e = t; e < n * m; e += blockDim.x) Bs[e] = B[(long)k * n * m + e];
        if (t < n) {
            double s = 0.0;
            if (c)
                for (int j = 0; j < n; ++j) s = __builtin_fma(P[t * n + j], c[(long)k * n + j], s);
            Dout[(long)k * n + t] = s;
        }
        __syncthreads();
        if (pack)
            for (int e = t; e < (n + m) * n; e += blockDim.x) {
                const int i = e / n, l = e % n;
                ABt[(long)k * (n + m) * n + e] = i < n ? As[l * n + i] : Bs[l * m + (i - n)];
            }
        mm_nn(PA, P, As, n, n, n);
        mm_nn(PB, P, Bs, n, n, m);
        mm_tn(Sux, Bs, PA, n, m, n);  // B_k^T P A_k
        mm_tn(Suu, Bs, PB, n, m, m);  // B_k^T P B_k
        if (t < m * m) Suu[t] += 2.0 * R[t] + ((t / m == t % m) ? rho : 0.0);
        __syncthreads();
        if (t == 0) {  // m x m inverse by Gauss-Jordan with partial pivoting (m <= 4), as in mpc_setup_body.h
            double a[SM][2 * SM];
            for (int i = 0; i < m; ++i)
                for (int j = 0; j < m; ++j) {
                    a[i][j] = Suu[i * m + j];
                    a[i][m + j] = (i == j) ? 1.0 : 0.0;
                }
            for (int cc = 0; cc < m; ++cc) {
                int pv = cc;
                for (int i = cc + 1; i < m; ++i)
                    if (__builtin_fabs(a[i][cc]) > __builtin_fabs(a[pv][cc])) pv = i;
                for (int j = 0; j < 2 * m; ++j) {
                    const double tmp = a[cc][j];
                    a[cc][j] = a[pv][j];
                    a[pv][j] = tmp;
                }
                const double inv = 1.0 / a[cc][cc];
                for (int j = 0; j < 2 * m; ++j) a[cc][j] *= inv;
                for (int i = 0; i < m; ++i)
                    if (i != cc) {
                        const double f = a[i][cc];
                        for (int j = 0; j < 2 * m; ++j) a[i][j] = __builtin_fma(-f, a[cc][j], a[i][j]);
                    }
            }
            for (int i = 0; i < m; ++i)
                for (int j = 0; j < m; ++j) Mi[i * m + j] = a[i][m + j];
        }
        __syncthreads();
        mm_nn(K, Mi, Sux, m, m, n);     // K_k = Suu^-1 B_k^T P A_k
        mm_tn(T1, As, PA, n, n, n);     // A_k^T P A_k
        mm_tn(T2, Sux, K, m, n, n);     // Sux^T K
        for (int e = t; e < n * n; e += blockDim.x)
            P[e] = (2.0 * Q[e] + ((e / n == e % n) ? rho : 0.0)) + T1[e] - T2[e];
        for (int e = t; e < m * n; e += blockDim.x) Kout[(long)k * m * n + e] = K[e];
        for (int e = t; e < m * m; e += blockDim.x) Minvout[(long)k * m * m + e] = Mi[e];
        __syncthreads();
    }
}

// ----------------------------------------------------------------------------------------------------------------
// solve: one lane per instance
// ----------------------------------------------------------------------------------------------------------------

// The hooks of the body (mpc_solve_lane_body.h) for the reference-tracking variant: nothing in the kernels without a reference, so
// those compile from the tokens they always had.
#define ZM_TRK_SETUP
#define ZM_TRK_FIRST
#define ZM_TRK_PREFETCH(k)
#define ZM_TRK_PX
#define ZM_TRK_QU(j)
#define ZM_TRK_ROTATE
#define ZM_TRK_ED(ed, dual)

// The shared tables are separate `const __restrict__` kernel arguments so that hipcc can prove them read-only and
// fetch them with scalar loads (wave-uniform addresses) instead of per-lane vector loads held in hundreds of VGPRs.
template <int NS, int MC>
__global__ __launch_bounds__(64) void mpc_solve_kernel(const double* __restrict__ A, const double* __restrict__ B,
                                                       const double* __restrict__ Ktab, const double* __restrict__ Mtab,
                                                       const double* __restrict__ x_lb, const double* __restrict__ x_ub,
                                                       const double* __restrict__ u_lb, const double* __restrict__ u_ub,
                                                       const MpcArgs g) {
#include "mpc_solve_lane_body.h"
}

// Per-problem data (zm_mpc_solve_batched_f64): the lane reads its problem index once, offsets its tables by it and takes the problem's
// penalty; the body is that of mpc_solve_kernel.  The tables are then per-lane vector loads instead of wave-uniform scalar loads (a
// coverage path).  A, B, the bounds: (P, ...); Ktab / Mtab: (P, n_levels, N, ...) already offset to level0 by the caller.
template <int NS, int MC>
__global__ __launch_bounds__(64) void mpc_solve_batched_kernel(const double* __restrict__ A, const double* __restrict__ B,
                                                               const double* __restrict__ Ktab, const double* __restrict__ Mtab,
                                                               const double* __restrict__ x_lb, const double* __restrict__ x_ub,
                                                               const double* __restrict__ u_lb, const double* __restrict__ u_ub,
                                                               const MpcArgs g_all, const MpcProb pb) {
    MpcArgs g = g_all;
    {
        const long inst = (long)blockIdx.x * 64 + threadIdx.x;
        if (inst >= g.batch) return;
        ZM_MPC_ENTER_PROBLEM(inst)
    }
#include "mpc_solve_lane_body.h"
}

// ----------------------------------------------------------------------------------------------------------------
// reference tracking (zm_mpc_solve_tracking_f64)
// ----------------------------------------------------------------------------------------------------------------

// The linear term of  sum_k (x_k - xr_k)' Q (x_k - xr_k) + (u_k - ur_k)' R (u_k - ur_k) + (x_N - xr_N)' Qf (x_N - xr_N)  in the stacked
// stage layout [x_{k+1} ; u_k] of the solve kernels: one thread per component,
//     g_x,k = -(W + W') xr_{k+1}   (W = Q for k < N-1, Qf for k = N-1),      g_u,k = -(R + R') ur_k.
// xr_0 only shifts the cost by a constant and is not read.  prob != NULL: instance b uses the weights of problem prob[b] (already
// checked against P on the host).  A NULL reference is zero.
__global__ __launch_bounds__(256) void mpc_track_linear_kernel(const double* __restrict__ Q, const double* __restrict__ R,
                                                               const double* __restrict__ Qf, const double* __restrict__ xRef,
                                                               const double* __restrict__ uRef, const int* __restrict__ prob,
                                                               const long batch, const int N, const int n, const int m,
                                                               double* __restrict__ g) {
    const int W = n + m;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= batch * N * W) return;
    const int i = (int)(e % W);
    const long s = e / W;
    const int k = (int)(s % N);
    const long b = s / N;
    const long p = prob ? prob[b] : 0;
    double acc = 0.0;
    if (i < n) {
        if (xRef) {
            const double* Wm = (k == N - 1 ? Qf : Q) + p * n * n;
            const double* xr = xRef + (b * (N + 1) + k + 1) * n;
            for (int j = 0; j < n; ++j) acc = __builtin_fma(Wm[i * n + j] + Wm[j * n + i], xr[j], acc);
        }
    } else if (uRef) {
        const int r = i - n;
        const double* Rm = R + p * m * m;
        const double* ur = uRef + (b * N + k) * m;
        for (int j = 0; j < m; ++j) acc = __builtin_fma(Rm[r * m + j] + Rm[j * m + r], ur[j], acc);
    }
    g[e] = -acc;
}

// The lane-per-instance body with the linear term: the lane's g_k (instance-major, as the wave kernel reads it: a coverage path) is
// fetched one stage ahead like (y, lam) and enters the costate and Qu next to -rho (y - lam); the dual tolerance scales with
// max(rho |lam|_inf, |g|_inf).  PB: per-problem data, the entry block of mpc_solve_batched_kernel.
#undef ZM_TRK_SETUP
#undef ZM_TRK_FIRST
#undef ZM_TRK_PREFETCH
#undef ZM_TRK_PX
#undef ZM_TRK_QU
#undef ZM_TRK_ROTATE
#undef ZM_TRK_ED
#define ZM_TRK_SETUP                                                                           \
    const double* gr = trk.g + ii * ((long)N * W);                                             \
    double gnorm = 0.0;                                                                        \
    for (long e = 0; e < (long)N * W; ++e) gnorm = __builtin_fmax(gnorm, __builtin_fabs(gr[e]));
#define ZM_TRK_FIRST \
    double gb[W];    \
    _Pragma("unroll") for (int i = 0; i < W; ++i) gb[i] = gr[(long)(N - 1) * W + i];
#define ZM_TRK_PREFETCH(k)                                                             \
    double gq[W];                                                                      \
    {                                                                                  \
        const int kp = k > 0 ? k - 1 : 0;                                              \
        _Pragma("unroll") for (int i = 0; i < W; ++i) gq[i] = gr[(long)kp * W + i];    \
    }
#define ZM_TRK_PX _Pragma("unroll") for (int i = 0; i < NS; ++i) p[i] += gb[i];
#define ZM_TRK_QU(j) +gb[NS + j]
#define ZM_TRK_ROTATE _Pragma("unroll") for (int i = 0; i < W; ++i) gb[i] = gq[i];
#define ZM_TRK_ED(ed, dual) \
    if (gnorm > dual) ed = g.eps_abs + g.eps_rel * gnorm;
template <int NS, int MC, bool PB>
__global__ __launch_bounds__(64) void mpc_solve_track_kernel(const double* __restrict__ A, const double* __restrict__ B,
                                                             const double* __restrict__ Ktab, const double* __restrict__ Mtab,
                                                             const double* __restrict__ x_lb, const double* __restrict__ x_ub,
                                                             const double* __restrict__ u_lb, const double* __restrict__ u_ub,
                                                             const MpcArgs g_all, const MpcProb pb, const MpcTrack trk) {
    MpcArgs g = g_all;
    if constexpr (PB) {
        const long inst = (long)blockIdx.x * 64 + threadIdx.x;
        if (inst >= g.batch) return;
        ZM_MPC_ENTER_PROBLEM(inst)
    }
#include "mpc_solve_lane_body.h"
}

// ----------------------------------------------------------------------------------------------------------------
// closed-loop run (zm_mpc_closed_loop_f64): the kernels of the host loop
// ----------------------------------------------------------------------------------------------------------------

// mpc_track_linear_kernel for a WINDOW of longer references: instance b keeps xrows rows of xRef and urows rows of uRef, and the solve of
// step `row0` tracks rows row0 .. row0 + N of xRef and row0 .. row0 + N - 1 of uRef.  The same sums in the same order, so a window gives
// the bits mpc_track_linear_kernel gives for the same rows handed to it as an (N + 1)- / N-row reference.
__global__ __launch_bounds__(256) void mpc_track_linear_window_kernel(const double* __restrict__ Q, const double* __restrict__ R,
                                                                      const double* __restrict__ Qf, const double* __restrict__ xRef,
                                                                      const double* __restrict__ uRef, const int* __restrict__ prob,
                                                                      const long batch, const int N, const int n, const int m,
                                                                      const long xrows, const long urows, const long row0,
                                                                      double* __restrict__ g) {
    const int W = n + m;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= batch * N * W) return;
    const int i = (int)(e % W);
    const long s = e / W;
    const int k = (int)(s % N);
    const long b = s / N;
    const long p = prob ? prob[b] : 0;
    double acc = 0.0;
    if (i < n) {
        if (xRef) {
            const double* Wm = (k == N - 1 ? Qf : Q) + p * n * n;
            const double* xr = xRef + (b * xrows + row0 + k + 1) * n;
            for (int j = 0; j < n; ++j) acc = __builtin_fma(Wm[i * n + j] + Wm[j * n + i], xr[j], acc);
        }
    } else if (uRef) {
        const int r = i - n;
        const double* Rm = R + p * m * m;
        const double* ur = uRef + (b * urows + row0 + k) * m;
        for (int j = 0; j < m; ++j) acc = __builtin_fma(Rm[r * m + j] + Rm[j * m + r], ur[j], acc);
    }
    g[e] = -acc;
}

// Between two solves of the host loop, one thread per (instance, component of [x ; u]):
//     state component i :  dst[b][i] = clip(src[b * src_stride + i] + dist[b][i])   into [x_lb + clip_tol, x_ub - clip_tol] of b's problem
//     control component j: udst[b][j] = usrc[b * usrc_stride + j]
// With src = row 1 of a step's rollout this is the successor state and the input applied; with src = x0 (dist, usrc NULL) the first state.
// dist NULL: nothing is added; clip_tol < 0: no clip; usrc NULL: the control threads do nothing.
__global__ __launch_bounds__(256) void mpc_advance_kernel(const double* src, const long src_stride, const double* dist, const double* x_lb,
                                                          const double* x_ub, const int* prob, const double clip_tol, double* dst,
                                                          const double* usrc, const long usrc_stride, double* udst, const long batch,
                                                          const int n, const int m) {
    const int W = n + m;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= batch * W) return;
    const int i = (int)(e % W);
    const long b = e / W;
    if (i < n) {
        double v = src[b * src_stride + i];
        if (dist) v += dist[b * n + i];
        if (clip_tol >= 0.0) {   // min(max(v, lo), hi): np.clip's order, a NaN passes through
            const long p = prob ? prob[b] : 0;
            const double lo = x_lb[p * n + i] + clip_tol, hi = x_ub[p * n + i] - clip_tol;
            v = v < lo ? lo : v;
            v = v > hi ? hi : v;
        }
        dst[b * n + i] = v;
    } else if (usrc) {
        const int j = i - n;
        udst[b * m + j] = usrc[b * usrc_stride + j];
    }
}

// ----------------------------------------------------------------------------------------------------------------
// real-time-iteration run (zm_mpc_rti_f64): the kernels between two solves (the expansion is linearize.hip's)
// ----------------------------------------------------------------------------------------------------------------

// The plant, one lane per instance: one step of the registered model from x[b] (first md.n of x_stride) under u[b] (first md.m of
// u_stride) by models.h's model_step -- the step function, not an expansion -- then mpc_advance_kernel's state rule with every instance
// its own problem:   dst[b][i] = clip(x+_i + dist[b][i])  into [x_lb[b][i] + clip_tol, x_ub[b][i] - clip_tol],  i < md.n.
// dist NULL: nothing is added; clip_tol < 0: no clip (the bounds are not read).  Components md.n .. dst_stride of dst (the padding of an
// embedded shape) are set to zero.  udst != NULL: udst[b] (mcw) = the first mcw components of u[b], the input applied.
// zm_model_step_f64 is this kernel with dist = NULL, clip_tol < 0, udst = NULL.
__global__ __launch_bounds__(64) void mpc_rti_plant_kernel(const zm_model_t md, const double* __restrict__ x, const long x_stride,
                                                           const double* __restrict__ u, const long u_stride,
                                                           const double* __restrict__ dist, const double* __restrict__ x_lb,
                                                           const double* __restrict__ x_ub, const double clip_tol,
                                                           double* __restrict__ dst, const int dst_stride, double* __restrict__ udst,
                                                           const int mcw, const long batch) {
    const long b = (long)blockIdx.x * 64 + threadIdx.x;
    if (b >= batch) return;
    const int n = md.n, m = md.m;
    double xv[MAXN], uv[MAXM], xn[MAXN];
#pragma unroll
    for (int i = 0; i < MAXN; ++i) xv[i] = (i < n) ? x[b * x_stride + i] : 0.0;
#pragma unroll
    for (int i = 0; i < MAXM; ++i) uv[i] = (i < m) ? u[b * u_stride + i] : 0.0;
    model_step<double>(md, xv, uv, xn);
#pragma unroll
    for (int i = 0; i < MAXN; ++i) {
        if (i < n) {
            double v = xn[i];
            if (dist) v += dist[b * dst_stride + i];
            if (clip_tol >= 0.0) {   // min(max(v, lo), hi): np.clip's order, a NaN passes through
                const double lo = x_lb[b * dst_stride + i] + clip_tol, hi = x_ub[b * dst_stride + i] - clip_tol;
                v = v < lo ? lo : v;
                v = v > hi ? hi : v;
            }
            dst[b * dst_stride + i] = v;
        }
    }
    for (int i = n; i < dst_stride; ++i) dst[b * dst_stride + i] = 0.0;
    if (udst)
        for (int j = 0; j < mcw; ++j) udst[b * mcw + j] = u[b * u_stride + j];
}

// The next expansion point, one thread per component: the step's rollout moved on by one stage, its last row repeated,
//     xPlan[b][k] (n) <- xTraj[b][min(k + 1, N)] (first n of ns),  k = 0 .. N;     uPlan[b][k] (m) <- uTraj[b][min(k + 1, N - 1)] (first m of mc).
// The head of the plan is the PREDICTED successor, not the measured one.
__global__ __launch_bounds__(256) void mpc_rti_shift_kernel(const double* __restrict__ xTraj, const double* __restrict__ uTraj,
                                                            double* __restrict__ xPlan, double* __restrict__ uPlan, const long batch,
                                                            const int N, const int n, const int m, const int ns, const int mc) {
    const long xper = (long)(N + 1) * n, per = xper + (long)N * m;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= batch * per) return;
    const long b = e / per;
    long r = e - b * per;
    if (r < xper) {
        const int k = (int)(r / n), i = (int)(r % n);
        const int src = k + 1 < N ? k + 1 : N;
        xPlan[b * xper + r] = xTraj[(b * (N + 1) + src) * ns + i];
    } else {
        r -= xper;
        const int k = (int)(r / m), j = (int)(r % m);
        const int src = k + 1 < N - 1 ? k + 1 : N - 1;
        uPlan[b * (long)N * m + r] = uTraj[(b * N + src) * mc + j];
    }
}

// ----------------------------------------------------------------------------------------------------------------
// host side: one shape ladder, one launcher, one routine behind the three solve entry points
// ----------------------------------------------------------------------------------------------------------------

// f(Int<NS>, Int<MC>) for the compiled shape (n, m); ZM_EUNSUPPORTED for any other
template <typename F>
static int for_mpc_shape(int n, int m, F f) {
    if (n == 24 && m == 8) return f(Int<24>{}, Int<8>{});   // beyond the 16-index tile: lane per instance, registers + scratch
    if (n == 12 && m == 4) return f(Int<12>{}, Int<4>{});
    if (n == 8 && m == 4) return f(Int<8>{}, Int<4>{});
    if (n == 4 && m == 2) return f(Int<4>{}, Int<2>{});
    if (n == 4 && m == 1) return f(Int<4>{}, Int<1>{});
    if (n == 2 && m == 2) return f(Int<2>{}, Int<2>{});
    if (n == 2 && m == 1) return f(Int<2>{}, Int<1>{});
    if (n == 1 && m == 1) return f(Int<1>{}, Int<1>{});
    return ZM_EUNSUPPORTED;
}

// pb != nullptr: per-problem data; trk != nullptr: the tracking variants
template <int NS, int MC>
static int launch_mpc(const MpcTabs& t, const MpcArgs& g, const MpcProb* pb, const MpcTrack* trk, hipStream_t st) {
    const auto go = [&](auto kernel, auto... more) -> int {
        hipLaunchKernelGGL(kernel, dim3((unsigned)((g.batch + 63) / 64)), dim3(64), 0, st, t.A, t.B, t.K, t.Minv, t.x_lb, t.x_ub, t.u_lb,
                           t.u_ub, g, more...);
        ZM_HIP_CHECK(hipGetLastError());
        return ZM_OK;
    };
    if (trk && pb) return go(mpc_solve_track_kernel<NS, MC, true>, *pb, *trk);
    if (trk) return go(mpc_solve_track_kernel<NS, MC, false>, MpcProb{}, *trk);
    return pb ? go(mpc_solve_batched_kernel<NS, MC>, *pb) : go(mpc_solve_kernel<NS, MC>);
}

// The argument checks of the solve entry points and of zm_mpc_closed_loop_f64, all before any launch.  `fn` is the entry point's name,
// the prefix of its error messages; `outputs` is false if one of the entry point's own output pointers is NULL.
static int mpc_check_args(const char* fn, bool per_problem, bool tracking, bool outputs, const double* A, const double* B, const double* Q,
                          const double* R, const double* Qf, const double* K, const double* Minv, int n_levels, int level0, double rho_step,
                          double alpha, const double* x_lb, const double* x_ub, const double* u_lb, const double* u_ub, const double* x0,
                          double rho, const double* rho_p, const int32_t* problem, int64_t P, int max_iter, const double* workspace,
                          int64_t batch, int N, int n, int m) {
    if (!(alpha > 0.0 && alpha < 2.0)) return set_error(ZM_EINVAL, "%s: alpha must lie in (0, 2)", fn);
    if (!A || !B || !K || !Minv || !x_lb || !x_ub || !u_lb || !u_ub || !x0 || !workspace || !outputs ||
        (tracking && (!Q || !R || !Qf)) || (per_problem && (!rho_p || !problem)))
        return set_error(ZM_EINVAL, "%s: null pointer", fn);
    if ((problem == nullptr) != (rho_p == nullptr))
        return set_error(ZM_EINVAL, "%s: the problem map and the per-problem rho come together", fn);
    if (batch < 0 || N < 1 || max_iter < 0 || (tracking && (n < 1 || m < 1)) || (problem ? P < 1 : !(rho > 0.0)))
        return set_error(ZM_EINVAL, tracking ? "%s: bad size / rho" : "%s: bad size", fn);
    if (n_levels < 1 || level0 < 0 || level0 >= n_levels || (n_levels > 1 && !(rho_step > 1.0)))
        return set_error(ZM_EINVAL, "%s: bad penalty levels", fn);
    const long blocks = ((long)batch * N * ((long)n + m) + 255) / 256;   // of mpc_track_linear_kernel
    if (tracking && blocks > 0x7fffffffL) return set_error(ZM_EINVAL, "%s: batch x N x (n + m) too large", fn);
    return ZM_OK;
}

// every instance's problem index must lie in [0, P): the kernels offset every table by it, so it is checked here, on the host,
// before anything is launched (one small copy of the index map; the solve's own results come back through a sync anyway)
static int mpc_check_map(const char* fn, const int32_t* problem, int64_t P, int64_t batch, hipStream_t st) {
    if (!problem) return ZM_OK;
    static thread_local std::vector<int32_t> h;
    h.resize((size_t)batch);
    ZM_HIP_CHECK(hipMemcpyAsync(h.data(), problem, (size_t)batch * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    ZM_HIP_CHECK(hipStreamSynchronize(st));
    for (int64_t i = 0; i < batch; ++i)
        if (h[i] < 0 || h[i] >= P)
            return set_error(ZM_EINVAL, "%s: instance %lld maps to problem %d outside [0, %lld)", fn, (long long)i, (int)h[i], (long long)P);
    return ZM_OK;
}

// ZOPT_AMD_MPC_PATH=lane forces the lane-per-instance kernels (read once per process)
static bool mpc_force_lane() {
    static const bool force_lane = [] {
        const char* e = fallback_env("ZOPT_AMD_MPC_PATH");
        return e && e[0] == 'l';
    }();
    return force_lane;
}

// One solve launch.  Default: 16 lanes per instance with the iterates in LDS (mpc_wave.hip); ZOPT_AMD_MPC_PATH=lane forces the
// lane-per-instance kernel below, which also takes the shapes and the horizons that do not fit LDS.  It runs every problem at its
// level0 table (fixed penalty).  `t` holds the whole tables (every level).
static int mpc_enqueue(const char* fn, MpcTabs t, const MpcArgs& g, const MpcProb* pb, const MpcTrack* trk, int n, int m, hipStream_t st) {
    if (!mpc_force_lane()) {
        const int rc = mpc_wave_dispatch(t, g, pb, trk, n, m, st);
        if (rc != ZM_EUNSUPPORTED) return rc;
    }
    t.K += (long)g.level0 * g.N * m * n;        // (+ p * n_levels * N * m * n in the kernel)
    t.Minv += (long)g.level0 * g.N * m * m;
    const int rc = for_mpc_shape(n, m, [&](auto ns, auto mc) { return launch_mpc<ns.value, mc.value>(t, g, pb, trk, st); });
    if (rc == ZM_EUNSUPPORTED) return set_error(ZM_EUNSUPPORTED, "%s: (n=%d, m=%d) not among the compiled shapes", fn, n, m);
    return rc;
}

// The three solve entry points.  `fn` is the entry point's name, the prefix of its error messages.
//   zm_mpc_solve_relaxed_f64 : one problem, scalar rho                          (problem, rho_p, Q, R, Qf, xRef, uRef NULL)
//   zm_mpc_solve_batched_f64 : per_problem -- problem and rho_p are required    (Q, R, Qf, xRef, uRef NULL)
//   zm_mpc_solve_tracking_f64: tracking -- Q, R, Qf are required, n and m are checked, the linear term is formed first; problem and
//                              rho_p come together or not at all
static int mpc_solve(const char* fn, bool per_problem, bool tracking, const double* A, const double* B, const double* Q, const double* R,
                     const double* Qf, const double* K, const double* Minv, int n_levels, int level0, double rho_step, double alpha,
                     const double* x_lb, const double* x_ub, const double* u_lb, const double* u_ub, const double* x0,
                     const double* xRef, const double* uRef, double rho, const double* rho_p, const int32_t* problem, int64_t P,
                     double eps_abs, double eps_rel, double eps_prim_inf, int max_iter, int warm_start, double* workspace, double* xTraj,
                     double* uTraj, int32_t* status, int32_t* iters, double* resid, int64_t batch, int N, int n, int m, void* stream) {
    if (batch == 0) return ZM_OK;   /* empty batch: nothing to do (pointers of empty arrays may be NULL) */
    int rc = mpc_check_args(fn, per_problem, tracking, xTraj && uTraj && status, A, B, Q, R, Qf, K, Minv, n_levels, level0, rho_step, alpha,
                            x_lb, x_ub, u_lb, u_ub, x0, rho, rho_p, problem, P, max_iter, workspace, batch, N, n, m);
    if (rc != ZM_OK) return rc;
    const long W = (long)n + m;
    hipStream_t st = (hipStream_t)stream;
    rc = mpc_check_map(fn, problem, P, batch, st);
    if (rc != ZM_OK) return rc;
    // tracking: the fifth block of the workspace holds the linear term g (batch, N, n + m)
    double* gbuf = tracking ? workspace + 4L * batch * N * W : nullptr;
    if (tracking) {
        const long blocks = ((long)batch * N * W + 255) / 256;
        hipLaunchKernelGGL(mpc_track_linear_kernel, dim3((unsigned)blocks), dim3(256), 0, st, Q, R, Qf, xRef, uRef, (const int*)problem,
                           (long)batch, N, n, m, gbuf);
        ZM_HIP_CHECK(hipGetLastError());
    }
    const MpcTabs t{A, B, K, Minv, x_lb, x_ub, u_lb, u_ub};
    // with per-problem data g.rho is unused (each instance takes its problem's pb.rho[p]); 1.0 keeps the struct well-formed
    const MpcArgs g{x0, problem ? 1.0 : rho, eps_abs, eps_rel, eps_prim_inf, max_iter, warm_start == 2 ? 2 : (warm_start ? 1 : 0), workspace,
                    xTraj, uTraj, (int*)status, (int*)iters, resid, (long)batch, N, n_levels, level0, rho_step, alpha};
    const MpcProb pbv{(const int*)problem, rho_p};
    const MpcTrack trkv{gbuf};
    return mpc_enqueue(fn, t, g, problem ? &pbv : nullptr, tracking ? &trkv : nullptr, n, m, st);
}

// zm_mpc_closed_loop_f64: `steps` receding-horizon solves of every instance, nothing but launches on `st` after the argument checks.
//   (a) regulator runs at the shapes and horizons of the 16-lanes-per-instance kernels: ONE launch, the step loop inside the kernel
//       (mpc_wave.hip: mpc_closed_loop_wave_kernel);
//   (b) everything else -- tracking, (24, 8), horizons beyond LDS, ZOPT_AMD_MPC_PATH=lane: a loop that enqueues, per step, the launches
//       of a single solve and mpc_advance_kernel, with no host synchronisation in between.
static int mpc_closed_loop(const char* fn, const double* A, const double* B, const double* Q, const double* R, const double* Qf,
                           const double* K, const double* Minv, int n_levels, int level0, double rho_step, double alpha, const double* x_lb,
                           const double* x_ub, const double* u_lb, const double* u_ub, const double* x0, const double* xRef,
                           const double* uRef, int xref_rows, int uref_rows, double rho, const double* rho_p, const int32_t* problem,
                           int64_t P, double eps_abs, double eps_rel, double eps_prim_inf, int max_iter, int warm_start, int steps,
                           double clip_tol, const double* disturbance, double* workspace, double* states, double* inputs, int32_t* status,
                           int32_t* iters, double* xPred, double* uPred, int64_t batch, int N, int n, int m, void* stream) {
    if (batch == 0) return ZM_OK;   /* empty batch: nothing to do (pointers of empty arrays may be NULL) */
    const bool tracking = xRef || uRef;
    int rc = mpc_check_args(fn, false, tracking, states && inputs && status && iters, A, B, Q, R, Qf, K, Minv, n_levels, level0, rho_step,
                            alpha, x_lb, x_ub, u_lb, u_ub, x0, rho, rho_p, problem, P, max_iter, workspace, batch, N, n, m);
    if (rc != ZM_OK) return rc;
    if (steps < 1) return set_error(ZM_EINVAL, "%s: steps must be at least 1", fn);
    if (n < 1 || m < 1) return set_error(ZM_EINVAL, "%s: bad size", fn);
    if ((xPred == nullptr) != (uPred == nullptr)) return set_error(ZM_EINVAL, "%s: the two prediction arrays come together", fn);
    if ((xRef && xref_rows != steps + N) || (uRef && uref_rows != steps + N - 1))
        return set_error(ZM_EINVAL, "%s: a reference needs steps + N rows of xRef and steps + N - 1 rows of uRef", fn);
    const long W = (long)n + m;
    const long ablocks = ((long)batch * W + 255) / 256;           // of mpc_advance_kernel
    const long gblocks = ((long)batch * N * W + 255) / 256;       // of mpc_track_linear_window_kernel
    if (ablocks > 0x7fffffffL) return set_error(ZM_EINVAL, "%s: batch x (n + m) too large", fn);
    hipStream_t st = (hipStream_t)stream;
    rc = mpc_check_map(fn, problem, P, batch, st);
    if (rc != ZM_OK) return rc;

    // workspace: the blocks of a solve (the fifth: the linear term of a tracking step), then -- unless the predictions are kept -- the
    // rollout every step overwrites
    double* gbuf = tracking ? workspace + 4L * batch * N * W : nullptr;
    double* scratch = workspace + (tracking ? 5L : 4L) * batch * N * W;
    const long xsz = (long)batch * (N + 1) * n, usz = (long)batch * N * m;
    const MpcLoop lp{steps, warm_start == 2 ? 2 : (warm_start ? 1 : 0), clip_tol, x0, disturbance, states, inputs, (int*)status, (int*)iters,
                     xPred ? xPred : scratch, uPred ? uPred : scratch + xsz, xPred ? xsz : 0, uPred ? usz : 0};
    const MpcTabs t{A, B, K, Minv, x_lb, x_ub, u_lb, u_ub};
    const MpcArgs g{x0, problem ? 1.0 : rho, eps_abs, eps_rel, eps_prim_inf, max_iter, 0, workspace, lp.xPred, lp.uPred, lp.status, lp.iters,
                    nullptr, (long)batch, N, n_levels, level0, rho_step, alpha};
    const MpcProb pbv{(const int*)problem, rho_p};
    const MpcProb* pb = problem ? &pbv : nullptr;
    if (!tracking && !mpc_force_lane()) {
        rc = mpc_wave_closed_loop_dispatch(t, g, pb, lp, n, m, st);
        if (rc != ZM_EUNSUPPORTED) return rc;
    }
    const MpcTrack trkv{gbuf};
    const auto advance = [&](const double* src, long src_stride, const double* dist, double* dst, const double* usrc, double* udst) -> int {
        hipLaunchKernelGGL(mpc_advance_kernel, dim3((unsigned)ablocks), dim3(256), 0, st, src, src_stride, dist, x_lb, x_ub,
                           (const int*)problem, clip_tol, dst, usrc, (long)N * m, udst, (long)batch, n, m);
        ZM_HIP_CHECK(hipGetLastError());
        return ZM_OK;
    };
    rc = advance(x0, n, nullptr, states, nullptr, nullptr);
    for (int s = 0; s < steps && rc == ZM_OK; ++s) {
        if (tracking) {
            hipLaunchKernelGGL(mpc_track_linear_window_kernel, dim3((unsigned)gblocks), dim3(256), 0, st, Q, R, Qf, xRef, uRef,
                               (const int*)problem, (long)batch, N, n, m, (long)xref_rows, (long)uref_rows, (long)s, gbuf);
            ZM_HIP_CHECK(hipGetLastError());
        }
        MpcArgs gs = g;
        gs.x0 = states + (long)s * batch * n;
        gs.xTraj = lp.xPred + s * lp.xpred_step;
        gs.uTraj = lp.uPred + s * lp.upred_step;
        gs.status = lp.status + (long)s * batch;
        gs.iters = lp.iters + (long)s * batch;
        gs.warm = s ? lp.warm : 0;
        rc = mpc_enqueue(fn, t, gs, pb, tracking ? &trkv : nullptr, n, m, st);
        if (rc != ZM_OK) break;
        rc = advance(gs.xTraj + n, (long)(N + 1) * n, disturbance ? disturbance + (long)s * batch * n : nullptr,
                     states + (long)(s + 1) * batch * n, gs.uTraj, inputs + (long)s * batch * m);
    }
    return rc;
}

// The models of the real-time-iteration entry points: a registered model of exactly (n, m); the quadcopters as a discrete step (dt > 0)
static int mpc_rti_check_model(const char* fn, const char* what, const zm_model_t* model, zm_model_t& md, int n, int m) {
    const int rc = check_model(model, md, fn);
    if (rc != ZM_OK) return rc;
    if (md.n != n || md.m != m)
        return set_error(ZM_EINVAL, "%s: the %s has (n=%d, m=%d), the problem (n=%d, m=%d)", fn, what, md.n, md.m, n, m);
    if (md.kind != ZM_MODEL_LINEAR && !(md.dt > 0.0)) return set_error(ZM_EINVAL, "%s: the %s needs a step dt > 0", fn, what);
    return ZM_OK;
}

// the shapes and horizons of the one kernel for stage-varying dynamics (mpc_wave.hip: mpc_wave_ltv_dispatch), refused before any launch
static int mpc_ltv_check_shape(const char* fn, int N, int n, int m) {
    if (for_mpc_shape(n, m, [](auto ns, auto mc) { return ns.value + mc.value <= 16 ? ZM_OK : ZM_EUNSUPPORTED; }) != ZM_OK)
        return set_error(ZM_EUNSUPPORTED, "%s: (n=%d, m=%d) not among the shapes of the 16-lanes-per-instance kernels", fn, n, m);
    if ((size_t)4 * N * 64 * sizeof(double) > 150 * 1024)
        return set_error(ZM_EUNSUPPORTED, "%s: N=%d beyond the horizons whose iterates fit LDS (N <= 75)", fn, N);
    return ZM_OK;
}

static int mpc_relinearize(const char* fn, const zm_model_t* model, const double* xPlan, const double* uPlan, double* A, double* B,
                           double* c, int64_t batch, int N, int n_user, int m_user, int ns, int mc, void* stream) {
    if (batch == 0) return ZM_OK;   /* empty batch: nothing to do (pointers of empty arrays may be NULL) */
    if (!xPlan || !uPlan || !A || !B || !c) return set_error(ZM_EINVAL, "%s: null pointer", fn);
    if (batch < 0 || N < 1 || n_user < 1 || m_user < 1 || ns < n_user || mc < m_user) return set_error(ZM_EINVAL, "%s: bad size", fn);
    if (ns > SN || mc > SM) return set_error(ZM_EUNSUPPORTED, "%s: (n=%d, m=%d) not covered (n <= 12, m <= 4)", fn, ns, mc);
    if (((long)batch * N + 15) / 16 > 0x7fffffffL) return set_error(ZM_EINVAL, "%s: batch x N too large", fn);
    zm_model_t md;
    const int rc = mpc_rti_check_model(fn, "model", model, md, n_user, m_user);
    if (rc != ZM_OK) return rc;
    return mpc_relinearize_enqueue(md, xPlan, uPlan, A, B, c, (long)batch, N, ns, mc, (hipStream_t)stream);
}

// zm_mpc_rti_f64: `steps` real-time iterations of every instance, nothing but launches on `st` after the argument checks and the one
// read-back of the problem map -- mpc_closed_loop's form (b) with the expansion and the table setup inside the loop:
//     relinearise about the plan -> mpc_setup_ltv_kernel -> mpc_track_linear_window_kernel -> the LTV solve -> plant step, plan shift
static int mpc_rti(const char* fn, const zm_model_t* model, const zm_model_t* plant, double* xPlan, double* uPlan, double* A, double* B,
                   double* c, const double* Q, const double* R, const double* Qf, const double* rho_tab, double* K, double* Minv, double* D,
                   double* ABt, int n_levels, int level0, double rho_step, double alpha, const double* x_lb, const double* x_ub,
                   const double* u_lb, const double* u_ub, const double* x0, const double* xRef, const double* uRef, int xref_rows,
                   int uref_rows, const double* rho_p, const int32_t* problem, double eps_abs, double eps_rel, double eps_prim_inf,
                   int max_iter, int warm_start, int steps, double clip_tol, const double* disturbance, double* workspace, double* states,
                   double* inputs, int32_t* status, int32_t* iters, double* resid, double* xPred, double* uPred, int64_t batch, int N,
                   int n_user, int m_user, int n, int m, void* stream) {
    if (batch == 0) return ZM_OK;   /* empty batch: nothing to do (pointers of empty arrays may be NULL) */
    int rc = mpc_check_args(fn, true, true, states && inputs && status && iters && xPlan && uPlan && c && D && ABt && rho_tab, A, B, Q, R,
                            Qf, K, Minv, n_levels, level0, rho_step, alpha, x_lb, x_ub, u_lb, u_ub, x0, 0.0, rho_p, problem, batch,
                            max_iter, workspace, batch, N, n, m);
    if (rc != ZM_OK) return rc;
    if (steps < 1) return set_error(ZM_EINVAL, "%s: steps must be at least 1", fn);
    if (n_user < 1 || m_user < 1 || n_user > n || m_user > m) return set_error(ZM_EINVAL, "%s: bad size", fn);
    if ((xPred == nullptr) != (uPred == nullptr)) return set_error(ZM_EINVAL, "%s: the two prediction arrays come together", fn);
    if ((xRef && xref_rows != steps + N) || (uRef && uref_rows != steps + N - 1))
        return set_error(ZM_EINVAL, "%s: a reference needs steps + N rows of xRef and steps + N - 1 rows of uRef", fn);
    if ((rc = mpc_ltv_check_shape(fn, N, n, m)) != ZM_OK) return rc;
    zm_model_t md, pl;
    if ((rc = mpc_rti_check_model(fn, "model", model, md, n_user, m_user)) != ZM_OK) return rc;
    if ((rc = mpc_rti_check_model(fn, "plant", plant ? plant : model, pl, n_user, m_user)) != ZM_OK) return rc;
    const long W = (long)n + m;
    const long ablocks = ((long)batch * W + 255) / 256;                                         // of mpc_advance_kernel
    const long gblocks = ((long)batch * N * W + 255) / 256;                                     // of mpc_track_linear_window_kernel
    const long sblocks = ((long)batch * ((long)(N + 1) * n_user + (long)N * m_user) + 255) / 256;   // of mpc_rti_shift_kernel
    if (gblocks > 0x7fffffffL || sblocks > 0x7fffffffL || (long)batch * n_levels > 0x7fffffffL)
        return set_error(ZM_EINVAL, "%s: batch x N x (n + m) too large", fn);
    hipStream_t st = (hipStream_t)stream;
    {   // every instance is its own problem: the map must be the identity (one small copy, as mpc_check_map's)
        static thread_local std::vector<int32_t> h;
        h.resize((size_t)batch);
        ZM_HIP_CHECK(hipMemcpyAsync(h.data(), problem, (size_t)batch * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        ZM_HIP_CHECK(hipStreamSynchronize(st));
        for (int64_t i = 0; i < batch; ++i)
            if (h[i] != (int32_t)i)
                return set_error(ZM_EINVAL, "%s: instance %lld maps to problem %d; every instance is its own problem here", fn, (long long)i,
                                 (int)h[i]);
    }

    // workspace: the five blocks of a tracking solve, then -- unless the predictions are kept -- the rollout every step overwrites
    double* gbuf = workspace + 4L * batch * N * W;
    double* scratch = workspace + 5L * batch * N * W;
    const long xsz = (long)batch * (N + 1) * n, usz = (long)batch * N * m;
    const long xstep = xPred ? xsz : 0, ustep = uPred ? usz : 0;
    double* xroll = xPred ? xPred : scratch;
    double* uroll = uPred ? uPred : scratch + xsz;
    const MpcTabs t{A, B, K, Minv, x_lb, x_ub, u_lb, u_ub};
    const MpcArgs g{x0, 1.0, eps_abs, eps_rel, eps_prim_inf, max_iter, 0, workspace, xroll, uroll, (int*)status, (int*)iters, resid, (long)batch,
                    N, n_levels, level0, rho_step, alpha};
    const MpcProb pb{(const int*)problem, rho_p};
    const int warm = warm_start == 2 ? 2 : (warm_start ? 1 : 0);
    hipLaunchKernelGGL(mpc_advance_kernel, dim3((unsigned)ablocks), dim3(256), 0, st, x0, (long)n, (const double*)nullptr, x_lb, x_ub,
                       (const int*)problem, clip_tol, states, (const double*)nullptr, 0L, (double*)nullptr, (long)batch, n, m);
    ZM_HIP_CHECK(hipGetLastError());
    for (int s = 0; s < steps; ++s) {
        if ((rc = mpc_relinearize_enqueue(md, xPlan, uPlan, A, B, c, (long)batch, N, n, m, st)) != ZM_OK) return rc;
        hipLaunchKernelGGL((mpc_setup_ltv_kernel<SN, SM>), dim3((unsigned)(batch * n_levels)), dim3(256), 0, st, A, B, c, Q, R, Qf, rho_tab,
                           n_levels, N, n, m, K, Minv, D, ABt);
        ZM_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(mpc_track_linear_window_kernel, dim3((unsigned)gblocks), dim3(256), 0, st, Q, R, Qf, xRef, uRef, (const int*)problem,
                           (long)batch, N, n, m, (long)xref_rows, (long)uref_rows, (long)s, gbuf);
        ZM_HIP_CHECK(hipGetLastError());
        MpcArgs gs = g;
        gs.x0 = states + (long)s * batch * n;
        gs.xTraj = xroll + s * xstep;
        gs.uTraj = uroll + s * ustep;
        gs.status = g.status + (long)s * batch;
        gs.iters = g.iters + (long)s * batch;
        gs.warm = s ? warm : 0;
        rc = mpc_wave_ltv_dispatch(t, gs, pb, MpcTrack{gbuf}, MpcLtv{c, D, ABt}, n, m, st);
        if (rc == ZM_EUNSUPPORTED) return set_error(ZM_EUNSUPPORTED, "%s: (n=%d, m=%d) not among the shapes of the 16-lanes-per-instance kernels", fn, n, m);
        if (rc != ZM_OK) return rc;
        hipLaunchKernelGGL(mpc_rti_plant_kernel, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, st, pl, gs.x0, (long)n, gs.uTraj,
                           (long)N * m, disturbance ? disturbance + (long)s * batch * n : nullptr, x_lb, x_ub, clip_tol,
                           states + (long)(s + 1) * batch * n, n, inputs + (long)s * batch * m, m, (long)batch);
        ZM_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(mpc_rti_shift_kernel, dim3((unsigned)sblocks), dim3(256), 0, st, gs.xTraj, gs.uTraj, xPlan, uPlan, (long)batch, N,
                           n_user, m_user, n, m);
        ZM_HIP_CHECK(hipGetLastError());
    }
    return ZM_OK;
}

}  // namespace zm

extern "C" int zm_mpc_setup_f64(const double* A, const double* B, const double* Q, const double* R, const double* Qf,
                                double rho, int N, int n, int m, double* K, double* Minv, void* stream) {
    if (!A || !B || !Q || !R || !Qf || !K || !Minv) return zm::set_error(ZM_EINVAL, "zm_mpc_setup_f64: null pointer");
    if (N < 1 || n < 1 || m < 1 || !(rho > 0.0)) return zm::set_error(ZM_EINVAL, "zm_mpc_setup_f64: bad size / rho");
    if (n > zm::SNL || m > zm::SML) return zm::set_error(ZM_EUNSUPPORTED, "zm_mpc_setup_f64: (n=%d, m=%d) not covered (n <= 24, m <= 8)", n, m);
    if (n <= zm::SN && m <= zm::SM)
        hipLaunchKernelGGL((zm::mpc_setup_kernel<zm::SN, zm::SM>), dim3(1), dim3(256), 0, (hipStream_t)stream, A, B, Q, R, Qf, rho, N, n,
                           m, K, Minv);
    else
        hipLaunchKernelGGL((zm::mpc_setup_kernel<zm::SNL, zm::SML>), dim3(1), dim3(256), 0, (hipStream_t)stream, A, B, Q, R, Qf, rho, N, n,
                           m, K, Minv);
    ZM_HIP_CHECK(hipGetLastError());
    return ZM_OK;
}

extern "C" int zm_mpc_solve_f64(const double* A, const double* B, const double* K, const double* Minv,
                                const double* x_lb, const double* x_ub, const double* u_lb, const double* u_ub,
                                const double* x0, double rho, double eps_abs, double eps_rel, double eps_prim_inf,
                                int max_iter, double* workspace, double* xTraj, double* uTraj, int32_t* status, int32_t* iters,
                                double* resid, int64_t batch, int N, int n, int m, void* stream) {
    if (batch == 0) return ZM_OK;   /* empty batch: nothing to do (pointers of empty arrays may be NULL) */
    return zm_mpc_solve_warm_f64(A, B, K, Minv, x_lb, x_ub, u_lb, u_ub, x0, rho, eps_abs, eps_rel, eps_prim_inf, max_iter, 0,
                                 workspace, xTraj, uTraj, status, iters, resid, batch, N, n, m, stream);
}

extern "C" int zm_mpc_solve_warm_f64(const double* A, const double* B, const double* K, const double* Minv,
                                     const double* x_lb, const double* x_ub, const double* u_lb, const double* u_ub,
                                     const double* x0, double rho, double eps_abs, double eps_rel, double eps_prim_inf,
                                     int max_iter, int warm_start, double* workspace, double* xTraj, double* uTraj,
                                     int32_t* status, int32_t* iters, double* resid, int64_t batch, int N, int n, int m,
                                     void* stream) {
    return zm_mpc_solve_adaptive_f64(A, B, K, Minv, 1, 0, 1.0, x_lb, x_ub, u_lb, u_ub, x0, rho, eps_abs, eps_rel, eps_prim_inf,
                                     max_iter, warm_start, workspace, xTraj, uTraj, status, iters, resid, batch, N, n, m, stream);
}

extern "C" int zm_mpc_solve_adaptive_f64(const double* A, const double* B, const double* K, const double* Minv, int n_levels,
                                         int level0, double rho_step, const double* x_lb, const double* x_ub,
                                         const double* u_lb, const double* u_ub, const double* x0, double rho, double eps_abs,
                                         double eps_rel, double eps_prim_inf, int max_iter, int warm_start, double* workspace,
                                         double* xTraj, double* uTraj, int32_t* status, int32_t* iters, double* resid,
                                         int64_t batch, int N, int n, int m, void* stream) {
    return zm_mpc_solve_relaxed_f64(A, B, K, Minv, n_levels, level0, rho_step, 1.0, x_lb, x_ub, u_lb, u_ub, x0, rho, eps_abs, eps_rel,
                                    eps_prim_inf, max_iter, warm_start, workspace, xTraj, uTraj, status, iters, resid, batch, N, n, m,
                                    stream);
}

extern "C" int zm_mpc_solve_relaxed_f64(const double* A, const double* B, const double* K, const double* Minv, int n_levels,
                                        int level0, double rho_step, double alpha, const double* x_lb, const double* x_ub,
                                        const double* u_lb, const double* u_ub, const double* x0, double rho, double eps_abs,
                                        double eps_rel, double eps_prim_inf, int max_iter, int warm_start, double* workspace,
                                        double* xTraj, double* uTraj, int32_t* status, int32_t* iters, double* resid,
                                        int64_t batch, int N, int n, int m, void* stream) {
    return zm::mpc_solve("zm_mpc_solve_relaxed_f64", false, false, A, B, nullptr, nullptr, nullptr, K, Minv, n_levels, level0, rho_step,
                         alpha, x_lb, x_ub, u_lb, u_ub, x0, nullptr, nullptr, rho, nullptr, nullptr, 0, eps_abs, eps_rel, eps_prim_inf,
                         max_iter, warm_start, workspace, xTraj, uTraj, status, iters, resid, batch, N, n, m, stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// per-problem data: P problems (A, B, Q, R, Qf, bounds, rho each with a leading P axis) solved in one launch
// ---------------------------------------------------------------------------------------------------------------------

extern "C" int zm_mpc_setup_batched_f64(const double* A, const double* B, const double* Q, const double* R, const double* Qf,
                                        const double* rho, int64_t P, int L, int N, int n, int m, double* K, double* Minv,
                                        void* stream) {
    if (P == 0) return ZM_OK;   /* no problems: nothing to do (pointers of empty arrays may be NULL) */
    if (!A || !B || !Q || !R || !Qf || !rho || !K || !Minv) return zm::set_error(ZM_EINVAL, "zm_mpc_setup_batched_f64: null pointer");
    if (P < 0 || L < 1 || N < 1 || n < 1 || m < 1 || P * L > 0x7fffffffL)
        return zm::set_error(ZM_EINVAL, "zm_mpc_setup_batched_f64: bad size");
    if (n > zm::SNL || m > zm::SML)
        return zm::set_error(ZM_EUNSUPPORTED, "zm_mpc_setup_batched_f64: (n=%d, m=%d) not covered (n <= 24, m <= 8)", n, m);
    const dim3 grid((unsigned)(P * L));
    if (n <= zm::SN && m <= zm::SM)
        hipLaunchKernelGGL((zm::mpc_setup_batched_kernel<zm::SN, zm::SM>), grid, dim3(256), 0, (hipStream_t)stream, A, B, Q, R, Qf,
                           rho, L, N, n, m, K, Minv);
    else
        hipLaunchKernelGGL((zm::mpc_setup_batched_kernel<zm::SNL, zm::SML>), grid, dim3(256), 0, (hipStream_t)stream, A, B, Q, R, Qf,
                           rho, L, N, n, m, K, Minv);
    ZM_HIP_CHECK(hipGetLastError());
    return ZM_OK;
}

extern "C" int zm_mpc_solve_batched_f64(const double* A, const double* B, const double* K, const double* Minv, int n_levels,
                                        int level0, double rho_step, double alpha, const double* x_lb, const double* x_ub,
                                        const double* u_lb, const double* u_ub, const double* x0, const double* rho,
                                        const int32_t* problem, int64_t P, double eps_abs, double eps_rel, double eps_prim_inf,
                                        int max_iter, int warm_start, double* workspace, double* xTraj, double* uTraj,
                                        int32_t* status, int32_t* iters, double* resid, int64_t batch, int N, int n, int m,
                                        void* stream) {
    return zm::mpc_solve("zm_mpc_solve_batched_f64", true, false, A, B, nullptr, nullptr, nullptr, K, Minv, n_levels, level0, rho_step,
                         alpha, x_lb, x_ub, u_lb, u_ub, x0, nullptr, nullptr, 0.0, rho, problem, P, eps_abs, eps_rel, eps_prim_inf,
                         max_iter, warm_start, workspace, xTraj, uTraj, status, iters, resid, batch, N, n, m, stream);
}

// reference tracking: xRef, uRef -> g (mpc_track_linear_kernel), then the tracking variants of the solve kernels
extern "C" int zm_mpc_solve_tracking_f64(const double* A, const double* B, const double* Q, const double* R, const double* Qf,
                                         const double* K, const double* Minv, int n_levels, int level0, double rho_step, double alpha,
                                         const double* x_lb, const double* x_ub, const double* u_lb, const double* u_ub,
                                         const double* x0, const double* xRef, const double* uRef, double rho,
                                         const double* rho_p, const int32_t* problem, int64_t P, double eps_abs, double eps_rel,
                                         double eps_prim_inf, int max_iter, int warm_start, double* workspace, double* xTraj,
                                         double* uTraj, int32_t* status, int32_t* iters, double* resid, int64_t batch, int N, int n,
                                         int m, void* stream) {
    return zm::mpc_solve("zm_mpc_solve_tracking_f64", false, true, A, B, Q, R, Qf, K, Minv, n_levels, level0, rho_step, alpha, x_lb,
                         x_ub, u_lb, u_ub, x0, xRef, uRef, rho, rho_p, problem, P, eps_abs, eps_rel, eps_prim_inf, max_iter, warm_start,
                         workspace, xTraj, uTraj, status, iters, resid, batch, N, n, m, stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// stage-varying dynamics: x+ = A_k x + B_k u + c_k per problem (16 lanes per instance only)
// ---------------------------------------------------------------------------------------------------------------------

extern "C" int zm_mpc_setup_ltv_f64(const double* A, const double* B, const double* c, const double* Q, const double* R, const double* Qf,
                                    const double* rho, int64_t P, int L, int N, int n, int m, double* K, double* Minv, double* D,
                                    double* ABt, void* stream) {
    if (P == 0) return ZM_OK;   /* no problems: nothing to do (pointers of empty arrays may be NULL) */
    if (!A || !B || !Q || !R || !Qf || !rho || !K || !Minv || !D || !ABt) return zm::set_error(ZM_EINVAL, "zm_mpc_setup_ltv_f64: null pointer");
    if (P < 0 || L < 1 || N < 1 || n < 1 || m < 1 || P * L > 0x7fffffffL) return zm::set_error(ZM_EINVAL, "zm_mpc_setup_ltv_f64: bad size");
    if (n > zm::SN || m > zm::SM)
        return zm::set_error(ZM_EUNSUPPORTED, "zm_mpc_setup_ltv_f64: (n=%d, m=%d) not covered (n <= 12, m <= 4)", n, m);
    hipLaunchKernelGGL((zm::mpc_setup_ltv_kernel<zm::SN, zm::SM>), dim3((unsigned)(P * L)), dim3(256), 0, (hipStream_t)stream, A, B, c, Q, R,
                       Qf, rho, L, N, n, m, K, Minv, D, ABt);
    ZM_HIP_CHECK(hipGetLastError());
    return ZM_OK;
}

extern "C" int zm_mpc_solve_ltv_f64(const double* A, const double* B, const double* c, const double* ABt, const double* Q, const double* R,
                                    const double* Qf, const double* K, const double* Minv, const double* D, int n_levels, int level0,
                                    double rho_step, double alpha, const double* x_lb, const double* x_ub, const double* u_lb,
                                    const double* u_ub, const double* x0, const double* xRef, const double* uRef, const double* rho_p,
                                    const int32_t* problem, int64_t P, double eps_abs, double eps_rel, double eps_prim_inf, int max_iter,
                                    int warm_start, double* workspace, double* xTraj, double* uTraj, int32_t* status, int32_t* iters,
                                    double* resid, int64_t batch, int N, int n, int m, void* stream) {
    const char* fn = "zm_mpc_solve_ltv_f64";
    if (batch == 0) return ZM_OK;   /* empty batch: nothing to do (pointers of empty arrays may be NULL) */
    int rc = zm::mpc_check_args(fn, true, true, xTraj && uTraj && status && c && D && ABt, A, B, Q, R, Qf, K, Minv, n_levels, level0, rho_step,
                                alpha, x_lb, x_ub, u_lb, u_ub, x0, 0.0, rho_p, problem, P, max_iter, workspace, batch, N, n, m);
    if (rc != ZM_OK) return rc;
    // the one kernel there is: refuse what it does not take before anything is launched
    if (zm::for_mpc_shape(n, m, [](auto ns, auto mc) { return ns.value + mc.value <= 16 ? ZM_OK : ZM_EUNSUPPORTED; }) != ZM_OK)
        return zm::set_error(ZM_EUNSUPPORTED, "%s: (n=%d, m=%d) not among the shapes of the 16-lanes-per-instance kernels", fn, n, m);
    if ((size_t)4 * N * 64 * sizeof(double) > 150 * 1024)
        return zm::set_error(ZM_EUNSUPPORTED, "%s: N=%d beyond the horizons whose iterates fit LDS (N <= 75)", fn, N);
    hipStream_t st = (hipStream_t)stream;
    rc = zm::mpc_check_map(fn, problem, P, batch, st);
    if (rc != ZM_OK) return rc;
    const long W = (long)n + m;
    // the fifth block of the workspace holds the linear term g (batch, N, n + m): a zero block without a reference
    double* gbuf = workspace + 4L * batch * N * W;
    const long blocks = ((long)batch * N * W + 255) / 256;
    hipLaunchKernelGGL(zm::mpc_track_linear_kernel, dim3((unsigned)blocks), dim3(256), 0, st, Q, R, Qf, xRef, uRef, (const int*)problem,
                       (long)batch, N, n, m, gbuf);
    ZM_HIP_CHECK(hipGetLastError());
    const zm::MpcTabs t{A, B, K, Minv, x_lb, x_ub, u_lb, u_ub};
    const zm::MpcArgs g{x0, 1.0, eps_abs, eps_rel, eps_prim_inf, max_iter, warm_start == 2 ? 2 : (warm_start ? 1 : 0), workspace, xTraj, uTraj,
                        (int*)status, (int*)iters, resid, (long)batch, N, n_levels, level0, rho_step, alpha};
    rc = zm::mpc_wave_ltv_dispatch(t, g, zm::MpcProb{(const int*)problem, rho_p}, zm::MpcTrack{gbuf}, zm::MpcLtv{c, D, ABt}, n, m, st);
    if (rc == ZM_EUNSUPPORTED)
        return zm::set_error(ZM_EUNSUPPORTED, "%s: (n=%d, m=%d) not among the shapes of the 16-lanes-per-instance kernels", fn, n, m);
    return rc;
}

// the receding-horizon loop as one call: see mpc_closed_loop
extern "C" int zm_mpc_closed_loop_f64(const double* A, const double* B, const double* Q, const double* R, const double* Qf, const double* K,
                                      const double* Minv, int n_levels, int level0, double rho_step, double alpha, const double* x_lb,
                                      const double* x_ub, const double* u_lb, const double* u_ub, const double* x0, const double* xRef,
                                      const double* uRef, int xref_rows, int uref_rows, double rho, const double* rho_p,
                                      const int32_t* problem, int64_t P, double eps_abs, double eps_rel, double eps_prim_inf, int max_iter,
                                      int warm_start, int steps, double clip_tol, const double* disturbance, double* workspace,
                                      double* states, double* inputs, int32_t* status, int32_t* iters, double* xPred, double* uPred,
                                      int64_t batch, int N, int n, int m, void* stream) {
    return zm::mpc_closed_loop("zm_mpc_closed_loop_f64", A, B, Q, R, Qf, K, Minv, n_levels, level0, rho_step, alpha, x_lb, x_ub, u_lb, u_ub,
                               x0, xRef, uRef, xref_rows, uref_rows, rho, rho_p, problem, P, eps_abs, eps_rel, eps_prim_inf, max_iter,
                               warm_start, steps, clip_tol, disturbance, workspace, states, inputs, status, iters, xPred, uPred, batch, N,
                               n, m, stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// real-time-iteration nonlinear MPC: a registered model expanded about a plan, per instance, at every step
// ---------------------------------------------------------------------------------------------------------------------

extern "C" int zm_model_step_f64(const zm_model_t* model, const double* x, const double* u, double* xNext, int64_t batch, void* stream) {
    const char* fn = "zm_model_step_f64";
    if (batch == 0) return ZM_OK;   /* empty batch: nothing to do (pointers of empty arrays may be NULL) */
    zm_model_t md;
    const int rc = zm::check_model(model, md, fn);
    if (rc != ZM_OK) return rc;
    if (!x || !u || !xNext) return zm::set_error(ZM_EINVAL, "%s: null pointer", fn);
    if (batch < 0 || (batch + 63) / 64 > 0x7fffffffL) return zm::set_error(ZM_EINVAL, "%s: bad size", fn);
    hipLaunchKernelGGL(zm::mpc_rti_plant_kernel, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, (hipStream_t)stream, md, x, (long)md.n, u,
                       (long)md.m, (const double*)nullptr, (const double*)nullptr, (const double*)nullptr, -1.0, xNext, md.n,
                       (double*)nullptr, 0, (long)batch);
    ZM_HIP_CHECK(hipGetLastError());
    return ZM_OK;
}

extern "C" int zm_mpc_relinearize_f64(const zm_model_t* model, const double* xPlan, const double* uPlan, double* A, double* B, double* c,
                                      int64_t batch, int N, int n_user, int m_user, int ns, int mc, void* stream) {
    return zm::mpc_relinearize("zm_mpc_relinearize_f64", model, xPlan, uPlan, A, B, c, batch, N, n_user, m_user, ns, mc, stream);
}

extern "C" int zm_mpc_rti_f64(const zm_model_t* model, const zm_model_t* plant, double* xPlan, double* uPlan, double* A, double* B, double* c,
                              const double* Q, const double* R, const double* Qf, const double* rho_tab, double* K, double* Minv,
                              double* D, double* ABt, int n_levels, int level0, double rho_step, double alpha, const double* x_lb,
                              const double* x_ub, const double* u_lb, const double* u_ub, const double* x0, const double* xRef,
                              const double* uRef, int xref_rows, int uref_rows, const double* rho_p, const int32_t* problem,
                              double eps_abs, double eps_rel, double eps_prim_inf, int max_iter, int warm_start, int steps,
                              double clip_tol, const double* disturbance, double* workspace, double* states, double* inputs,
                              int32_t* status, int32_t* iters, double* resid, double* xPred, double* uPred, int64_t batch, int N,
                              int n_user, int m_user, int ns, int mc, void* stream) {
    return zm::mpc_rti("zm_mpc_rti_f64", model, plant, xPlan, uPlan, A, B, c, Q, R, Qf, rho_tab, K, Minv, D, ABt, n_levels, level0, rho_step,
                       alpha, x_lb, x_ub, u_lb, u_ub, x0, xRef, uRef, xref_rows, uref_rows, rho_p, problem, eps_abs, eps_rel, eps_prim_inf,
                       max_iter, warm_start, steps, clip_tol, disturbance, workspace, states, inputs, status, iters, resid, xPred, uPred,
                       batch, N, n_user, m_user, ns, mc, stream);
}
