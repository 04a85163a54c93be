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
#include "traced.h"

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
// mpc_setup_kernel, so every (p, l) slice is bit for bit what zm_mpc_setup_f64 writes for that problem and penalty.  The weights are
// symmetric (the host layer passes symmetric parts) and the body stores its value matrix symmetrised; so do the two copies below.
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
        if (t == 0) {  // m x m inverse by Gauss-Jordan with partial pivoting (m <= SM), as in mpc_setup_body.h
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
            T1[e] = (2.0 * Q[e] + ((e / n == e % n) ? rho : 0.0)) + T1[e] - T2[e];
        __syncthreads();
        for (int e = t; e < n * n; e += blockDim.x) P[e] = 0.5 * (T1[e] + T1[(e % n) * n + e / n]);   // symmetrised, as in mpc_setup_body.h
        for (int e = t; e < m * n; e += blockDim.x) Kout[(long)k * m * n + e] = K[e];
        for (int e = t; e < m * m; e += blockDim.x) Minvout[(long)k * m * m + e] = Mi[e];
        __syncthreads();
    }
}

// Stage-varying weights (zm_mpc_setup_ltv_stage_f64): mpc_setup_ltv_kernel with Qs (P,N,n,n), Rs (P,N,m,m) in place of Q, R, Qf -- Qs_k
// weights x_{k+1} (row N - 1 is the terminal weight), Rs_k weights u_k:  P_N = 2 Qs_{N-1} + rho I, stage k adds 2 Rs_k + rho I to Suu, and
// the value update that leaves stage k >= 1 adds 2 Qs_{k-1} + rho I.  A sibling, not a flag: that kernel stays as it is.  The same products
// in the same order, so constant rows (Qs_k = Q, Qs_{N-1} = Qf, Rs_k = R) give that kernel's K, Minv, D and ABt bit for bit.
template <int SN, int SM>
__global__ __launch_bounds__(256) void mpc_setup_ltv_stage_kernel(const double* __restrict__ A, const double* __restrict__ B,
                                                                  const double* __restrict__ c, const double* __restrict__ Qs,
                                                                  const double* __restrict__ Rs, const double* __restrict__ rho_tab,
                                                                  const int L, const int N, const int n, const int m,
                                                                  double* __restrict__ Kout, double* __restrict__ Minvout,
                                                                  double* __restrict__ Dout, double* __restrict__ ABt) {
    const long b = blockIdx.x, p = b / L;
    const bool pack = (b % L) == 0;
    A += p * N * n * n;
    B += p * N * n * m;
    if (c) c += p * N * n;
    Qs += p * N * n * n;
    Rs += p * N * m * m;
    Kout += b * N * m * n;
    Minvout += b * N * m * m;
    Dout += b * N * n;
    ABt += p * N * (n + m) * n;
    const double rho = rho_tab[b];
    __shared__ double As[SN * SN], Bs[SN * SM], P[SN * SN], PA[SN * SN], PB[SN * SM], Sux[SM * SN], Suu[SM * SM], Mi[SM * SM], K[SM * SN],
        T1[SN * SN], T2[SN * SN];
    const int t = threadIdx.x;
    for (int e = t; e < n * n; e += blockDim.x) P[e] = 2.0 * Qs[(long)(N - 1) * n * n + e] + ((e / n == e % n) ? rho : 0.0);  // P_N = 2 Qs_{N-1} + rho I
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
        if (t < m * m) Suu[t] += 2.0 * Rs[(long)k * m * m + t] + ((t / m == t % m) ? rho : 0.0);
        __syncthreads();
        if (t == 0) {  // m x m inverse by Gauss-Jordan with partial pivoting (m <= SM), as in mpc_setup_body.h
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
        const double* Q = Qs + (long)(k >= 1 ? k - 1 : 0) * n * n;   // the weight of x_k; nothing reads the value matrix of x_0
        for (int e = t; e < n * n; e += blockDim.x)
            T1[e] = (2.0 * Q[e] + ((e / n == e % n) ? rho : 0.0)) + T1[e] - T2[e];
        __syncthreads();
        for (int e = t; e < n * n; e += blockDim.x) P[e] = 0.5 * (T1[e] + T1[(e % n) * n + e / n]);   // symmetrised, as in mpc_setup_body.h
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

// mpc_track_linear_kernel with the stage's own weights (zm_mpc_solve_ltv_stage_f64): Qs (P,N,n,n) weights x_{k+1}, Rs (P,N,m,m) weights u_k,
//     g_x,k = -(Qs_k + Qs_k') xr_{k+1},      g_u,k = -(Rs_k + Rs_k') ur_k,
// one thread per component, that kernel's sums in its order (constant rows give its bits).  prob is required here.
__global__ __launch_bounds__(256) void mpc_track_linear_stage_kernel(const double* __restrict__ Qs, const double* __restrict__ Rs,
                                                                     const double* __restrict__ xRef, const double* __restrict__ uRef,
                                                                     const int* __restrict__ prob, const long batch, const int N,
                                                                     const int n, const int m, double* __restrict__ g) {
    const int W = n + m;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= batch * N * W) return;
    const int i = (int)(e % W);
    const long s = e / W;
    const int k = (int)(s % N);
    const long b = s / N;
    const long p = prob[b];
    double acc = 0.0;
    if (i < n) {
        if (xRef) {
            const double* Wm = Qs + (p * N + k) * n * n;
            const double* xr = xRef + (b * (N + 1) + k + 1) * n;
            for (int j = 0; j < n; ++j) acc = __builtin_fma(Wm[i * n + j] + Wm[j * n + i], xr[j], acc);
        }
    } else if (uRef) {
        const int r = i - n;
        const double* Rm = Rs + (p * N + k) * m * m;
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

// mpc_advance_kernel for a softened object (zm_mpc_closed_loop_soft_f64, the queue of launches): the same rule, but a state component
// whose l1 (soft_l1 (P,n+m), the stacked layout; one row without a problem map) is finite is never clipped -- it stays the plant's state.
// A sibling rather than one more parameter: mpc_advance_kernel keeps its arguments and its code.
__global__ __launch_bounds__(256) void mpc_advance_soft_kernel(const double* src, const long src_stride, const double* dist,
                                                               const double* x_lb, const double* x_ub, const double* soft_l1,
                                                               const int* prob, const double clip_tol, double* dst, const double* usrc,
                                                               const long usrc_stride, double* udst, const long batch, const int n,
                                                               const int m) {
    const int W = n + m;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= batch * W) return;
    const int i = (int)(e % W);
    const long b = e / W;
    if (i < n) {
        double v = src[b * src_stride + i];
        if (dist) v += dist[b * n + i];
        const long p = prob ? prob[b] : 0;
        if (clip_tol >= 0.0 && !(soft_l1[p * W + i] < __builtin_inf())) {   // min(max(v, lo), hi): np.clip's order, a NaN passes through
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
// host side: every solve and run entry point (relaxed, batched, tracking, ltv; closed loop, rti) fills one call record by name; the
// checks, the kernels' argument blocks, the workspace layout and the per-step offsets are each written once and read from it
// ----------------------------------------------------------------------------------------------------------------

// What an MPC entry point receives.  Host only: no kernel takes it.  An entry fills the fields it has and leaves the rest zero.
struct MpcCall {
    const char* fn;                                                    // the entry point's name, the prefix of its error messages
    const double *A, *B, *c, *Q, *R, *Qf, *x_lb, *x_ub, *u_lb, *u_ub;  // the problem(s)
    const double *K, *Minv, *D, *ABt, *rho_tab;                        // the tables of every penalty level
    int n_levels, level0;
    double rho_step, alpha, rho;                                       // rho: the shared problem's penalty ...
    const double* rho_p;                                               // ... per-problem data: one per problem, with the map
    const int32_t* problem;                                            // instance -> problem in [0, P)
    int64_t P;
    const double *x0, *xRef, *uRef;
    int xref_rows, uref_rows;                                          // rows per instance of a run's references
    double eps_abs, eps_rel, eps_prim_inf;
    int max_iter, warm_start;
    int steps;                                                         // a run: its steps, MpcLoop's clip_tol and disturbance
    double clip_tol;
    const double* disturbance;
    double* workspace;
    double *xTraj, *uTraj, *resid;                                     // outputs of a solve (resid also of zm_mpc_rti_f64) ...
    double *states, *inputs, *xPred, *uPred;                           // ... of a run
    int32_t *status, *iters;
    int64_t batch;
    int N, n, m;                                                       // (n, m): the compiled shape the data is laid out in
    int n_user, m_user;                                                // zm_mpc_rti_f64: the model's own (n, m) inside it
    // zm_mpc_solve_ltv_stage_f64: Q, R hold Qs (P,N,n,n), Rs (P,N,m,m) and Qf stays NULL; x_lb, x_ub hold the box of x_0 (P,n) and
    // u_lb, u_ub the stacked lo, hi (P,N,n+m) -- the slots the kernel takes them in (mpc_common.h: mpc_wave_ltv_dispatch)
    bool stage;
    // zm_mpc_solve_ltv_soft_f64: the stage form with penalty weights (P,n+m) on the box; soft_l2 may be NULL (zeros).
    // zm_mpc_solve_soft_f64, zm_mpc_closed_loop_soft_f64: `soft` without `stage` -- lqrMpc's data with the weights, (1,n+m) without a map
    bool soft;
    const double *soft_l1, *soft_l2;
    void* stream;
};

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

static long blocks256(long threads) { return (threads + 255) / 256; }

// The argument checks every solve and run entry point shares, all before any launch.  The flags are the entry's decisions:
// per_problem -- the map and rho_p are required; tracking -- Q, R, Qf are required and n, m are checked; outputs -- false if one of the
// entry's own output pointers is NULL.
static int mpc_check_args(const MpcCall& a, bool per_problem, bool tracking, bool outputs) {
    if (!(a.alpha > 0.0 && a.alpha < 2.0)) return set_error(ZM_EINVAL, "%s: alpha must lie in (0, 2)", a.fn);
    if (!a.A || !a.B || !a.K || !a.Minv || !a.x_lb || !a.x_ub || !a.u_lb || !a.u_ub || !a.x0 || !a.workspace || !outputs ||
        (tracking && (!a.Q || !a.R || (!a.Qf && !a.stage))) || (per_problem && (!a.rho_p || !a.problem)))
        return set_error(ZM_EINVAL, "%s: null pointer", a.fn);
    if ((a.problem == nullptr) != (a.rho_p == nullptr))
        return set_error(ZM_EINVAL, "%s: the problem map and the per-problem rho come together", a.fn);
    if (a.batch < 0 || a.N < 1 || a.max_iter < 0 || (tracking && (a.n < 1 || a.m < 1)) || (a.problem ? a.P < 1 : !(a.rho > 0.0)))
        return set_error(ZM_EINVAL, tracking ? "%s: bad size / rho" : "%s: bad size", a.fn);
    if (a.n_levels < 1 || a.level0 < 0 || a.level0 >= a.n_levels || (a.n_levels > 1 && !(a.rho_step > 1.0)))
        return set_error(ZM_EINVAL, "%s: bad penalty levels", a.fn);
    if (tracking && blocks256((long)a.batch * a.N * ((long)a.n + a.m)) > 0x7fffffffL)   // of mpc_track_linear_kernel
        return set_error(ZM_EINVAL, "%s: batch x N x (n + m) too large", a.fn);
    return ZM_OK;
}

// The checks of a run (zm_mpc_closed_loop_f64, zm_mpc_rti_f64) that follow mpc_check_args.  `sizes_ok` is the entry's own test of its
// sizes, refused after `steps` and before the prediction arrays.
static int mpc_check_run(const MpcCall& a, bool sizes_ok) {
    if (a.steps < 1) return set_error(ZM_EINVAL, "%s: steps must be at least 1", a.fn);
    if (!sizes_ok) return set_error(ZM_EINVAL, "%s: bad size", a.fn);
    if ((a.xPred == nullptr) != (a.uPred == nullptr)) return set_error(ZM_EINVAL, "%s: the two prediction arrays come together", a.fn);
    if ((a.xRef && a.xref_rows != a.steps + a.N) || (a.uRef && a.uref_rows != a.steps + a.N - 1))
        return set_error(ZM_EINVAL, "%s: a reference needs steps + N rows of xRef and steps + N - 1 rows of uRef", a.fn);
    return ZM_OK;
}

// The problem map is read back and checked on the host before anything is launched (one small copy; the results come back through a
// sync anyway): the kernels offset every table by it.  Every index must lie in [0, P) -- or, `identity`, be the instance's own.
static int mpc_check_map(const MpcCall& a, bool identity, hipStream_t st) {
    if (!a.problem) return ZM_OK;
    static thread_local std::vector<int32_t> h;
    h.resize((size_t)a.batch);
    ZM_HIP_CHECK(hipMemcpyAsync(h.data(), a.problem, (size_t)a.batch * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    ZM_HIP_CHECK(hipStreamSynchronize(st));
    for (int64_t i = 0; i < a.batch; ++i) {
        if (identity && h[i] != (int32_t)i)
            return set_error(ZM_EINVAL, "%s: instance %lld maps to problem %d; every instance is its own problem here", a.fn, (long long)i,
                             (int)h[i]);
        if (!identity && (h[i] < 0 || h[i] >= a.P))
            return set_error(ZM_EINVAL, "%s: instance %lld maps to problem %d outside [0, %lld)", a.fn, (long long)i, (int)h[i],
                             (long long)a.P);
    }
    return ZM_OK;
}

// the shapes and horizons of the one kernel for stage-varying dynamics (mpc_wave.hip: mpc_wave_ltv_dispatch), refused before any launch
static int mpc_ltv_check_shape(const MpcCall& a) {
    if (for_mpc_shape(a.n, a.m, [](auto ns, auto mc) { return ns.value + mc.value <= 16 ? ZM_OK : ZM_EUNSUPPORTED; }) != ZM_OK)
        return set_error(ZM_EUNSUPPORTED, "%s: (n=%d, m=%d) not among the shapes of the 16-lanes-per-instance kernels", a.fn, a.n, a.m);
    if (!mpc_iterates_fit_lds(a.N))
        return set_error(ZM_EUNSUPPORTED, "%s: N=%d beyond the horizons whose iterates fit LDS (N <= 75)", a.fn, a.N);
    return ZM_OK;
}

static MpcTabs mpc_tabs(const MpcCall& a) { return {a.A, a.B, a.K, a.Minv, a.x_lb, a.x_ub, a.u_lb, a.u_ub}; }

static int mpc_warm(const MpcCall& a) { return a.warm_start == 2 ? 2 : (a.warm_start ? 1 : 0); }

// The kernels' options block; `warm` and the rollout arrays are those of a solve, or of the first step of a run.  With per-problem data
// g.rho is unused (each instance takes its problem's rho_p[p]); 1.0 keeps the struct well-formed.
static MpcArgs mpc_args(const MpcCall& a, int warm, double* xTraj, double* uTraj) {
    return {a.x0,     a.problem ? 1.0 : a.rho, a.eps_abs, a.eps_rel,    a.eps_prim_inf, a.max_iter, warm,       a.workspace, xTraj, uTraj,
            (int*)a.status, (int*)a.iters,     a.resid,   (long)a.batch, a.N,           a.n_levels, a.level0,   a.rho_step,  a.alpha};
}

// The workspace: the four blocks of a solve (batch, N, n + m each), with `tracking` a fifth for the linear term of the cost, then -- a
// run that does not keep its predictions -- the one rollout every step overwrites.
struct MpcLayout {
    double* gbuf;            // the linear term; nullptr without `tracking`
    double *xroll, *uroll;   // the rollout of step 0: the prediction arrays, else the scratch behind the blocks
    long xstep, ustep;       // doubles from one step's rollout to the next: one rollout when predictions are kept, else 0
};
static MpcLayout mpc_layout(const MpcCall& a, bool tracking) {
    const long blk = (long)a.batch * a.N * ((long)a.n + a.m);
    const long xsz = (long)a.batch * (a.N + 1) * a.n, usz = (long)a.batch * a.N * a.m;
    double* scratch = a.workspace + (tracking ? 5 : 4) * blk;
    return {tracking ? a.workspace + 4 * blk : nullptr, a.xPred ? a.xPred : scratch, a.uPred ? a.uPred : scratch + xsz,
            a.xPred ? xsz : 0, a.uPred ? usz : 0};
}

static MpcLoop mpc_loop(const MpcCall& a, const MpcLayout& lay) {
    return {a.steps,  mpc_warm(a),    a.clip_tol,    a.x0,      a.disturbance, a.states, a.inputs, (int*)a.status,
            (int*)a.iters, lay.xroll, lay.uroll, lay.xstep, lay.ustep};
}

// step s of a run sees the layouts of a single solve through offset pointers (the device's copy: mpc_closed_loop_wave_kernel)
static MpcArgs mpc_step_args(MpcArgs g, const MpcLoop& lp, int n, int s) {
    g.x0 = lp.states + (long)s * g.batch * n;
    g.xTraj = lp.xPred + s * lp.xpred_step;
    g.uTraj = lp.uPred + s * lp.upred_step;
    g.status = lp.status + (long)s * g.batch;
    g.iters = lp.iters + (long)s * g.batch;
    g.warm = s ? lp.warm : 0;
    return g;
}

// the linear term of step s of a run (s < 0: of a solve, whose references are one window) into lay.gbuf
static int mpc_track_linear(const MpcCall& a, const MpcLayout& lay, int s, hipStream_t st) {
    const dim3 grid((unsigned)blocks256((long)a.batch * a.N * ((long)a.n + a.m)));
    if (a.stage)   // (a solve: there is no run with stage-varying weights)
        hipLaunchKernelGGL(mpc_track_linear_stage_kernel, grid, dim3(256), 0, st, a.Q, a.R, a.xRef, a.uRef, (const int*)a.problem,
                           (long)a.batch, a.N, a.n, a.m, lay.gbuf);
    else if (s < 0)
        hipLaunchKernelGGL(mpc_track_linear_kernel, grid, dim3(256), 0, st, a.Q, a.R, a.Qf, a.xRef, a.uRef, (const int*)a.problem,
                           (long)a.batch, a.N, a.n, a.m, lay.gbuf);
    else
        hipLaunchKernelGGL(mpc_track_linear_window_kernel, grid, dim3(256), 0, st, a.Q, a.R, a.Qf, a.xRef, a.uRef, (const int*)a.problem,
                           (long)a.batch, a.N, a.n, a.m, (long)a.xref_rows, (long)a.uref_rows, (long)s, lay.gbuf);
    ZM_HIP_CHECK(hipGetLastError());
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
// level0 table (fixed penalty).  `t` holds the whole tables (every level).  sf != nullptr: soft box constraints -- the 16-lane kernel that
// takes the weights, whatever ZOPT_AMD_MPC_PATH says (there is no lane-per-instance kernel for them).
static int mpc_enqueue(const char* fn, MpcTabs t, const MpcArgs& g, const MpcProb* pb, const MpcTrack* trk, const MpcSoft* sf, int n, int m,
                       hipStream_t st) {
    if (sf) return mpc_wave_soft_dispatch(t, g, pb, trk, *sf, n, m, st);   // (its shape and horizon were checked: mpc_ltv_check_shape)
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

// The four solve entry points.
//   zm_mpc_solve_relaxed_f64 : one problem, scalar rho                          (problem, rho_p, Q, R, Qf, xRef, uRef NULL)
//   zm_mpc_solve_batched_f64 : per_problem -- problem and rho_p are required    (Q, R, Qf, xRef, uRef NULL)
//   zm_mpc_solve_tracking_f64: tracking -- Q, R, Qf are required, n and m are checked, the linear term is formed first; problem and
//                              rho_p come together or not at all
//   zm_mpc_solve_ltv_f64     : ltv -- per_problem and tracking (a zero linear term without a reference) with c, D, ABt; the one kernel
//                              there is (mpc_wave.hip), so what it does not take is refused before anything is launched
//   zm_mpc_solve_ltv_stage_f64: the same with a.stage -- weights and box per stage, the sibling kernels for the linear term and the solve
//   zm_mpc_solve_ltv_soft_f64: the stage entry with a.soft -- penalty weights on the box, the solve kernel that takes them
//   zm_mpc_solve_soft_f64    : the tracking entry with a.soft (tracking only with a reference); 16 lanes per instance only, as ltv
static int mpc_solve(const MpcCall& a, bool per_problem, bool tracking, bool ltv) {
    if (a.batch == 0) return ZM_OK;   /* empty batch: nothing to do (pointers of empty arrays may be NULL) */
    int rc = mpc_check_args(a, per_problem, tracking, a.xTraj && a.uTraj && a.status && (!ltv || (a.c && a.D && a.ABt)) && (!a.soft || a.soft_l1));
    if (rc != ZM_OK) return rc;
    if ((ltv || a.soft) && (rc = mpc_ltv_check_shape(a)) != ZM_OK) return rc;
    hipStream_t st = (hipStream_t)a.stream;
    if ((rc = mpc_check_map(a, false, st)) != ZM_OK) return rc;
    const MpcLayout lay = mpc_layout(a, tracking);
    if (tracking && (rc = mpc_track_linear(a, lay, -1, st)) != ZM_OK) return rc;
    const MpcTabs t = mpc_tabs(a);
    const MpcArgs g = mpc_args(a, mpc_warm(a), a.xTraj, a.uTraj);
    const MpcProb pb{(const int*)a.problem, a.rho_p};
    const MpcTrack trk{lay.gbuf};
    const MpcSoft sf{a.soft_l1, a.soft_l2};
    if (!ltv) return mpc_enqueue(a.fn, t, g, a.problem ? &pb : nullptr, tracking ? &trk : nullptr, a.soft ? &sf : nullptr, a.n, a.m, st);
    rc = a.soft ? mpc_wave_ltv_soft_dispatch(t, g, pb, trk, MpcLtv{a.c, a.D, a.ABt}, sf, a.n, a.m, st)
                : mpc_wave_ltv_dispatch(t, g, pb, trk, MpcLtv{a.c, a.D, a.ABt}, a.stage, a.n, a.m, st);
    if (rc == ZM_EUNSUPPORTED)
        return set_error(ZM_EUNSUPPORTED, "%s: (n=%d, m=%d) not among the shapes of the 16-lanes-per-instance kernels", a.fn, a.n, a.m);
    return rc;
}

// zm_mpc_closed_loop_f64: `steps` receding-horizon solves of every instance, nothing but launches on `st` after the argument checks.
//   (a) regulator runs at the shapes and horizons of the 16-lanes-per-instance kernels: ONE launch, the step loop inside the kernel
//       (mpc_wave.hip: mpc_closed_loop_wave_kernel);
//   (b) everything else -- tracking, (24, 8), horizons beyond LDS, ZOPT_AMD_MPC_PATH=lane: a loop that enqueues, per step, the launches
//       of a single solve and mpc_advance_kernel, with no host synchronisation in between.
// zm_mpc_closed_loop_soft_f64 (a.soft): the same two forms with the kernels that take the weights -- (a) mpc_closed_loop_wave_soft_kernel,
// (b), for tracking runs, the soft solve kernel and mpc_advance_soft_kernel; the shapes and horizons beyond the 16-lane kernels are refused.
static int mpc_closed_loop(const MpcCall& a) {
    if (a.batch == 0) return ZM_OK;   /* empty batch: nothing to do (pointers of empty arrays may be NULL) */
    const bool tracking = a.xRef || a.uRef;
    const int N = a.N, n = a.n, m = a.m;
    int rc = mpc_check_args(a, false, tracking, a.states && a.inputs && a.status && a.iters && (!a.soft || a.soft_l1));
    if (rc != ZM_OK) return rc;
    if ((rc = mpc_check_run(a, n >= 1 && m >= 1)) != ZM_OK) return rc;
    if (a.soft && (rc = mpc_ltv_check_shape(a)) != ZM_OK) return rc;
    const long ablocks = blocks256((long)a.batch * ((long)n + m));   // of mpc_advance_kernel
    if (ablocks > 0x7fffffffL) return set_error(ZM_EINVAL, "%s: batch x (n + m) too large", a.fn);
    hipStream_t st = (hipStream_t)a.stream;
    if ((rc = mpc_check_map(a, false, st)) != ZM_OK) return rc;

    const MpcLayout lay = mpc_layout(a, tracking);
    const MpcLoop lp = mpc_loop(a, lay);
    const MpcTabs t = mpc_tabs(a);
    const MpcArgs g = mpc_args(a, 0, lay.xroll, lay.uroll);
    const MpcProb pbv{(const int*)a.problem, a.rho_p};
    const MpcProb* pb = a.problem ? &pbv : nullptr;
    const MpcSoft sfv{a.soft_l1, a.soft_l2};
    const MpcSoft* sf = a.soft ? &sfv : nullptr;
    if (!tracking && sf) return mpc_wave_closed_loop_soft_dispatch(t, g, pb, lp, sfv, n, m, st);
    if (!tracking && !mpc_force_lane()) {
        rc = mpc_wave_closed_loop_dispatch(t, g, pb, lp, n, m, st);
        if (rc != ZM_EUNSUPPORTED) return rc;
    }
    const MpcTrack trkv{lay.gbuf};
    const auto advance = [&](const double* src, long src_stride, const double* dist, double* dst, const double* usrc, double* udst) -> int {
        if (sf)
            hipLaunchKernelGGL(mpc_advance_soft_kernel, dim3((unsigned)ablocks), dim3(256), 0, st, src, src_stride, dist, a.x_lb, a.x_ub,
                               a.soft_l1, (const int*)a.problem, a.clip_tol, dst, usrc, (long)N * m, udst, (long)a.batch, n, m);
        else
            hipLaunchKernelGGL(mpc_advance_kernel, dim3((unsigned)ablocks), dim3(256), 0, st, src, src_stride, dist, a.x_lb, a.x_ub,
                               (const int*)a.problem, a.clip_tol, dst, usrc, (long)N * m, udst, (long)a.batch, n, m);
        ZM_HIP_CHECK(hipGetLastError());
        return ZM_OK;
    };
    rc = advance(a.x0, n, nullptr, a.states, nullptr, nullptr);
    for (int s = 0; s < a.steps && rc == ZM_OK; ++s) {
        if (tracking && (rc = mpc_track_linear(a, lay, s, st)) != ZM_OK) break;
        const MpcArgs gs = mpc_step_args(g, lp, n, s);
        rc = mpc_enqueue(a.fn, t, gs, pb, tracking ? &trkv : nullptr, sf, n, m, st);
        if (rc != ZM_OK) break;
        rc = advance(gs.xTraj + n, (long)(N + 1) * n, a.disturbance ? a.disturbance + (long)s * a.batch * n : nullptr,
                     a.states + (long)(s + 1) * a.batch * n, gs.uTraj, a.inputs + (long)s * a.batch * m);
    }
    return rc;
}

// The models of the real-time-iteration entry points: a registered model of exactly (n, m); the quadcopters as a discrete step (dt > 0)
static int mpc_rti_check_model(const char* fn, const char* what, const zm_model_t* model, zm_model_t& md, int n, int m) {
    const int rc = check_model(model, md, fn);
    if (rc != ZM_OK) return rc;
    if (md.kind == ZM_MODEL_TRACED)
        return set_error(ZM_EUNSUPPORTED, "%s: the %s is a traced model; the real-time iteration on the tape interpreter is not built", fn,
                         what);
    if (md.n != n || md.m != m)
        return set_error(ZM_EINVAL, "%s: the %s has (n=%d, m=%d), the problem (n=%d, m=%d)", fn, what, md.n, md.m, n, m);
    if (md.kind != ZM_MODEL_LINEAR && !(md.dt > 0.0)) return set_error(ZM_EINVAL, "%s: the %s needs a step dt > 0", fn, what);
    return ZM_OK;
}

// what zm_mpc_rti_f64 writes at every step besides its outputs: the plan it expands about, the expansion, the tables of the expansion
// (the record holds the same A .. ABt as the read-only pointers the solve takes)
struct MpcRtiWork {
    double *xPlan, *uPlan, *A, *B, *c, *K, *Minv, *D, *ABt;
};

// zm_mpc_rti_f64: `steps` real-time iterations of every instance, nothing but launches on `st` after the argument checks and the one
// read-back of the problem map -- mpc_closed_loop's form (b) with the expansion and the table setup inside the loop:
//     relinearise about the plan -> mpc_setup_ltv_kernel -> mpc_track_linear_window_kernel -> the LTV solve -> plant step, plan shift
// Every instance is its own problem (P = batch, the map the identity); the steps and the shape are refused before the map is read.
static int mpc_rti(const MpcCall& a, const zm_model_t* model, const zm_model_t* plant, const MpcRtiWork& w) {
    if (a.batch == 0) return ZM_OK;   /* empty batch: nothing to do (pointers of empty arrays may be NULL) */
    const int N = a.N, n = a.n, m = a.m;
    const long batch = (long)a.batch;
    int rc = mpc_check_args(a, true, true,
                            a.states && a.inputs && a.status && a.iters && w.xPlan && w.uPlan && a.c && a.D && a.ABt && a.rho_tab);
    if (rc != ZM_OK) return rc;
    if ((rc = mpc_check_run(a, a.n_user >= 1 && a.m_user >= 1 && a.n_user <= n && a.m_user <= m)) != ZM_OK) return rc;
    if ((rc = mpc_ltv_check_shape(a)) != ZM_OK) return rc;
    zm_model_t md, pl;
    if ((rc = mpc_rti_check_model(a.fn, "model", model, md, a.n_user, a.m_user)) != ZM_OK) return rc;
    if ((rc = mpc_rti_check_model(a.fn, "plant", plant ? plant : model, pl, a.n_user, a.m_user)) != ZM_OK) return rc;
    const long ablocks = blocks256(batch * ((long)n + m));                                          // of mpc_advance_kernel
    const long sblocks = blocks256(batch * ((long)(N + 1) * a.n_user + (long)N * a.m_user));        // of mpc_rti_shift_kernel
    if (blocks256(batch * N * ((long)n + m)) > 0x7fffffffL || sblocks > 0x7fffffffL || batch * a.n_levels > 0x7fffffffL)
        return set_error(ZM_EINVAL, "%s: batch x N x (n + m) too large", a.fn);
    hipStream_t st = (hipStream_t)a.stream;
    if ((rc = mpc_check_map(a, true, st)) != ZM_OK) return rc;

    const MpcLayout lay = mpc_layout(a, true);
    const MpcLoop lp = mpc_loop(a, lay);
    const MpcTabs t = mpc_tabs(a);
    const MpcArgs g = mpc_args(a, 0, lay.xroll, lay.uroll);
    const MpcProb pb{(const int*)a.problem, a.rho_p};
    hipLaunchKernelGGL(mpc_advance_kernel, dim3((unsigned)ablocks), dim3(256), 0, st, a.x0, (long)n, (const double*)nullptr, a.x_lb, a.x_ub,
                       (const int*)a.problem, a.clip_tol, a.states, (const double*)nullptr, 0L, (double*)nullptr, batch, n, m);
    ZM_HIP_CHECK(hipGetLastError());
    for (int s = 0; s < a.steps; ++s) {
        if ((rc = mpc_relinearize_enqueue(md, w.xPlan, w.uPlan, w.A, w.B, w.c, batch, N, n, m, st)) != ZM_OK) return rc;
        // (a.X and w.X are one buffer: `a` holds what the kernels read, `w` what this call writes -- the expansion, then its tables)
        hipLaunchKernelGGL((mpc_setup_ltv_kernel<SN, SM>), dim3((unsigned)(batch * a.n_levels)), dim3(256), 0, st, a.A, a.B, a.c, a.Q, a.R,
                           a.Qf, a.rho_tab, a.n_levels, N, n, m, w.K, w.Minv, w.D, w.ABt);
        ZM_HIP_CHECK(hipGetLastError());
        if ((rc = mpc_track_linear(a, lay, s, st)) != ZM_OK) return rc;
        const MpcArgs gs = mpc_step_args(g, lp, n, s);
        rc = mpc_wave_ltv_dispatch(t, gs, pb, MpcTrack{lay.gbuf}, MpcLtv{a.c, a.D, a.ABt}, false, n, m, st);
        if (rc == ZM_EUNSUPPORTED)
            return set_error(ZM_EUNSUPPORTED, "%s: (n=%d, m=%d) not among the shapes of the 16-lanes-per-instance kernels", a.fn, n, m);
        if (rc != ZM_OK) return rc;
        hipLaunchKernelGGL(mpc_rti_plant_kernel, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, st, pl, gs.x0, (long)n, gs.uTraj,
                           (long)N * m, a.disturbance ? a.disturbance + (long)s * batch * n : nullptr, a.x_lb, a.x_ub, a.clip_tol,
                           a.states + (long)(s + 1) * batch * n, n, a.inputs + (long)s * batch * m, m, batch);
        ZM_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(mpc_rti_shift_kernel, dim3((unsigned)sblocks), dim3(256), 0, st, gs.xTraj, gs.uTraj, w.xPlan, w.uPlan, batch, N,
                           a.n_user, a.m_user, n, m);
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
    zm::MpcCall a{};
    a.fn = "zm_mpc_solve_relaxed_f64";
    a.A = A, a.B = B, a.K = K, a.Minv = Minv, a.x_lb = x_lb, a.x_ub = x_ub, a.u_lb = u_lb, a.u_ub = u_ub;
    a.n_levels = n_levels, a.level0 = level0, a.rho_step = rho_step, a.alpha = alpha, a.x0 = x0;
    a.eps_abs = eps_abs, a.eps_rel = eps_rel, a.eps_prim_inf = eps_prim_inf, a.max_iter = max_iter, a.warm_start = warm_start;
    a.workspace = workspace, a.xTraj = xTraj, a.uTraj = uTraj, a.status = status, a.iters = iters, a.resid = resid;
    a.batch = batch, a.N = N, a.n = n, a.m = m, a.stream = stream;
    a.rho = rho;
    return zm::mpc_solve(a, false, false, false);
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
    zm::MpcCall a{};
    a.fn = "zm_mpc_solve_batched_f64";
    a.A = A, a.B = B, a.K = K, a.Minv = Minv, a.x_lb = x_lb, a.x_ub = x_ub, a.u_lb = u_lb, a.u_ub = u_ub;
    a.n_levels = n_levels, a.level0 = level0, a.rho_step = rho_step, a.alpha = alpha, a.x0 = x0;
    a.eps_abs = eps_abs, a.eps_rel = eps_rel, a.eps_prim_inf = eps_prim_inf, a.max_iter = max_iter, a.warm_start = warm_start;
    a.workspace = workspace, a.xTraj = xTraj, a.uTraj = uTraj, a.status = status, a.iters = iters, a.resid = resid;
    a.batch = batch, a.N = N, a.n = n, a.m = m, a.stream = stream;
    a.rho_p = rho, a.problem = problem, a.P = P;
    return zm::mpc_solve(a, true, false, false);
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
    zm::MpcCall a{};
    a.fn = "zm_mpc_solve_tracking_f64";
    a.A = A, a.B = B, a.K = K, a.Minv = Minv, a.x_lb = x_lb, a.x_ub = x_ub, a.u_lb = u_lb, a.u_ub = u_ub;
    a.n_levels = n_levels, a.level0 = level0, a.rho_step = rho_step, a.alpha = alpha, a.x0 = x0;
    a.eps_abs = eps_abs, a.eps_rel = eps_rel, a.eps_prim_inf = eps_prim_inf, a.max_iter = max_iter, a.warm_start = warm_start;
    a.workspace = workspace, a.xTraj = xTraj, a.uTraj = uTraj, a.status = status, a.iters = iters, a.resid = resid;
    a.batch = batch, a.N = N, a.n = n, a.m = m, a.stream = stream;
    a.Q = Q, a.R = R, a.Qf = Qf, a.xRef = xRef, a.uRef = uRef, a.rho = rho, a.rho_p = rho_p, a.problem = problem, a.P = P;
    return zm::mpc_solve(a, false, true, false);
}

// soft box constraints on lqrMpc's data: the tracking entry with the penalty weights; tracking only with a reference
extern "C" int zm_mpc_solve_soft_f64(const double* A, const double* B, const double* Q, const double* R, const double* Qf, const double* K,
                                     const double* Minv, int n_levels, int level0, double rho_step, double alpha, const double* x_lb,
                                     const double* x_ub, const double* u_lb, const double* u_ub, const double* soft_l1,
                                     const double* soft_l2, const double* x0, const double* xRef, const double* uRef, double rho,
                                     const double* rho_p, const int32_t* problem, int64_t P, double eps_abs, double eps_rel,
                                     double eps_prim_inf, int max_iter, int warm_start, double* workspace, double* xTraj, double* uTraj,
                                     int32_t* status, int32_t* iters, double* resid, int64_t batch, int N, int n, int m, void* stream) {
    zm::MpcCall a{};
    a.fn = "zm_mpc_solve_soft_f64";
    a.A = A, a.B = B, a.K = K, a.Minv = Minv, a.x_lb = x_lb, a.x_ub = x_ub, a.u_lb = u_lb, a.u_ub = u_ub;
    a.n_levels = n_levels, a.level0 = level0, a.rho_step = rho_step, a.alpha = alpha, a.x0 = x0;
    a.eps_abs = eps_abs, a.eps_rel = eps_rel, a.eps_prim_inf = eps_prim_inf, a.max_iter = max_iter, a.warm_start = warm_start;
    a.workspace = workspace, a.xTraj = xTraj, a.uTraj = uTraj, a.status = status, a.iters = iters, a.resid = resid;
    a.batch = batch, a.N = N, a.n = n, a.m = m, a.stream = stream;
    a.Q = Q, a.R = R, a.Qf = Qf, a.xRef = xRef, a.uRef = uRef, a.rho = rho, a.rho_p = rho_p, a.problem = problem, a.P = P;
    a.soft = true, a.soft_l1 = soft_l1, a.soft_l2 = soft_l2;
    return zm::mpc_solve(a, false, xRef || uRef, false);
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
    zm::MpcCall a{};
    a.fn = "zm_mpc_solve_ltv_f64";
    a.A = A, a.B = B, a.K = K, a.Minv = Minv, a.x_lb = x_lb, a.x_ub = x_ub, a.u_lb = u_lb, a.u_ub = u_ub;
    a.n_levels = n_levels, a.level0 = level0, a.rho_step = rho_step, a.alpha = alpha, a.x0 = x0;
    a.eps_abs = eps_abs, a.eps_rel = eps_rel, a.eps_prim_inf = eps_prim_inf, a.max_iter = max_iter, a.warm_start = warm_start;
    a.workspace = workspace, a.xTraj = xTraj, a.uTraj = uTraj, a.status = status, a.iters = iters, a.resid = resid;
    a.batch = batch, a.N = N, a.n = n, a.m = m, a.stream = stream;
    a.c = c, a.D = D, a.ABt = ABt, a.Q = Q, a.R = R, a.Qf = Qf, a.xRef = xRef, a.uRef = uRef, a.rho_p = rho_p, a.problem = problem, a.P = P;
    return zm::mpc_solve(a, true, true, true);
}

// stage-varying weights and bounds on top of the stage-varying dynamics
extern "C" int zm_mpc_setup_ltv_stage_f64(const double* A, const double* B, const double* c, const double* Qs, const double* Rs,
                                          const double* rho, int64_t P, int L, int N, int n, int m, double* K, double* Minv, double* D,
                                          double* ABt, void* stream) {
    const char* fn = "zm_mpc_setup_ltv_stage_f64";
    if (P == 0) return ZM_OK;   /* no problems: nothing to do (pointers of empty arrays may be NULL) */
    if (!A || !B || !Qs || !Rs || !rho || !K || !Minv || !D || !ABt) return zm::set_error(ZM_EINVAL, "%s: null pointer", fn);
    if (P < 0 || L < 1 || N < 1 || n < 1 || m < 1 || P * L > 0x7fffffffL) return zm::set_error(ZM_EINVAL, "%s: bad size", fn);
    if (n > zm::SN || m > zm::SM) return zm::set_error(ZM_EUNSUPPORTED, "%s: (n=%d, m=%d) not covered (n <= 12, m <= 4)", fn, n, m);
    hipLaunchKernelGGL((zm::mpc_setup_ltv_stage_kernel<zm::SN, zm::SM>), dim3((unsigned)(P * L)), dim3(256), 0, (hipStream_t)stream, A, B, c,
                       Qs, Rs, rho, L, N, n, m, K, Minv, D, ABt);
    ZM_HIP_CHECK(hipGetLastError());
    return ZM_OK;
}

extern "C" int zm_mpc_solve_ltv_stage_f64(const double* A, const double* B, const double* c, const double* ABt, const double* Qs,
                                          const double* Rs, const double* K, const double* Minv, const double* D, int n_levels, int level0,
                                          double rho_step, double alpha, const double* x_lb0, const double* x_ub0, const double* lo,
                                          const double* hi, const double* x0, const double* xRef, const double* uRef, const double* rho_p,
                                          const int32_t* problem, int64_t P, double eps_abs, double eps_rel, double eps_prim_inf,
                                          int max_iter, int warm_start, double* workspace, double* xTraj, double* uTraj, int32_t* status,
                                          int32_t* iters, double* resid, int64_t batch, int N, int n, int m, void* stream) {
    zm::MpcCall a{};
    a.fn = "zm_mpc_solve_ltv_stage_f64";
    a.A = A, a.B = B, a.K = K, a.Minv = Minv, a.x_lb = x_lb0, a.x_ub = x_ub0, a.u_lb = lo, a.u_ub = hi;
    a.n_levels = n_levels, a.level0 = level0, a.rho_step = rho_step, a.alpha = alpha, a.x0 = x0;
    a.eps_abs = eps_abs, a.eps_rel = eps_rel, a.eps_prim_inf = eps_prim_inf, a.max_iter = max_iter, a.warm_start = warm_start;
    a.workspace = workspace, a.xTraj = xTraj, a.uTraj = uTraj, a.status = status, a.iters = iters, a.resid = resid;
    a.batch = batch, a.N = N, a.n = n, a.m = m, a.stream = stream;
    a.c = c, a.D = D, a.ABt = ABt, a.Q = Qs, a.R = Rs, a.xRef = xRef, a.uRef = uRef, a.rho_p = rho_p, a.problem = problem, a.P = P;
    a.stage = true;
    return zm::mpc_solve(a, true, true, true);
}

// soft box constraints on top of the stage form: the same call with the penalty weights, its own solve kernel
extern "C" int zm_mpc_solve_ltv_soft_f64(const double* A, const double* B, const double* c, const double* ABt, const double* Qs,
                                         const double* Rs, const double* K, const double* Minv, const double* D, int n_levels, int level0,
                                         double rho_step, double alpha, const double* x_lb0, const double* x_ub0, const double* lo,
                                         const double* hi, const double* soft_l1, const double* soft_l2, const double* x0,
                                         const double* xRef, const double* uRef, const double* rho_p, const int32_t* problem, int64_t P,
                                         double eps_abs, double eps_rel, double eps_prim_inf, int max_iter, int warm_start,
                                         double* workspace, double* xTraj, double* uTraj, int32_t* status, int32_t* iters, double* resid,
                                         int64_t batch, int N, int n, int m, void* stream) {
    zm::MpcCall a{};
    a.fn = "zm_mpc_solve_ltv_soft_f64";
    a.A = A, a.B = B, a.K = K, a.Minv = Minv, a.x_lb = x_lb0, a.x_ub = x_ub0, a.u_lb = lo, a.u_ub = hi;
    a.n_levels = n_levels, a.level0 = level0, a.rho_step = rho_step, a.alpha = alpha, a.x0 = x0;
    a.eps_abs = eps_abs, a.eps_rel = eps_rel, a.eps_prim_inf = eps_prim_inf, a.max_iter = max_iter, a.warm_start = warm_start;
    a.workspace = workspace, a.xTraj = xTraj, a.uTraj = uTraj, a.status = status, a.iters = iters, a.resid = resid;
    a.batch = batch, a.N = N, a.n = n, a.m = m, a.stream = stream;
    a.c = c, a.D = D, a.ABt = ABt, a.Q = Qs, a.R = Rs, a.xRef = xRef, a.uRef = uRef, a.rho_p = rho_p, a.problem = problem, a.P = P;
    a.stage = true, a.soft = true, a.soft_l1 = soft_l1, a.soft_l2 = soft_l2;
    return zm::mpc_solve(a, true, true, true);
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
    zm::MpcCall a{};
    a.fn = "zm_mpc_closed_loop_f64";
    a.A = A, a.B = B, a.K = K, a.Minv = Minv, a.x_lb = x_lb, a.x_ub = x_ub, a.u_lb = u_lb, a.u_ub = u_ub;
    a.n_levels = n_levels, a.level0 = level0, a.rho_step = rho_step, a.alpha = alpha, a.x0 = x0;
    a.eps_abs = eps_abs, a.eps_rel = eps_rel, a.eps_prim_inf = eps_prim_inf, a.max_iter = max_iter, a.warm_start = warm_start;
    a.Q = Q, a.R = R, a.Qf = Qf, a.xRef = xRef, a.uRef = uRef, a.xref_rows = xref_rows, a.uref_rows = uref_rows;
    a.rho_p = rho_p, a.problem = problem, a.steps = steps, a.clip_tol = clip_tol, a.disturbance = disturbance;
    a.workspace = workspace, a.states = states, a.inputs = inputs, a.status = status, a.iters = iters, a.xPred = xPred, a.uPred = uPred;
    a.batch = batch, a.N = N, a.n = n, a.m = m, a.stream = stream;
    a.rho = rho, a.P = P;
    return zm::mpc_closed_loop(a);
}

// the same run of a softened object: the weights, and a clip that leaves the soft state components alone
extern "C" int zm_mpc_closed_loop_soft_f64(const double* A, const double* B, const double* Q, const double* R, const double* Qf,
                                           const double* K, const double* Minv, int n_levels, int level0, double rho_step, double alpha,
                                           const double* x_lb, const double* x_ub, const double* u_lb, const double* u_ub,
                                           const double* soft_l1, const double* soft_l2, const double* x0, const double* xRef,
                                           const double* uRef, int xref_rows, int uref_rows, double rho, const double* rho_p,
                                           const int32_t* problem, int64_t P, double eps_abs, double eps_rel, double eps_prim_inf,
                                           int max_iter, int warm_start, int steps, double clip_tol, const double* disturbance,
                                           double* workspace, double* states, double* inputs, int32_t* status, int32_t* iters,
                                           double* xPred, double* uPred, int64_t batch, int N, int n, int m, void* stream) {
    zm::MpcCall a{};
    a.fn = "zm_mpc_closed_loop_soft_f64";
    a.A = A, a.B = B, a.K = K, a.Minv = Minv, a.x_lb = x_lb, a.x_ub = x_ub, a.u_lb = u_lb, a.u_ub = u_ub;
    a.n_levels = n_levels, a.level0 = level0, a.rho_step = rho_step, a.alpha = alpha, a.x0 = x0;
    a.eps_abs = eps_abs, a.eps_rel = eps_rel, a.eps_prim_inf = eps_prim_inf, a.max_iter = max_iter, a.warm_start = warm_start;
    a.Q = Q, a.R = R, a.Qf = Qf, a.xRef = xRef, a.uRef = uRef, a.xref_rows = xref_rows, a.uref_rows = uref_rows;
    a.rho_p = rho_p, a.problem = problem, a.steps = steps, a.clip_tol = clip_tol, a.disturbance = disturbance;
    a.workspace = workspace, a.states = states, a.inputs = inputs, a.status = status, a.iters = iters, a.xPred = xPred, a.uPred = uPred;
    a.batch = batch, a.N = N, a.n = n, a.m = m, a.stream = stream;
    a.rho = rho, a.P = P;
    a.soft = true, a.soft_l1 = soft_l1, a.soft_l2 = soft_l2;
    return zm::mpc_closed_loop(a);
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
    if (md.kind == ZM_MODEL_TRACED) return zm::traced_step(md, x, u, xNext, (long)batch, (hipStream_t)stream);   // traced.hip
    hipLaunchKernelGGL(zm::mpc_rti_plant_kernel, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, (hipStream_t)stream, md, x, (long)md.n, u,
                       (long)md.m, (const double*)nullptr, (const double*)nullptr, (const double*)nullptr, -1.0, xNext, md.n,
                       (double*)nullptr, 0, (long)batch);
    ZM_HIP_CHECK(hipGetLastError());
    return ZM_OK;
}

extern "C" int zm_mpc_relinearize_f64(const zm_model_t* model, const double* xPlan, const double* uPlan, double* A, double* B, double* c,
                                      int64_t batch, int N, int n_user, int m_user, int ns, int mc, void* stream) {
    const char* fn = "zm_mpc_relinearize_f64";
    if (batch == 0) return ZM_OK;   /* empty batch: nothing to do (pointers of empty arrays may be NULL) */
    if (!xPlan || !uPlan || !A || !B || !c) return zm::set_error(ZM_EINVAL, "%s: null pointer", fn);
    if (batch < 0 || N < 1 || n_user < 1 || m_user < 1 || ns < n_user || mc < m_user) return zm::set_error(ZM_EINVAL, "%s: bad size", fn);
    if (ns > zm::SN || mc > zm::SM) return zm::set_error(ZM_EUNSUPPORTED, "%s: (n=%d, m=%d) not covered (n <= 12, m <= 4)", fn, ns, mc);
    if (((long)batch * N + 15) / 16 > 0x7fffffffL) return zm::set_error(ZM_EINVAL, "%s: batch x N too large", fn);
    zm_model_t md;
    const int rc = zm::mpc_rti_check_model(fn, "model", model, md, n_user, m_user);
    if (rc != ZM_OK) return rc;
    return zm::mpc_relinearize_enqueue(md, xPlan, uPlan, A, B, c, (long)batch, N, ns, mc, (hipStream_t)stream);
}

// every instance is its own problem: P = batch, and no shared rho
extern "C" int zm_mpc_rti_f64(const zm_model_t* model, const zm_model_t* plant, double* xPlan, double* uPlan, double* A, double* B, double* c,
                              const double* Q, const double* R, const double* Qf, const double* rho_tab, double* K, double* Minv,
                              double* D, double* ABt, int n_levels, int level0, double rho_step, double alpha, const double* x_lb,
                              const double* x_ub, const double* u_lb, const double* u_ub, const double* x0, const double* xRef,
                              const double* uRef, int xref_rows, int uref_rows, const double* rho_p, const int32_t* problem,
                              double eps_abs, double eps_rel, double eps_prim_inf, int max_iter, int warm_start, int steps,
                              double clip_tol, const double* disturbance, double* workspace, double* states, double* inputs,
                              int32_t* status, int32_t* iters, double* resid, double* xPred, double* uPred, int64_t batch, int N,
                              int n_user, int m_user, int ns, int mc, void* stream) {
    zm::MpcCall a{};
    a.fn = "zm_mpc_rti_f64";
    a.A = A, a.B = B, a.K = K, a.Minv = Minv, a.x_lb = x_lb, a.x_ub = x_ub, a.u_lb = u_lb, a.u_ub = u_ub;
    a.n_levels = n_levels, a.level0 = level0, a.rho_step = rho_step, a.alpha = alpha, a.x0 = x0;
    a.eps_abs = eps_abs, a.eps_rel = eps_rel, a.eps_prim_inf = eps_prim_inf, a.max_iter = max_iter, a.warm_start = warm_start;
    a.Q = Q, a.R = R, a.Qf = Qf, a.xRef = xRef, a.uRef = uRef, a.xref_rows = xref_rows, a.uref_rows = uref_rows;
    a.rho_p = rho_p, a.problem = problem, a.steps = steps, a.clip_tol = clip_tol, a.disturbance = disturbance;
    a.workspace = workspace, a.states = states, a.inputs = inputs, a.status = status, a.iters = iters, a.xPred = xPred, a.uPred = uPred;
    a.batch = batch, a.N = N, a.n = ns, a.m = mc, a.n_user = n_user, a.m_user = m_user, a.stream = stream;
    a.c = c, a.D = D, a.ABt = ABt, a.rho_tab = rho_tab, a.P = batch, a.resid = resid;
    return zm::mpc_rti(a, model, plant, zm::MpcRtiWork{xPlan, uPlan, A, B, c, K, Minv, D, ABt});
}
