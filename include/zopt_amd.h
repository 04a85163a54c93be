/* zopt_amd -- C ABI of the MI355X-native batched LQR / iLQR / MPC solve engine.
 *
 * The reference (zprihoda/zopt) is pure Python and has NO FFI layer: its boundary for this path is
 * the Python signatures of zopt/lqrUtils.py, zopt/ilqrUtils.py and zopt/mpcUtils.py.  This header is
 * the C-ABI a maintainer would bind underneath those signatures (ctypes stub: INTEGRATION.md).
 * Each entry point names the reference function (file:line) whose arithmetic it replaces.
 *
 * Conventions
 *   - All arrays are C-contiguous with the reference's time-first layout (lqrUtils.py:156-159) and ONE
 *     extra leading axis `batch` (new in the build; the reference is batch == 1).
 *   - `*_f64` entry points take DEVICE pointers (hipMalloc / torch ROCm `data_ptr()`), launch
 *     asynchronously on `stream` (a hipStream_t passed as void*, NULL = default stream) and return
 *     without synchronising.  `*_host_*` variants take HOST pointers, stage through device memory
 *     they allocate and free themselves, and synchronise before returning.
 *   - The caller owns every buffer; the library never retains a pointer after the call returns.
 *   - Return value: 0 = ok; <0 = ZM_E* below (bad argument / unsupported shape); >0 = hipError_t.
 *     `zm_last_error()` gives a thread-local message for the last non-zero return.
 *   - Numerics follow the reference: a singular `solve` propagates inf/NaN, nothing throws.
 */
#ifndef ZOPT_AMD_H
#define ZOPT_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZM_OK 0
#define ZM_EINVAL (-1)       /* null pointer, non-positive size */
#define ZM_EUNSUPPORTED (-2) /* shape outside what the compiled kernels cover (see zm_lqr_backward_supported) */

/* Library version (major*10000 + minor*100 + patch). */
int zm_version(void);

/* Thread-local description of the last error returned on this thread ("" if none). */
const char* zm_last_error(void);

/* Releases the few host-side resources the library keeps between calls (one pinned int32 + one event per device and concurrent
 * zm_ilqr_solve_f64 caller, used for the drivers' host round trips); returns how many were released.  Call it before unloading the
 * library or destroying the HIP context; calling it at any other time is harmless (the next solve re-creates what it needs). */
int zm_shutdown(void);

/* 1 if (n, m) is covered by the compiled LQR sweep kernels for the given element size, else 0.
 *   8 = fp64: tile-16 MFMA kernels for n <= 12, m <= 4 (the LDS-DMA fast path at n in {8, 12}, m = 4: ~1.5e9 steps/s at (12, 4));
 *             register-tile fp64 MFMA kernel for n <= 64, m <= 16: three tile rows with a prefetched operand set up to n = 48
 *             (54 M steps/s at (48, 16)), four tile rows without it for 48 < n <= 64 (17 M steps/s at (64, 16); the LDS-resident
 *             coverage kernel it replaced there ran 1.4 M and stays selectable with ZOPT_AMD_LQR_PATH=lds);
 *   4 = fp32: zm_lqr_backward_f32, n <= 64, m <= 16 (n in {8, 12}, m = 4 with 16-B aligned arrays: fp32 storage, fp64 arithmetic on
 *             the LDS-DMA ring kernel -- 1.8e9 steps/s at (12, 4); the other shapes up to 16: the fp32 MFMA tile kernel). */
int zm_lqr_backward_supported(int n, int m, int elem_size);

/* Batched discrete finite-horizon LQR backward Riccati recursion (Joseph-form value update).
 * Replaces: zopt/lqrUtils.py:144-173  discreteFiniteHorizonLqr(A, B, Q, R, N) -> L
 *     V <- Q[T-1];  for k = T-1..0:  L_k = solve(R_k + B_k^T V B_k, B_k^T V A_k)              (:168)
 *                                    V = Q_k + L_k^T R_k L_k + (A_k-B_k L_k)^T V (A_k-B_k L_k) (:169)
 * in : A (batch,T,n,n)  B (batch,T,n,m)  Q (batch,T,n,n)  R (batch,T,m,m)
 * out: L (batch,T,m,n)          control law u = -L x (lqrUtils.py:151)
 */
int zm_lqr_backward_f64(const double* A, const double* B, const double* Q, const double* R, double* L,
                        int64_t batch, int T, int n, int m, void* stream);

/* Finite-horizon LQR with bilinear cost (cross term H), affine dynamics (offset d) and linear costs (q, r).
 * Replaces: zopt/lqrUtils.py:207-262  bilinearAffineLqr(A, B, d, Q, R, H, q, r, q0, N) -> (L, l)
 *     carry (V, v) <- (Q[T-1], q[T-1]);  Su = r + v^T B + d^T V B   Suu = R + B^T V B   Sux = H + B^T V A   (:244-246)
 *     L = solve(Suu, Sux)  l = solve(Suu, Su)  V' = Q + A^T V A - L^T Suu L  v' = q + A^T (v + V d) - Sux^T l  (:248-252)
 * (q0 / v0 never influence L or l and are not taken.)          control law u = -L x - l
 * in : A (batch,T,n,n) B (batch,T,n,m) d (batch,T,n) Q (batch,T,n,n) R (batch,T,m,m) H (batch,T,m,n) q (batch,T,n) r (batch,T,m)
 * out: L (batch,T,m,n)  l (batch,T,m)
 */
int zm_lqr_backward_affine_f64(const double* A, const double* B, const double* d, const double* Q, const double* R,
                               const double* H, const double* q, const double* r, double* L, double* l,
                               int64_t batch, int T, int n, int m, void* stream);

/* Batched discrete-time infinite-horizon LQR (DARE) by Riccati value iteration from V = Q on registers.
 * Replaces: zopt/lqrUtils.py:176-204 discreteInfiniteHorizonLqr (SciPy solve_discrete_are + one solve).
 * in : A (batch,n,n)  B (batch,n,m)  Q (batch,n,n)  R (batch,m,m)   [device]; n <= 64, m <= 16 (n <= 12, m <= 4: K1's step with the
 *      operands in registers; beyond: the fp64 tile kernel's Joseph-form step on time-invariant operands; both stop on
 *      max|V' - V| <= tol max|V'|, tested every 4th (tile-16) / 8th (tile kernel) iteration and on the last allowed one)
 *      tol: stop when max|V' - V| <= tol * max|V'| (or at the rounding floor); max_iter: iteration cap
 * out: L (batch,m,n) with u = -L x;  P (batch,n,n) or NULL: the value matrix;
 *      iters (batch) or NULL: +k = converged after k iterations (also when k == max_iter), -k = the cap ended the loop after k
 *      iterations without the stopping test being met (the gain is then not a stationary one)
 */
int zm_dare_f64(const double* A, const double* B, const double* Q, const double* R, double* L, double* P, int32_t* iters,
                int64_t batch, int n, int m, double tol, int max_iter, void* stream);

/* Batched continuous-time infinite-horizon LQR (CARE  A^T P + P A - P B R^-1 B^T P + Q = 0) by the structure-preserving
 * doubling algorithm, one wave per design.
 * Replaces: zopt/lqrUtils.py:13-36 infiniteHorizonLqr (SciPy solve_continuous_are + one solve); with the integral-augmented
 *           system of lqrUtils.py:101-141 also infiniteHorizonIntegralLqr.
 * in : A (batch,n,n)  B (batch,n,m)  Q (batch,n,n)  R (batch,m,m)   [device]; n <= 16, m <= 16; Q, R symmetric
 *      tol: stop when max|P' - P| <= tol * max|P'|; max_iter: cap on doubling steps (each squares the contraction: ~10 suffice)
 * out: K (batch,m,n) = R^-1 B^T P with u = -K x;  P (batch,n,n) or NULL;
 *      info (batch) or NULL: doubling steps taken, -1 not converged, -2 singular pivot / no stabilising solution
 */
int zm_care_f64(const double* A, const double* B, const double* Q, const double* R, double* K, double* P, int32_t* info,
                int64_t batch, int n, int m, double tol, int max_iter, void* stream);

/* Batched continuous-time finite-horizon LQR value function: dV/dt = -Q + V S V - V A - A^T V, V(T) = Qf, S = B R^-1 B^T,
 * integrated backwards with an adaptive Dormand-Prince 5(4) pair, output at t_j = j T / (N - 1), j = 0..N-1.
 * Replaces: zopt/lqrUtils.py:39-98 finiteHorizonLqr (_lqrHjb + jax.experimental.ode.odeint; its gain interpolation,
 *           jaxUtils.py:7-24, stays on the host side of the boundary).
 * in : A_s, Q_s (batch,n_samples,n,n), B_s (batch,n_samples,n,m), Rinv_s (batch,n_samples,m,m) [device]: coefficients sampled
 *      at linspace(0, T, n_samples), linear in between (n_samples = 1: time-invariant);  Qf (batch,n,n);  n <= 16, m <= 16;
 *      rtol, atol: local error control (odeint: 1.4e-8 both)
 * out: V (batch,N,n,n);  info (batch) or NULL: integration steps taken, -1 step cap reached, -2 NaN (finite escape time)
 */
int zm_riccati_ode_f64(const double* A_s, const double* B_s, const double* Rinv_s, const double* Q_s, const double* Qf,
                       double* V, int32_t* info, int64_t batch, int n, int m, int n_samples, int N, double T, double rtol,
                       double atol, int max_steps, void* stream);

/* fp32 batched finite-horizon LQR backward sweep (n <= 64, m <= 16): the fp32 MFMA tile kernel; at the fast-path shapes (n in {8, 12},
 * m = 4, 16-B aligned arrays) the LDS-DMA ring kernel on fp32 storage with fp64 arithmetic (the fp64 result rounded once).
 * Replaces: zopt/lqrUtils.py:144-173 discreteFiniteHorizonLqr when JAX runs in its default fp32 mode (x64 disabled, quirk Q8);
 *           the "large-state stress" shape n=64, m=16, T=200 of BASELINE configs[4].
 * in : A (batch,T,n,n)  B (batch,T,n,m)  Q (batch,T,n,n)  R (batch,T,m,m)   [device, C-contiguous float]
 * out: L (batch,T,m,n)
 */
int zm_lqr_backward_f32(const float* A, const float* B, const float* Q, const float* R, float* L, int64_t batch, int T, int n,
                        int m, void* stream);

/* zm_lqr_backward_f64 with HOST pointers (NumPy arrays): allocates device staging, copies in, solves, copies L back. */
int zm_lqr_backward_host_f64(const double* A, const double* B, const double* Q, const double* R, double* L,
                             int64_t batch, int T, int n, int m);

/* Batched iLQR backward pass: affine policy (l, L) from the quadratic model along a trajectory.
 * Replaces: zopt/ilqrUtils.py:153-181  riccatiStep_ilqr / backwardPass_ilqr(dynamics, cost, Vf) -> AffinePolicy
 *     Q_x = c_x + f_x^T v_x   Q_u = c_u + f_u^T v_x   Q_xx = c_xx + f_x^T v_xx f_x   Q_uu = c_uu + f_u^T v_xx f_u
 *     Q_ux = c_ux + f_u^T v_xx f_x   l = -solve(Q_uu, Q_u)   L = -solve(Q_uu, Q_ux)                     (:160-168)
 *     v_x' = Q_x - L^T Q_uu l        v_xx' = Q_xx - L^T Q_uu L                                          (:170)
 * (the scalar terms c, v and AffineDynamics.f do not influence the returned policy and are not taken)
 * in : f_x (batch,T,n,n) f_u (batch,T,n,m)                          AffineDynamics   (pytrees.py:129-136)
 *      c_x (batch,T,n) c_u (batch,T,m) c_xx (batch,T,n,n) c_ux (batch,T,m,n) c_uu (batch,T,m,m)   QuadraticCostFunction (:84-98)
 *      vf_x (batch,n) vf_xx (batch,n,n)                             QuadraticValueFunction Vf (:58-69)
 * out: l (batch,T,m)  L (batch,T,m,n)                               AffinePolicy (:207-213), u = alpha*l + L dx + uPrev
 * Shapes: n <= 12, m <= 4 on the tile-16 kernels (LDS-DMA ring at n in {8, 12}, m = 4); beyond, up to n <= 48, m <= 16, on the fp64
 * MFMA tile sweep (sweep_tiled_f64.hip: V, [f_x | f_u] and every product as 16 x 16 register tiles, one wave per trajectory);
 * ZM_EUNSUPPORTED above.  zm_lqr_backward_affine_f64 takes the same shapes.
 */
int zm_ilqr_backward_f64(const double* f_x, const double* f_u, const double* c_x, const double* c_u,
                         const double* c_xx, const double* c_ux, const double* c_uu, const double* vf_x,
                         const double* vf_xx, double* l, double* L, int64_t batch, int T, int n, int m, void* stream);

/* ---- registered device models (the reference differentiates / rolls out arbitrary Python callables with JAX;
 *      a kernel needs the model in device code) ------------------------------------------------------------------ */
#define ZM_MODEL_LINEAR 1     /* x+ = A x + B u, A (n,n), B (n,m) device pointers shared by the whole batch           */
#define ZM_MODEL_QUADCOPTER 2 /* x+ = x + dt * Quadcopter.inertialDynamics(x,u)  (zopt/quadcopter.py:116-144), n=12, m=4; dt = 0: the derivative */
#define ZM_MODEL_QUADCOPTER_RB 3 /* same with Quadcopter.rigidBodyDynamics (:70-113), n=8, m=4; wind_ned holds the BODY-frame wind */
/* ZM_MODEL_TRACED: x+ = f(x, u) or f(x, u, p) for a user-written straight-line expression, recorded once on the host (Python:
 * zopt_amd.models.TracedModel) and evaluated by an interpreter inside the kernels on double, dual and hyper-dual numbers -- the part
 * jax.jit / jax.jacobian / jax.hessian play for the reference's callables (zopt/ilqrUtils.py:260-269, pytrees.py:139-194).
 *   tape:  ONE device buffer of 8-byte words: n_const fp64 constants, then n_instr 32-bit instruction words, then n 32-bit output
 *          slot numbers.  An instruction is  op | a_is_const << 6 | b_is_const << 7 | dst << 8 | a << 16 | b << 24  with op in
 *          0 add, 1 sub, 2 mul, 3 div, 4 neg, 5 sin, 6 cos, 7 tan, 8 sqrt, 9 mov (unary: a only); dst, a, b index the slot file, an
 *          operand flagged as a constant the constant table.  Slots 0 .. n-1 hold x, n .. n+m-1 hold u, the next n_params hold p;
 *          no instruction writes them, and none reads a slot before it is written (the recorder guarantees both; the host entry
 *          points check the counts and pointers, not the words).
 *   caps:  n <= 12, m <= 4, n_params <= 8, n_instr <= 1024, n + m + n_params <= n_slots <= 64, n_const <= 256.
 *   params: (.., n_params) device doubles, row of trajectory t at params + t * param_stride (0: one row shared by the batch); NULL
 *          when n_params == 0.  Per-problem constants: no derivative is taken with respect to them.
 *   `reserved` holds the structural mask of zm_model_nonlinear_mask (the variables f is not affine in); no Hessian pairs are declared.
 * Taken by zm_rollout_linesearch(_list)_f64, zm_linearize_dynamics(_list)_f64, zm_quadratic_dynamics(_list)_f64, zm_model_step_f64
 * and zm_ilqr_solve(_trace)_f64 (ddp = 0 / 1); ZM_EUNSUPPORTED from the tracking, box, state, packed-pair and MPC entry points. */
#define ZM_MODEL_TRACED 4
#define ZM_TRACED_MAX_INSTR 1024
#define ZM_TRACED_MAX_SLOTS 64
#define ZM_TRACED_MAX_CONSTS 256
#define ZM_TRACED_MAX_PARAMS 8
typedef struct zm_traced_t {    /* 40 bytes, held in the bytes of zm_model_t's A, B and wind_ned (offset 24) when kind == ZM_MODEL_TRACED */
    const void* tape;
    const double* params;
    int64_t param_stride;
    int32_t n_instr, n_const;
    int32_t n_slots, n_params;
} zm_traced_t;
typedef struct zm_model_t {     /* 64 bytes whatever the kind: every kernel takes the struct by value */
    int kind, n, m, reserved;   /* reserved: 0; traced: the structural mask (bit i state i, bit n + j control j) */
    double dt;              /* quadcopter: Euler step (demos/iterativeLqr.py:23,35) */
    const double* A;        /* linear: device pointers; else NULL.  traced: A, B and wind_ned are the storage of a zm_traced_t -- */
    const double* B;        /*   fill it with memcpy(&model.A, &descriptor, sizeof(zm_traced_t)); the fields keep their declarations */
    double wind_ned[3];     /* quadcopter: constant wind in the north-east-down frame (quadcopter.py:117,138; the closed-loop
                               simulation of demos/iterativeLqr.py:48 uses (3,1,0)); zeros for the solvers */
} zm_model_t;

/* c(x,u) = x^T Q x + u^T R u,  c_f(x) = x^T Qf x  (demos/iterativeLqr.py:12-13,37; no 1/2).  Device pointers. */
typedef struct zm_quadcost_t {
    const double* Q;        /* (n,n) */
    const double* R;        /* (m,m) */
    const double* Qf;       /* (n,n) */
    int32_t diagonal;       /* 1: the caller asserts that Q, R and Qf are diagonal (the demos' weights) -- off-diagonal entries are
                               then never read and the rollout runs a leaner kernel; 0: unknown, the kernels look for themselves */
    int32_t reserved;
} zm_quadcost_t;

/* Batched policy rollout with a parallel line search over step sizes.
 * Replaces: zopt/ilqrUtils.py:33-66 trajectoryRollout (n_alpha = 1, cost may be NULL) and :116-150 forwardPass2
 *           (n_alpha = 16, alphas = 0.5^j), with AffinePolicy.__call__ (pytrees.py:215-220) and CostFunction.__call__
 *           (pytrees.py:49-52):
 *     for each alpha:  x_0 = x0;  u_k = alpha*l_k + L_k (x_k - xPrev_k) + uPrev_k;  x_{k+1} = f(x_k, u_k)
 *                      J = sum_k c(x_k,u_k) + c_f(x_T);        result = the rollout with the smallest J (NaN wins, as argmin)
 * in : x0 (batch,n)  l (batch,T,m)  L (batch,T,m,n)  xPrev (batch,T+1,n)  uPrev (batch,T,m)  alphas (n_alpha) [device]
 *      active (batch) int32 or NULL: trajectories with active==0 are skipped (their outputs are left untouched)
 * out: xTraj (batch,T+1,n)  uTraj (batch,T,m)  J (batch) or NULL  alpha_idx (batch) int32 or NULL
 * Shapes: registered models with n <= 12, m <= 4 (one lane per rollout; the (12, 4) fast paths of rollout_fast.hip / rollout_quad.hip);
 *      ZM_MODEL_LINEAR also beyond, up to n <= 64, m <= 16 (rollout_wide.hip: one wave per rollout, lane i owns state i; four waves
 *      per trajectory share the 16 step sizes, the winner is rolled out once more with stores; no scratch).
 */
int zm_rollout_linesearch_f64(const zm_model_t* model, const zm_quadcost_t* cost, const double* x0, const double* l,
                              const double* L, const double* xPrev, const double* uPrev, const double* alphas,
                              int n_alpha, const int32_t* active, double* xTraj, double* uTraj, double* J,
                              int32_t* alpha_idx, int64_t batch, int T, void* stream);

/* Same, over a compacted list of trajectory ids: only list[0..count) are processed (densely packed into waves), all
 * other trajectories keep their outputs.  Arrays keep their full (batch, ...) shapes and are indexed by trajectory id.
 * Used by the iLQR / DDP drivers once most of the batch has converged (a mask would leave mostly idle waves).  `active`
 * (batch) int32 or NULL: listed trajectories with active == 0 are skipped as well, so a list may be a few iterations old. */
int zm_rollout_linesearch_list_f64(const zm_model_t* model, const zm_quadcost_t* cost, const double* x0, const double* l,
                                   const double* L, const double* xPrev, const double* uPrev, const double* alphas,
                                   int n_alpha, const int32_t* list, int64_t count, const int32_t* active, double* xTraj,
                                   double* uTraj, double* J, int32_t* alpha_idx, int64_t batch, int T, void* stream);

/* Acceptance step of the iLQR / DDP loop (zopt/ilqrUtils.py:316-320) for the trajectories in list[0..count):
 *     converged = |J - Jn| <= tol;  J <- Jn;  xTraj <- xTrajNew;  uTraj <- uTrajNew;  active <- !converged
 * Arrays keep their (batch, ...) shapes; rows of trajectories not listed -- or listed but with active == 0 -- are left untouched. */
int zm_ilqr_accept_f64(const int32_t* list, int64_t count, double* J, const double* Jn, double* xTraj, const double* xTrajNew,
                       double* uTraj, const double* uTrajNew, int32_t* converged, int32_t* active, double tol, int64_t batch,
                       int T, int n, int m, void* stream);

/* First-order expansion of a registered model along a trajectory.
 * Replaces: zopt/pytrees.py:139-153 AffineDynamics.from_function / from_trajectory (jax.jacobian of dynFun at
 *           (xTraj[:-1], uTraj)):  f = dynFun(x_k,u_k), f_x = d dynFun/dx, f_u = d dynFun/du.
 * in : xTraj (batch,T+1,n)  uTraj (batch,T,m)   active (batch) int32 or NULL (inactive trajectories are skipped)
 * out: f (batch,T,n) or NULL   f_x (batch,T,n,n)   f_u (batch,T,n,m)
 */
int zm_linearize_dynamics_f64(const zm_model_t* model, const double* xTraj, const double* uTraj, const int32_t* active,
                              double* f, double* f_x, double* f_u, int64_t batch, int T, void* stream);

/* Second-order expansion of the registered quadratic cost along a trajectory, and of the terminal cost at x_T.
 * Replaces: zopt/pytrees.py:100-115 QuadraticCostFunction.from_function / from_trajectory and :72-81
 *           QuadraticValueFunction.fromTerminalCostFunction for c = x'Qx + u'Ru, c_f = x'Qf x:
 *     c_x = (Q+Q')x  c_u = (R+R')u  c_xx = Q+Q'  c_ux = 0  c_uu = R+R'    v = x'Qf x  v_x = (Qf+Qf')x  v_xx = Qf+Qf'
 * The Hessians do not depend on the trajectory: they are written ONCE (c_xx (n,n), c_ux (m,n), c_uu (m,m),
 * v_xx (n,n)) and consumed with `shared_hessian = 1` by zm_ilqr_backward_ex_f64.
 * in : xTraj (batch,T+1,n)  uTraj (batch,T,m)  active or NULL
 * out: c (batch,T)  c_x (batch,T,n)  c_u (batch,T,m)  v (batch)  v_x (batch,n)   (each may be NULL)
 *      c_xx (n,n)  c_ux (m,n)  c_uu (m,m)  v_xx (n,n)                              (each may be NULL)
 */
int zm_quadratize_cost_f64(const zm_quadcost_t* cost, int n, int m, const double* xTraj, const double* uTraj,
                           const int32_t* active, double* c, double* c_x, double* c_u, double* v, double* v_x,
                           double* c_xx, double* c_ux, double* c_uu, double* v_xx, int64_t batch, int T, void* stream);

/* zm_ilqr_backward_f64 with (a) an `active` mask (inactive trajectories keep their previous l, L) and
 * (b) `shared_hessian` != 0: c_xx (n,n), c_ux (m,n), c_uu (m,m) and vf_xx (n,n) are single matrices shared by every
 * trajectory and step (time-invariant quadratic cost) instead of (batch,T,.,.) / (batch,.,.) arrays. */
int zm_ilqr_backward_ex_f64(const double* f_x, const double* f_u, const double* c_x, const double* c_u,
                            const double* c_xx, const double* c_ux, const double* c_uu, const double* vf_x,
                            const double* vf_xx, const int32_t* active, int shared_hessian, double* l, double* L,
                            int64_t batch, int T, int n, int m, void* stream);

/* Batched DDP backward pass: zm_ilqr_backward_ex_f64 plus the second-order dynamics terms.
 * Replaces: zopt/ilqrUtils.py:184-214 riccatiStep_ddp / backwardPass_ddp and :237-251 conditionQuadraticDynamics:
 *     vf_.. = einsum('i,ijk', v_x, f_..);  [[vf_xx, vf_ux^T],[vf_ux, vf_uu]] <- ensurePositiveDefinite(.)  per step,
 *     Q_xx += vf_xx, Q_uu += vf_uu, Q_ux += vf_ux, then the iLQR step.
 * in : as zm_ilqr_backward_ex_f64, plus QuadraticDynamics (pytrees.py:165-177)
 *      f_xx (batch,T,n,n,n)  f_ux (batch,T,n,m,n)  f_uu (batch,T,n,m,m)     [f_..[i,j,k] = d2 f_i / d._j d._k]
 *      (f_ux and f_uu both NULL: identically zero, i.e. dynamics affine in the controls)
 * out: l (batch,T,m)  L (batch,T,m,n)
 */
int zm_ddp_backward_f64(const double* f_x, const double* f_u, const double* f_xx, const double* f_ux, const double* f_uu,
                        const double* c_x, const double* c_u, const double* c_xx, const double* c_ux, const double* c_uu,
                        const double* vf_x, const double* vf_xx, const int32_t* active, int shared_hessian, double* l,
                        double* L, int64_t batch, int T, int n, int m, void* stream);

/* The same sweeps, also returning the quadratic value function they end with -- what the reference's single-step helpers
 * riccatiStep_ilqr (ilqrUtils.py:153-173) and riccatiStep_ddp (:184-206) return next to the policy (T = 1), and the value at the
 * trajectory start for T > 1:   v' = (c + v) - 1/2 l^T Q_uu l,  v_x' = Q_x - L^T Q_uu l,  v_xx' = Q_xx - L^T Q_uu L   (:170).
 * in : as zm_ilqr_backward_f64, plus c (batch,T) or NULL and vf (batch) or NULL (the scalar terms);
 *      f_xx, f_ux, f_uu all NULL: iLQR step; all given: DDP step (PD-projected second-order dynamics terms)
 * out: l, L as before;  v_out (batch), vx_out (batch,n), vxx_out (batch,n,n), each may be NULL  * Shapes: n <= 12, m <= 4; the iLQR form (f_xx == f_ux == f_uu == NULL) also up to n <= 48, m <= 16 on the tile sweep (sweep_tiled_f64.hip;
 * the three value outputs are then required).
 */
int zm_riccati_value_f64(const double* f_x, const double* f_u, const double* f_xx, const double* f_ux, const double* f_uu,
                         const double* c, const double* c_x, const double* c_u, const double* c_xx, const double* c_ux,
                         const double* c_uu, const double* vf, const double* vf_x, const double* vf_xx, double* l, double* L,
                         double* v_out, double* vx_out, double* vxx_out, int64_t batch, int T, int n, int m, void* stream);

/* zm_ilqr_backward_ex_f64 / zm_ddp_backward_f64 over a compacted list of trajectory ids: one wave per LISTED trajectory (grid =
 * count), so that the few hundred stragglers of a solve spread over the whole chip instead of sharing SIMDs among 8192 mostly idle
 * blocks.  Arrays keep their (batch, ...) shapes; listed trajectories with active == 0 are skipped; list == NULL: all of them. */
int zm_ilqr_backward_list_f64(const double* f_x, const double* f_u, const double* c_x, const double* c_u, const double* c_xx,
                              const double* c_ux, const double* c_uu, const double* vf_x, const double* vf_xx, const int32_t* list,
                              int64_t count, const int32_t* active, int shared_hessian, double* l, double* L, int64_t batch, int T,
                              int n, int m, void* stream);
int zm_ddp_backward_list_f64(const double* f_x, const double* f_u, const double* f_xx, const double* f_ux, const double* f_uu,
                             const double* c_x, const double* c_u, const double* c_xx, const double* c_ux, const double* c_uu,
                             const double* vf_x, const double* vf_xx, const int32_t* list, int64_t count, const int32_t* active,
                             int shared_hessian, double* l, double* L, int64_t batch, int T, int n, int m, void* stream);

/* The three expansions over a compacted list of trajectory ids (as zm_rollout_linesearch_list_f64): only list[0..count) are expanded
 * -- the grids shrink with the list -- all arrays keep their full (batch, ...) shapes and are indexed by trajectory id; listed
 * trajectories with active == 0 are skipped.  list == NULL: every trajectory, i.e. the plain entry points below / above. */
int zm_linearize_dynamics_list_f64(const zm_model_t* model, const double* xTraj, const double* uTraj, const int32_t* list,
                                   int64_t count, const int32_t* active, double* f, double* f_x, double* f_u, int64_t batch, int T,
                                   void* stream);
int zm_quadratize_cost_list_f64(const zm_quadcost_t* cost, int n, int m, const double* xTraj, const double* uTraj,
                                const int32_t* list, int64_t count, const int32_t* active, double* c, double* c_x, double* c_u,
                                double* v, double* v_x, double* c_xx, double* c_ux, double* c_uu, double* v_xx, int64_t batch,
                                int T, void* stream);
int zm_quadratic_dynamics_list_f64(const zm_model_t* model, const double* xTraj, const double* uTraj, const int32_t* list,
                                   int64_t count, const int32_t* active, double* f_xx, double* f_ux, double* f_uu, int64_t batch,
                                   int T, void* stream);

/* Variables in which a registered model is NOT affine: bit i = state i, bit n + j = control j.  Only pairs of these have a nonzero
 * second derivative -- the second-order expansion evaluates only those pairs, and a driver need not materialise the zero blocks. */
int zm_model_nonlinear_mask(const zm_model_t* model, uint32_t* mask);

/* Second-order expansion of a registered model along a trajectory (forward-mode hyper-dual numbers).
 * Replaces: zopt/pytrees.py:180-194 QuadraticDynamics.from_function / from_trajectory (jax.hessian of dynFun):
 * in : xTraj (batch,T+1,n)  uTraj (batch,T,m)  active or NULL
 * out: f_xx (batch,T,n,n,n)  f_ux (batch,T,n,m,n)  f_uu (batch,T,n,m,m)
 *      f_ux and f_uu may both be NULL for a model that is affine in its controls (no control bit in zm_model_nonlinear_mask):
 *      they are identically zero and zm_ddp_backward_f64 / zm_riccati_value_f64 take NULL for them as well.
 */
int zm_quadratic_dynamics_f64(const zm_model_t* model, const double* xTraj, const double* uTraj, const int32_t* active,
                              double* f_xx, double* f_ux, double* f_uu, int64_t batch, int T, void* stream);

/* Batched trim of the quadcopter (the producer side of the path).
 * Replaces: zopt/quadcopter.py:146-177 Quadcopter.trim(uvwTrim): find x = [uvw, p,q,r,phi,theta], u = [thrust,mx,my,mz] with
 *           rigidBodyDynamics(x, u) = 0 (the reference minimises the squared residual with SciPy BFGS; its test accepts
 *           |residual| <= 1e-3).  Levenberg-Marquardt from the reference's start point, one lane per instance.
 * in : uvw (batch,3) [device]; wind_body (3) HOST pointer or NULL (body-frame wind, zeros in the reference's trim)
 * out: xTrim (batch,8)  uTrim (batch,4)  resid (batch) = |rigidBodyDynamics|_2 or NULL  ok (batch) int32 (resid <= tol) or NULL */
int zm_quadcopter_trim_f64(const double* uvw, const double* wind_body, double* xTrim, double* uTrim, double* resid, int32_t* ok,
                           int64_t batch, double tol, void* stream);

/* Batched projection onto the positive definite cone: A <- V max(w, eps) V^T with (w, V) = eigh((A + A^T)/2).
 * Replaces: zopt/ilqrUtils.py:217-219 ensurePositiveDefinite (jnp.linalg.eigh symmetrises its input) and its users
 *           :254-257 conditionValueFunction (k = n).       in/out: A (count,k,k) in place, k <= 64: one wave per matrix, matrix-sign
 *           iterations on fp64 MFMA tiles instead of an eigen-decomposition -- one 16 x 16 tile up to k = 16 (psd.hip, ns16.h), NT x NT
 *           tiles beyond (psd_tiled.hip; the same iteration, constants and caps).  zm_condition_cost_f64 likewise for n + m <= 64;
 *           zm_condition_dynamics_f64 (the DDP path) stays at n + m <= 16.
 */
int zm_psd_project_f64(double* A, int64_t count, int k, double eps, void* stream);

/* Same projection applied to the stacked cost Hessian [[c_xx, c_ux^T],[c_ux, c_uu]] of every step, written back
 * into its blocks.  Replaces: zopt/ilqrUtils.py:222-234 conditionQuadraticCost.
 * in/out: c_xx (count,n,n)  c_ux (count,m,n)  c_uu (count,m,m) in place (count = batch*T, or 1 for a shared Hessian)
 */
int zm_condition_cost_f64(double* c_xx, double* c_ux, double* c_uu, int64_t count, int n, int m, double eps,
                          void* stream);

/* Second-order dynamics terms of the DDP step, PD-conditioned.
 * Replaces: zopt/ilqrUtils.py:237-251 conditionQuadraticDynamics(quadratic_dynamics, v_x):
 *     vf_.. = einsum('i,ijk', v_x, f_..);  [[vf_xx, vf_ux^T],[vf_ux, vf_uu]] <- ensurePositiveDefinite(.);  blocks sliced back
 * in : f_xx (count,n,n,n)  f_ux (count,n,m,n)  f_uu (count,n,m,m)  v_x (count,n)
 * out: vf_xx (count,n,n)  vf_ux (count,m,n)  vf_uu (count,m,m) */
int zm_condition_dynamics_f64(const double* f_xx, const double* f_ux, const double* f_uu, const double* v_x, double* vf_xx,
                              double* vf_ux, double* vf_uu, int64_t count, int n, int m, double eps, void* stream);

/* ---- box-constrained LQ-MPC (reference: zopt/mpcUtils.py:12-81, class lqrMpc; the reference hands this QP to
 *      cvxpy -> OSQP, whose arithmetic is not in the reference tree: numeric parity is "unpinned", acceptance is by KKT
 *      residuals -- see DESIGN.md) -------------------------------------------------------------------------------
 *   min  sum_{k<N} (x_k'Q x_k + u_k'R u_k) + x_N'Qf x_N        (mpcUtils.py:52-54, no 1/2)
 *   s.t. x_{k+1} = A x_k + B u_k,  x_lb <= x_k <= x_ub (k = 0..N),  u_lb <= u_k <= u_ub,  x_0 = x0      (:55-58)
 * Method: ADMM on the splitting {dynamics-feasible trajectory w} / {box copy y}; the w-update is an LQ tracking
 * problem solved exactly by a Riccati factorisation that does not depend on the iterates (zm_mpc_setup_f64, once per
 * problem), so one ADMM iteration is an affine backward sweep + a forward rollout + a clip.
 */
#define ZM_MPC_OPTIMAL 1            /* cvxpy status "optimal"            */
#define ZM_MPC_INFEASIBLE 2         /* "infeasible"                      */
#define ZM_MPC_USER_LIMIT 3         /* "user_limit" (max_iter reached)   */
#define ZM_MPC_OPTIMAL_INACCURATE 4 /* "optimal_inaccurate": max_iter reached with both residuals within 10x their tolerances -- OSQP's
                                       "solved inaccurate", which cvxpy reports under this name (mpcUtils.py:74,78).  The rest of cvxpy's
                                       vocabulary cannot arise here: "unbounded" needs a direction of unbounded descent, which a cost
                                       with Q, Qf >= 0 and R > 0 over dynamics-feasible trajectories does not have, and
                                       "infeasible_inaccurate" is reported as "user_limit" (an uncertified instance at the cap) */

/* Riccati tables of the ADMM w-update for penalty rho:  K (N,m,n), Minv (N,m,m)   [all device pointers]
 * in : A (n,n) B (n,m) Q (n,n) R (m,m) Qf (n,n); n <= 24, m <= 8.
 * The weights Q, R, Qf (and Qs, Rs of the stage-varying entry points below) must be SYMMETRIC: the setup forms the Hessians as 2 W, the
 * tracking kernels the linear term with W + W', and the recursion stores its value matrix symmetrised -- P_N = 2 Qf + rho I,
 * P <- sym((2 Q + rho I) + A'PA - (B'PA)' K), sym(X) = (X + X') / 2 -- which removes the antisymmetric rounding error that an
 * open-loop-unstable A would otherwise amplify along the horizon.  (The Python mirror passes the symmetric part of what it is given.)
 * Shapes of the solve entry points: (n, m) in {(12,4), (8,4), (4,2), (4,1), (2,2), (2,1), (1,1)} (16 lanes per instance, adaptive penalty
 * levels; the Python mirror embeds any smaller shape with inert padding) and (24, 8) (one lane per instance, the penalty of `level0`
 * only; registers + scratch: a coverage path for problems beyond the 16-index tile). */
int zm_mpc_setup_f64(const double* A, const double* B, const double* Q, const double* R, const double* Qf, double rho,
                     int N, int n, int m, double* K, double* Minv, void* stream);

/* Solve `batch` instances (one per initial state) of the QP above.
 * in : A, B (shared), K, Minv from zm_mpc_setup_f64 (same rho), bounds x_lb, x_ub (n), u_lb, u_ub (m) (+-inf allowed),
 *      x0 (batch,n); workspace: 4 * batch * N * (n+m) doubles
 * out: xTraj (batch,N+1,n)  uTraj (batch,N,m)  status (batch) ZM_MPC_*  iters (batch) or NULL
 *      resid (batch,2) = final (primal, dual) residual inf-norms, or NULL
 */
int zm_mpc_solve_f64(const double* A, const double* B, const double* K, const double* Minv, const double* x_lb,
                     const double* x_ub, const double* u_lb, const double* u_ub, const double* x0, double rho,
                     double eps_abs, double eps_rel, double eps_prim_inf, int max_iter, double* workspace, double* xTraj,
                     double* uTraj,
                     int32_t* status, int32_t* iters, double* resid, int64_t batch, int N, int n, int m, void* stream);

/* Same, with OSQP-style warm starting (cvxpy's default `warm_start=True`, mpcUtils.py:77): with warm_start != 0 the
 * workspace must be the one a previous call for the same (batch, N, n, m, rho) left behind; its iterates (box copy y,
 * scaled dual lam) start the ADMM instead of zeros; warm_start == 2 additionally advances them by one horizon step
 * (iterate k <- iterate k+1, the last one repeated), the natural guess when x0 is the previous plan's x_1 as in the
 * receding-horizon loop (demos/lqrMpc.py:41-48).  Only instances whose previous solve ended "optimal" are warm-started. */
int zm_mpc_solve_warm_f64(const double* A, const double* B, const double* K, const double* Minv, const double* x_lb,
                          const double* x_ub, const double* u_lb, const double* u_ub, const double* x0, double rho,
                          double eps_abs, double eps_rel, double eps_prim_inf, int max_iter, int warm_start,
                          double* workspace, double* xTraj, double* uTraj, int32_t* status, int32_t* iters, double* resid,
                          int64_t batch, int N, int n, int m, void* stream);

/* Same, with OSQP's adaptive penalty (`adaptive_rho`, on by default in OSQP / cvxpy): K and Minv hold the tables of
 * zm_mpc_setup_f64 for n_levels penalties rho * rho_step^(l - level0), level-major (n_levels, N, m, n) / (n_levels, N, m, m).
 * Every 8 iterations an instance moves to the level nearest (on the log scale) rho * sqrt(primal / dual residual ratio),
 * rescaling its scaled dual.  n_levels = 1 is the fixed-penalty solve above. */
int zm_mpc_solve_adaptive_f64(const double* A, const double* B, const double* K, const double* Minv, int n_levels, int level0,
                              double rho_step, const double* x_lb, const double* x_ub, const double* u_lb, const double* u_ub,
                              const double* x0, double rho, double eps_abs, double eps_rel, double eps_prim_inf, int max_iter,
                              int warm_start, double* workspace, double* xTraj, double* uTraj, int32_t* status, int32_t* iters,
                              double* resid, int64_t batch, int N, int n, int m, void* stream);

/* Second derivatives in PACKED form, for models that declare which variable pairs can have a nonzero second derivative.
 * zm_model_hessian_pairs: pairs (2 * npairs int32, host, may be NULL) <- (a, b), a <= b, in the stacked variable index (states
 *     0..n-1, controls n..n+m-1); npairs (host) <- their number, 0 if the model declares none.  The quadcopter declares 28.
 * zm_quadratic_dynamics_pairs_list_f64: H (batch,T,npairs,n) <- d2 f_i / dz_a dz_b: the nonzero entries of
 *     QuadraticDynamics.from_trajectory's f_xx / f_ux / f_uu (zopt/pytrees.py:180-194), 2 688 B per point for the quadcopter
 *     instead of 19 968 B of mostly zeros; `list` / `active` as in zm_quadratic_dynamics_list_f64 (list may be NULL).
 * zm_ddp_backward_pairs_list_f64: zm_ddp_backward_list_f64 (zopt/ilqrUtils.py:184-214, 237-251) reading H instead of the three
 *     tensors -- the contraction sum_i v_x[i] H[p][i] runs in the same order, so the policy is bitwise the same.  Used by
 *     zm_ilqr_solve_f64; the array-level API (full tensors) is zm_ddp_backward_f64. */
int zm_model_hessian_pairs(const zm_model_t* model, int32_t* pairs, int32_t* npairs);
int zm_quadratic_dynamics_pairs_list_f64(const zm_model_t* model, const double* xTraj, const double* uTraj, const int32_t* list,
                                         int64_t count, const int32_t* active, double* H, int64_t batch, int T, void* stream);
int zm_ddp_backward_pairs_list_f64(const zm_model_t* model, const double* f_x, const double* f_u, const double* H,
                                   const double* c_x, const double* c_u, const double* c_xx, const double* c_ux,
                                   const double* c_uu, const double* vf_x, const double* vf_xx, const int32_t* list, int64_t count,
                                   const int32_t* active, int shared_hessian, double* l, double* L, int64_t batch, int T,
                                   void* stream);

/* The whole iLQR / DDP solve of a batch as one call: the outer loop of zopt/ilqrUtils.py:290-327 (iterativeLqr, ddp = 0) and
 * :360-397 (differentialDynamicProgramming, ddp != 0) for a registered model and quadratic cost -- initial rollout of
 * (uGuess, L = 0), then per iteration the expansions along the trajectory, the PD-conditioned Hessians, the backward pass, the
 * 16-way line search and `converged = |J - J_new| <= tol`, each over the compacted list of the trajectories that have not
 * converged yet (rebuilt on the device every `sync_every` >= 1 iterations; results do not depend on it).
 * HOST-SYNCHRONOUS, unlike the other `*_f64` entry points: the host side of the loop runs inside this call and BLOCKS the calling
 * thread on an event every `sync_every` iterations (it must learn how many trajectories are left to size the next launches), so the
 * call returns only when the loop has ended -- after `max_iter` iterations or once every trajectory has converged -- with the last
 * iteration's kernels and the final collect possibly still queued on `stream` (synchronise it before reading the outputs).  Work
 * queued on OTHER streams overlaps as usual.
 * in : x0 (batch,n)  uGuess (batch,T,m)  [device]
 *      workspace: at least zm_ilqr_solve_workspace_f64(model, batch, T, ddp) doubles, 16-B aligned [device]
 *      iwork: 2 * batch + 2 int32 [device]
 * out: xTraj (batch,T+1,n)  uTraj (batch,T,m)  L (batch,T,m,n)  J (batch)  converged (batch) int32  [device]
 *      iterations: HOST int32 or NULL -- iterations the loop ran (<= max_iter) */
int64_t zm_ilqr_solve_workspace_f64(const zm_model_t* model, int64_t batch, int T, int ddp);
int zm_ilqr_solve_f64(const zm_model_t* model, const zm_quadcost_t* cost, const double* x0, const double* uGuess, int ddp,
                      int max_iter, double tol, int sync_every, double* workspace, int64_t workspace_doubles, int32_t* iwork,
                      double* xTraj, double* uTraj, double* L, double* J, int32_t* converged, int32_t* iterations, int64_t batch,
                      int T, void* stream);
/* The same solve with a per-iteration record (diagnostics; the parity tests compare it with the oracle loop iteration by
 * iteration, zopt/ilqrUtils.py:305-322): J_trace (max_iter, batch) [device, may be NULL]: row i <- every trajectory's cost after
 * iteration i's acceptance step (`J_new` of :316-320; the cost it retired with once it has converged); alpha_trace (max_iter, batch)
 * int32 [device, may be NULL]: row i <- index into 0.5**arange(16) of the step size forwardPass2's argmin picked (:145-149),
 * meaningful for the trajectories that were still active in iteration i.  Rows >= *iterations are not written. */
int zm_ilqr_solve_trace_f64(const zm_model_t* model, const zm_quadcost_t* cost, const double* x0, const double* uGuess, int ddp,
                            int max_iter, double tol, int sync_every, double* workspace, int64_t workspace_doubles, int32_t* iwork,
                            double* xTraj, double* uTraj, double* L, double* J, int32_t* converged, int32_t* iterations,
                            int64_t batch, int T, void* stream, double* J_trace, int32_t* alpha_trace);

/* ---- tracking cost: the quadratic cost about a goal or a reference trajectory -------------------------------------------------
 *     J = sum_{k<T} (x_k - xr_k)'Q(x_k - xr_k) + (u_k - ur_k)'R(u_k - ur_k)  +  (x_T - xr_T)'Qf(x_T - xr_T)          (no 1/2)
 *     c_x = (Q+Q')(x_k - xr_k)   c_u = (R+R')(u_k - ur_k)   v_x = (Qf+Qf')(x_T - xr_T);   c_xx, c_ux, c_uu, v_xx as zm_quadcost_t's
 * The reference's drivers take cost callables (zopt/ilqrUtils.py:260-269); the fused drivers took zm_quadcost_t only, i.e. the
 * demo's cost about the origin (demos/iterativeLqr.py:12-13,37).  Q, R, Qf, diagonal: as zm_quadcost_t.
 * xRef, uRef: device pointers, NULL = zeros.  Row k of trajectory t (k = 0..T for xRef, 0..T-1 for uRef) starts at
 *     xRef + t * xref_traj_stride + k * xref_step_stride          (strides in doubles; the n resp. m entries of a row are contiguous)
 * and a stride may be 0: (0, 0) is one goal for every step and trajectory, (n, 0) a goal per trajectory, ((T+1) n, n) a full
 * reference per trajectory, (0, n) one reference shared by the batch.  Every kernel forms the difference first and then applies
 * the operations of its zm_quadcost_t sibling to it: a zero (or NULL) reference gives that sibling's results bit for bit.
 * Shapes: n <= 12, m <= 4 (the fused drivers' shapes; the wide rollouts take no tracking cost). */
typedef struct zm_trackcost_t {
    const double* Q;        /* (n,n) */
    const double* R;        /* (m,m) */
    const double* Qf;       /* (n,n) */
    int32_t diagonal;       /* as zm_quadcost_t.diagonal */
    int32_t reserved;
    const double* xRef;     /* NULL: zeros */
    const double* uRef;     /* NULL: zeros */
    int64_t xref_traj_stride, xref_step_stride;
    int64_t uref_traj_stride, uref_step_stride;
} zm_trackcost_t;

/* zm_rollout_linesearch_f64 / zm_rollout_linesearch_list_f64 (zopt/ilqrUtils.py:33-66, :116-150; CostFunction.__call__,
 * pytrees.py:49-52) with the tracking cost.  `cost` is required.  References are read by (trajectory id, step), also through a list. */
int zm_rollout_linesearch_tracking_f64(const zm_model_t* model, const zm_trackcost_t* cost, const double* x0, const double* l,
                                       const double* L, const double* xPrev, const double* uPrev, const double* alphas,
                                       int n_alpha, const int32_t* active, double* xTraj, double* uTraj, double* J,
                                       int32_t* alpha_idx, int64_t batch, int T, void* stream);
int zm_rollout_linesearch_tracking_list_f64(const zm_model_t* model, const zm_trackcost_t* cost, const double* x0, const double* l,
                                            const double* L, const double* xPrev, const double* uPrev, const double* alphas,
                                            int n_alpha, const int32_t* list, int64_t count, const int32_t* active, double* xTraj,
                                            double* uTraj, double* J, int32_t* alpha_idx, int64_t batch, int T, void* stream);
/* zm_quadratize_cost_f64 / zm_quadratize_cost_list_f64 (zopt/pytrees.py:100-115, :72-81) with the tracking cost: c, c_x, c_u about
 * (xr_k, ur_k), v, v_x about xr_T; the Hessians do not depend on the reference. */
int zm_quadratize_cost_tracking_f64(const zm_trackcost_t* cost, int n, int m, const double* xTraj, const double* uTraj,
                                    const int32_t* active, double* c, double* c_x, double* c_u, double* v, double* v_x,
                                    double* c_xx, double* c_ux, double* c_uu, double* v_xx, int64_t batch, int T, void* stream);
int zm_quadratize_cost_tracking_list_f64(const zm_trackcost_t* cost, int n, int m, const double* xTraj, const double* uTraj,
                                         const int32_t* list, int64_t count, const int32_t* active, double* c, double* c_x,
                                         double* c_u, double* v, double* v_x, double* c_xx, double* c_ux, double* c_uu,
                                         double* v_xx, int64_t batch, int T, void* stream);
/* zm_ilqr_solve_f64 / zm_ilqr_solve_trace_f64 (zopt/ilqrUtils.py:290-327, :360-397) with the tracking cost: the same loop and the
 * same launches; workspace and iwork as there (zm_ilqr_solve_workspace_f64). */
int zm_ilqr_solve_tracking_f64(const zm_model_t* model, const zm_trackcost_t* cost, const double* x0, const double* uGuess, int ddp,
                               int max_iter, double tol, int sync_every, double* workspace, int64_t workspace_doubles,
                               int32_t* iwork, double* xTraj, double* uTraj, double* L, double* J, int32_t* converged,
                               int32_t* iterations, int64_t batch, int T, void* stream);
int zm_ilqr_solve_tracking_trace_f64(const zm_model_t* model, const zm_trackcost_t* cost, const double* x0, const double* uGuess,
                                     int ddp, int max_iter, double tol, int sync_every, double* workspace,
                                     int64_t workspace_doubles, int32_t* iwork, double* xTraj, double* uTraj, double* L, double* J,
                                     int32_t* converged, int32_t* iterations, int64_t batch, int T, void* stream, double* J_trace,
                                     int32_t* alpha_trace);

/* ---- input box: iLQR and DDP with bounds u_lb <= u <= u_ub on the inputs (control-limited DDP: Tassa, Mansard, Todorov 2014) -------------
 * Every entry of this section is an extension; the reference has no counterpart (its iLQR is unconstrained, ilqrUtils.py:260-327).
 *   rollout / line search:  u_k = clip(alpha l_k + L_k (x_k - xPrev_k) + uPrev_k, lb, ub); the clip lets a NaN through.  With
 *                           infinite bounds the results are those of the unconstrained entries bit for bit.
 *   backward step:          l_k = argmin_d 1/2 d' sym(Q_uu) d + Q_u' d  over  lb - u_k <= d <= ub - u_k  (u_k: the current trajectory's
 *                           input); C = the components at a bound with a multiplier of the right sign (lb == ub: always), F the rest;
 *                           L_k[C,:] = 0, L_k[F,:] = -Q_uu[F,F]^-1 Q_ux[F,:];  v_x' = Q_x + Q_ux' l_k,  v_xx' = Q_xx - L_k' Q_uu L_k.
 *   DDP backward step:      the same step after Q_xx, Q_ux, Q_uu have received the blocks of the PD-projected (1e-3)
 *                           vf_zz = sum_i v_x[i] d2f_i/dz2, as in zm_ddp_backward_f64.
 * lb, ub: device pointers to m doubles per row, row t * stride belongs to trajectory t: stride 0 = one box for every trajectory,
 * stride m = a box per trajectory.  An entry may be -inf / +inf; lb <= ub is the caller's to ensure.  Shapes: n <= 12, m <= 4.
 * Stage-varying bounds (step_stride): the bounds of trajectory t at step k (the box of u_k, k = 0..T-1) are the m doubles at
 *     lb + t * stride + k * step_stride,   ub + t * stride + k * step_stride.
 *   step_stride == 0: one box for the whole horizon (the layout above; a struct built from three fields leaves it zero),
 *                     stride is 0 or m;
 *   step_stride == m: a row per step, (T, m) per trajectory; stride is 0 (one schedule for every trajectory) or T * m (a schedule
 *                     per trajectory), T the horizon of the call.
 * Every other (stride, step_stride) pair is ZM_EINVAL, from host code before anything is launched.  Every *_box_* entry takes both
 * forms; the *_state_* entries (state box around an input box) take step_stride == 0 only (ZM_EUNSUPPORTED otherwise).  With the same
 * row repeated over the steps the stage form gives the results of the constant form bit for bit. */
typedef struct zm_inputbox_t {
    const double* lb;
    const double* ub;
    int64_t stride;
    int64_t step_stride;
} zm_inputbox_t;

/* The box-QP of the backward step, batched, one problem per lane (test entry of the device routine the sweep runs wave-uniform):
 * d = argmin 1/2 d' sym(H) d + g' d over lo <= d <= hi.  H (batch, m, m), g, lo, hi, d_out (batch, m); m <= 4.  clamped_out
 * (optional): bit i set where component i is clamped; iters_out (optional): passes of the active-set iteration (24 = its cap). */
int zm_boxqp_f64(const double* H, const double* g, const double* lo, const double* hi, double* d_out, int32_t* clamped_out,
                 int32_t* iters_out, int64_t batch, int m, void* stream);
/* zm_ilqr_backward_list_f64 with the box: uTraj (batch, T, m) is the trajectory the expansions were taken along.  qp_capped
 * (optional, int32 per trajectory): += the steps whose QP ended at its pass cap (the last feasible iterate is used there).
 * list / active: as zm_ilqr_backward_list_f64 (list may be NULL). */
int zm_ilqr_backward_box_list_f64(const double* f_x, const double* f_u, const double* c_x, const double* c_u, const double* c_xx,
                                  const double* c_ux, const double* c_uu, const double* vf_x, const double* vf_xx, const double* uTraj,
                                  const zm_inputbox_t* box, const int32_t* list, int64_t count, const int32_t* active,
                                  int shared_hessian, double* l, double* L, int32_t* qp_capped, int64_t batch, int T, int n, int m,
                                  void* stream);
int zm_ilqr_backward_box_f64(const double* f_x, const double* f_u, const double* c_x, const double* c_u, const double* c_xx,
                             const double* c_ux, const double* c_uu, const double* vf_x, const double* vf_xx, const double* uTraj,
                             const zm_inputbox_t* box, int shared_hessian, double* l, double* L, int32_t* qp_capped, int64_t batch, int T,
                             int n, int m, void* stream);
/* zm_ddp_backward_list_f64 / zm_ddp_backward_f64 / zm_ddp_backward_pairs_list_f64 with the box: their arguments and rules (f_ux and
 * f_uu may be NULL together; the pairs form needs a model that declares Hessian pairs) plus uTraj, box and qp_capped as above.  The
 * three forms of second derivatives are contracted in the same summation order: equal operands give bitwise equal l, L.  Every
 * argument is checked before anything is launched. */
int zm_ddp_backward_box_list_f64(const double* f_x, const double* f_u, const double* f_xx, const double* f_ux, const double* f_uu,
                                 const double* c_x, const double* c_u, const double* c_xx, const double* c_ux, const double* c_uu,
                                 const double* vf_x, const double* vf_xx, const double* uTraj, const zm_inputbox_t* box,
                                 const int32_t* list, int64_t count, const int32_t* active, int shared_hessian, double* l, double* L,
                                 int32_t* qp_capped, int64_t batch, int T, int n, int m, void* stream);
int zm_ddp_backward_box_f64(const double* f_x, const double* f_u, const double* f_xx, const double* f_ux, const double* f_uu,
                            const double* c_x, const double* c_u, const double* c_xx, const double* c_ux, const double* c_uu,
                            const double* vf_x, const double* vf_xx, const double* uTraj, const zm_inputbox_t* box, int shared_hessian,
                            double* l, double* L, int32_t* qp_capped, int64_t batch, int T, int n, int m, void* stream);
int zm_ddp_backward_pairs_box_list_f64(const zm_model_t* model, const double* f_x, const double* f_u, const double* H, const double* c_x,
                                       const double* c_u, const double* c_xx, const double* c_ux, const double* c_uu, const double* vf_x,
                                       const double* vf_xx, const double* uTraj, const zm_inputbox_t* box, const int32_t* list,
                                       int64_t count, const int32_t* active, int shared_hessian, double* l, double* L,
                                       int32_t* qp_capped, int64_t batch, int T, void* stream);
/* zm_rollout_linesearch_f64 / _list_f64 with the box.  The cost is `cost` or `track` (exactly one; both NULL only for a plain
 * rollout, n_alpha == 1).  One lane per rollout, two passes. */
int zm_rollout_linesearch_box_f64(const zm_model_t* model, const zm_quadcost_t* cost, const zm_trackcost_t* track,
                                  const zm_inputbox_t* box, const double* x0, const double* l, const double* L, const double* xPrev,
                                  const double* uPrev, const double* alphas, int n_alpha, const int32_t* active, double* xTraj,
                                  double* uTraj, double* J, int32_t* alpha_idx, int64_t batch, int T, void* stream);
int zm_rollout_linesearch_box_list_f64(const zm_model_t* model, const zm_quadcost_t* cost, const zm_trackcost_t* track,
                                       const zm_inputbox_t* box, const double* x0, const double* l, const double* L,
                                       const double* xPrev, const double* uPrev, const double* alphas, int n_alpha, const int32_t* list,
                                       int64_t count, const int32_t* active, double* xTraj, double* uTraj, double* J, int32_t* alpha_idx,
                                       int64_t batch, int T, void* stream);
/* zm_ilqr_solve_f64 / zm_ilqr_solve_trace_f64 with the box: the same loop on the box sweep and the box line search (full Jacobians,
 * alternating buffers; uGuess is clipped into the box by the initial rollout, every stored uTraj is feasible).  The cost is `cost`
 * or `track` (exactly one).  ddp = 1: the DDP loop on the box DDP sweep (second derivatives as pairs where the model declares them,
 * the full tensors otherwise).  qp_capped (optional): int32 per trajectory, set to the number of capped QPs over the whole solve.
 * Workspace: zm_ilqr_solve_workspace_f64(model, batch, T, ddp). */
int zm_ilqr_solve_box_f64(const zm_model_t* model, const zm_quadcost_t* cost, const zm_trackcost_t* track, const zm_inputbox_t* box,
                          const double* x0, const double* uGuess, int ddp, int max_iter, double tol, int sync_every, double* workspace,
                          int64_t workspace_doubles, int32_t* iwork, double* xTraj, double* uTraj, double* L, double* J,
                          int32_t* converged, int32_t* iterations, int32_t* qp_capped, int64_t batch, int T, void* stream);
int zm_ilqr_solve_box_trace_f64(const zm_model_t* model, const zm_quadcost_t* cost, const zm_trackcost_t* track,
                                const zm_inputbox_t* box, const double* x0, const double* uGuess, int ddp, int max_iter, double tol,
                                int sync_every, double* workspace, int64_t workspace_doubles, int32_t* iwork, double* xTraj,
                                double* uTraj, double* L, double* J, int32_t* converged, int32_t* iterations, int32_t* qp_capped,
                                int64_t batch, int T, void* stream, double* J_trace, int32_t* alpha_trace);

/* ---- state box: iLQR with bounds x_lb <= x_k <= x_ub on the states, k = 1..T, by an augmented-Lagrangian (AL) outer loop around the
 * fused iLQR (AL-iLQR: Howell, Jackson, Manchester 2019) --------------------------------------------------------------------------------
 * Every entry of this section is an extension; the reference has no counterpart (its iLQR is unconstrained, ilqrUtils.py:260-327).
 * Per trajectory t a penalty mu_t > 0 and multipliers lam_ub[k][i] >= 0, lam_lb[k][i] >= 0; row k = 0 is never constrained (x_0 is
 * given).  For k = 1..T, i < n, with pos(s) = s > 0 ? s : 0 (a NaN gives 0):
 *     s_ub = lam_ub + mu (x_i - ub_i),   s_lb = lam_lb + mu (lb_i - x_i)
 *     psi  = (pos(s_ub)^2 - lam_ub^2 + pos(s_lb)^2 - lam_lb^2) / (2 mu),   g_i = pos(s_ub) - pos(s_lb),   h_i = mu ((s_ub > 0) + (s_lb > 0))
 *   cost:        J_AL = J_cost + P, P = sum_{k=1..T} sum_i psi in an accumulator of its own (k, i ascending), added once at the end.
 *                With infinite bounds and zero multipliers P is exactly 0.0.
 *   expansion:   c_x[k] += g_k (1 <= k < T), v_x += g_T; the cost Hessian of step k is c_xx + diag h_k, the terminal one v_xx + diag h_T.
 *   outer loop:  lam = 0, mu = mu0; per outer iteration an inner iLQR solve on J_AL over the trajectories that are not done (from the
 *                stored inputs, policy (u, L = 0)), then viol_t = max(0, max(x - ub), max(lb - x)) over k >= 1 (NaN if a state is);
 *                done = the inner solve converged and viol_t <= ctol -- nothing of a done trajectory is touched again; otherwise, if
 *                another outer iteration follows, lam <- pos(s) and mu_t <- min(mu_t growth, mu_max).
 * lb, ub: device pointers to n doubles per row, row t * stride belongs to trajectory t (stride 0: shared, n: per trajectory); an entry
 * may be -inf / +inf, lb == ub is allowed.  lam_lb, lam_ub: (batch, T+1, n); mu: (batch).  Shapes: n <= 12, m <= 4. */
typedef struct zm_statebox_t {
    const double* lb;
    const double* ub;
    int64_t stride;
    double* lam_lb;
    double* lam_ub;
    double* mu;
} zm_statebox_t;

/* zm_rollout_linesearch_box_f64 / _list_f64 on J_AL: `box` may be NULL (no input bounds); the cost is `cost` or `track` (exactly one).
 * J <- J_AL, J_cost (optional) <- the cost without the penalty, both of the winner.  One lane per rollout, two passes. */
int zm_rollout_linesearch_state_f64(const zm_model_t* model, const zm_quadcost_t* cost, const zm_trackcost_t* track,
                                    const zm_inputbox_t* box, const zm_statebox_t* sbox, const double* x0, const double* l, const double* L,
                                    const double* xPrev, const double* uPrev, const double* alphas, int n_alpha, const int32_t* active,
                                    double* xTraj, double* uTraj, double* J, double* J_cost, int32_t* alpha_idx, int64_t batch, int T,
                                    void* stream);
int zm_rollout_linesearch_state_list_f64(const zm_model_t* model, const zm_quadcost_t* cost, const zm_trackcost_t* track,
                                         const zm_inputbox_t* box, const zm_statebox_t* sbox, const double* x0, const double* l,
                                         const double* L, const double* xPrev, const double* uPrev, const double* alphas, int n_alpha,
                                         const int32_t* list, int64_t count, const int32_t* active, double* xTraj, double* uTraj,
                                         double* J, double* J_cost, int32_t* alpha_idx, int64_t batch, int T, void* stream);
/* The penalty's part of the expansion along xTraj (batch, T+1, n), after the cost's: c_x (batch, T, n) rows 1..T-1 += g_k,
 * v_x (batch, n) += g_T, h (batch, T+1, n) <- the diagonal addend (row 0 zero).  list (may be NULL) / active: as elsewhere; the rows
 * of other trajectories are not touched. */
int zm_state_penalty_expand_list_f64(const zm_statebox_t* sbox, const double* xTraj, const int32_t* list, int64_t count,
                                     const int32_t* active, double* c_x, double* v_x, double* h, int64_t batch, int T, int n,
                                     void* stream);
/* zm_ilqr_backward_list_f64 / _box_list_f64 on the cost Hessians c_xx + diag h_k (k = 0..T-1) and v_xx + diag h_T, h (batch, T+1, n):
 * every row is read, row 0 included (zm_state_penalty_expand_list_f64 writes zeros there; a caller's own h must do the same if step 0
 * is to keep its Hessian).  box and uTraj may be NULL together (no input bounds).  The register-prefetch sweep only (n <= 12, m <= 4). */
int zm_ilqr_backward_state_f64(const double* f_x, const double* f_u, const double* c_x, const double* c_u, const double* c_xx,
                               const double* c_ux, const double* c_uu, const double* vf_x, const double* vf_xx, const double* h,
                               const double* uTraj, const zm_inputbox_t* box, int shared_hessian, double* l, double* L,
                               int32_t* qp_capped, int64_t batch, int T, int n, int m, void* stream);
int zm_ilqr_backward_state_list_f64(const double* f_x, const double* f_u, const double* c_x, const double* c_u, const double* c_xx,
                                    const double* c_ux, const double* c_uu, const double* vf_x, const double* vf_xx, const double* h,
                                    const double* uTraj, const zm_inputbox_t* box, const int32_t* list, int64_t count,
                                    const int32_t* active, int shared_hessian, double* l, double* L, int32_t* qp_capped, int64_t batch,
                                    int T, int n, int m, void* stream);
/* Between two inner solves, for every trajectory with active[t] != 0 (the others are not touched): violation[t] <- viol_t;
 * done = converged[t] && viol_t <= ctol; converged[t] <- done, active[t] <- !done; where not done and `update` != 0: lam <- pos(s),
 * mu_t <- min(mu_t growth, mu_max).  outer_count (optional, int32 per trajectory) += 1; remaining (optional, one int32) += the number
 * of trajectories that are not done. */
int zm_state_multiplier_update_f64(const zm_statebox_t* sbox, const double* xTraj, int32_t* active, int32_t* converged,
                                   double* violation, int32_t* outer_count, int32_t* remaining, double ctol, double growth,
                                   double mu_max, int update, int64_t batch, int T, int n, void* stream);
/* Doubles of workspace zm_ilqr_solve_state_f64 needs (-1: cannot be sized); iwork as zm_ilqr_solve_f64 (2 batch + 2 int32). */
int64_t zm_ilqr_solve_state_workspace_f64(const zm_model_t* model, int64_t batch, int T);
/* The AL loop as one call (host code around the loop of zm_ilqr_solve_f64, nothing in between but launches).  The cost is `cost` or
 * `track` (exactly one); `box` (optional) adds input bounds: rollouts clip, the backward step is the box-QP step.  ddp must be 0
 * (ZM_EUNSUPPORTED otherwise).  sbox: the caller's bounds and its arrays for the multipliers and mu (outputs: started at 0 / mu0).
 * Outputs per trajectory: J <- the cost WITHOUT the penalty of the returned trajectory, converged <- done, violation,
 * outer_iterations (optional) <- the outer iterations it took part in, inner_iterations (optional, (outer, batch)) <- its iLQR
 * iterations in each of them; iterations (host, optional) <- outer iterations run.  Every argument is checked before any launch.
 * The trace form adds J_trace / alpha_trace ((outer * max_iter, batch): row j * max_iter + it <- J_AL after the acceptance step and
 * the winning step index) and violation_trace / mu_trace ((outer, batch): after / during outer iteration j); each may be NULL. */
int zm_ilqr_solve_state_f64(const zm_model_t* model, const zm_quadcost_t* cost, const zm_trackcost_t* track, const zm_inputbox_t* box,
                            const zm_statebox_t* sbox, double mu0, double growth, double mu_max, int outer, double ctol, const double* x0,
                            const double* uGuess, int ddp, int max_iter, double tol, int sync_every, double* workspace,
                            int64_t workspace_doubles, int32_t* iwork, double* xTraj, double* uTraj, double* L, double* J,
                            int32_t* converged, double* violation, int32_t* outer_iterations, int32_t* inner_iterations,
                            int32_t* iterations, int32_t* qp_capped, int64_t batch, int T, void* stream);
int zm_ilqr_solve_state_trace_f64(const zm_model_t* model, const zm_quadcost_t* cost, const zm_trackcost_t* track,
                                  const zm_inputbox_t* box, const zm_statebox_t* sbox, double mu0, double growth, double mu_max, int outer,
                                  double ctol, const double* x0, const double* uGuess, int ddp, int max_iter, double tol, int sync_every,
                                  double* workspace, int64_t workspace_doubles, int32_t* iwork, double* xTraj, double* uTraj, double* L,
                                  double* J, int32_t* converged, double* violation, int32_t* outer_iterations,
                                  int32_t* inner_iterations, int32_t* iterations, int32_t* qp_capped, int64_t batch, int T, void* stream,
                                  double* J_trace, int32_t* alpha_trace, double* violation_trace, double* mu_trace);

/* Same, with OSQP's over-relaxation `alpha` in (0, 2) (OSQP / cvxpy default 1.6, which is what the reference's
 * `prob.solve(**kwargs)` runs with, mpcUtils.py:77): the relaxed iterate alpha w + (1 - alpha) y_prev enters the projection and
 * the dual update; residuals are those of the unrelaxed iterate.  alpha = 1 is zm_mpc_solve_adaptive_f64. */
int zm_mpc_solve_relaxed_f64(const double* A, const double* B, const double* K, const double* Minv, int n_levels, int level0,
                             double rho_step, double alpha, const double* x_lb, const double* x_ub, const double* u_lb,
                             const double* u_ub, const double* x0, double rho, double eps_abs, double eps_rel, double eps_prim_inf,
                             int max_iter, int warm_start, double* workspace, double* xTraj, double* uTraj, int32_t* status,
                             int32_t* iters, double* resid, int64_t batch, int N, int n, int m, void* stream);

/* Per-problem data (reference: zopt/mpcUtils.py:14-81, class lqrMpc, one problem per object there): P problems of the same
 * (N, n, m), each with its own A, B, Q, R, Qf, bounds and penalty, set up and solved in one launch each.
 * zm_mpc_setup_batched_f64: the tables of zm_mpc_setup_f64 for every problem p and level l, bit for bit those of P * L calls of it
 *     (one workgroup per (p, l), the same arithmetic).  Symmetric weights, as there.
 *     in : A (P,n,n) B (P,n,m) Q (P,n,n) R (P,m,m) Qf (P,n,n) rho (P,L) -- the penalty of each (problem, level)   [device]
 *     out: K (P,L,N,m,n)  Minv (P,L,N,m,m), problem-major (one problem's levels are contiguous)                    [device] */
int zm_mpc_setup_batched_f64(const double* A, const double* B, const double* Q, const double* R, const double* Qf,
                             const double* rho, int64_t P, int L, int N, int n, int m, double* K, double* Minv, void* stream);
/* zm_mpc_solve_batched_f64: zm_mpc_solve_relaxed_f64 with per-problem data.  Instance i solves problem problem[i] in [0, P): A (P,n,n),
 * B (P,n,m), K / Minv (P,n_levels,N,...) from zm_mpc_setup_batched_f64, bounds (P,n) / (P,m), rho (P) -- the penalty of level0 of
 * each problem (the levels are rho[p] * rho_step^(l - level0)); x0, workspace and outputs as in zm_mpc_solve_relaxed_f64.  Same
 * dispatch (16 lanes per instance where the shape and horizon fit it and ZOPT_AMD_MPC_PATH is not `lane`, else one lane per instance at
 * the fixed penalty of level0), same bits per instance as a zm_mpc_solve_relaxed_f64 call on its problem alone.  Reads the index map
 * back to the host to check it (ZM_EINVAL for an index outside [0, P)), so the call waits for the work queued on `stream` before it. */
int zm_mpc_solve_batched_f64(const double* A, const double* B, const double* K, const double* Minv, int n_levels, int level0,
                             double rho_step, double alpha, const double* x_lb, const double* x_ub, const double* u_lb,
                             const double* u_ub, const double* x0, const double* rho, const int32_t* problem, int64_t P,
                             double eps_abs, double eps_rel, double eps_prim_inf, int max_iter, int warm_start, double* workspace,
                             double* xTraj, double* uTraj, int32_t* status, int32_t* iters, double* resid, int64_t batch, int N,
                             int n, int m, void* stream);

/* Reference tracking: the cost of zopt/mpcUtils.py:52-54 about a reference,
 *     sum_{k<N} (x_k - xr_k)'Q(x_k - xr_k) + (u_k - ur_k)'R(u_k - ur_k)  +  (x_N - xr_N)'Qf(x_N - xr_N),
 * under the unchanged constraints of :55-58 (the reference regulates to the origin: xr = 0, ur = 0).  A reference only adds a linear
 * term to the w-update's LQ problem, g_x,k = -(W + W') xr_{k+1} (W = Q, Qf at the last stage), g_u,k = -(R + R') ur_k, constant over
 * the ADMM iterations: the tables K, Minv of zm_mpc_setup_f64 / zm_mpc_setup_batched_f64, the projection and the infeasibility
 * certificate are those of zm_mpc_solve_relaxed_f64; the backward stage uses -rho (y - lam) + g_k and the dual tolerance scales with
 * max(rho |lam|_inf, |g|_inf) (OSQP's ||q|| term).  With xr = 0 and ur = 0 the iterates are those of zm_mpc_solve_relaxed_f64 /
 * zm_mpc_solve_batched_f64, move for move.  With a non-zero reference the 16-lanes-per-instance kernels also guard the adaptive penalty
 * against a limit cycle: the third level move in a row that undoes the one before is refused and the penalty then stays fixed.
 * Affine dynamics offsets x+ = A x + B u + c are NOT covered (they need their own setup tables).
 *     in : everything zm_mpc_solve_batched_f64 takes, and the weights Q, R, Qf the tables were set up with   [device]
 *          xRef (batch,N+1,n)  uRef (batch,N,m): the references; either may be NULL (zero).  Row 0 of xRef is not read.   [device]
 *          shared problem: problem = NULL, rho_p = NULL, the penalty in `rho`, every array without the P axis (P is ignored);
 *          per-problem data: problem (batch) int32 and rho_p (P) as in zm_mpc_solve_batched_f64 (`rho` is ignored), Q, R, Qf (P,...)
 *          workspace: 5 * batch * N * (n + m) doubles -- the four blocks of zm_mpc_solve_f64 (the warm start lives there) and
 *                     g (batch,N,n+m), which the call forms from the references before it launches the solve
 *     out: as zm_mpc_solve_relaxed_f64.  Same dispatch, ZOPT_AMD_MPC_PATH=lane included. */
int zm_mpc_solve_tracking_f64(const double* A, const double* B, const double* Q, const double* R, const double* Qf, const double* K,
                              const double* Minv, int n_levels, int level0, double rho_step, double alpha, const double* x_lb,
                              const double* x_ub, const double* u_lb, const double* u_ub, const double* x0, const double* xRef,
                              const double* uRef, double rho, const double* rho_p, const int32_t* problem, int64_t P, double eps_abs,
                              double eps_rel, double eps_prim_inf, int max_iter, int warm_start, double* workspace, double* xTraj,
                              double* uTraj, int32_t* status, int32_t* iters, double* resid, int64_t batch, int N, int n, int m,
                              void* stream);

/* The receding-horizon loop of the reference's demo (demos/lqrMpc.py:40-47) as ONE call: `steps` solves of every instance in a row, each
 * from the state the previous one led to,
 *     x <- clip(x, x_lb + clip_tol, x_ub - clip_tol);  states[s] = x;  solve from x (step 0 cold, later steps with `warm_start`);
 *     inputs[s] = uTraj_s[0];  x <- xTraj_s[1] + disturbance[s];                        states[steps] = clip(x, ...)
 * -- exactly what a loop of zm_mpc_solve_relaxed_f64 / zm_mpc_solve_batched_f64 / zm_mpc_solve_tracking_f64 calls computes (one entry
 * point for the three forms: problem, rho_p, Q, R, Qf, xRef, uRef, disturbance may be NULL with the meanings they have there), whatever
 * the status of a step: a step that does not end "optimal" still leaves a rollout, and the step after it starts cold.
 * Regulator runs (xRef = uRef = NULL) at the shapes and horizons of the 16-lanes-per-instance kernels are ONE launch: the step loop runs
 * inside the kernel, and a wave goes on to its next step as soon as its own four instances are through (the gain over a launch per step
 * is per wave, not per instance).  Tracking runs, (n, m) = (24, 8), horizons beyond LDS and ZOPT_AMD_MPC_PATH=lane take a host loop that
 * enqueues the launches of a single solve and a small advance kernel per step.  Neither synchronises or copies anything to the host,
 * apart from the one check of the problem map that zm_mpc_solve_batched_f64 documents.
 *     in : the arguments of zm_mpc_solve_tracking_f64 with the same meanings; x0 (batch,n)   [device]
 *          xRef (batch,xref_rows,n) with xref_rows = steps + N, uRef (batch,uref_rows,m) with uref_rows = steps + N - 1: step s tracks
 *          rows s .. s + N of xRef and s .. s + N - 1 of uRef; either may be NULL (its row count is then ignored)   [device]
 *          warm_start: 0 / 1 / 2 (shifted) for the steps after the first;  clip_tol >= 0, or negative for no clip
 *          disturbance (steps,batch,n) or NULL   [device]
 *          workspace: (tracking ? 5 : 4) * batch * N * (n + m) doubles, plus batch * ((N + 1) * n + N * m) doubles when xPred is NULL
 *                     (the rollout every step overwrites)   [device]
 *     out: STEP-MAJOR.  states (steps+1,batch,n)  inputs (steps,batch,m)  status, iters (steps,batch) int32   [device]
 *          xPred (steps,batch,N+1,n)  uPred (steps,batch,N,m): the rollout of every step; both NULL to skip   [device] */
int zm_mpc_closed_loop_f64(const double* A, const double* B, const double* Q, const double* R, const double* Qf, const double* K,
                           const double* Minv, int n_levels, int level0, double rho_step, double alpha, const double* x_lb,
                           const double* x_ub, const double* u_lb, const double* u_ub, const double* x0, const double* xRef,
                           const double* uRef, int xref_rows, int uref_rows, double rho, const double* rho_p, const int32_t* problem,
                           int64_t P, double eps_abs, double eps_rel, double eps_prim_inf, int max_iter, int warm_start, int steps,
                           double clip_tol, const double* disturbance, double* workspace, double* states, double* inputs,
                           int32_t* status, int32_t* iters, double* xPred, double* uPred, int64_t batch, int N, int n, int m,
                           void* stream);

/* Soft box constraints on lqrMpc's problem (extension): the QP of zopt/mpcUtils.py:48-59 (about a reference or not) in which a component
 * i of the stacked [x ; u] with a finite l1_i >= 0 is not held inside its box (:55-58) but pays
 *     l1_i d + l2_i d^2,   d = max(0, v - ub_i, lb_i - v),   for every x_k,i (k >= 1) / u_k,i,
 * so a start, or a state a disturbance has led to, outside the box in such a component is solved from and flown back, where the hard
 * problem is "infeasible" (Replaces: nothing in the reference, whose bounds are all hard; with every l1 = +inf these entries compute what
 * zm_mpc_solve_relaxed_f64 / _batched_f64 / _tracking_f64 and zm_mpc_closed_loop_f64 compute, bit for bit).  l1_i = +inf is a hard
 * component (l2_i must be 0 there).  soft_l1, soft_l2 (P,n+m), the stacked layout [x ; u], one row for the shared problem  [device];
 * soft_l2 may be NULL (zeros).  The tables do not depend on the weights: zm_mpc_setup_f64 / zm_mpc_setup_batched_f64 set up.
 * The ADMM differs from zm_mpc_solve_tracking_f64's where zm_mpc_solve_ltv_soft_f64 (below) differs from its hard form, and nowhere else:
 * a soft component of x0 is not tested against the box; the y-update is the proximal map of the penalty, t = l1 / rho and
 * a = rho / (rho + 2 l2) following the adaptive penalty; a soft component has the bounds -inf / +inf in the certificate's support term;
 * the cycle guard is on when the reference term is nonzero or the instance's problem has a soft component.
 * zm_mpc_solve_soft_f64: the arguments of zm_mpc_solve_tracking_f64 with soft_l1, soft_l2 after u_ub.  Q, R, Qf are read, and the
 *     workspace has its fifth block, only when xRef or uRef is given (4 * batch * N * (n + m) doubles without a reference).
 * zm_mpc_closed_loop_soft_f64: the arguments of zm_mpc_closed_loop_f64 with soft_l1, soft_l2 after u_ub.  The clip between the steps
 *     applies to the HARD state components only: a soft component of states[s + 1] is xTraj_s[1] + disturbance[s], the plant's state.
 *     A regulator run is one launch with the step loop inside, a tracking run the queue of launches, as there.
 * 16 lanes per instance only: ZM_EUNSUPPORTED for (n, m) outside the compiled shapes with n + m <= 16 and for N > 75;
 * ZOPT_AMD_MPC_PATH does not apply.  ZM_EINVAL for a NULL soft_l1 and for whatever the hard entries refuse; all but the map check before
 * any launch. */
int zm_mpc_solve_soft_f64(const double* A, const double* B, const double* Q, const double* R, const double* Qf, const double* K,
                          const double* Minv, int n_levels, int level0, double rho_step, double alpha, const double* x_lb,
                          const double* x_ub, const double* u_lb, const double* u_ub, const double* soft_l1, const double* soft_l2,
                          const double* x0, const double* xRef, const double* uRef, double rho, const double* rho_p,
                          const int32_t* problem, int64_t P, double eps_abs, double eps_rel, double eps_prim_inf, int max_iter,
                          int warm_start, double* workspace, double* xTraj, double* uTraj, int32_t* status, int32_t* iters, double* resid,
                          int64_t batch, int N, int n, int m, void* stream);
int zm_mpc_closed_loop_soft_f64(const double* A, const double* B, const double* Q, const double* R, const double* Qf, const double* K,
                                const double* Minv, int n_levels, int level0, double rho_step, double alpha, const double* x_lb,
                                const double* x_ub, const double* u_lb, const double* u_ub, const double* soft_l1, const double* soft_l2,
                                const double* x0, const double* xRef, const double* uRef, int xref_rows, int uref_rows, double rho,
                                const double* rho_p, const int32_t* problem, int64_t P, double eps_abs, double eps_rel,
                                double eps_prim_inf, int max_iter, int warm_start, int steps, double clip_tol, const double* disturbance,
                                double* workspace, double* states, double* inputs, int32_t* status, int32_t* iters, double* xPred,
                                double* uPred, int64_t batch, int N, int n, int m, void* stream);

/* Stage-varying dynamics (extension; what linearising a model about a TRAJECTORY gives): the QP of zopt/mpcUtils.py:48-59 with
 *     x_{k+1} = A_k x_k + B_k u_k + c_k,   k = 0 .. N-1,
 * per problem, under the cost, bounds, ADMM, termination and status codes of zm_mpc_solve_tracking_f64 in its per-problem form.
 * zm_mpc_setup_ltv_f64: the Riccati recursion of zm_mpc_setup_batched_f64 with the stage's own A_k, B_k (constant A_k, B_k give its
 *     tables bit for bit), one workgroup per (problem, level), one launch.  It also emits D_k = P_{k+1} c_k, the offset's share of the
 *     costate (P_{k+1}: the value matrix the recursion holds on entering stage k, P_N = 2 Qf + rho I), and ABt, the columns of
 *     [A_k | B_k] as contiguous rows, which the backward sweep of the solve reads per lane.  Symmetric weights, as zm_mpc_setup_f64.
 *     in : A (P,N,n,n)  B (P,N,n,m)  c (P,N,n) or NULL (zero)  Q (P,n,n)  R (P,m,m)  Qf (P,n,n)  rho (P,L)   [device]
 *     out: K (P,L,N,m,n)  Minv (P,L,N,m,m)  D (P,L,N,n)  ABt (P,N,n+m,n): row i < n is column i of A_k, row n + j column j of B_k [device]
 *     n <= 12 and m <= 4 (ZM_EUNSUPPORTED beyond: there is no lane-per-instance kernel for stage-varying dynamics).
 * zm_mpc_solve_ltv_f64: instance i solves problem problem[i] in [0, P).  The backward stage is p = p' + z_x + g_x + D_k,
 *     Qu = z_u + g_u + B_k' p, kf = Suu_k^-1 Qu, p' = A_k' p - K_k' Qu; the forward stage u = -K_k x - kf, x+ = A_k x + B_k u + c_k; the
 *     free response of the infeasibility certificate carries the offsets.  The dual tolerance scales with max(rho |lam|_inf, |g|_inf) (c
 *     sits in the constraints, not in the cost); the cycle guard of the adaptive penalty is on when g != 0 or the problem's c != 0.
 *     With constant A_k, B_k and c = 0 the iterates are those of zm_mpc_solve_tracking_f64 on the same data, move for move.
 *     in : the arguments of zm_mpc_solve_tracking_f64 in its per-problem form (rho_p and problem are required), with A, B per stage
 *          as above, and c (P,N,n) (a zero array where zm_mpc_setup_ltv_f64 was given NULL), D and ABt from that call   [device]
 *          xRef, uRef: either may be NULL (zero).  workspace: 5 * batch * N * (n + m) doubles, as zm_mpc_solve_tracking_f64.
 *     out: as zm_mpc_solve_tracking_f64.
 *     16 lanes per instance only: ZM_EUNSUPPORTED for (n, m) outside the compiled shapes with n + m <= 16 and for horizons whose
 *     iterates do not fit LDS (4 * N * 64 * 8 B > 150 KiB, i.e. N > 75); ZOPT_AMD_MPC_PATH does not apply.  Reads the index map back
 *     to the host to check it, like zm_mpc_solve_batched_f64. */
int zm_mpc_setup_ltv_f64(const double* A, const double* B, const double* c, const double* Q, const double* R, const double* Qf,
                         const double* rho, int64_t P, int L, int N, int n, int m, double* K, double* Minv, double* D, double* ABt,
                         void* stream);
int zm_mpc_solve_ltv_f64(const double* A, const double* B, const double* c, const double* ABt, const double* Q, const double* R,
                         const double* Qf, const double* K, const double* Minv, const double* D, int n_levels, int level0,
                         double rho_step, double alpha, const double* x_lb, const double* x_ub, const double* u_lb, const double* u_ub,
                         const double* x0, const double* xRef, const double* uRef, const double* rho_p, const int32_t* problem,
                         int64_t P, double eps_abs, double eps_rel, double eps_prim_inf, int max_iter, int warm_start, double* workspace,
                         double* xTraj, double* uTraj, int32_t* status, int32_t* iters, double* resid, int64_t batch, int N, int n, int m,
                         void* stream);

/* Stage-varying weights and bounds on top of the stage-varying dynamics (extension): the QP above with
 *     cost  sum_{k<N} (x_{k+1} - xr_{k+1})' Qs_k (x_{k+1} - xr_{k+1}) + (u_k - ur_k)' Rs_k (u_k - ur_k)   (Qs_{N-1}: the terminal weight)
 *     box   x_lb0 <= x_0 <= x_ub0,   lo_k <= [x_{k+1} ; u_k] <= hi_k,   k = 0 .. N-1    (+-inf allowed anywhere)
 * -- corridors and gates that move along the horizon, a terminal set tighter than the stage box, tube tightening, waypoint weights,
 * discounted costs.  ADMM, termination, certificate, status codes, workspace and outputs are zm_mpc_solve_ltv_f64's.
 * zm_mpc_setup_ltv_stage_f64 replaces zm_mpc_setup_ltv_f64:  P_N = 2 Qs_{N-1} + rho I, stage k uses Rs_k, the value update that leaves
 *     stage k >= 1 uses Qs_{k-1} (the one that leaves stage 0 is read by nothing).  The same products in the same order: with constant
 *     rows (Qs_k = Q for k < N-1, Qs_{N-1} = Qf, Rs_k = R) the tables are zm_mpc_setup_ltv_f64's bit for bit.  Every Qs_k, Rs_k symmetric.
 *     in : A (P,N,n,n)  B (P,N,n,m)  c (P,N,n) or NULL (zero)  Qs (P,N,n,n)  Rs (P,N,m,m)  rho (P,L)   [device]
 *     out: K (P,L,N,m,n)  Minv (P,L,N,m,m)  D (P,L,N,n)  ABt (P,N,n+m,n), as zm_mpc_setup_ltv_f64 writes them   [device]
 *     ZM_EINVAL for a null pointer or a bad size, ZM_EUNSUPPORTED beyond n <= 12, m <= 4; both before any launch.
 * zm_mpc_solve_ltv_stage_f64 replaces zm_mpc_solve_ltv_f64: its arguments with (Q, R, Qf) -> (Qs, Rs) -- read for the linear term of a
 *     reference only, g_x,k = -(Qs_k + Qs_k') xr_{k+1}, g_u,k = -(Rs_k + Rs_k') ur_k -- and (x_lb, x_ub, u_lb, u_ub) ->
 *     x_lb0, x_ub0 (P,n): the box of x_0, an x0 outside it is ZM_MPC_INFEASIBLE at once;
 *     lo, hi (P,N,n+m):  row k = [bound of x_{k+1} ; bound of u_k], the kernels' stacked stage layout.                [device]
 *     The stage's bounds are fetched with the stage's other data, three stages ahead; with constant rows the iterates are
 *     zm_mpc_solve_ltv_f64's bit for bit.  The same refusals: ZM_EINVAL for a null pointer, a bad size, bad penalty levels or a map
 *     entry outside [0, P); ZM_EUNSUPPORTED for (n, m) outside the compiled shapes with n + m <= 16 and for N > 75; all but the map
 *     check before any launch. */
int zm_mpc_setup_ltv_stage_f64(const double* A, const double* B, const double* c, const double* Qs, const double* Rs, const double* rho,
                               int64_t P, int L, int N, int n, int m, double* K, double* Minv, double* D, double* ABt, void* stream);
int zm_mpc_solve_ltv_stage_f64(const double* A, const double* B, const double* c, const double* ABt, const double* Qs, const double* Rs,
                               const double* K, const double* Minv, const double* D, int n_levels, int level0, double rho_step,
                               double alpha, const double* x_lb0, const double* x_ub0, const double* lo, const double* hi,
                               const double* x0, const double* xRef, const double* uRef, const double* rho_p, const int32_t* problem,
                               int64_t P, double eps_abs, double eps_rel, double eps_prim_inf, int max_iter, int warm_start,
                               double* workspace, double* xTraj, double* uTraj, int32_t* status, int32_t* iters, double* resid,
                               int64_t batch, int N, int n, int m, void* stream);

/* Soft box constraints on top of the stage form (extension): with d_i(v) = max(0, v - hi_k,i, lo_k,i - v) the QP of
 * zm_mpc_solve_ltv_stage_f64 gains
 *     + sum_{k<N} sum_i  l1_i d_i(w_k,i) + l2_i d_i(w_k,i)^2,     w_k = [x_{k+1} ; u_k],  i over the n + m stacked components
 * for every component i with a finite l1_i >= 0 (soft: its bounds no longer constrain w; l2_i >= 0 finite).  l1_i = +inf is a hard
 * component, exactly as in zm_mpc_solve_ltv_stage_f64 (l2_i must be 0 there).  The weights are per problem and per component, constant
 * over the stages: soft_l1, soft_l2 (P,n+m) in the stacked layout [x ; u]  [device]; soft_l2 may be NULL (zeros).  A violation is paid
 * for, not forbidden, so a soft problem always has a solution; with l1 above the hard problem's multipliers (an exact penalty) the hard
 * solution comes back whenever there is one.  The tables do not depend on the weights: zm_mpc_setup_ltv_stage_f64 sets up.
 * What changes in the ADMM of zm_mpc_solve_ltv_stage_f64, and nothing else does (residuals, tolerances, the level rule, the workspace
 * and the statuses are its own):
 *     x0:          a soft state component of x0 is not tested against x_lb0, x_ub0 (its violation is a constant of the problem); a hard
 *                  one is, as before.
 *     projection:  the y-update is the proximal map of the penalty.  With v = w_hat + lam, t = l1 / rho, a = rho / (rho + 2 l2):
 *                      v < lo:  e = a ((lo - v) - t);  y = e > 0 ? lo - e : lo
 *                      v > hi:  e = a ((v - hi) - t);  y = e > 0 ? hi + e : hi          else y = v
 *                  t and a follow rho whenever the adaptive penalty moves.  l1 = +inf gives y = the bound, bit for bit the clip.
 *     certificate: in the support term of the primal-infeasibility certificate a soft component has the bounds -inf / +inf (its y
 *                  ranges over the whole line), so no certificate can rest on it.
 *     cycle guard: on when g != 0, or the problem's c != 0, or the problem has a soft component.
 * With every l1 = +inf the solve is zm_mpc_solve_ltv_stage_f64's bit for bit.  The same refusals as zm_mpc_solve_ltv_stage_f64, and
 * ZM_EINVAL for a NULL soft_l1; all but the map check before any launch. */
int zm_mpc_solve_ltv_soft_f64(const double* A, const double* B, const double* c, const double* ABt, const double* Qs, const double* Rs,
                              const double* K, const double* Minv, const double* D, int n_levels, int level0, double rho_step,
                              double alpha, const double* x_lb0, const double* x_ub0, const double* lo, const double* hi,
                              const double* soft_l1, const double* soft_l2, const double* x0, const double* xRef, const double* uRef,
                              const double* rho_p, const int32_t* problem, int64_t P, double eps_abs, double eps_rel,
                              double eps_prim_inf, int max_iter, int warm_start, double* workspace, double* xTraj, double* uTraj,
                              int32_t* status, int32_t* iters, double* resid, int64_t batch, int N, int n, int m, void* stream);

/* Real-time-iteration nonlinear MPC (extension): zm_mpc_solve_ltv_f64 on the linearisation of a REGISTERED MODEL about a plan, every
 * instance its own problem (P = batch, problem[i] = i).  Shapes: the model's (n_user, m_user) embedded in a compiled (ns, mc) of the
 * 16-lanes-per-instance kernels, as zopt_amd/mpcUtils.py embeds them; models: ZM_MODEL_QUADCOPTER (12, 4) and ZM_MODEL_QUADCOPTER_RB
 * (8, 4) with dt > 0, ZM_MODEL_LINEAR with n <= 12, m <= 4.
 * zm_model_step_f64: xNext[b] = f(x[b], u[b]), one step of the model's step function per instance.
 *     Replaces: calling the reference's dynamics callable (zopt/quadcopter.py:116-144 under demos/iterativeLqr.py:35's Euler step) per
 *     instance; it is the plant of zm_mpc_rti_f64 as a call of its own (the same kernel).
 *     in : x (batch,n)  u (batch,m)   out: xNext (batch,n)   [device]
 * zm_mpc_relinearize_f64: the expansion of zm_linearize_dynamics_f64 (the same device functions) about stage k of instance b's plan,
 *     written as the problem data of zm_mpc_setup_ltv_f64 / zm_mpc_solve_ltv_f64:
 *         A[b][k] <- f_x,  B[b][k] <- f_u  (the leading n_user x n_user / n_user x m_user blocks; padding is left as it is),
 *         c[b][k] <- f - f_x xbar_k - f_u ubar_k  (the first n_user components), each component ONE FMA chain in this order:
 *         s = f_i;  s = fma(-f_x[i][j], xbar_k[j], s), j = 0 .. n_user-1;  then  s = fma(-f_u[i][j], ubar_k[j], s), j = 0 .. m_user-1.
 *     Replaces: AffineDynamics.from_trajectory (zopt/pytrees.py:147-153) followed by the host-side c_k of ltvMpc.fromExpansion and the
 *     copies of ltvMpc.update (zopt_amd/mpcUtils.py).
 *     in : xPlan (batch,N+1,n_user)  uPlan (batch,N,m_user), absolute coordinates   [device]
 *     out: A (batch,N,ns,ns)  B (batch,N,ns,mc)  c (batch,N,ns)   [device]
 * zm_mpc_rti_f64: `steps` real-time iterations of every instance as ONE call,
 *         x <- clip(x0);  states[0] = x
 *         per step s:  zm_mpc_relinearize_f64 about the plan;  zm_mpc_setup_ltv_f64;  zm_mpc_solve_ltv_f64 from states[s], tracking rows
 *                      s .. s + N of xRef and s .. s + N - 1 of uRef (step 0 cold, later steps with `warm_start`);  inputs[s] = uTraj_s[0];
 *                      states[s + 1] = clip(f_plant(states[s], inputs[s]) + disturbance[s]);
 *                      plan <- rows 1 .. N of xTraj_s and 1 .. N - 1 of uTraj_s, the last row repeated (its head is the PREDICTED successor)
 *     -- exactly what that loop of calls computes, whatever the status of a step: a step that does not end "optimal" still leaves a
 *     rollout, and the step after it starts cold.  The plant step is the model's step function (zm_model_step_f64), not an expansion.
 *     Replaces: the Python loop of tools/examples/mpc_ltv.py (real-time iteration with zopt's pytrees.AffineDynamics.from_trajectory,
 *     zopt/pytrees.py:147-153, around an MPC solve, zopt/mpcUtils.py:61-81, as demos/lqrMpc.py:40-47 loops around it).
 *     After the argument checks and one read-back of `problem` (it must be the identity) the call only enqueues on `stream`: per step the
 *     expansion, the table setup, the linear term of the window, the solve, the plant step and the plan shift; nothing is synchronised or
 *     copied to the host inside the loop.
 *     in : model; plant: the model the state is advanced with, of the same (n, m) (NULL: `model`)
 *          xPlan (batch,N+1,n_user)  uPlan (batch,N,m_user): the first expansion point; on return the plan after the last step's shift
 *          A, B, c as zm_mpc_relinearize_f64 writes them (their padding must hold what zm_mpc_solve_ltv_f64 expects: zero); on return
 *          the last step's linearisation.  Q (batch,ns,ns)  R (batch,mc,mc)  Qf (batch,ns,ns)  bounds (batch,ns) / (batch,mc)
 *          rho_tab (batch,n_levels): the penalty of each (problem, level), as zm_mpc_setup_ltv_f64 takes it;  rho_p (batch): level0's
 *          K, Minv, D, ABt: the tables of zm_mpc_setup_ltv_f64 (P = batch), written at every step; on return those of the last step
 *          x0 (batch,ns);  xRef (batch,xref_rows,ns), uRef (batch,uref_rows,mc) with xref_rows = steps + N, uref_rows = steps + N - 1,
 *          either may be NULL;  disturbance (steps,batch,ns) or NULL;  clip_tol >= 0, or negative for no clip;  warm_start 0 / 1 / 2
 *          workspace: 5 * batch * N * (ns + mc) doubles (on return the warm-start state of the last step), plus
 *                     batch * ((N + 1) * ns + N * mc) doubles when xPred is NULL   [device]
 *     out: STEP-MAJOR, as zm_mpc_closed_loop_f64: states (steps+1,batch,ns)  inputs (steps,batch,mc)  status, iters (steps,batch) int32
 *          resid (batch,2) or NULL: the residuals of the last step;  xPred (steps,batch,N+1,ns)  uPred (steps,batch,N,mc) or both NULL
 *     ZM_EUNSUPPORTED, before any launch, for (ns, mc) and N outside zm_mpc_solve_ltv_f64's. */
int zm_model_step_f64(const zm_model_t* model, const double* x, const double* u, double* xNext, int64_t batch, void* stream);
int zm_mpc_relinearize_f64(const zm_model_t* model, const double* xPlan, const double* uPlan, double* A, double* B, double* c,
                           int64_t batch, int N, int n_user, int m_user, int ns, int mc, void* stream);
int zm_mpc_rti_f64(const zm_model_t* model, const zm_model_t* plant, double* xPlan, double* uPlan, double* A, double* B, double* c,
                   const double* Q, const double* R, const double* Qf, const double* rho_tab, double* K, double* Minv, double* D,
                   double* ABt, int n_levels, int level0, double rho_step, double alpha, const double* x_lb, const double* x_ub,
                   const double* u_lb, const double* u_ub, const double* x0, const double* xRef, const double* uRef, int xref_rows,
                   int uref_rows, const double* rho_p, const int32_t* problem, double eps_abs, double eps_rel, double eps_prim_inf,
                   int max_iter, int warm_start, int steps, double clip_tol, const double* disturbance, double* workspace,
                   double* states, double* inputs, int32_t* status, int32_t* iters, double* resid, double* xPred, double* uPred,
                   int64_t batch, int N, int n_user, int m_user, int ns, int mc, void* stream);

/* ---- Recorded cost functions (Python: zopt_amd.models.TracedCost): runningCost(x, u[, p]) and terminalCost(x[, p]) as two tapes of the
 *      ZM_MODEL_TRACED interpreter with ONE output each -- the part the reference's cost callables play (zopt/ilqrUtils.py:260-269,
 *      pytrees.py:27-55, :72-115).  Both tapes use the input slot layout [x | u | p]; the terminal tape leaves its control slots unread.
 *      A tape is n_const fp64 constants, n_instr instruction words, then ONE 32-bit output slot number (zero padded to 8 bytes).
 *      running_mask / terminal_mask: the variables the tape is not affine in (bit i state i, bit n + j control j): only pairs of those
 *      have second derivatives.  params / param_stride / n_params of each tape: as zm_traced_t (normally the same rows for both).
 *      Caps: those of zm_traced_t, 1 <= n <= 12, 1 <= m <= 4. */
typedef struct zm_tracedcost_t {   /* 96 bytes */
    zm_traced_t running;
    zm_traced_t terminal;
    int32_t n, m;
    uint32_t running_mask, terminal_mask;
} zm_tracedcost_t;

/* zm_rollout_linesearch_list_f64 with a recorded cost in place of the zm_quadcost_t (list may be NULL: all trajectories; n_alpha is 1 or
 * up to 16).  Per step: the policy, J += c(x_k, u_k, p) (k ascending, a plain add), the model step (a registered model with n <= 12,
 * m <= 4, or a traced one); after the last step J += v(x_T, p).  A NaN cost wins the argmin, the first index wins among equals; the
 * winner is rolled out again with the same arithmetic and stored.  The interpreter's value path has contraction off: the per-step
 * costs equal a host build's bit for bit. */
int zm_traced_cost_linesearch_list_f64(const zm_model_t* model, const zm_tracedcost_t* tcost, const double* x0, const double* l,
                                       const double* L, const double* xPrev, const double* uPrev, const double* alphas, int n_alpha,
                                       const int32_t* list, int64_t count, const int32_t* active, double* xTraj, double* uTraj,
                                       double* J, int32_t* alpha_idx, int64_t batch, int T, void* stream);
/* Second-order expansion of a recorded cost along xTraj (batch,T+1,n), uTraj (batch,T,m): replaces QuadraticCostFunction.from_trajectory
 * (zopt/pytrees.py:109-115), QuadraticValueFunction.fromTerminalCostFunction (:72-81) and CostFunction.__call__ (:40-55, through c, v).
 * out: c (batch,T)  c_x (batch,T,n)  c_u (batch,T,m)  c_xx (batch,T,n,n)  c_ux (batch,T,m,n)  c_uu (batch,T,m,m)  v (batch)
 *      v_x (batch,n)  v_xx (batch,n,n); any may be NULL and is then skipped (c_xx, c_ux, c_uu: all or none).  Values and gradients on
 *      dual numbers (16 lanes per point, lane j owns entry j of [c_x | c_u]), Hessians on hyper-dual numbers over the unordered pairs of
 *      the tape's mask, every other entry zero.  list (may be NULL) / active: as zm_linearize_dynamics_list_f64. */
int zm_traced_cost_expand_list_f64(const zm_tracedcost_t* tcost, const double* xTraj, const double* uTraj, const int32_t* list,
                                   int64_t count, const int32_t* active, double* c, double* c_x, double* c_u, double* c_xx, double* c_ux,
                                   double* c_uu, double* v, double* v_x, double* v_xx, int64_t batch, int T, void* stream);
/* The iLQR (ddp = 0) / DDP (ddp = 1) loop of zm_ilqr_solve_f64 with a recorded cost: the line search above, the model's own expansion
 * with full Jacobians plus the cost expansion above, the PD projections of zm_condition_cost_f64 / zm_psd_project_f64 applied in every
 * iteration to the per-point Hessians of the listed trajectories (zopt/ilqrUtils.py:309-313), and the list sweeps with
 * shared_hessian = 0.  No packed Jacobians, no all-store line search, no ring sweep.  Arguments as zm_ilqr_solve_f64 /
 * zm_ilqr_solve_trace_f64; the workspace is zm_ilqr_solve_workspace_f64's with the four shared Hessians replaced by per-point arrays of
 * batch*T*(n*n + m*n + m*m) + batch*n*n doubles (each piece rounded up to an even count) and without the all-store block:
 * zm_traced_cost_solve_workspace_f64 returns the total, -1 if it cannot. */
int64_t zm_traced_cost_solve_workspace_f64(const zm_model_t* model, const zm_tracedcost_t* tcost, int64_t batch, int T, int ddp);
int zm_traced_cost_solve_f64(const zm_model_t* model, const zm_tracedcost_t* tcost, const double* x0, const double* uGuess, int ddp,
                             int max_iter, double tol, int sync_every, double* workspace, int64_t workspace_doubles, int32_t* iwork,
                             double* xTraj, double* uTraj, double* L, double* J, int32_t* converged, int32_t* iterations, int64_t batch,
                             int T, void* stream);
int zm_traced_cost_solve_trace_f64(const zm_model_t* model, const zm_tracedcost_t* tcost, const double* x0, const double* uGuess, int ddp,
                                   int max_iter, double tol, int sync_every, double* workspace, int64_t workspace_doubles,
                                   int32_t* iwork, double* xTraj, double* uTraj, double* L, double* J, int32_t* converged,
                                   int32_t* iterations, int64_t batch, int T, void* stream, double* J_trace, int32_t* alpha_trace);

/* ---- Recorded inequality constraints (Python: zopt_amd.models.TracedConstraint): g(x, u[, p]) <= 0 with n_con values on (x_k, u_k),
 *      k = 0 .. T-1, and terminal(x[, p]) <= 0 with n_con_terminal values on x_T, as two tapes of the ZM_MODEL_TRACED interpreter with
 *      SEVERAL outputs each.  Extends zm_tracedcost_t (the same slot layout [x | u | p], the same blob with n_con resp. n_con_terminal
 *      output slot numbers behind the instruction words) and zm_statebox_t (the same augmented Lagrangian on g in place of the box
 *      distances):  s_i = lam_i + mu g_i,  pos(s) = s > 0 ? s : 0 (a NaN gives 0),  psi = sum_i (pos(s_i)^2 - lam_i^2) / (2 mu),
 *      gradient G^T pos(s) with G = dg/d(x, u), Gauss-Newton Hessian mu G^T diag(s_i > 0) G (no second derivatives of g).
 *      A tape with no outputs (n_con == 0 resp. n_con_terminal == 0) is absent: its tape pointer is not read.  At least one is present.
 *      lam (batch, T, n_con), lam_terminal (batch, n_con_terminal), mu (batch): the caller's device arrays, as lam_lb / lam_ub / mu of
 *      zm_statebox_t.  Caps: those of zm_traced_t, 1 <= n <= 12, 1 <= m <= 4, n_con <= 8, n_con_terminal <= 8. */
#define ZM_TRACEDCON_MAX 8
typedef struct zm_tracedcon_t {   /* 120 bytes */
    zm_traced_t stage;
    zm_traced_t terminal;
    int32_t n, m, n_con, n_con_terminal;
    double* lam;
    double* lam_terminal;
    double* mu;
} zm_tracedcon_t;

/* g along given trajectories: g (batch, T, n_con) <- g(x_k, u_k, p), g_terminal (batch, n_con_terminal) <- terminal(x_T, p); either
 * may be NULL.  The interpreter's value path: bits equal to a host build's.  lam, lam_terminal and mu are not read. */
int zm_traced_con_values_f64(const zm_tracedcon_t* con, const double* xTraj, const double* uTraj, double* g, double* g_terminal,
                             int64_t batch, int T, void* stream);
/* zm_rollout_linesearch_state_list_f64 on the constraint's penalty: the cost is `cost` or `track` (exactly one; a traced model takes
 * `cost` only).  Per step: the policy, the cost, the stage tape with psi accumulated into an accumulator of its own (k ascending, i
 * ascending, terminal rows last), the model step; the penalty joins the cost once, at the end.  J <- cost + penalty, J_cost
 * (optional) <- the cost without it, written by the store pass.  n_alpha is 1 or 16. */
int zm_traced_con_linesearch_list_f64(const zm_model_t* model, const zm_quadcost_t* cost, const zm_trackcost_t* track,
                                      const zm_tracedcon_t* con, const double* x0, const double* l, const double* L, const double* xPrev,
                                      const double* uPrev, const double* alphas, int n_alpha, const int32_t* list, int64_t count,
                                      const int32_t* active, double* xTraj, double* uTraj, double* J, double* J_cost, int32_t* alpha_idx,
                                      int64_t batch, int T, void* stream);
/* zm_state_penalty_expand_list_f64 for the recorded constraint: behind the cost expansion, per listed active trajectory
 * c_x[k] += G_x^T pos(s), c_u[k] += G_u^T pos(s), v_x += G_T^T pos(s_T), and the per-point Hessians
 * [c_xx c_ux^T; c_ux c_uu][k] <- the shared (conditioned) set sc_xx (n,n), sc_ux (m,n), sc_uu (m,m) + mu G^T diag(s > 0) G,
 * v_xx (batch,n,n) <- sv_xx (n,n) + the same of the terminal rows.  16 lanes per point: lane j runs the tape on dual numbers seeded
 * e_j and owns entry j of the gradient and row j of the Hessian.  Rows of trajectories not listed or not active are not touched. */
int zm_traced_con_expand_list_f64(const zm_tracedcon_t* con, const double* xTraj, const double* uTraj, const int32_t* list, int64_t count,
                                  const int32_t* active, const double* sc_xx, const double* sc_ux, const double* sc_uu,
                                  const double* sv_xx, double* c_x, double* c_u, double* v_x, double* c_xx, double* c_ux, double* c_uu,
                                  double* v_xx, int64_t batch, int T, void* stream);
/* zm_state_multiplier_update_f64 for the recorded constraint: viol_t = max over the rows and i of pos(g_i), NaN if any g is NaN; the
 * done test, the masks, the counters and the update lam <- pos(lam + mu g), mu <- min(mu growth, mu_max) as there. */
int zm_traced_con_multiplier_update_f64(const zm_tracedcon_t* con, const double* xTraj, const double* uTraj, int32_t* active,
                                        int32_t* converged, double* violation, int32_t* outer_count, int32_t* remaining, double ctol,
                                        double growth, double mu_max, int update, int64_t batch, int T, void* stream);
/* zm_ilqr_solve_state_f64 with the recorded constraint in place of the state box: the same outer loop around the loop of
 * zm_ilqr_solve_f64 with the line search, the expansion and the multiplier update above, per-point Hessians (the workspace of
 * zm_traced_cost_solve_workspace_f64 plus one shared conditioned set) and the list sweeps with shared_hessian = 0.  ddp must be 0.
 * Every argument is checked before any launch.  Outputs and traces as zm_ilqr_solve_state_f64 / zm_ilqr_solve_state_trace_f64. */
int64_t zm_traced_con_solve_workspace_f64(const zm_model_t* model, int64_t batch, int T);
int zm_traced_con_solve_f64(const zm_model_t* model, const zm_quadcost_t* cost, const zm_trackcost_t* track, const zm_tracedcon_t* con,
                            double mu0, double growth, double mu_max, int outer, double ctol, const double* x0, const double* uGuess,
                            int ddp, int max_iter, double tol, int sync_every, double* workspace, int64_t workspace_doubles,
                            int32_t* iwork, double* xTraj, double* uTraj, double* L, double* J, int32_t* converged, double* violation,
                            int32_t* outer_iterations, int32_t* inner_iterations, int32_t* iterations, int64_t batch, int T,
                            void* stream);
int zm_traced_con_solve_trace_f64(const zm_model_t* model, const zm_quadcost_t* cost, const zm_trackcost_t* track,
                                  const zm_tracedcon_t* con, double mu0, double growth, double mu_max, int outer, double ctol,
                                  const double* x0, const double* uGuess, int ddp, int max_iter, double tol, int sync_every,
                                  double* workspace, int64_t workspace_doubles, int32_t* iwork, double* xTraj, double* uTraj, double* L,
                                  double* J, int32_t* converged, double* violation, int32_t* outer_iterations,
                                  int32_t* inner_iterations, int32_t* iterations, int64_t batch, int T, void* stream, double* J_trace,
                                  int32_t* alpha_trace, double* violation_trace, double* mu_trace);

#ifdef __cplusplus
}
#endif
#endif /* ZOPT_AMD_H */
