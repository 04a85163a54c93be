// zm_tracedcon_t: recorded inequality constraints on the interpreter of tape_model.h -- g(x, u, p) <= 0 and terminal(x, p) <= 0 as two
// tapes with SEVERAL outputs each (recorder: zopt_amd/tape.py with n_out = n_con; Python handle: zopt_amd.models.TracedConstraint).
//
// Both tapes use the input slot layout [x | u | p] of a traced model, as the cost tapes of tape_cost.h do, so one slot file serves
// both and a traced model's step between them.  The value path is tape_run's: contraction off, bits equal to the host build's
// (tests/tape_con_shim.cpp).
//
// The augmented Lagrangian is state_box.h's on g in place of the box distances:
//   s_i = lam_i + mu g_i,  pos(s) = s > 0 ? s : 0  (a NaN gives 0),  psi = sum_i (pos(s_i)^2 - lam_i^2) / (2 mu)
//   gradient G^T pos(s), Gauss-Newton Hessian mu G^T diag(s_i > 0) G with G = dg / d(x, u)
#pragma once
#include "tape_model.h"

namespace zm {

constexpr int MAXC = ZM_TRACEDCON_MAX;

// One evaluation of the tape `t` with nc outputs: g(x, u, p) with CONTROLS, terminal(x, p) without.  Entries nc .. MAXC-1 are zero.
template <typename S, bool CONTROLS, typename SLOTS>
__device__ __forceinline__ void tape_con(const zm_traced_t& t, const int n, const int m, const int nc, SLOTS& f, const S (&x)[MAXN],
                                         const S (&u)[MAXM], const double* __restrict__ prow, S (&g)[MAXC]) {
    const double* consts = (const double*)t.tape;
    const uint32_t* code = (const uint32_t*)(consts + t.n_const);
    const uint32_t* outs = code + t.n_instr;
#pragma unroll
    for (int i = 0; i < MAXN; ++i)
        if (i < n) f.set(i, x[i]);
    if (CONTROLS) {
#pragma unroll
        for (int j = 0; j < MAXM; ++j)
            if (j < m) f.set(n + j, u[j]);
    }
    for (int q = 0; q < t.n_params; ++q) f.set(n + m + q, TapeNum<S>::lift(prow[q]));
    tape_run<S, SLOTS>(code, t.n_instr, consts, f);
#pragma unroll
    for (int i = 0; i < MAXC; ++i)
        g[i] = (i < nc) ? f.get((int)(tape_uniform(outs[i]) & (unsigned)(ZM_TRACED_MAX_SLOTS - 1))) : TapeNum<S>::lift(0.0);
}

__host__ __device__ inline const double* tape_con_params(const zm_traced_t& t, const long traj) {
    return t.params ? t.params + traj * t.param_stride : nullptr;
}

__device__ __forceinline__ double con_pos(const double s) { return s > 0.0 ? s : 0.0; }   // NaN -> 0

// s and psi of one row entry: every operation rounds on its own (no contraction), so that NumPy restates the bits
__device__ __forceinline__ double con_slack(const double g, const double lam, const double mu) {
#pragma clang fp contract(off)
    return lam + mu * g;
}
__device__ __forceinline__ double con_psi(const double g, const double lam, const double mu) {
#pragma clang fp contract(off)
    const double p = con_pos(con_slack(g, lam, mu));
    return (p * p - lam * lam) / (2.0 * mu);
}

}  // namespace zm
