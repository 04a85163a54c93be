// zm_tracedcost_t: a recorded cost function on the interpreter of tape_model.h -- runningCost(x, u, p) and terminalCost(x, p) as two
// tapes with ONE output each (recorder: zopt_amd/tape.py with n_out = 1; Python handle: zopt_amd.models.TracedCost).
//
// Both tapes use the input slot layout [x | u | p] of a traced model, so one slot file serves both (and a traced model's step between
// them): the launch sizes the file by the largest slot count it runs.  The terminal tape never reads its control slots, and they are
// not written for it.  The value path is tape_run's: contraction off, bits equal to the host build's (tests/tape_cost_shim.cpp).
#pragma once
#include "tape_model.h"

namespace zm {

// One evaluation of the tape `t` of a cost over (n, m): c(x, u, p) with CONTROLS, v(x, p) without.
template <typename S, bool CONTROLS, typename SLOTS>
__device__ __forceinline__ S tape_cost(const zm_traced_t& t, const int n, const int m, SLOTS& f, const S (&x)[MAXN], const S (&u)[MAXM],
                                       const double* __restrict__ prow) {
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
    return f.get((int)(tape_uniform(outs[0]) & (unsigned)(ZM_TRACED_MAX_SLOTS - 1)));
}

__host__ __device__ inline const double* tape_cost_params(const zm_traced_t& t, const long traj) {
    return t.params ? t.params + traj * t.param_stride : nullptr;
}

}  // namespace zm
