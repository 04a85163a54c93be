// Host build of the recorded constraints' interpreter (zopt_amd/csrc/tape_con.h around tape_model.h) for tests/test_traced_con.py and
// tests/test_traced_con_gpu.py: the same headers the kernels include, compiled by g++ -ffp-contract=off, so that g can be held bit for
// bit against NumPy and against the device, and its Dual Jacobian and the penalty's arithmetic checked, without a GPU.  The qualifiers
// are defined away and <hip/hip_runtime.h> is met by an empty file of that name on the include path, as in tests/tape_cost_shim.cpp.
// The slot file is the private-array policy (ArraySlots).
#define __device__
#define __host__
#define __forceinline__ inline
#include "tape_con.h"

namespace {
// blob: the tape as the device reads it (constants, instruction words, the nc output slots); controls = 0: a terminal tape
zm_traced_t descriptor(const void* blob, int n_instr, int n_const, int n_slots, int np) {
    return zm_traced_t{blob, nullptr, 0, n_instr, n_const, n_slots, np};
}
template <typename S>
void eval(const zm_traced_t& t, int n, int m, int nc, int controls, const S (&x)[zm::MAXN], const S (&u)[zm::MAXM], const double* prow,
          S (&g)[zm::MAXC]) {
    zm::ArraySlots<S> f;
    if (controls) zm::tape_con<S, true>(t, n, m, nc, f, x, u, prow, g);
    else zm::tape_con<S, false>(t, n, m, nc, f, x, u, prow, g);
}
}  // namespace

// g (P, nc) on double
extern "C" void con_value(const void* blob, int n_instr, int n_const, int n_slots, int n, int m, int np, int nc, int controls,
                          const double* x, const double* u, const double* p, long p_stride, long P, double* g) {
    const zm_traced_t t = descriptor(blob, n_instr, n_const, n_slots, np);
    for (long i = 0; i < P; ++i) {
        double xs[zm::MAXN] = {}, us[zm::MAXM] = {}, gs[zm::MAXC];
        for (int a = 0; a < n; ++a) xs[a] = x[i * n + a];
        for (int a = 0; a < m; ++a) us[a] = controls ? u[i * m + a] : 0.0;
        eval<double>(t, n, m, nc, controls, xs, us, p ? p + i * p_stride : nullptr, gs);
        for (int r = 0; r < nc; ++r) g[i * nc + r] = gs[r];
    }
}

// G (P, nc, n + m) on Dual, one seed direction per evaluation
extern "C" void con_jacobian(const void* blob, int n_instr, int n_const, int n_slots, int n, int m, int np, int nc, int controls,
                             const double* x, const double* u, const double* p, long p_stride, long P, double* G) {
    const zm_traced_t t = descriptor(blob, n_instr, n_const, n_slots, np);
    const int K = n + m;
    for (long i = 0; i < P; ++i)
        for (int j = 0; j < K; ++j) {
            zm::Dual xs[zm::MAXN] = {}, us[zm::MAXM] = {}, gs[zm::MAXC];
            for (int a = 0; a < n; ++a) xs[a] = zm::Dual{x[i * n + a], a == j ? 1.0 : 0.0};
            for (int a = 0; a < m; ++a) us[a] = zm::Dual{controls ? u[i * m + a] : 0.0, n + a == j ? 1.0 : 0.0};
            eval<zm::Dual>(t, n, m, nc, controls, xs, us, p ? p + i * p_stride : nullptr, gs);
            for (int r = 0; r < nc; ++r) G[(i * nc + r) * K + j] = gs[r].d;
        }
}

// psi (count) of the line search's penalty terms: (pos(lam + mu g)^2 - lam^2) / (2 mu), each operation rounded on its own
extern "C" void con_psi(const double* g, const double* lam, const double* mu, long count, double* psi) {
    for (long i = 0; i < count; ++i) psi[i] = zm::con_psi(g[i], lam[i], mu[i]);
}
