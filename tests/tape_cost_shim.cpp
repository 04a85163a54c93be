// Host build of the recorded costs' interpreter (zopt_amd/csrc/tape_cost.h around tape_model.h) for tests/test_traced_cost.py and
// tests/test_traced_cost_gpu.py: the same headers the kernels include, compiled by g++ -ffp-contract=off, so that the costs can be held
// bit for bit against NumPy and against the device, and their Dual / Hyper derivatives against the long-double references, without a
// GPU.  The qualifiers are defined away and <hip/hip_runtime.h> is met by an empty file of that name on the include path, as in
// tests/tape_shim.cpp.  The slot file is the private-array policy (ArraySlots).
#define __device__
#define __host__
#define __forceinline__ inline
#include "tape_cost.h"

namespace {
// blob: the tape as the device reads it (constants, instruction words, the output slot); controls = 0: a terminal tape
zm_traced_t descriptor(const void* blob, int n_instr, int n_const, int n_slots, int np) {
    return zm_traced_t{blob, nullptr, 0, n_instr, n_const, n_slots, np};
}
template <typename S>
S eval(const zm_traced_t& t, int n, int m, int controls, const S (&x)[zm::MAXN], const S (&u)[zm::MAXM], const double* prow) {
    zm::ArraySlots<S> f;
    return controls ? zm::tape_cost<S, true>(t, n, m, f, x, u, prow) : zm::tape_cost<S, false>(t, n, m, f, x, u, prow);
}
}  // namespace

// c (P) on double
extern "C" void cost_value(const void* blob, int n_instr, int n_const, int n_slots, int n, int m, int np, int controls, const double* x,
                           const double* u, const double* p, long p_stride, long P, double* c) {
    const zm_traced_t t = descriptor(blob, n_instr, n_const, n_slots, np);
    for (long i = 0; i < P; ++i) {
        double xs[zm::MAXN] = {}, us[zm::MAXM] = {};
        for (int a = 0; a < n; ++a) xs[a] = x[i * n + a];
        for (int a = 0; a < m; ++a) us[a] = controls ? u[i * m + a] : 0.0;
        c[i] = eval<double>(t, n, m, controls, xs, us, p ? p + i * p_stride : nullptr);
    }
}

// g (P, n + m) = [c_x | c_u] on Dual, one seed direction per evaluation
extern "C" void cost_gradient(const void* blob, int n_instr, int n_const, int n_slots, int n, int m, int np, int controls, const double* x,
                              const double* u, const double* p, long p_stride, long P, double* g) {
    const zm_traced_t t = descriptor(blob, n_instr, n_const, n_slots, np);
    const int K = n + m;
    for (long i = 0; i < P; ++i)
        for (int j = 0; j < K; ++j) {
            zm::Dual xs[zm::MAXN] = {}, us[zm::MAXM] = {};
            for (int a = 0; a < n; ++a) xs[a] = zm::Dual{x[i * n + a], a == j ? 1.0 : 0.0};
            for (int a = 0; a < m; ++a) us[a] = zm::Dual{controls ? u[i * m + a] : 0.0, n + a == j ? 1.0 : 0.0};
            g[i * K + j] = eval<zm::Dual>(t, n, m, controls, xs, us, p ? p + i * p_stride : nullptr).d;
        }
}

// H (P, K, K), K = n + m, on Hyper: every pair a <= b evaluated once and mirrored
extern "C" void cost_hessian(const void* blob, int n_instr, int n_const, int n_slots, int n, int m, int np, int controls, const double* x,
                             const double* u, const double* p, long p_stride, long P, double* H) {
    const zm_traced_t t = descriptor(blob, n_instr, n_const, n_slots, np);
    const int K = n + m;
    for (long i = 0; i < P; ++i)
        for (int a = 0; a < K; ++a)
            for (int b = a; b < K; ++b) {
                zm::Hyper xs[zm::MAXN] = {}, us[zm::MAXM] = {};
                for (int c = 0; c < n; ++c) xs[c] = zm::Hyper{x[i * n + c], c == a ? 1.0 : 0.0, c == b ? 1.0 : 0.0, 0.0};
                for (int c = 0; c < m; ++c) us[c] = zm::Hyper{controls ? u[i * m + c] : 0.0, n + c == a ? 1.0 : 0.0, n + c == b ? 1.0 : 0.0, 0.0};
                const double h = eval<zm::Hyper>(t, n, m, controls, xs, us, p ? p + i * p_stride : nullptr).d12;
                H[(i * K + a) * K + b] = h;
                H[(i * K + b) * K + a] = h;
            }
}
