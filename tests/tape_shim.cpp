// Host build of the traced models' interpreter (zopt_amd/csrc/tape_model.h) for tests/test_traced_model.py and
// tests/test_traced_model_gpu.py: the same header the kernels include, compiled by g++ -ffp-contract=off, so that its values can be
// held bit for bit against the NumPy evaluator (tests/tape_ref.py) and against the device, and its Dual / Hyper derivatives against the
// long-double references, without a GPU.  The qualifiers are defined away and <hip/hip_runtime.h> is met by an empty file of that name
// on the include path, as in tests/trig_shim.cpp.  The slot file is the private-array policy (ArraySlots).
#define __device__
#define __host__
#define __forceinline__ inline
#include "tape_model.h"

namespace {
// (zm::tape_step reads one blob of constants, code and outputs; the tests pass the three pieces, so this runs the pieces directly)
template <typename S>
void run_point(const uint32_t* code, int n_instr, const double* consts, const uint32_t* outs, int n, int m, int np, const S* x,
               const S* u, const double* prow, S* xn) {
    zm::ArraySlots<S> f;
    for (int i = 0; i < n; ++i) f.set(i, x[i]);
    for (int j = 0; j < m; ++j) f.set(n + j, u[j]);
    for (int q = 0; q < np; ++q) f.set(n + m + q, zm::TapeNum<S>::lift(prow[q]));
    zm::tape_run<S, zm::ArraySlots<S>>(code, n_instr, consts, f);
    for (int i = 0; i < n; ++i) xn[i] = f.get((int)outs[i]);
}
}  // namespace

// x+ (P, n) on double
extern "C" void tape_step(const void* code, int n_instr, const void* consts, const void* outs, int n, int m, int np, const double* x,
                          const double* u, const void* p, long p_stride, long P, double* xn) {
    for (long i = 0; i < P; ++i)
        run_point<double>((const uint32_t*)code, n_instr, (const double*)consts, (const uint32_t*)outs, n, m, np, x + i * n, u + i * m,
                          p ? (const double*)p + i * p_stride : nullptr, xn + i * n);
}

// f (P, n) and [f_x | f_u] (P, n, n + m) on Dual, one seed direction per evaluation
extern "C" void tape_jacobian(const void* code, int n_instr, const void* consts, const void* outs, int n, int m, int np,
                              const double* x, const double* u, const void* p, long p_stride, long P, double* f, double* J) {
    const int K = n + m;
    for (long i = 0; i < P; ++i)
        for (int j = 0; j < K; ++j) {
            zm::Dual xs[zm::MAXN], us[zm::MAXM], xn[zm::MAXN];
            for (int a = 0; a < n; ++a) xs[a] = zm::Dual{x[i * n + a], a == j ? 1.0 : 0.0};
            for (int a = 0; a < m; ++a) us[a] = zm::Dual{u[i * m + a], n + a == j ? 1.0 : 0.0};
            run_point<zm::Dual>((const uint32_t*)code, n_instr, (const double*)consts, (const uint32_t*)outs, n, m, np, xs, us,
                                p ? (const double*)p + i * p_stride : nullptr, xn);
            for (int a = 0; a < n; ++a) {
                J[(i * n + a) * K + j] = xn[a].d;
                if (j == 0) f[i * n + a] = xn[a].v;
            }
        }
}

// H (P, n, K, K), K = n + m: H[i][a][b] = d2 f_i / dz_a dz_b on Hyper, every pair a <= b evaluated once and mirrored
extern "C" void tape_hessian(const void* code, int n_instr, const void* consts, const void* outs, int n, int m, int np,
                             const double* x, const double* u, const void* p, long p_stride, long P, double* H) {
    const int K = n + m;
    for (long i = 0; i < P; ++i)
        for (int a = 0; a < K; ++a)
            for (int b = a; b < K; ++b) {
                zm::Hyper xs[zm::MAXN], us[zm::MAXM], xn[zm::MAXN];
                for (int c = 0; c < n; ++c) xs[c] = zm::Hyper{x[i * n + c], c == a ? 1.0 : 0.0, c == b ? 1.0 : 0.0, 0.0};
                for (int c = 0; c < m; ++c) us[c] = zm::Hyper{u[i * m + c], n + c == a ? 1.0 : 0.0, n + c == b ? 1.0 : 0.0, 0.0};
                run_point<zm::Hyper>((const uint32_t*)code, n_instr, (const double*)consts, (const uint32_t*)outs, n, m, np, xs, us,
                                     p ? (const double*)p + i * p_stride : nullptr, xn);
                for (int c = 0; c < n; ++c) {
                    H[((i * n + c) * K + a) * K + b] = xn[c].d12;
                    H[((i * n + c) * K + b) * K + a] = xn[c].d12;
                }
            }
}
