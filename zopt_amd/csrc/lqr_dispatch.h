// Host side of the LQR family: every dispatch function that one source file defines and another calls, declared once, and the two
// choices of a kernel instantiation by the state dimension.  Host only: no kernel sees this header.
#pragma once
#include <cstdint>
#include <type_traits>

#include <hip/hip_runtime.h>

namespace zm {

// What the discrete entries cover (zm_lqr_backward_supported is defined by these two and nothing else restates them).
constexpr int LQR_MAX_N = 64, LQR_MAX_M = 16;

// Each takes what the entry point in front of it has checked (zm_common.h: zm_check_sweep_args / zm_check_design_args) and returns ZM_OK,
// a HIP error, or ZM_EUNSUPPORTED for a shape / alignment it does not serve -- the caller then goes on to its fallback kernel.
// lqr_backward_dma.hip: the LDS-DMA ring (K1) for (n, m) in {(8, 4), (12, 4)} on 16-byte aligned arrays, fp64 and fp32 storage
int lqr_backward_dma_dispatch(const double* A, const double* B, const double* Q, const double* R, double* L, int64_t batch, int T,
                              int n, int m, hipStream_t stream);
int lqr_backward_dma_dispatch_f32io(const float* A, const float* B, const float* Q, const float* R, float* L, int64_t batch, int T,
                                    int n, int m, hipStream_t stream);
// lqr_backward_lds_f64.hip: the coverage kernel, any n <= 64, m <= 16
int lqr_backward_lds_dispatch(const double* A, const double* B, const double* Q, const double* R, double* L, int64_t batch, int T,
                              int n, int m, hipStream_t st);
// lqr_backward_tiled_f64.hip: the fp64 MFMA tile kernel (n <= 64, m <= 16), as a sweep and as the DARE's value iteration
int lqr_backward_tiled_f64_dispatch(const double* A, const double* B, const double* Q, const double* R, double* L, int64_t batch,
                                    int T, int n, int m, hipStream_t st);
int lqr_dare_tiled_f64_dispatch(const double* A, const double* B, const double* Q, const double* R, double* L, double* P, int* iters,
                                int64_t batch, int n, int m, double tol, int max_iter, hipStream_t st);

// The register-tile sweep kernels are instantiated per KS = ceil(n / 4) tile rows, n <= 12: calls f(ks) with ks an integral_constant,
// so that a kernel family is written once as `[&](auto ks) { launch family<decltype(ks)::value> }`.
template <typename F>
static void with_ks(const int n, F&& f) {
    if (n <= 4) f(std::integral_constant<int, 1>{});
    else if (n <= 8) f(std::integral_constant<int, 2>{});
    else f(std::integral_constant<int, 3>{});
}

// The MFMA tile kernels are instantiated per NT = ceil(n / 16) tile rows, n <= 64: returns f(nt, prefetch), both integral constants.
// `prefetch` is false in one place, the fourth tile row of fp64 (FP64): V + F + Y alone take 448 of the 512 registers there, so that
// instantiation has no second operand set (lqr_backward_tiled_f64.hip).
template <bool FP64, typename F>
static int with_nt(const int n, F&& f) {
    if (n <= 16) return f(std::integral_constant<int, 1>{}, std::true_type{});
    if (n <= 32) return f(std::integral_constant<int, 2>{}, std::true_type{});
    if (n <= 48) return f(std::integral_constant<int, 3>{}, std::true_type{});
    return f(std::integral_constant<int, 4>{}, std::integral_constant<bool, !FP64>{});
}

}  // namespace zm
