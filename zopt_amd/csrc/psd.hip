// K5  psd_project -- batched PD projection of symmetric matrices (the eigenvalue clamp of an eigen-decomposition); fp64, gfx950.
//
// Replaces zopt/ilqrUtils.py:217-219 ensurePositiveDefinite(a, eps):  w, v = eigh(a);  (v * max(w, eps)) @ v.T
// (jnp.linalg.eigh symmetrises its input: (a + a^T)/2) and its users conditionQuadraticCost (:222-234) and
// conditionValueFunction (:254-257).  The result is a spectral function of the matrix, so it does not depend on
// the eigenvector signs / ordering an eigensolver happens to return.
//
// One wave64 per matrix (k <= 16): the k x k matrix sits zero-padded in one 16 x 16 MFMA tile and is projected there without an
// eigen-decomposition, by the matrix-sign iteration of ns16.h (V max(w, eps) V^T = eps I + (X + |X|) / 2 with X = a - eps I).
// 16 < k <= 64: psd_tiled.hip.
#include "ns16.h"
#include "psd_mats.h"
#include "zm_common.h"

namespace zm {

// lane (g, c) holds rows 4r+g of column c of the tile; the projection is ~100-200 fp64 MFMAs (the cyclic Jacobi through LDS it
// replaced took ~10 sweeps and was bound by LDS bandwidth: DESIGN 2.5)
template <class Mat, int KSZ>
__device__ __forceinline__ void psd_project_tile(const Mat& M, const long mat, const int k, const double eps, double* T) {
    const int lane = threadIdx.x, g = lane >> 4, c = lane & 15;
    d4 a;
    bool live[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = 4 * r + g;
        const bool in = (i < k) && (c < k);
        a[r] = in ? M.load(mat, in ? i : 0, in ? c : 0) : 0.0;
        live[r] = in && (i == c);
    }
    psd_project_ns<KSZ>(a, live, eps, T, g, c);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = 4 * r + g;
        if (i < k && c < k) M.store(mat, i, c, a[r]);
    }
}

template <class Mat>
__global__ __launch_bounds__(64) void psd_project_kernel(const Mat M, const int k, const double eps, const long count) {
    __shared__ double T[NS_LDS_DOUBLES];
    const long mat = blockIdx.x;
    if (mat >= count) return;
    if (k <= 4) psd_project_tile<Mat, 1>(M, mat, k, eps, T);
    else if (k <= 8) psd_project_tile<Mat, 2>(M, mat, k, eps, T);
    else if (k <= 12) psd_project_tile<Mat, 3>(M, mat, k, eps, T);
    else psd_project_tile<Mat, 4>(M, mat, k, eps, T);
}

// psd_tiled.hip: the same projection on NT x NT tiles for 16 < k <= 64
int psd_project_tiled_plain(double* A, int64_t count, int k, double eps, hipStream_t st);
int psd_project_tiled_cost(double* c_xx, double* c_ux, double* c_uu, int64_t count, int n, int m, double eps, hipStream_t st);

// The launches of zm_condition_cost_f64 / zm_psd_project_f64 with the matrix index mapped through the id list of a solve: the stacked
// Hessians of the T points of each listed trajectory (c_xx (batch,T,n,n), c_ux (batch,T,m,n), c_uu (batch,T,m,m)), resp. its one
// terminal Hessian (A (batch,k,k)).  One tile: n + m <= 16, k <= 16 (the caller's shapes: n <= 12, m <= 4).
int condition_cost_listed(double* c_xx, double* c_ux, double* c_uu, const int* list, long count, int T, int n, int m, double eps,
                          hipStream_t st) {
    if (count == 0) return ZM_OK;
    if (!c_xx || !c_ux || !c_uu || !list) return set_error(ZM_EINVAL, "condition_cost_listed: null pointer");
    if (count < 0 || T < 1 || n < 1 || m < 1 || n + m > PK || count * T >= (1L << 31)) return set_error(ZM_EINVAL, "condition_cost_listed: bad size");
    hipLaunchKernelGGL((psd_project_kernel<Listed<StackedCost>>), dim3((unsigned)(count * T)), dim3(64), 0, st,
                       Listed<StackedCost>{StackedCost{c_xx, c_ux, c_uu, n, m}, list, T}, n + m, eps, count * T);
    ZM_HIP_CHECK(hipGetLastError());
    return ZM_OK;
}
int psd_project_listed(double* A, const int* list, long count, int k, double eps, hipStream_t st) {
    if (count == 0) return ZM_OK;
    if (!A || !list) return set_error(ZM_EINVAL, "psd_project_listed: null pointer");
    if (count < 0 || k < 1 || k > PK || count >= (1L << 31)) return set_error(ZM_EINVAL, "psd_project_listed: bad size");
    hipLaunchKernelGGL((psd_project_kernel<Listed<PlainMat>>), dim3((unsigned)count), dim3(64), 0, st,
                       Listed<PlainMat>{PlainMat{A, k}, list, 1}, k, eps, count);
    ZM_HIP_CHECK(hipGetLastError());
    return ZM_OK;
}

}  // namespace zm

extern "C" int zm_psd_project_f64(double* A, int64_t count, int k, double eps, void* stream) {
    if (count == 0) return ZM_OK;   /* empty batch: nothing to do (pointers of empty arrays may be NULL) */
    if (!A) return zm::set_error(ZM_EINVAL, "zm_psd_project_f64: null pointer");
    if (count < 0 || k < 1) return zm::set_error(ZM_EINVAL, "zm_psd_project_f64: bad size");
    if (k > 64) return zm::set_error(ZM_EUNSUPPORTED, "zm_psd_project_f64: k=%d > 64", k);
    if (k > zm::PK) return zm::psd_project_tiled_plain(A, count, k, eps, (hipStream_t)stream);
    hipLaunchKernelGGL((zm::psd_project_kernel<zm::PlainMat>), dim3((unsigned)count), dim3(64), 0, (hipStream_t)stream,
                       zm::PlainMat{A, k}, k, eps, (long)count);
    ZM_HIP_CHECK(hipGetLastError());
    return ZM_OK;
}

extern "C" int zm_condition_cost_f64(double* c_xx, double* c_ux, double* c_uu, int64_t count, int n, int m, double eps,
                                     void* stream) {
    if (count == 0) return ZM_OK;   /* empty batch: nothing to do (pointers of empty arrays may be NULL) */
    if (!c_xx || !c_ux || !c_uu) return zm::set_error(ZM_EINVAL, "zm_condition_cost_f64: null pointer");
    if (count < 0 || n < 1 || m < 1) return zm::set_error(ZM_EINVAL, "zm_condition_cost_f64: bad size");
    if (n + m > 64) return zm::set_error(ZM_EUNSUPPORTED, "zm_condition_cost_f64: n+m=%d > 64", n + m);
    if (n + m > zm::PK) return zm::psd_project_tiled_cost(c_xx, c_ux, c_uu, count, n, m, eps, (hipStream_t)stream);
    hipLaunchKernelGGL((zm::psd_project_kernel<zm::StackedCost>), dim3((unsigned)count), dim3(64), 0, (hipStream_t)stream,
                       zm::StackedCost{c_xx, c_ux, c_uu, n, m}, n + m, eps, (long)count);
    ZM_HIP_CHECK(hipGetLastError());
    return ZM_OK;
}

extern "C" int zm_condition_dynamics_f64(const double* f_xx, const double* f_ux, const double* f_uu, const double* v_x,
                                         double* vf_xx, double* vf_ux, double* vf_uu, int64_t count, int n, int m, double eps,
                                         void* stream) {
    if (count == 0) return ZM_OK;   /* empty batch: nothing to do (pointers of empty arrays may be NULL) */
    if (!f_xx || !f_ux || !f_uu || !v_x || !vf_xx || !vf_ux || !vf_uu)
        return zm::set_error(ZM_EINVAL, "zm_condition_dynamics_f64: null pointer");
    if (count < 0 || n < 1 || m < 1) return zm::set_error(ZM_EINVAL, "zm_condition_dynamics_f64: bad size");
    if (n + m > zm::PK) return zm::set_error(ZM_EUNSUPPORTED, "zm_condition_dynamics_f64: n+m=%d > 16", n + m);
    hipLaunchKernelGGL((zm::psd_project_kernel<zm::ContractedDynamics>), dim3((unsigned)count), dim3(64), 0, (hipStream_t)stream,
                       zm::ContractedDynamics{f_xx, f_ux, f_uu, v_x, vf_xx, vf_ux, vf_uu, n, m}, n + m, eps, (long)count);
    ZM_HIP_CHECK(hipGetLastError());
    return ZM_OK;
}
