// Shared host-side helpers for the zopt_amd C ABI (error reporting, argument checks).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>

#include "../../include/zopt_amd.h"

namespace zm {

// Run-time switches.  A PRODUCT build reads exactly four environment variables, each selecting a FALLBACK kernel -- the one that
// also serves the shapes / alignments its fast path refuses, so it is product code either way:
//     ZOPT_AMD_LQR_PATH=lds|reg   ZOPT_AMD_ILQR_PATH=reg   ZOPT_AMD_ROLLOUT_PATH=generic   ZOPT_AMD_MPC_PATH=lane
// Every other ZOPT_AMD_* variable is an A/B switch of the kernel lab (ring depth, packed / full operands, tail thresholds, ...):
// it exists only in a -DZM_LAB build (`make lab` -> libzopt_amd_lab.so, loaded through ZOPT_AMD_LIB by the A/B tests and the lab
// tools); in the product library lab_env() is the constant nullptr and the compiler removes the branch it guards.
inline const char* fallback_env(const char* name) { return getenv(name); }
inline const char* lab_env(const char* name) {
#ifdef ZM_LAB
    return getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}

// Thread-local last-error buffer behind zm_last_error().
char* last_error_buf();
int set_error(int code, const char* fmt, ...);

// A registered model as the kernels take it: *md <- *model with (n, m) of its kind (a quadcopter's are fixed: (12, 4), rigid body
// (8, 4); a linear model's are its own, and it needs A and B; a traced model's are its own, and its descriptor is checked against the
// interpreter's caps).  An unknown kind is refused.  `who`: the entry the message names.
inline zm_model_t model_sized(zm_model_t md) {
    if (md.kind == ZM_MODEL_QUADCOPTER) md.n = 12, md.m = 4;
    if (md.kind == ZM_MODEL_QUADCOPTER_RB) md.n = 8, md.m = 4;
    return md;
}
int traced_check(const zm_model_t* model, const char* who);   // traced.hip: counts, pointers and mask of a ZM_MODEL_TRACED descriptor
inline int model_check(const zm_model_t* model, const char* who, zm_model_t* md) {
    *md = model_sized(*model);
    if (md->kind == ZM_MODEL_LINEAR) {
        if (!md->A || !md->B) return set_error(ZM_EINVAL, "%s: linear model needs A, B", who);
    } else if (md->kind == ZM_MODEL_TRACED) {
        return traced_check(md, who);
    } else if (md->kind != ZM_MODEL_QUADCOPTER && md->kind != ZM_MODEL_QUADCOPTER_RB) {
        return set_error(ZM_EUNSUPPORTED, "%s: unknown model kind %d", who, md->kind);
    }
    return ZM_OK;
}

// The sizes of a backward sweep, checked after "nothing to do" and the operands: who has T steps of an n x n matrix per trajectory and
// covers n <= n_max, m <= m_max.
inline int check_sweep_args(const char* who, int64_t batch, int T, int n, int m, int n_max, int m_max) {
    if (batch < 0 || T < 1 || n < 1 || m < 1)
        return set_error(ZM_EINVAL, "%s: bad size batch=%lld T=%d n=%d m=%d", who, (long long)batch, T, n, m);
    if (n > n_max || m > m_max)
        return set_error(ZM_EUNSUPPORTED, "%s: (n=%d, m=%d) not covered (need n<=%d, m<=%d)", who, n, m, n_max, m_max);
    if ((int64_t)T * n * n >= (int64_t)1 << 31 || batch >= ((int64_t)1 << 31))
        return set_error(ZM_EUNSUPPORTED, "%s: T*n*n or batch too large", who);
    return ZM_OK;
}

// What the one-design-per-wave entries (DARE, CARE, Riccati ODE) check alike, in this order: the operands (`operands`: the entry's own
// "all given"), the entry's own arguments (`arguments`: its own "all in range"), the shape.  The bound on the batch comes after it:
// the ODE's covers its sample counts too and reads differently, so each entry keeps that line.
inline int check_design_args(const char* who, bool operands, bool arguments, int n, int m, int n_max, int m_max) {
    if (!operands) return set_error(ZM_EINVAL, "%s: null pointer", who);
    if (!arguments) return set_error(ZM_EINVAL, "%s: bad argument", who);
    if (n > n_max || m > m_max)
        return set_error(ZM_EUNSUPPORTED, "%s: (n=%d, m=%d) not covered (need n<=%d, m<=%d)", who, n, m, n_max, m_max);
    return ZM_OK;
}

#define ZM_HIP_CHECK(expr)                                                              \
    do {                                                                                \
        hipError_t _e = (expr);                                                         \
        if (_e != hipSuccess)                                                           \
            return zm::set_error((int)_e, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)


// Ordering of an LDS write against a later LDS read of the same bytes by ANOTHER LANE OF THE SAME WAVE (one-wave workgroups).
// The hardware runs a wave's DS instructions in issue order, so only the compiler must keep the program order of the two
// memory operations: a compiler-level memory barrier -- register-only instructions (MFMA, VALU) may be scheduled
// across it.  Measured against wavefront-scope fences around a wave barrier, which is also a scheduling barrier for everything: K1 on
// resident data 112 -> 106 us, outputs bit for bit the same (profiles/r02_k1_lab12.txt).
__device__ __forceinline__ void wave_lds_sync() {
    asm volatile("" ::: "memory");
}

// 32-bit halves of a double through one DPP move each (VALU speed; __shfl_xor is two ds_bpermute round trips through the LDS crossbar
// per level).  mov_dpp with bound_ctrl: every lane of these in-row permutations has a valid source, so the destination needs no
// initial value.
template <int CTRL>
__device__ __forceinline__ double dpp_mov64(const double v) {
    const long long b = __builtin_bit_cast(long long, v);
    const int lo = __builtin_amdgcn_mov_dpp((int)b, CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_mov_dpp((int)(b >> 32), CTRL, 0xf, 0xf, true);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
}
// Sum / maximum over the 16 lanes of a row, the result in every lane of the row: butterflies by quad_perm (xor 1, xor 2),
// row_half_mirror and row_mirror.  The same bits as the __shfl_xor butterfly over offsets 1, 2, 4, 8: after the quad steps every lane of
// a quad holds the quad's value, so the mirrored partner of a step holds exactly what the xor partner holds, and + / max commute.
__device__ __forceinline__ double row16_sum(double v) {
    v += dpp_mov64<0xB1>(v);
    v += dpp_mov64<0x4E>(v);
    v += dpp_mov64<0x141>(v);
    v += dpp_mov64<0x140>(v);
    return v;
}
// The same sum in the order of a ladder that starts at offset 8: row_ror:8 is lane ^ 8 on 16 lanes; after it the values repeat with
// period 8, so row_ror:4 delivers what lane ^ 4 holds; then the quad steps.  Bits of `for (off = 8; off >= 1; off >>= 1) v += shfl_xor`.
__device__ __forceinline__ double row16_sum_from8(double v) {
    v += dpp_mov64<0x128>(v);
    v += dpp_mov64<0x124>(v);
    v += dpp_mov64<0x4E>(v);
    v += dpp_mov64<0xB1>(v);
    return v;
}
__device__ __forceinline__ double row16_max(double v) {
    v = __builtin_fmax(v, dpp_mov64<0xB1>(v));
    v = __builtin_fmax(v, dpp_mov64<0x4E>(v));
    v = __builtin_fmax(v, dpp_mov64<0x141>(v));
    v = __builtin_fmax(v, dpp_mov64<0x140>(v));
    return v;
}

// v + (the value of lane ^ 16) resp. lane ^ 32, by the gfx950 row / half-wave swaps (VALU; __shfl_xor across rows is a ds_bpermute
// round trip through LDS on the dependency chain).  permlane16_swap(a, b): odd rows of a <-> even rows of b; with a = b = v the two
// results hold the even-row resp. odd-row partner values of every row pair, whose sum is the butterfly sum in both rows (fp addition
// commutes: the same bits as v + __shfl_xor(v, 16)).  permlane32_swap likewise for the two half waves.
__device__ __forceinline__ double sum_xor16(const double v) {
    const long long b = __builtin_bit_cast(long long, v);
    const auto lo = __builtin_amdgcn_permlane16_swap((unsigned)b, (unsigned)b, false, false);
    const auto hi = __builtin_amdgcn_permlane16_swap((unsigned)(b >> 32), (unsigned)(b >> 32), false, false);
    const double x = __builtin_bit_cast(double, ((unsigned long long)hi[0] << 32) | (unsigned long long)lo[0]);
    const double y = __builtin_bit_cast(double, ((unsigned long long)hi[1] << 32) | (unsigned long long)lo[1]);
    return x + y;
}
__device__ __forceinline__ double sum_xor32(const double v) {
    const long long b = __builtin_bit_cast(long long, v);
    const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)b, (unsigned)b, false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)(b >> 32), (unsigned)(b >> 32), false, false);
    const double x = __builtin_bit_cast(double, ((unsigned long long)hi[0] << 32) | (unsigned long long)lo[0]);
    const double y = __builtin_bit_cast(double, ((unsigned long long)hi[1] << 32) | (unsigned long long)lo[1]);
    return x + y;
}

// The line search's argmin over a group of W lanes (lane ids STRIDE apart) with jnp.argmin semantics: a NaN key beats every number
// (also -inf), the first index wins among equals.  A lane brings its cost and its index; a dead lane brings +inf, and an index past
// the live ones where a live +inf must beat it.  Every lane of the group returns the winner's index.
// (The operands come by reference: by value, the scratch of one rollout_ls_fast_kernel instantiation grew from 28 to 36 bytes.)
template <int W, int STRIDE = 1>
__device__ __forceinline__ int argmin_nan_first(const double& cost, const int& index) {
    double key = cost;
    int isn = (key != key) ? 1 : 0, who = index;
#pragma unroll
    for (int off = W * STRIDE / 2; off >= STRIDE; off >>= 1) {
        const double ok = __shfl_xor(key, off);
        const int on = __shfl_xor(isn, off);
        const int ow = __shfl_xor(who, off);
        const bool better = (on > isn) || (on == isn && ((on == 0 && ok < key) || ((on == 1 || ok == key) && ow < who)));
        key = better ? ok : key;
        isn = better ? on : isn;
        who = better ? ow : who;
    }
    return who;
}

}  // namespace zm
