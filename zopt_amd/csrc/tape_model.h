// ZM_MODEL_TRACED: the interpreter of a recorded dynamics function (include/zopt_amd.h: zm_traced_t; recorder: zopt_amd/tape.py).
//
// One tape serves the rollouts (S = double), the Jacobians (S = Dual) and the second derivatives (S = Hyper): the same instruction
// stream evaluated on another scalar type, as the registered models of models.h are one template evaluated three ways.
//
//   * The tape is wave-uniform: the instruction word is fetched at a uniform index and pinned to the scalar unit (tape_uniform), so
//     fetch, decode and the branch per opcode run on the scalar ALU and no lane diverges; only the operand traffic and the arithmetic
//     are vector work.
//   * The slot file is indexed at run time, so it cannot live in registers.  SLOTS is the policy:
//       LdsSlots    [slot][component][lane] in LDS: every access is one conflict-free 8-byte read or write per lane; a wave needs
//                   n_slots * components * 512 B (the launch sizes it by the model's slot count, not by the cap);
//       ArraySlots  a private array: scratch on the device (what a dynamically indexed local array becomes), and the slot file of
//                   the host build (tests/tape_shim.cpp compiles this header with g++ -ffp-contract=off).
//   * Value path: every instruction is one IEEE operation (or zm_sincos, trig.h) between a load and a store of the slot file, and
//     contraction is off in the loop: the bits do not depend on the kernel the interpreter is inlined into, and equal the host build's.
//
// The qualifiers are models.h's (`__device__ __forceinline__`); the host build defines them away, as tests/trig_shim.cpp does.
#pragma once
#include <stdint.h>

#include "models.h"

namespace zm {

enum TapeOp { TP_ADD = 0, TP_SUB = 1, TP_MUL = 2, TP_DIV = 3, TP_NEG = 4, TP_SIN = 5, TP_COS = 6, TP_TAN = 7, TP_SQRT = 8, TP_MOV = 9 };
constexpr unsigned TP_A_CONST = 0x40u, TP_B_CONST = 0x80u;

// a value every lane of the wave holds alike, moved to a scalar register (decode and branches then stay on the scalar unit)
__device__ __forceinline__ unsigned tape_uniform(const unsigned v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (unsigned)__builtin_amdgcn_readfirstlane((int)v);
#else
    return v;
#endif
}

// the descriptor of a traced model: a copy of the 40 bytes that A, B and wind_ned occupy (zm_model_t keeps its declaration, so that
// the kernels of the registered models, which take it by value, compile to what they were)
static_assert(sizeof(zm_traced_t) == 40 && sizeof(zm_model_t) == 64 && __builtin_offsetof(zm_model_t, A) == 24, "zm_traced_t overlays A, B, wind_ned");
__host__ __device__ inline zm_traced_t traced_of(const zm_model_t& md) {
    zm_traced_t t;
    __builtin_memcpy(&t, &md.A, sizeof(t));
    return t;
}

// components of a scalar type as consecutive doubles
template <typename S> struct TapeNum;
template <> struct TapeNum<double> {
    static constexpr int NC = 1;
    static __device__ __forceinline__ double lift(const double c) { return c; }
    static __device__ __forceinline__ double load(const double* p, const int st) { return p[0]; }
    static __device__ __forceinline__ void store(double* p, const int st, const double v) { p[0] = v; }
};
template <> struct TapeNum<Dual> {
    static constexpr int NC = 2;
    static __device__ __forceinline__ Dual lift(const double c) { return Dual{c, 0.0}; }
    static __device__ __forceinline__ Dual load(const double* p, const int st) { return Dual{p[0], p[st]}; }
    static __device__ __forceinline__ void store(double* p, const int st, const Dual v) { p[0] = v.v, p[st] = v.d; }
};
template <> struct TapeNum<Hyper> {
    static constexpr int NC = 4;
    static __device__ __forceinline__ Hyper lift(const double c) { return Hyper{c, 0.0, 0.0, 0.0}; }
    static __device__ __forceinline__ Hyper load(const double* p, const int st) { return Hyper{p[0], p[st], p[2 * st], p[3 * st]}; }
    static __device__ __forceinline__ void store(double* p, const int st, const Hyper v) {
        p[0] = v.v, p[st] = v.d1, p[2 * st] = v.d2, p[3 * st] = v.d12;
    }
};

// slot file in LDS: component c of slot s of this lane at col[(s * NC + c) * lanes], col = base + lane
template <typename S>
struct LdsSlots {
    double* col;
    int lanes;
    __device__ __forceinline__ S get(const int s) const { return TapeNum<S>::load(col + s * (TapeNum<S>::NC * lanes), lanes); }
    __device__ __forceinline__ void set(const int s, const S v) { TapeNum<S>::store(col + s * (TapeNum<S>::NC * lanes), lanes, v); }
    static __host__ __device__ constexpr long bytes(const int n_slots, const int lanes) {
        return (long)n_slots * TapeNum<S>::NC * lanes * (long)sizeof(double);
    }
};

// slot file in a private array
template <typename S>
struct ArraySlots {
    S v[ZM_TRACED_MAX_SLOTS];
    __device__ __forceinline__ S get(const int s) const { return v[s]; }
    __device__ __forceinline__ void set(const int s, const S x) { v[s] = x; }
};

#define ZM_TAPE_BINARY(A, B) (op == TP_ADD ? (A) + (B) : op == TP_SUB ? (A) - (B) : op == TP_MUL ? (A) * (B) : (A) / (B))

// the instruction loop; the inputs are in their slots
template <typename S, typename SLOTS>
__device__ __forceinline__ void tape_run(const uint32_t* __restrict__ code, const int n_instr, const double* __restrict__ consts,
                                         SLOTS& f) {
#pragma clang fp contract(off)
    for (int pc = 0; pc < n_instr; ++pc) {
        const unsigned w = tape_uniform(code[pc]);
        const unsigned op = w & 0x3Fu;
        constexpr int SM = ZM_TRACED_MAX_SLOTS - 1;   // slot numbers stay inside the file whatever the word says
        const int dst = (int)((w >> 8) & SM), ia = (int)((w >> 16) & 0xFFu), ib = (int)(w >> 24);
        S r;
        if (op <= TP_DIV) {
            if (w & TP_A_CONST) {           // (both constants: folded by the recorder)
                const double a = consts[ia];
                const S b = f.get(ib & SM);
                r = ZM_TAPE_BINARY(a, b);
            } else if (w & TP_B_CONST) {
                const S a = f.get(ia & SM);
                const double b = consts[ib];
                r = ZM_TAPE_BINARY(a, b);
            } else {
                const S a = f.get(ia & SM), b = f.get(ib & SM);
                r = ZM_TAPE_BINARY(a, b);
            }
        } else {
            const S a = (w & TP_A_CONST) ? TapeNum<S>::lift(consts[ia]) : f.get(ia & SM);
            switch (op) {
                case TP_NEG: r = -a; break;
                case TP_SIN: r = zsin(a); break;
                case TP_COS: r = zcos(a); break;
                case TP_TAN: r = ztan(a); break;
                case TP_SQRT: r = zsqrt(a); break;
                default: r = a; break;      // TP_MOV
            }
        }
        f.set(dst, r);
    }
}
#undef ZM_TAPE_BINARY

// One step x+ = f(x, u, p) of a traced model on the slot file `f`: prow = the parameter row of this trajectory (nullptr without
// parameters).  Components n .. MAXN-1 of xn are zero, as model_step leaves them.
template <typename S, typename SLOTS>
__device__ __forceinline__ void tape_step(const zm_model_t& md, SLOTS& f, const S (&x)[MAXN], const S (&u)[MAXM],
                                          const double* __restrict__ prow, S (&xn)[MAXN]) {
    const zm_traced_t t = traced_of(md);
    const double* consts = (const double*)t.tape;
    const uint32_t* code = (const uint32_t*)(consts + t.n_const);
    const uint32_t* outs = code + t.n_instr;
    const int n = md.n, m = md.m;
#pragma unroll
    for (int i = 0; i < MAXN; ++i)
        if (i < n) f.set(i, x[i]);
#pragma unroll
    for (int j = 0; j < MAXM; ++j)
        if (j < m) f.set(n + j, u[j]);
    for (int q = 0; q < t.n_params; ++q) f.set(n + m + q, TapeNum<S>::lift(prow[q]));
    tape_run<S, SLOTS>(code, t.n_instr, consts, f);
#pragma unroll
    for (int i = 0; i < MAXN; ++i) xn[i] = (i < n) ? f.get((int)tape_uniform(outs[i])) : TapeNum<S>::lift(0.0);
}

}  // namespace zm
