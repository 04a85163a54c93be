// K3  ilqr_backward -- batched iLQR backward pass (affine policy from a quadratic value sweep), fp64, gfx950.
//
// Replaces the arithmetic of zopt/ilqrUtils.py:153-181 (riccatiStep_ilqr / backwardPass_ilqr), per trajectory,
// for k = T-1 .. 0 with carry (v_x, v_xx) <- Vf:
//     Q_x  = c_x  + f_x^T v_x                 Q_u  = c_u  + f_u^T v_x                              (:161-162)
//     Q_xx = c_xx + f_x^T v_xx f_x   Q_uu = c_uu + f_u^T v_xx f_u   Q_ux = c_ux + f_u^T v_xx f_x    (:163-165)
//     l = -solve(Q_uu, Q_u)          L = -solve(Q_uu, Q_ux)                                        (:167-168)
//     v_x' = Q_x - L^T Q_uu l        v_xx' = Q_xx - L^T Q_uu L                                     (:170)
// The scalar part (c, v) never influences l or L and backwardPass_ilqr returns only the policy, so it is not
// carried.  `Q_uu l` is taken as -Q_u (its value by construction of l); the difference is the residual of the
// m x m solve (rounding level).
//
// Tile-16 mapping (tile16_f64.h): one wave64 per trajectory, F = [f_x | f_u] as a 16-column tile,
//     Y = v_xx^T F (KS MFMA),  G = Y^T F + [[c_xx, .],[c_ux, c_uu]] (KS MFMA)  ->  Q_xx (rows < NP), [Q_ux | Q_uu] (row NP+g)
//     q = [c_x ; c_u] + F^T v_x : 3 FMAs per lane + a 4-group xor reduction (column-indexed, replicated over g)
//     solve: the 4 x 16 tile [Q_ux | Q_uu] and the row q through LDS; lane c < n solves column c of Q_ux,
//            lane c == NP solves Q_u.  -x[g] is L_k[g][c] resp. l_k[g].
//     T1 = Q_uu L (1 MFMA),  v_xx' = Q_xx - L^T T1 (1 MFMA, negated A operand)
// 2*KS + 2 MFMAs per step.  Inputs are read once with 8-byte loads straight into their register layouts, two steps
// ahead (register double buffer).  Shapes: n <= 12, m <= 4.
//
// MODE 2 = K4 ddp_backward: zopt/ilqrUtils.py:184-214 (riccatiStep_ddp / backwardPass_ddp) = MODE 0 plus, per step,
//     vf_zz = [[vf_xx, vf_ux^T],[vf_ux, vf_uu]],  vf_.. = einsum('i,ijk', v_x, f_..)                  (:240-247)
//     vf_zz <- ensurePositiveDefinite(vf_zz)   (eigenvalue clamp 1e-3, INSIDE the sequential sweep)    (:248)
//     Q_xx += vf_xx,  Q_uu += vf_uu,  Q_ux += vf_ux                                                    (:196-198)
// The contraction reads f_xx (n,n,n), f_ux (n,m,n), f_uu (n,m,m) of the step straight from HBM (n terms per tile
// element); the (n+m) x (n+m) matrix stays on the tile, zero-padded, is PD-projected there by the matrix-sign iteration of
// ns16.h and becomes an accumulator init of G.
//
// MODE 1 = K2 lqr_backward_affine: the same sweep for zopt/lqrUtils.py:207-262 (bilinearAffineLqr), i.e. with
//     f_x,f_u <- A,B   c_xx,c_ux,c_uu <- Q,H,R   c_x,c_u <- q,r   and the affine-dynamics offset d:
//     Su  = r + B^T (v + V^T d)      Suu = R + B^T V B      Sux = H + B^T V A                       (:244-246)
//     L = solve(Suu, Sux)   l = solve(Suu, Su)       (no sign flip; law u = -L x - l)                (:248-249)
//     V' = Q + A^T V A - L^T Suu L      v' = q + A^T (v + V d) - Sux^T l                             (:251-252)
// (v0 / q0 never influence L or l and are not carried.)  V d is a row reduction of the V registers (4 xor-shuffles per
// K-step), V^T d a column reduction (2 shuffles) re-laid out through LDS; both are kept apart so that a
// nonsymmetric V is treated exactly as the reference does.
//
// BOX (MODE 0 and MODE 2; an extension, the reference has no counterpart) = the backward pass of control-limited DDP for bounds lb <= u <= ub
// on the inputs (Tassa, Mansard, Todorov 2014): per step, with u_k the current trajectory's input,
//     l = argmin_d 1/2 d^T sym(Q_uu) d + Q_u^T d   over   lb - u_k <= d <= ub - u_k          (boxqp4.h, wave-uniform on registers)
//     C = the components at a bound with a multiplier of the right sign, F the rest:  L[C,:] = 0,  L[F,:] = -Q_uu[F,F]^-1 Q_ux[F,:]
//     v_x' = Q_x + Q_ux^T l        v_xx' = Q_xx - L^T Q_uu L
#include "boxqp4.h"
#include "dma_ring.h"
#include "lqr_dispatch.h"
#include "models.h"
#include "ns16.h"
#include "tile16_f64.h"
#include "zm_common.h"

#include <type_traits>

namespace zm {

template <int KS>
struct IlqrStepRegs {
    double F[KS];   // [f_x | f_u][4s+g][c]
    double C[KS];   // c_xx[4s+g][c]
    double Cu;      // row NP+g of the stacked cost Hessian: c_ux[g][c] (c < n) | c_uu[g][c-NP] | identity padding
    double cv;      // [c_x ; c_u][c]  (column-indexed)
    double dc;      // MODE 1: d[c]       (column-indexed)
    double dr[KS];  // MODE 1: d[4s+g]    (row-indexed)
    double hd;      // PEN: h_k[c] on the lanes of the Hessian's diagonal (row == c), 0 elsewhere
};

// optional compacted list of trajectory ids: block b works on list[b] (grid = count) instead of on trajectory b (grid = batch)
struct TrajList {
    const int* list;
    long count;
};

template <int KS>
struct IlqrAddr {
    const double* pF0;   // K-step s adds (rowok ? s*dF : 0)
    const double* pC0;   // K-step s adds (rowok ? s*4n : 0)
    const double* pCu;
    const double* pcv;
    const double* pdc;   // MODE 1
    const double* pdr0;  // MODE 1: K-step s adds (rowok ? 4 s : 0)
    const double* pz[4]; // MODE 2: element (4r+g, c) of the stacked second-derivative tensor slice i = 0; +i*sz[r]
    int sz[4], stz[4];   // MODE 2: stride over i, stride over the time step
    int zc[4];           // MODE 2: >= 0 where tile element (4r+g, c) belongs to the (n+m) x (n+m) matrix, -1 on padding
    bool zlive[4];       // MODE 2: tile element (4r+g, c) is a diagonal entry of the live (state, control) index set
    double* pOut;        // L_k[g][c] (c < n) or l_k[g] (c == NP)
    int dF, dC, sF, sC, sCu, scv, sOut, sd;
    bool rowok[KS], vF[KS], vC[KS], vCu, vcv, vOut, vL, cA;
    double vsum = 0.0;     // MODE 0/2, lanes c == NP: sum over the steps of -1/2 l^T Q_uu l  (scalar part of the value function)
    double cu_pad;
};

// PEN: what a step of a sweep with a state-box penalty (ilqr_backward_pen_t16_f64, ilqr_backward_box_pen_t16_f64) carries besides the
// operands: the diagonal addend h_k (batch, T+1, n) of the step's cost Hessian, one double per lane of the tile's diagonal
struct PenStep {
    const double* ph;   // the lane's entry of h_k (element 0 of the row off the diagonal), walks back by sh
    int sh;
    int hs;             // the K-step s whose tile element (4s+g, c) is the diagonal one; -1 off the diagonal
    bool hv;
};

template <int KS, int MODE, bool PEN = false>
__device__ __forceinline__ void ilqr_load_step(IlqrStepRegs<KS>& d, IlqrAddr<KS>& a, PenStep* pn = nullptr) {
    double f[KS], cc[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) f[s] = a.pF0[a.rowok[s] ? s * a.dF : 0];
    a.pF0 -= a.sF;
#pragma unroll
    for (int s = 0; s < KS; ++s) cc[s] = a.pC0[a.rowok[s] ? s * a.dC : 0];
    a.pC0 -= a.sC;
    const double cu = *a.pCu;
    a.pCu -= a.sCu;
    const double cv = *a.pcv;
    a.pcv -= a.scv;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        d.F[s] = a.vF[s] ? f[s] : 0.0;
        d.C[s] = a.vC[s] ? cc[s] : 0.0;
    }
    d.Cu = a.vCu ? cu : a.cu_pad;
    d.cv = a.vcv ? cv : 0.0;
    if constexpr (PEN) {
        const double hh = *pn->ph;
        pn->ph -= pn->sh;
        d.hd = pn->hv ? hh : 0.0;
    }
    if constexpr (MODE == 1) {
        const double dc = *a.pdc;
        double dr[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) dr[s] = a.pdr0[a.rowok[s] ? 4 * s : 0];
        a.pdc -= a.sd;
        a.pdr0 -= a.sd;
        d.dc = a.cA ? dc : 0.0;
#pragma unroll
        for (int s = 0; s < KS; ++s) d.dr[s] = a.rowok[s] ? dr[s] : 0.0;
    }
}

// LDS per wave (doubles): [0,64) tile rows 0..3 = [Q_ux | Q_uu]; [64,80) row 4 = q; [80,96) v_x' (column-indexed)
//                       MODE 1: [96,112) V^T d (column-indexed); [112,116) l
constexpr int ILQR_LDS_DOUBLES = 116;

// Diagnostic build (-DZM_SWEEP_LAB): s_memtime stamps at the phase boundaries of a step of the ring kernel, summed by wave 0 of block 0
// into zm_sweep_stamps (read back with zm_lab_sweep_stamps).  The stamps' waits forbid overlaps the product has: read SHARES.
#ifdef ZM_SWEEP_LAB
__device__ unsigned long long zm_sweep_stamps[10];
struct SweepLab {
    unsigned long long acc[8], last;
};
#define ZM_SWEEP_STAMP(lab, q)                                                                         \
    do {                                                                                              \
        unsigned long long t_;                                                                        \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                    \
        (lab)->acc[q] += t_ - (lab)->last;                                                            \
        (lab)->last = t_;                                                                             \
    } while (0)
#else
struct SweepLab {};
#define ZM_SWEEP_STAMP(lab, q) do { } while (0)
#endif

__device__ __forceinline__ void ilqr_lds_sync() { wave_lds_sync(); }

// BOX: what a step of a box-constrained sweep (ilqr_backward_box_t16_f64, ddp_backward_box_t16_f64) carries besides the operands
struct BoxStep {
    const double* pu;      // u_k of the step (the current trajectory's input), walks back by m
    double lb[4], ub[4];   // the trajectory's bounds; -inf / +inf beyond m
    int capped;            // steps of this trajectory whose QP ended at its pass cap
    // STG (stage-varying bounds): lb / ub above are not held; row k of the trajectory's schedule is read with u_k
    const double* plb;     // lb_k, ub_k of the step, walk back by m
    const double* pub;
};

// ZIN (MODE 2, the DMA kernel): the caller has contracted vf_zz = sum_i v_x[i] d2f_i/dz2 already (operands in its LDS ring) and
// passes the tile in `zin`
// BOX (MODE 0 and 2): l_k is the minimiser of the step's QP over lb - u_k <= d <= ub - u_k (boxqp4.h), the rows of L_k of its clamped
// components are zero, the others solve the system whose clamped rows and columns are the identity's; v_x' = Q_x + Q_ux^T l_k.
// In MODE 2 Q_xx, Q_ux, Q_uu carry the projected vf_zz blocks; nothing else differs.
// PEN (MODE 0): the step's cost Hessian is c_xx + diag h_k, formed before anything is accumulated onto it.
// STG (with BOX): the bounds are those of the step, lo = lb_k - u_k, hi = ub_k - u_k: row k is fetched with u_k at the head of the step
// (every lane the same row) and is in flight under the same products; nothing of the bounds is held across steps.
template <int KS, int MODE, bool PREFETCH, bool ZIN = false, bool BOX = false, bool PEN = false, bool STG = false>
__device__ __forceinline__ void ilqr_step(double (&Vxx)[KS], double (&vxr)[KS], IlqrStepRegs<KS>& d, IlqrAddr<KS>& a,
                                          double* sm, const int g, const int c, const int ob0, const int ob1,
                                          const int ob2, const int ob3, const int oqa, double* jA, const int n,
                                          const int m, const d4 zin = d4{0.0, 0.0, 0.0, 0.0}, SweepLab* lab = nullptr,
                                          BoxStep* bx = nullptr, PenStep* pn = nullptr) {
    constexpr int NP = 4 * KS;
    static_assert(!BOX || MODE != 1, "the box-constrained step is the iLQR or the DDP one");
    static_assert(!STG || (BOX && !PEN), "stage-varying bounds: the box step without a state-box penalty");
    double uk[4] = {0.0, 0.0, 0.0, 0.0};
    double lbk[STG ? 4 : 1], ubk[STG ? 4 : 1];
    if constexpr (BOX) {   // in flight under the products of G (MODE 2: and under the projection); every lane reads the same row
#pragma unroll
        for (int i = 0; i < 4; ++i) uk[i] = bx->pu[i < m ? i : 0];
        bx->pu -= m;
    }
    if constexpr (STG) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            lbk[i] = bx->plb[i < m ? i : 0];
            ubk[i] = bx->pub[i < m ? i : 0];
        }
        bx->plb -= m;
        bx->pub -= m;
    }
    // MODE 2: vf_zz = sum_i v_x[i] * d2f_i/dz2, PD-projected, as extra accumulator init
    d4 pz = zero4();
    if constexpr (MODE == 2 && ZIN) {
        d4 zt = zin;
        psd_project_ns<KS + 1, true>(zt, a.zlive, 1e-3, jA, g, c);   // (the ring kernel's contraction is bitwise symmetric)
        pz = zt;
    } else if constexpr (MODE == 2) {
        double z[4] = {0.0, 0.0, 0.0, 0.0};
        // the loads of 4 slices (16 per lane) are in flight before their FMAs (unrolled, unconditional: slices i >= n
        // re-read slice 0 with weight 0); more in flight would cost the second wave per SIMD its registers
#pragma unroll
        for (int i0 = 0; i0 < NP; i0 += 4) {
            double fz[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int ic = (i0 + i) < n ? (i0 + i) : 0;
#pragma unroll
                for (int r = 0; r < 4; ++r) fz[i][r] = a.pz[r][(long)ic * a.sz[r]];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const double vxi = (i0 + i) < n ? sm[80 + i0 + i] : 0.0;
#pragma unroll
                for (int r = 0; r < 4; ++r) z[r] = __builtin_fma(vxi, fz[i][r], z[r]);
            }
        }
        // PD projection on the tile itself by matrix-sign iterations on the fp64 MFMA pipe (ns16.h); jA: transpose buffers
        d4 zt;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            a.pz[r] -= a.stz[r];
            zt[r] = (a.zc[r] >= 0) ? z[r] : 0.0;   // padding lanes contracted don't-care data
        }
        psd_project_ns<KS + 1>(zt, a.zlive, 1e-3, jA, g, c);
        pz = zt;
    }
    // Y = v_xx^T F
    d4 y = zero4();
#pragma unroll
    for (int s = 0; s < KS; ++s) y = mfma(Vxx[s], d.F[s], y);
    // G = Y^T F + C0
    d4 gacc = zero4();
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        if constexpr (PEN) gacc[s] = ((pn->hs == s) ? d.C[s] + d.hd : d.C[s]) + pz[s];
        else gacc[s] = d.C[s] + pz[s];
    }
    gacc[KS] = d.Cu + pz[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) gacc = mfma(y[s], d.F[s], gacc);
    // q[c] = cv[c] + sum_k F[k][c] w[k]   (partial over this lane's rows, then over the 4 lane groups);
    // MODE 0: w = v_x.  MODE 1: w = v + V d under the state columns (A^T (v + V d), :252) and v + V^T d under the
    // control columns (v^T B + d^T V B, :244).
    double qp = 0.0;
    if constexpr (MODE == 1) {
        double vtd = 0.0;  // (V^T d)[c]: column reduction
#pragma unroll
        for (int s = 0; s < KS; ++s) vtd = __builtin_fma(Vxx[s], d.dr[s], vtd);
        vtd = sum_xor16(vtd);
        vtd = sum_xor32(vtd);
        if (g == 0) sm[96 + c] = a.cA ? vtd : 0.0;
        ilqr_lds_sync();
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            double vd = Vxx[s] * d.dc;  // (V d)[4s+g]: row reduction over the 16 lanes of the group
            vd = row16_sum(vd);   // (DPP butterflies: the bits of the __shfl_xor ladder over 1, 2, 4, 8 without its eight ds_bpermute)
            const double w = vxr[s] + (a.cA ? vd : sm[96 + 4 * s + g]);
            qp = __builtin_fma(d.F[s], w, qp);
        }
    } else {
#pragma unroll
        for (int s = 0; s < KS; ++s) qp = __builtin_fma(d.F[s], vxr[s], qp);
    }
    qp = sum_xor16(qp);     // over the four lane groups: gfx950 row / half-wave swaps instead of two ds_bpermute round trips
    qp = sum_xor32(qp);
    const double qv = d.cv + qp;
    if constexpr (PREFETCH) ilqr_load_step<KS, MODE, PEN>(d, a, pn);

    ZM_SWEEP_STAMP(lab, 2);   // projection (MODE 2), the six MFMAs of G, the vector terms
    // solve: tile + q row through LDS
    sm[g * 16 + c] = gacc[KS];
    if (g == 0) sm[64 + c] = qv;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    double S[4][4], b[4], x[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) S[i][jj] = sm[i * 16 + NP + jj];
    }
    b[0] = sm[ob0];
    b[1] = sm[ob1];
    b[2] = sm[ob2];
    b[3] = sm[ob3];
    const double quu_a = sm[oqa];  // Q_uu[c][g]: A operand of Q_uu L (0-padded through the address choice below)
    double gq[4] = {0.0, 0.0, 0.0, 0.0};
    if constexpr (BOX) {
#pragma unroll
        for (int i = 0; i < 4; ++i) gq[i] = sm[64 + NP + i];   // Q_u (zero beyond m)
    }
    __builtin_amdgcn_wave_barrier();
    const double b0[4] = {b[0], b[1], b[2], b[3]};  // original right-hand side (Sux column) for MODE 1's v' update
    ZM_SWEEP_STAMP(lab, 3);   // the exchange through LDS
    double dq[4] = {0.0, 0.0, 0.0, 0.0};
    int cl = 0;
    if constexpr (BOX) {   // wave-uniform: every lane holds the same Q_uu, Q_u, bounds and u_k
        double lo[4], hi[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if constexpr (STG) {
                lo[i] = (i < m ? lbk[i] : -__builtin_inf()) - uk[i];
                hi[i] = (i < m ? ubk[i] : __builtin_inf()) - uk[i];
            } else {
                lo[i] = bx->lb[i] - uk[i];
                hi[i] = bx->ub[i] - uk[i];
            }
        }
        bool capped;
        boxqp4(S, gq, lo, hi, dq, cl, capped);
        bx->capped += capped ? 1 : 0;
        double Sm[4][4];
        boxqp_mask(Sm, S, cl);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) S[i][jj] = Sm[i][jj];
            b[i] = ((cl >> i) & 1) ? 0.0 : b[i];
        }
    }
    if (__builtin_amdgcn_ballot_w64(!lu_solve4_nopivot(S, b, x)) != 0ull) lu_solve4_fallback(S, b, x);
    {
        double keep = x[0] + x[1] + x[2] + x[3];
        asm volatile("" : "+v"(keep));
    }
    ZM_SWEEP_STAMP(lab, 4);   // the 4 x 4 solve
    if constexpr (BOX) {
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = ((cl >> i) & 1) ? 0.0 : x[i];   // (exact zeros also where another row holds a NaN)
    }
    const double x01 = (g & 1) ? x[1] : x[0];
    const double x23 = (g & 1) ? x[3] : x[2];
    const double xg = (g & 2) ? x23 : x01;
    double out = (MODE == 1) ? xg : -xg;  // L_k[g][c] for c < n, l_k[g] for c == NP
    if constexpr (BOX) {
        const double d01 = (g & 1) ? dq[1] : dq[0];
        const double d23 = (g & 1) ? dq[3] : dq[2];
        out = (c == NP) ? ((g & 2) ? d23 : d01) : out;
    }
    if (a.vOut) *a.pOut = out;
    a.pOut -= a.sOut;
    const double lv = a.vL ? out : 0.0;
    // Q_u (zero beyond m) is read only now: eight registers fewer across the solve; its LDS row is rewritten in the next step
    double qu[4];
    if constexpr (MODE != 1) {
#pragma unroll
        for (int i = 0; i < 4; ++i) qu[i] = sm[64 + NP + i];
    }
    if constexpr (MODE != 1 && !BOX) {
        // -1/2 l^T Q_uu l with l = -x, Q_uu x = Q_u  (ilqrUtils.py:170 / :203), on the lanes that solved for l
        if (c == NP) a.vsum -= 0.5 * ((x[0] * qu[0] + x[1] * qu[1]) + (x[2] * qu[2] + x[3] * qu[3]));
    }

    double vxn = qv;
    if constexpr (MODE == 1) {
        // v'[c] = (q + A^T (v + V d))[c] - sum_i Sux[i][c] l[i]                                   (lqrUtils.py:252)
        if (g == 0 && c == NP) {
#pragma unroll
            for (int i = 0; i < 4; ++i) sm[112 + i] = x[i];
        }
        ilqr_lds_sync();
#pragma unroll
        for (int i = 0; i < 4; ++i) vxn = __builtin_fma(-b0[i], sm[112 + i], vxn);
    } else if constexpr (BOX) {
        // v_x'[c] = Q_x[c] + sum_i Q_ux[i][c] l[i]     (the general form's other terms L^T (Q_u + Q_uu l) vanish: L is zero on the
        //                                               clamped rows, Q_u + Q_uu l on the free ones)
#pragma unroll
        for (int i = 0; i < 4; ++i) vxn = __builtin_fma(b0[i], dq[i], vxn);
    } else {
        // v_x'[c] = Q_x[c] + sum_i L[i][c] Q_u[i]      (= Q_x - L^T Q_uu l with Q_uu l = -Q_u)
#pragma unroll
        for (int i = 0; i < 4; ++i) vxn = __builtin_fma(-x[i], qu[i], vxn);
    }
    if (g == 0) sm[80 + c] = a.cA ? vxn : 0.0;
    // T1 = Q_uu L ;  v_xx' = Q_xx - L^T T1
    const d4 t1 = mfma(quu_a, lv, zero4());
    d4 vacc = zero4();
#pragma unroll
    for (int s = 0; s < KS; ++s) vacc[s] = gacc[s];
    vacc = mfma<true>(lv, t1[0], vacc);
#pragma unroll
    for (int s = 0; s < KS; ++s) Vxx[s] = vacc[s];
    ilqr_lds_sync();
#pragma unroll
    for (int s = 0; s < KS; ++s) vxr[s] = sm[80 + 4 * s + g];
    __builtin_amdgcn_wave_barrier();
    ZM_SWEEP_STAMP(lab, 5);   // store, value terms, the two MFMAs of V', v_x through LDS
}

template <int KS, int MODE>
__global__ __launch_bounds__(64, 2) void ilqr_backward_t16_f64(
    const double* __restrict__ f_x, const double* __restrict__ f_u, const double* __restrict__ c_x,
    const double* __restrict__ c_u, const double* __restrict__ c_xx, const double* __restrict__ c_ux,
    const double* __restrict__ c_uu, const double* __restrict__ vf_x, const double* __restrict__ vf_xx,
    const double* __restrict__ dvec, const double* __restrict__ f_xx, const double* __restrict__ f_ux,
    const double* __restrict__ f_uu, const long svx, const long svxx, const int* __restrict__ active,
    const int shared_h, double* __restrict__ lout, double* __restrict__ Lout, const int T, const int n, const int m,
    const double* __restrict__ c_s, const double* __restrict__ vf_s, double* __restrict__ v_out,
    double* __restrict__ vx_out, double* __restrict__ vxx_out, const TrajList tl, const double* __restrict__ Hpk,
    const PairTab ptab) {
#define ZM_BOX_SETUP
#define ZM_BOX_FLAGS
#define ZM_BOX_ARGS
#define ZM_PEN_LOAD_FLAG
#define ZM_PEN_LOAD_ARG
#define ZM_PEN_TERMINAL
#include "ilqr_backward_t16_body.h"
#undef ZM_BOX_SETUP
#undef ZM_BOX_FLAGS
#undef ZM_BOX_ARGS
}

// The hooks of the body header for the two kernels with input bounds (ilqr_backward_box_t16_f64, ddp_backward_box_t16_f64)
// (STG: the bounds are a row per step, m doubles apart -- the one step stride zm_inputbox_t takes, so the kernels keep the constant
//  form's argument list; the sweep starts at row T - 1 and walks back)
#define ZM_BOX_SETUP                                                              \
    bx.pu = uTraj + last * m;                                                     \
    bx.capped = 0;                                                                \
    if constexpr (STG) {                                                          \
        bx.plb = lb + traj * bstride + (long)(T - 1) * m;                         \
        bx.pub = ub + traj * bstride + (long)(T - 1) * m;                         \
    } else {                                                                      \
        for (int i = 0; i < 4; ++i) {                                             \
            bx.lb[i] = (i < m) ? lb[traj * bstride + i] : -__builtin_inf();       \
            bx.ub[i] = (i < m) ? ub[traj * bstride + i] : __builtin_inf();        \
        }                                                                         \
    }
#define ZM_BOX_FLAGS , false, true, false, STG
#define ZM_BOX_ARGS , d4{0.0, 0.0, 0.0, 0.0}, nullptr, &bx

// The same kernel (MODE 0) with input bounds lb <= u <= ub: per step it also reads u_k of the current trajectory and runs the box-QP
// before the gain solve.  Bounds: row traj * bstride of lb / ub (bstride 0: one box for every trajectory).  qp_capped (optional):
// += the steps of the trajectory whose QP ended at its pass cap.  STG: stage-varying bounds, row traj * bstride + k * m at step k
// (zm_inputbox_t.step_stride == m); the constant form is the kernel's other instantiation.
template <int KS, bool STG>
__global__ __launch_bounds__(64, 2) void ilqr_backward_box_t16_f64(
    const double* __restrict__ f_x, const double* __restrict__ f_u, const double* __restrict__ c_x,
    const double* __restrict__ c_u, const double* __restrict__ c_xx, const double* __restrict__ c_ux,
    const double* __restrict__ c_uu, const double* __restrict__ vf_x, const double* __restrict__ vf_xx,
    const double* __restrict__ uTraj, const double* __restrict__ lb, const double* __restrict__ ub, const long bstride,
    const long svx, const long svxx, const int* __restrict__ active, const int shared_h, double* __restrict__ lout,
    double* __restrict__ Lout, int* __restrict__ qp_capped, const int T, const int n, const int m, const TrajList tl) {
    constexpr int MODE = 0;
    // what the other modes and the value outputs of the shared body read
    const double *const dvec = nullptr, *const f_xx = nullptr, *const f_ux = nullptr, *const f_uu = nullptr, *const Hpk = nullptr;
    const double *const c_s = nullptr, *const vf_s = nullptr;
    double *const v_out = nullptr, *const vx_out = nullptr, *const vxx_out = nullptr;
    const PairTab ptab = PairTab{};
    BoxStep bx;
#include "ilqr_backward_t16_body.h"
    if (qp_capped && lane == 0) qp_capped[traj] += bx.capped;
}

// Waves per SIMD the register budget is set for.  With two, the projection on top of the box step spills at KS = 2 (60 B of scratch)
// and KS = 3 (220 B); with one, the unified register file holds everything (DESIGN 2.5 has the figures).  The sweep is latency-bound
// on ~100 dependent matrix products per step: measured at n = 12, one wave without scratch is 6 - 12 % faster per solve than two with
// it (profiles/ddp_box_bench.txt).  KS = 1 fits two waves without scratch.
template <int KS>
constexpr int DDP_BOX_WAVES = (KS == 1) ? 2 : 1;

// The DDP sweep (MODE 2) with the same input bounds: per step the contraction and PD projection of vf_zz, then the box step above on
// the augmented Q.  Second derivatives as ilqr_backward_t16_f64 takes them: the full tensors, f_ux = f_uu = nullptr (control-affine),
// or the packed pairs Hpk / ptab.  STG: as ilqr_backward_box_t16_f64.
template <int KS, bool STG>
__global__ __launch_bounds__(64, DDP_BOX_WAVES<KS>) void ddp_backward_box_t16_f64(
    const double* __restrict__ f_x, const double* __restrict__ f_u, const double* __restrict__ c_x,
    const double* __restrict__ c_u, const double* __restrict__ c_xx, const double* __restrict__ c_ux,
    const double* __restrict__ c_uu, const double* __restrict__ vf_x, const double* __restrict__ vf_xx,
    const double* __restrict__ uTraj, const double* __restrict__ lb, const double* __restrict__ ub, const long bstride,
    const double* __restrict__ f_xx, const double* __restrict__ f_ux, const double* __restrict__ f_uu, const long svx, const long svxx,
    const int* __restrict__ active, const int shared_h, double* __restrict__ lout, double* __restrict__ Lout, int* __restrict__ qp_capped,
    const int T, const int n, const int m, const TrajList tl, const double* __restrict__ Hpk, const PairTab ptab) {
    constexpr int MODE = 2;
    const double* const dvec = nullptr;
    const double *const c_s = nullptr, *const vf_s = nullptr;
    double *const v_out = nullptr, *const vx_out = nullptr, *const vxx_out = nullptr;
    BoxStep bx;
#include "ilqr_backward_t16_body.h"
    if (qp_capped && lane == 0) qp_capped[traj] += bx.capped;
}
#undef ZM_BOX_SETUP
#undef ZM_BOX_FLAGS
#undef ZM_BOX_ARGS
#undef ZM_PEN_LOAD_FLAG
#undef ZM_PEN_LOAD_ARG
#undef ZM_PEN_TERMINAL

// The hooks of the body header for the two kernels with a state-box penalty: the second pair (ZM_PEN_LOAD_FLAG / ZM_PEN_LOAD_ARG) makes
// the operand fetch read the lane's entry of h_k with the step's other operands (prefetched two steps ahead like them), the step adds
// it to the loaded cost Hessian; ZM_PEN_TERMINAL adds h_T to the terminal V_xx.
#define ZM_PEN_SETUP                                                              \
    pn.hv = cA && ((c & 3) == g);                                                 \
    pn.hs = pn.hv ? (c >> 2) : -1;                                                \
    pn.sh = n;                                                                    \
    pn.ph = hdiag + (traj * (long)(T + 1) + (T - 1)) * n + (pn.hv ? c : 0);
#define ZM_PEN_LOAD_FLAG , true
#define ZM_PEN_LOAD_ARG , &pn
#define ZM_PEN_TERMINAL                                                                   \
    {                                                                                     \
        const double hT = hdiag[(traj * (long)(T + 1) + T) * n + (pn.hv ? c : 0)];        \
        _Pragma("unroll") for (int s = 0; s < KS; ++s) Vxx[s] = (pn.hs == s) ? Vxx[s] + hT : Vxx[s]; \
    }

// ilqr_backward_t16_f64<KS, 0> on the cost Hessians c_xx + diag h_k (k < T) and v_xx + diag h_T: hdiag (batch, T+1, n).  Row 0 IS read
// and added to step 0's c_xx like every other row (the penalty expansion writes zeros there: x_0 is never constrained).
#define ZM_BOX_SETUP ZM_PEN_SETUP
#define ZM_BOX_FLAGS , false, false, true
#define ZM_BOX_ARGS , d4{0.0, 0.0, 0.0, 0.0}, nullptr, nullptr, &pn
template <int KS>
__global__ __launch_bounds__(64, 2) void ilqr_backward_pen_t16_f64(
    const double* __restrict__ f_x, const double* __restrict__ f_u, const double* __restrict__ c_x,
    const double* __restrict__ c_u, const double* __restrict__ c_xx, const double* __restrict__ c_ux,
    const double* __restrict__ c_uu, const double* __restrict__ vf_x, const double* __restrict__ vf_xx,
    const double* __restrict__ hdiag, const long svx, const long svxx, const int* __restrict__ active, const int shared_h,
    double* __restrict__ lout, double* __restrict__ Lout, const int T, const int n, const int m, const TrajList tl) {
    constexpr int MODE = 0;
    const double *const dvec = nullptr, *const f_xx = nullptr, *const f_ux = nullptr, *const f_uu = nullptr, *const Hpk = nullptr;
    const double *const c_s = nullptr, *const vf_s = nullptr;
    double *const v_out = nullptr, *const vx_out = nullptr, *const vxx_out = nullptr;
    const PairTab ptab = PairTab{};
    PenStep pn;
#include "ilqr_backward_t16_body.h"
}
#undef ZM_BOX_SETUP
#undef ZM_BOX_FLAGS
#undef ZM_BOX_ARGS

// ... and ilqr_backward_box_t16_f64 on the same Hessians
#define ZM_BOX_SETUP                                                              \
    bx.pu = uTraj + last * m;                                                     \
    bx.capped = 0;                                                                \
    for (int i = 0; i < 4; ++i) {                                                 \
        bx.lb[i] = (i < m) ? lb[traj * bstride + i] : -__builtin_inf();           \
        bx.ub[i] = (i < m) ? ub[traj * bstride + i] : __builtin_inf();            \
    }                                                                             \
    ZM_PEN_SETUP
#define ZM_BOX_FLAGS , false, true, true
#define ZM_BOX_ARGS , d4{0.0, 0.0, 0.0, 0.0}, nullptr, &bx, &pn
template <int KS>
__global__ __launch_bounds__(64, 2) void ilqr_backward_box_pen_t16_f64(
    const double* __restrict__ f_x, const double* __restrict__ f_u, const double* __restrict__ c_x,
    const double* __restrict__ c_u, const double* __restrict__ c_xx, const double* __restrict__ c_ux,
    const double* __restrict__ c_uu, const double* __restrict__ vf_x, const double* __restrict__ vf_xx,
    const double* __restrict__ hdiag, const double* __restrict__ uTraj, const double* __restrict__ lb, const double* __restrict__ ub,
    const long bstride, const long svx, const long svxx, const int* __restrict__ active, const int shared_h, double* __restrict__ lout,
    double* __restrict__ Lout, int* __restrict__ qp_capped, const int T, const int n, const int m, const TrajList tl) {
    constexpr int MODE = 0;
    const double *const dvec = nullptr, *const f_xx = nullptr, *const f_ux = nullptr, *const f_uu = nullptr, *const Hpk = nullptr;
    const double *const c_s = nullptr, *const vf_s = nullptr;
    double *const v_out = nullptr, *const vx_out = nullptr, *const vxx_out = nullptr;
    const PairTab ptab = PairTab{};
    BoxStep bx;
    PenStep pn;
#include "ilqr_backward_t16_body.h"
    if (qp_capped && lane == 0) qp_capped[traj] += bx.capped;
}
#undef ZM_BOX_SETUP
#undef ZM_BOX_FLAGS
#undef ZM_BOX_ARGS
#undef ZM_PEN_SETUP
#undef ZM_PEN_LOAD_FLAG
#undef ZM_PEN_LOAD_ARG
#undef ZM_PEN_TERMINAL

// Test entry of the box-QP (boxqp4.h): one problem per lane.  H (batch, m, m), g, lo, hi (batch, m) -> d (batch, m), the clamped set
// as a bit mask, the passes taken (BOXQP_CAP where the cap was reached).
__global__ __launch_bounds__(64) void boxqp_kernel(const double* __restrict__ H, const double* __restrict__ g, const double* __restrict__ lo,
                                                   const double* __restrict__ hi, double* __restrict__ d_out, int* __restrict__ clamped_out,
                                                   int* __restrict__ iters_out, const long batch, const int m) {
    const long p = (long)blockIdx.x * 64 + threadIdx.x;
    if (p >= batch) return;
    double Hm[4][4], gv[4], lv[4], hv[4], d[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) Hm[i][j] = (i < m && j < m) ? H[p * m * m + i * m + j] : (i == j ? 1.0 : 0.0);
        gv[i] = (i < m) ? g[p * m + i] : 0.0;
        lv[i] = (i < m) ? lo[p * m + i] : -__builtin_inf();
        hv[i] = (i < m) ? hi[p * m + i] : __builtin_inf();
    }
    int cl = 0;
    bool capped = false;
    const int it = boxqp4(Hm, gv, lv, hv, d, cl, capped);
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (i < m) d_out[p * m + i] = d[i];
    if (clamped_out) clamped_out[p] = cl;
    if (iters_out) iters_out[p] = it;
}

}  // namespace zm

// ---------------------------------------------------------------------------------------------------------------------
// K3-DMA: the iLQR sweep (MODE 0) with its per-step operands staged through an LDS ring by DMA, as K1 does
// (lqr_backward_dma.hip): no operand prefetch registers, no per-step address arithmetic for loads, no vector-memory
// latency on the chain.  n in {8, 12}, m = 4, 16-B aligned pointers; every other case runs ilqr_backward_t16_f64.
// Cache policy of the operand DMA: the default one (aux 0).  Unlike K1 (lqr_backward_dma.hip, where
// non-temporal loads are worth 10 %), the sweeps measured 7 % SLOWER with nt at 8192 x 100 steps (per-step Hessians 616 -> 660 us,
// affine 722 -> 754 us, shared Hessians unchanged; profiles/r02_ilqr_nt_ab.txt).

// Slot image of one step (16-B chunks): f_x | f_u | c_x | c_u [| c_xx | c_ux | c_uu unless the Hessians are shared] | zeros.
namespace zm {

// NJP > 0: [f_x | f_u] arrives PACKED -- NJP doubles per step (the structurally nonzero entries of the model's Jacobian, positions in a
// JacTab; everything else is the identity's 0 or 1, served from two constant chunks in the slot's padding) instead of N (N + M).
struct JacTab {
    unsigned char pos[12 * 16];   // packed position of entry (i, j) of [f_x | f_u], 255: not stored
};
// NHS > 0 (MODE 2): the second derivatives arrive SPARSE -- NHS doubles per step (their structurally nonzero entries, dense positions in
// an HTab), scattered every step into a dense [NPAIR][N] image that lives once in LDS (its other entries stay zero).
struct HTab {
    unsigned short dense[96];   // dense index pair * N + i of sparse entry k
    int n;                      // entries (<= 96)
};
template <int N, int M, bool SHARED, int MODE, int NPAIR = 0, int NJP = 0, int NHS = 0>
struct IlqrDmaGeom {
    static constexpr int KS = N / 4;
    static constexpr int CFX = NJP ? NJP / 2 : N * N / 2, CFU = NJP ? 0 : N * M / 2, CCX = N / 2, CCU = M / 2;
    static constexpr int CXX = SHARED ? 0 : N * N / 2, CUX = SHARED ? 0 : N * M / 2, CUU = SHARED ? 0 : M * M / 2;
    static constexpr int CD = (MODE == 1) ? N / 2 : 0;   // MODE 1: the affine term d of the dynamics
    static constexpr int CH = (MODE == 2) ? (NHS ? NHS / 2 : NPAIR * N / 2) : 0;   // MODE 2: the second derivatives H[pair][i] of the step
    static constexpr int CT = CFX + CFU + CCX + CCU + CXX + CUX + CUU + CD + CH;
    static constexpr int NI = (CT + 63) / 64;
    static constexpr int SLOT = NI * 1024;
    static constexpr int OFX = 0, OFU = CFX * 16, OCX = OFU + CFU * 16, OCU = OCX + CCX * 16;
    static constexpr int OXX = OCU + CCU * 16, OUX = OXX + CXX * 16, OUU = OUX + CUX * 16;
    static constexpr int OD = OUU + CUU * 16;
    static constexpr int OH = OD + CD * 16;
    static constexpr int OZ = CT * 16;
    static constexpr int OONE = OZ + 16;   // NJP: a chunk of ones behind the chunk of zeros
    static_assert(NJP % 2 == 0 && (NJP == 0 || (N == 12 && SHARED)), "packed Jacobians: n = 12, 16-B rows, shared cost Hessians");
    static_assert(NJP == 0 || SLOT - OZ >= 32, "slot needs a zero and a one chunk");
    static_assert(N % 4 == 0 && N >= 8 && N <= 12 && M == 4, "fast path: all K-step rows live, m = 4");
    static_assert(MODE == 0 || (MODE == 1 && !SHARED) || (MODE == 2 && SHARED && N == 12 && NPAIR > 0 && NPAIR <= ZM_MAX_PAIRS),
                  "iLQR, affine LQR, or DDP with shared cost Hessians and packed second derivatives");
    static_assert(SLOT - OZ >= 16, "slot needs zero padding");
};

// W: waves per workgroup, wave w of block b works on slot b * W + w (list form only).  The waves share nothing; what W = 4 buys is
// PLACEMENT when few trajectories are left: the four waves of a workgroup go to the four SIMDs of a CU, whereas single-wave workgroups
// start doubling up on SIMDs beyond three per CU (768 waves: measured 148 against 119 us per sweep at 808 resp. 758 trajectories).
// Waves per SIMD the register budget is set for: the projection of the DDP sweep (MODE 2) needs the registers of two
constexpr int ILQR_DMA_WAVES = 3, DDP_DMA_WAVES = 2;
template <int N, int M, int D, bool SHARED, int MODE, int NPAIR = 0, int NJP = 0, int NHS = 0, int W = 1>
__global__ __launch_bounds__(64 * W, MODE == 2 ? DDP_DMA_WAVES : ILQR_DMA_WAVES) void ilqr_backward_dma_f64(
    const double* __restrict__ f_x, const double* __restrict__ f_u, const double* __restrict__ c_x,
    const double* __restrict__ c_u, const double* __restrict__ c_xx, const double* __restrict__ c_ux,
    const double* __restrict__ c_uu, const double* __restrict__ vf_x, const double* __restrict__ vf_xx,
    const double* __restrict__ dvec, const long svx, const long svxx, const int* __restrict__ active,
    double* __restrict__ lout, double* __restrict__ Lout, const int T, const TrajList tl, const double* __restrict__ Hpk,
    const PairTab ptab, const JacTab jtab, const HTab htab) {
    using G = IlqrDmaGeom<N, M, SHARED, MODE, NPAIR, NJP, NHS>;
    static_assert(NHS % 2 == 0 && NHS <= 96 && (NHS == 0 || MODE == 2), "sparse second derivatives: DDP mode, 16-B rows");
    constexpr int KS = G::KS, NI = G::NI, SLOT = G::SLOT, NP = N;
    constexpr int nn = N * N, nm = N * M, mm = M * M;
    constexpr int SMO = D * SLOT;
    constexpr int HDN = NHS ? NPAIR * N : 0;   // dense image of the sparse second derivatives
    constexpr int PER_WAVE = SMO + ILQR_LDS_DOUBLES * 8 + (MODE == 2 ? NS_LDS_DOUBLES * 8 : 0) + HDN * 8;
    static_assert(PER_WAVE % 16 == 0, "per-wave LDS slices stay 16-B aligned");
    __shared__ __attribute__((aligned(16))) char lds_all[W * PER_WAVE];
    const int wave = (W == 1) ? 0 : __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    char* const lds = lds_all + wave * PER_WAVE;
    double* sm = (double*)(lds + SMO);
    double* jA = (double*)(lds + SMO + ILQR_LDS_DOUBLES * 8);   // MODE 2: transpose buffers of the sign iteration (ns16.h)
    double* hd = jA + NS_LDS_DOUBLES;
    const int lane = threadIdx.x & 63;
    const long slot_ = (long)blockIdx.x * W + wave;
    if (W > 1 && slot_ >= tl.count) return;    // (W > 1: list form; whole waves only, no barrier anywhere in this kernel)
    const long traj = tl.list ? (long)tl.list[slot_] : slot_;
    if (active && active[traj] == 0) return;   // whole wave leaves: this trajectory keeps its previous policy
    const int g = lane >> 4, c = lane & 15;
    const bool cA = c < N, cB = (c >= N) && (c < N + M);

    // DMA sources: chunk q of the step image -> (array, offset)
    const char* p[NI];
    int st[NI];
    {
        const long last = traj * T + (T - 1);
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            int q = i * 64 + lane;
            const char* src = (NJP && q == G::CT + 1) ? (const char*)zm_one_src : (const char*)zm_zero_src;
            int stride = 0;
            if (q < G::CFX) {
                if constexpr (NJP != 0) {   // f_x points to the packed images
                    src = (const char*)(f_x + last * NJP) + q * 16;  stride = NJP * 8;
                } else {
                    src = (const char*)(f_x + last * nn) + q * 16;  stride = nn * 8;
                }
            } else if ((q -= G::CFX) < G::CFU) {
                src = (const char*)(f_u + last * nm) + q * 16;  stride = nm * 8;
            } else if ((q -= G::CFU) < G::CCX) {
                src = (const char*)(c_x + last * N) + q * 16;   stride = N * 8;
            } else if ((q -= G::CCX) < G::CCU) {
                src = (const char*)(c_u + last * M) + q * 16;   stride = M * 8;
            } else if constexpr (MODE == 2) {
                if ((q -= G::CCU) < G::CH) {
                    constexpr int HROW = NHS ? NHS : NPAIR * N;   // doubles per step in HBM
                    src = (const char*)(Hpk + last * (long)HROW) + q * 16;  stride = HROW * 8;
                }
            } else if constexpr (!SHARED) {
                if ((q -= G::CCU) < G::CXX) {
                    src = (const char*)(c_xx + last * nn) + q * 16;  stride = nn * 8;
                } else if ((q -= G::CXX) < G::CUX) {
                    src = (const char*)(c_ux + last * nm) + q * 16;  stride = nm * 8;
                } else if ((q -= G::CUX) < G::CUU) {
                    src = (const char*)(c_uu + last * mm) + q * 16;  stride = mm * 8;
                } else if constexpr (MODE == 1) {
                    if ((q -= G::CUU) < G::CD) {
                        src = (const char*)(dvec + last * N) + q * 16;  stride = N * 8;
                    }
                }
            }
            p[i] = src;
            st[i] = stride;
        }
    }
    auto dma = [&](char* slot) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            __builtin_amdgcn_global_load_lds((glb_void_t*)p[i], (lds_void_t*)(slot + i * 1024), 16, 0, 0);
            p[i] -= st[i];
        }
    };
    // LDS offsets of this lane's operands inside a slot (lanes outside a matrix read the zero padding)
    const int oF = cA ? (G::OFX + (g * N + c) * 8) : cB ? (G::OFU + (g * M + (c - N)) * 8) : G::OZ;
    const int dF = cA ? 4 * N * 8 : cB ? 4 * M * 8 : 0;
    int oFp[KS];   // NJP: slot offset of F[4s+g][c] -- its packed entry, or the chunk of zeros / ones
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int row = 4 * s + g;
        const int p = NJP ? (int)jtab.pos[row * 16 + c] : 255;
        oFp[s] = (p != 255) ? (G::OFX + p * 8) : ((row == c) ? G::OONE : G::OZ);
    }
    const int ocv = cA ? (G::OCX + c * 8) : cB ? (G::OCU + (c - N) * 8) : G::OZ;
    const int oC = cA ? (G::OXX + (g * N + c) * 8) : G::OZ;       // !SHARED only
    const int dC = cA ? 4 * N * 8 : 0;
    const int oCu = cA ? (G::OUX + (g * N + c) * 8) : cB ? (G::OUU + (g * M + (c - N)) * 8) : G::OZ;   // (g < M always)
    const int odc = cA ? (G::OD + c * 8) : G::OZ;                  // MODE 1: d[c]; d[4 s + g] is read at OD + (4 s + g) 8

    // the pieces of IlqrAddr the step still uses: outputs and lane roles
    IlqrAddr<KS> a;
    a.cA = cA;
    a.vL = cA;                                  // (g < m always: M == 4)
    const bool vl = (c == NP);
    a.vOut = a.vL || vl;
    {
        const long last = traj * T + (T - 1);
        a.pOut = a.vL ? (Lout + last * nm + g * N + c) : (lout + last * M + g);
    }
    a.sOut = vl ? M : nm;
    // MODE 2: tile element (4r+g, c) of vf_zz is pair (min, max) of the model's table (row of the packed image) or structurally zero
    int oH[4];
    bool zok[4];
    if constexpr (MODE == 2) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 4 * r + g;
            const int lo = row < c ? row : c, hi = row < c ? c : row;
            int pidx = -1;
            for (int q = 0; q < NPAIR; ++q) pidx = (ptab.ab[q] == (unsigned char)(lo * 16 + hi)) ? q : pidx;
            zok[r] = pidx >= 0;
            oH[r] = (NHS ? 0 : G::OH) + (pidx >= 0 ? pidx : 0) * (N * 8);   // NHS: relative to the dense image, else to the slot
            a.zlive[r] = (row == c);   // n + m = 16: every tile index is a live (state or control) index
        }
    }
    const bool rhs_qu = (c == NP);
    const int ob0 = rhs_qu ? (64 + NP + 0) : (0 * 16 + c);
    const int ob1 = rhs_qu ? (64 + NP + 1) : (1 * 16 + c);
    const int ob2 = rhs_qu ? (64 + NP + 2) : (2 * 16 + c);
    const int ob3 = rhs_qu ? (64 + NP + 3) : (3 * 16 + c);
    const int oqa = (c < 4) ? (c * 16 + NP + g) : (g * 16 + c);

    // shared (time-invariant) cost Hessian: once, into registers
    double Csh[KS], Cush = 0.0;
#pragma unroll
    for (int s = 0; s < KS; ++s) Csh[s] = 0.0;
    if constexpr (SHARED) {
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const double t = c_xx[cA ? (4 * s + g) * N + c : 0];
            Csh[s] = cA ? t : 0.0;
        }
        const double tu = cA ? c_ux[g * N + c] : (cB ? c_uu[g * M + (c - N)] : 0.0);
        Cush = tu;
    }
    // terminal value function
    double Vxx[KS], vxr[KS];
    {
        const double* vxx = SHARED ? vf_xx : vf_xx + traj * svxx;
        const double* vx = vf_x + traj * svx;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int row = 4 * s + g;
            const double t = vxx[cA ? row * N + c : 0];
            Vxx[s] = cA ? t : 0.0;
            vxr[s] = vx[row];
        }
        if (g == 0) sm[80 + c] = cA ? vx[c] : 0.0;
    }
    int hdst0 = 0, hdst1 = 0;   // NHS: dense positions of sparse entries lane, lane + 64
    if constexpr (NHS != 0) {
        for (int e = lane; e < HDN; e += 64) hd[e] = 0.0;
        hdst0 = (lane < htab.n) ? (int)htab.dense[lane] : -1;
        hdst1 = (lane + 64 < htab.n) ? (int)htab.dense[(lane + 64) % 96] : -1;
    }
    ilqr_lds_sync();

#pragma unroll
    for (int i = 0; i < D; ++i)
        if (T - 1 - i >= 0) dma(lds + i * SLOT);
    int j = T - 1;
#ifdef ZM_SWEEP_LAB
    SweepLab labv;
    for (int q = 0; q < 8; ++q) labv.acc[q] = 0ull;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(labv.last)::"memory");
    SweepLab* const lab = &labv;
#else
    SweepLab* const lab = nullptr;
#endif
    for (;;) {
#pragma unroll
        for (int si = 0; si < D; ++si) {
            char* slot = lds + si * SLOT;
            wait_for_step<NI, D>(j);
            ZM_SWEEP_STAMP(lab, 0);   // waiting for the step's DMA
            IlqrStepRegs<KS> d;
#pragma unroll
            for (int s = 0; s < KS; ++s) d.F[s] = *(const double*)(slot + (NJP ? oFp[s] : oF + s * dF));
            d.cv = *(const double*)(slot + ocv);
            if constexpr (SHARED) {
#pragma unroll
                for (int s = 0; s < KS; ++s) d.C[s] = Csh[s];
                d.Cu = Cush;
            } else {
#pragma unroll
                for (int s = 0; s < KS; ++s) d.C[s] = *(const double*)(slot + oC + s * dC);
                d.Cu = *(const double*)(slot + oCu);
            }
            if constexpr (MODE == 1) {
                d.dc = *(const double*)(slot + odc);
#pragma unroll
                for (int s = 0; s < KS; ++s) d.dr[s] = *(const double*)(slot + G::OD + (4 * s + g) * 8);
            }
            d4 zin = zero4();
            if constexpr (NHS != 0) {   // this step's nonzero second derivatives into the dense image
                const double* hs = (const double*)(slot + G::OH);
                const double h0 = hs[lane], h1 = hs[(lane + 64 < NHS) ? lane + 64 : 0];
                if (hdst0 >= 0) hd[hdst0] = h0;
                if (hdst1 >= 0) hd[hdst1] = h1;
                ilqr_lds_sync();
            }
            if constexpr (MODE == 2) {
                // vf_zz[4r+g][c] = sum_i v_x[i] H[pair][i], i ascending (the order of the register kernel's contraction); v_x is
                // this wave's LDS row sm[80 ..], written by the previous step
                double vx[N];
#pragma unroll
                for (int i = 0; i < N; ++i) vx[i] = sm[80 + i];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double* h = NHS ? (const double*)((const char*)hd + oH[r]) : (const double*)(slot + oH[r]);
                    double z = 0.0;
#pragma unroll
                    for (int i = 0; i < N; ++i) z = __builtin_fma(vx[i], h[i], z);
                    zin[r] = zok[r] ? z : 0.0;
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // operands are in registers: the slot may be refilled
            if (j - D >= 0) dma(slot);
            ZM_SWEEP_STAMP(lab, 1);   // operand reads (and MODE 2's contraction), DMA issue
            ilqr_step<KS, MODE, false, MODE == 2>(Vxx, vxr, d, a, sm, g, c, ob0, ob1, ob2, ob3, oqa, jA, N, M, zin, lab);
            if (--j < 0) {
#ifdef ZM_SWEEP_LAB
                if (blockIdx.x == 0 && threadIdx.x == 0) {
                    for (int q = 0; q < 8; ++q) atomicAdd(&zm_sweep_stamps[q], labv.acc[q]);
                    atomicAdd(&zm_sweep_stamps[8], 1ull);
                }
#endif
                return;
            }
        }
    }
}

// ZM_EUNSUPPORTED unless (n in {8, 12}, m = 4, 16-B aligned pointers): the caller then runs the register-prefetch kernel
template <int MODE>
static int ilqr_backward_dma_dispatch(const double* f_x, const double* f_u, const double* c_x, const double* c_u,
                                      const double* c_xx, const double* c_ux, const double* c_uu, const double* vf_x,
                                      const double* vf_xx, const double* dvec, long svx, long svxx, const int* act, int sh,
                                      double* l, double* L, int64_t batch, int T, int n, int m, hipStream_t st,
                                      TrajList tl = TrajList{nullptr, 0}) {
    static const bool off = [] {
        const char* e = zm::fallback_env("ZOPT_AMD_ILQR_PATH");
        return e && e[0] == 'r';   // "reg": force the register-prefetch kernel
    }();
    if (off || m != 4 || (n != 8 && n != 12)) return ZM_EUNSUPPORTED;
    const uintptr_t al = (uintptr_t)f_x | (uintptr_t)f_u | (uintptr_t)c_x | (uintptr_t)c_u | (uintptr_t)dvec |
                         (sh ? 0 : ((uintptr_t)c_xx | (uintptr_t)c_ux | (uintptr_t)c_uu));
    if (al & 15) return ZM_EUNSUPPORTED;
    const dim3 grid((unsigned)(tl.list ? tl.count : batch)), block(64);
    // ring depth: 3 steps in flight when the step image is 2 KB (shared Hessians), 2 when it is 4 KB (measured: profiles/)
    constexpr int DS = 3, DF = 2;
#define ZM_LAUNCH_ILQR_DMA(NN, DD, SH)                                                                                     \
    hipLaunchKernelGGL((ilqr_backward_dma_f64<NN, 4, DD, SH, MODE>), grid, block, 0, st, f_x, f_u, c_x, c_u, c_xx, c_ux, c_uu, \
                       vf_x, vf_xx, dvec, svx, svxx, act, l, L, T, tl, (const double*)nullptr, PairTab{}, JacTab{}, HTab{})
    if constexpr (MODE == 0) {
        if (n == 12) {
            if (sh) ZM_LAUNCH_ILQR_DMA(12, DS, true); else ZM_LAUNCH_ILQR_DMA(12, DF, false);
        } else {
            if (sh) ZM_LAUNCH_ILQR_DMA(8, DS, true); else ZM_LAUNCH_ILQR_DMA(8, DF, false);
        }
    } else {
        if (n == 12) ZM_LAUNCH_ILQR_DMA(12, DF, false); else ZM_LAUNCH_ILQR_DMA(8, DF, false);
    }
#undef ZM_LAUNCH_ILQR_DMA
    ZM_HIP_CHECK(hipGetLastError());
    return ZM_OK;
}

// K4-DMA: the DDP sweep with shared cost Hessians and the PACKED second derivatives (the solver's form) on the same LDS ring -- the
// step image grows by the pairs' rows (28 x 12 doubles for the quadcopter: 4.3 KB per step), the contraction reads them from LDS.
// ZM_EUNSUPPORTED unless (n = 12, m = 4, 28 declared pairs, 16-B aligned pointers): the caller then runs ilqr_backward_t16_f64.
static int ddp_backward_dma_dispatch(const double* f_x, const double* f_u, const double* Hpk, const PairTab& ptab, const double* c_x,
                                     const double* c_u, const double* c_xx, const double* c_ux, const double* c_uu, const double* vf_x,
                                     const double* vf_xx, long svx, const int* act, int sh, double* l, double* L, int64_t batch, int T,
                                     int n, int m, hipStream_t st, TrajList tl) {
    static const bool off = [] {
        const char* e = zm::fallback_env("ZOPT_AMD_ILQR_PATH");
        return e && e[0] == 'r';   // "reg": force the register kernel
    }();
    if (off || !sh || n != 12 || m != 4 || ptab.n != 28 || !Hpk) return ZM_EUNSUPPORTED;
    if (((uintptr_t)f_x | (uintptr_t)f_u | (uintptr_t)c_x | (uintptr_t)c_u | (uintptr_t)Hpk) & 15) return ZM_EUNSUPPORTED;
    const dim3 grid((unsigned)(tl.list ? tl.count : batch)), block(64);
    hipLaunchKernelGGL((ilqr_backward_dma_f64<12, 4, 2, true, 2, 28>), grid, block, 0, st, f_x, f_u, c_x, c_u, c_xx, c_ux, c_uu, vf_x,
                       vf_xx, (const double*)nullptr, svx, 0L, act, l, L, T, tl, Hpk, ptab, JacTab{}, HTab{});
    ZM_HIP_CHECK(hipGetLastError());
    return ZM_OK;
}

// Solver-internal (ilqr_solve.hip): the iLQR (Hpk == nullptr) or DDP sweep of the listed trajectories with PACKED Jacobians Fp
// (njp doubles per step: 56 or 60, positions `pos`; written by linearize.hip's packed expansion), shared cost Hessians, n = 12, m = 4.
// nhs > 0: Hpk holds the SPARSE second derivatives, nhs doubles per step (70 or 86), dense positions `hdense` (nh of them).
int sweep_packed_jacobians(const double* Fp, int njp, const unsigned char* pos, const double* Hpk, const PairTab& ptab, const double* c_x,
                           const double* c_u, const double* c_xx, const double* c_ux, const double* c_uu, const double* vf_x,
                           const double* vf_xx, const int* act, double* l, double* L, int64_t batch, int T, hipStream_t st, TrajList tl,
                           int nhs, const unsigned short* hdense, int nh) {
    if (((uintptr_t)Fp | (uintptr_t)c_x | (uintptr_t)c_u | (uintptr_t)Hpk) & 15) return ZM_EUNSUPPORTED;
    if ((njp != 56 && njp != 60) || (Hpk && ptab.n != 28)) return ZM_EUNSUPPORTED;
    if (nhs && !(Hpk && ((njp == 56 && nhs == 70) || (njp == 60 && nhs == 86)) && hdense && nh > 0 && nh <= nhs)) return ZM_EUNSUPPORTED;
    JacTab jt;
    for (int e = 0; e < 192; ++e) jt.pos[e] = pos[e];
    HTab ht{};
    for (int e = 0; e < nh && nhs; ++e) ht.dense[e] = hdense[e];
    ht.n = nhs ? nh : 0;
    const long nslot = tl.list ? tl.count : batch;
    // few trajectories left (at most one wave per SIMD): four-wave workgroups, one wave per SIMD of a CU
    static const long wg4_max = [] {   // ZOPT_AMD_SWEEP_WG4=<n>: four-wave workgroups up to n listed trajectories (A/B)
        const char* e = zm::lab_env("ZOPT_AMD_SWEEP_WG4");
        return e ? atol(e) : 2048L;   // (round 3, same-box A/B of the 8192-problem solve: 34.8-34.9 ms at 1024, 34.3-34.5 at 2048, 34.2-34.7 at 3072 / 4096)
    }();
    const bool quad_wg = tl.list && nslot <= wg4_max;
    const dim3 grid((unsigned)(quad_wg ? (nslot + 3) / 4 : nslot)), block(quad_wg ? 256 : 64);
#define ZM_LAUNCH_PACKED(DD, MODE_, NPAIR_, NJP_, NHS_)                                                                               \
    do {                                                                                                                              \
        if (quad_wg)                                                                                                                  \
            hipLaunchKernelGGL((ilqr_backward_dma_f64<12, 4, DD, true, MODE_, NPAIR_, NJP_, NHS_, 4>), grid, block, 0, st, Fp,         \
                               (const double*)nullptr, c_x, c_u, c_xx, c_ux, c_uu, vf_x, vf_xx, (const double*)nullptr, 12L, 0L, act, l, \
                               L, T, tl, Hpk, ptab, jt, ht);                                                                          \
        else                                                                                                                          \
            hipLaunchKernelGGL((ilqr_backward_dma_f64<12, 4, DD, true, MODE_, NPAIR_, NJP_, NHS_>), grid, block, 0, st, Fp,            \
                               (const double*)nullptr, c_x, c_u, c_xx, c_ux, c_uu, vf_x, vf_xx, (const double*)nullptr, 12L, 0L, act, l, \
                               L, T, tl, Hpk, ptab, jt, ht);                                                                          \
    } while (0)
    if (Hpk && nhs) {
        if (njp == 56) ZM_LAUNCH_PACKED(2, 2, 28, 56, 70); else ZM_LAUNCH_PACKED(2, 2, 28, 60, 86);
    } else if (Hpk) {
        if (njp == 56) ZM_LAUNCH_PACKED(2, 2, 28, 56, 0); else ZM_LAUNCH_PACKED(2, 2, 28, 60, 0);
    } else {
        if (njp == 56) ZM_LAUNCH_PACKED(3, 0, 0, 56, 0); else ZM_LAUNCH_PACKED(3, 0, 0, 60, 0);
    }
#undef ZM_LAUNCH_PACKED
    ZM_HIP_CHECK(hipGetLastError());
    return ZM_OK;
}

}  // namespace zm

namespace zm {
struct DdpTensors {
    const double *f_xx, *f_ux, *f_uu;
    const double* Hpk = nullptr;   // packed second derivatives of the model's declared pairs (instead of the three tensors)
    PairTab ptab = PairTab{};
};
struct ValueIO {   // optional scalar inputs / value-function outputs
    const double *c, *vf;
    double *v_out, *vx_out, *vxx_out;
};

template <int MODE>
static int launch_ilqr(const double* f_x, const double* f_u, const double* c_x, const double* c_u, const double* c_xx,
                       const double* c_ux, const double* c_uu, const double* vf_x, const double* vf_xx, const double* d,
                       long svx, long svxx, const int* act, int sh, double* l, double* L, int64_t batch, int T, int n, int m,
                       hipStream_t st, DdpTensors z = DdpTensors{nullptr, nullptr, nullptr},
                       ValueIO v = ValueIO{nullptr, nullptr, nullptr, nullptr, nullptr}, TrajList tl = TrajList{nullptr, 0}) {
    const dim3 grid((unsigned)(tl.list ? tl.count : batch)), block(64);
    with_ks(n, [&](auto ks) {
        hipLaunchKernelGGL((ilqr_backward_t16_f64<decltype(ks)::value, MODE>), grid, block, 0, st, f_x, f_u, c_x, c_u, c_xx, c_ux, c_uu, vf_x,
                           vf_xx, d, z.f_xx, z.f_ux, z.f_uu, svx, svxx, act, sh, l, L, T, n, m, v.c, v.vf, v.v_out, v.vx_out, v.vxx_out, tl, z.Hpk, z.ptab);
    });
    ZM_HIP_CHECK(hipGetLastError());
    return ZM_OK;
}
}  // namespace zm

namespace zm {
// sweep_tiled_f64.hip: the iLQR (mode 0) / bilinear-affine (mode 1) sweeps on fp64 MFMA tiles for n <= 48, m <= 16
int sweep_tiled_f64_dispatch(int mode, const double* f_x, const double* f_u, const double* c_x, const double* c_u, const double* c_xx,
                             const double* c_ux, const double* c_uu, const double* vf_x, const double* vf_xx, const double* dvec,
                             long svx, long svxx, const int* active, int shared_hessian, double* l, double* L, int64_t batch, int T,
                             int n, int m, hipStream_t st, const int* list, long count, const double* cs = nullptr,
                             const double* vf = nullptr, double* v_out = nullptr, double* vx_out = nullptr, double* vxx_out = nullptr);
}  // namespace zm

// tiled: the entry point also has the large-state tile kernel (n <= 48, m <= 16) behind it
static int zm_check_sweep_args(const char* who, int64_t batch, int T, int n, int m, bool tiled = false) {
    return zm::check_sweep_args(who, batch, T, n, m, tiled ? 48 : 12, tiled ? 16 : 4);
}

// What the list entries check first, in this order: nothing to do (*rc <- ZM_OK; pointers of empty arrays may be NULL), the list's
// length, the operands (`operands`: the entry's own "all given"), the sizes.  true: the entry returns *rc.  `who_list` names the entry
// in the list-length message, `who` in the others (for some entries the name of the dense form), as they always did.
static bool sweep_prologue(int* rc, const char* who_list, const char* who, const int32_t* list, int64_t count, bool operands, int64_t batch,
                           int T, int n, int m, bool tiled = false, const char* null_note = "") {
    *rc = ZM_OK;
    if (batch == 0 || (list && count == 0)) return true;
    if (list && (count < 0 || count > batch)) *rc = zm::set_error(ZM_EINVAL, "%s: bad list length", who_list);
    else if (!operands) *rc = zm::set_error(ZM_EINVAL, "%s: null pointer%s", who, null_note);
    else *rc = zm_check_sweep_args(who, batch, T, n, m, tiled);
    return *rc != ZM_OK;
}
static const char* const ZM_DDP_NULL_NOTE = " (f_ux and f_uu may be NULL together: identically zero)";

extern "C" int zm_ilqr_backward_list_f64(const double* f_x, const double* f_u, const double* c_x, const double* c_u,
                                         const double* c_xx, const double* c_ux, const double* c_uu, const double* vf_x,
                                         const double* vf_xx, const int32_t* list, int64_t count, const int32_t* active,
                                         int shared_hessian, double* l, double* L, int64_t batch, int T, int n, int m,
                                         void* stream) {
    int rc;
    if (sweep_prologue(&rc, "zm_ilqr_backward_list_f64", "zm_ilqr_backward_f64", list, count,
                       f_x && f_u && c_x && c_u && c_xx && c_ux && c_uu && vf_x && vf_xx && l && L, batch, T, n, m, true))
        return rc;
    const zm::TrajList tl{(const int*)list, (long)count};
    if (n > 12 || m > 4)   // large states: fp64 MFMA tile sweep (sweep_tiled_f64.hip)
        return zm::sweep_tiled_f64_dispatch(0, f_x, f_u, c_x, c_u, c_xx, c_ux, c_uu, vf_x, vf_xx, nullptr, (long)n, (long)n * n,
                                            (const int*)active, shared_hessian ? 1 : 0, l, L, batch, T, n, m, (hipStream_t)stream,
                                            (const int*)list, (long)count);
    if (zm::ilqr_backward_dma_dispatch<0>(f_x, f_u, c_x, c_u, c_xx, c_ux, c_uu, vf_x, vf_xx, nullptr, (long)n, (long)n * n,
                                       (const int*)active, shared_hessian ? 1 : 0, l, L, batch, T, n, m,
                                       (hipStream_t)stream, tl) == ZM_OK)
        return ZM_OK;
    return zm::launch_ilqr<0>(f_x, f_u, c_x, c_u, c_xx, c_ux, c_uu, vf_x, vf_xx, nullptr, (long)n, (long)n * n,
                              (const int*)active, shared_hessian ? 1 : 0, l, L, batch, T, n, m, (hipStream_t)stream,
                              zm::DdpTensors{nullptr, nullptr, nullptr}, zm::ValueIO{nullptr, nullptr, nullptr, nullptr, nullptr}, tl);
}

// Extension; the reference has no counterpart: the iLQR backward pass with input bounds (control-limited DDP).
extern "C" int zm_ilqr_backward_box_list_f64(const double* f_x, const double* f_u, const double* c_x, const double* c_u,
                                             const double* c_xx, const double* c_ux, const double* c_uu, const double* vf_x,
                                             const double* vf_xx, const double* uTraj, const zm_inputbox_t* box, const int32_t* list,
                                             int64_t count, const int32_t* active, int shared_hessian, double* l, double* L,
                                             int32_t* qp_capped, int64_t batch, int T, int n, int m, void* stream) {
    const char* who = "zm_ilqr_backward_box_f64";
    int rc;
    if (sweep_prologue(&rc, who, who, list, count, f_x && f_u && c_x && c_u && c_xx && c_ux && c_uu && vf_x && vf_xx && uTraj && l && L,
                       batch, T, n, m))
        return rc;
    if (const int rb = zm::box_check(box, m, T, who)) return rb;
    const zm::TrajList tl{(const int*)list, (long)count};
    const dim3 grid((unsigned)(tl.list ? tl.count : batch)), block(64);
    hipStream_t st = (hipStream_t)stream;
    const int sh = shared_hessian ? 1 : 0;
    zm::with_ks(n, [&](auto ks) {
        if (box->step_stride != 0)
            hipLaunchKernelGGL((zm::ilqr_backward_box_t16_f64<decltype(ks)::value, true>), grid, block, 0, st, f_x, f_u, c_x, c_u, c_xx,
                               c_ux, c_uu, vf_x, vf_xx, uTraj, box->lb, box->ub, (long)box->stride, (long)n,
                               (long)n * n, (const int*)active, sh, l, L, (int*)qp_capped, T, n, m, tl);
        else
            hipLaunchKernelGGL((zm::ilqr_backward_box_t16_f64<decltype(ks)::value, false>), grid, block, 0, st, f_x, f_u, c_x, c_u, c_xx,
                               c_ux, c_uu, vf_x, vf_xx, uTraj, box->lb, box->ub, (long)box->stride, (long)n, (long)n * n,
                               (const int*)active, sh, l, L, (int*)qp_capped, T, n, m, tl);
    });
    ZM_HIP_CHECK(hipGetLastError());
    return ZM_OK;
}

extern "C" int zm_ilqr_backward_box_f64(const double* f_x, const double* f_u, const double* c_x, const double* c_u,
                                        const double* c_xx, const double* c_ux, const double* c_uu, const double* vf_x,
                                        const double* vf_xx, const double* uTraj, const zm_inputbox_t* box, int shared_hessian,
                                        double* l, double* L, int32_t* qp_capped, int64_t batch, int T, int n, int m, void* stream) {
    return zm_ilqr_backward_box_list_f64(f_x, f_u, c_x, c_u, c_xx, c_ux, c_uu, vf_x, vf_xx, uTraj, box, nullptr, 0, nullptr,
                                         shared_hessian, l, L, qp_capped, batch, T, n, m, stream);
}

// Extension; the reference has no counterpart: the iLQR backward pass on the cost Hessians c_xx + diag h_k, v_xx + diag h_T (the
// augmented-Lagrangian penalty of a state box), without (box == uTraj == NULL) or with input bounds.  Register path only.
extern "C" int zm_ilqr_backward_state_list_f64(const double* f_x, const double* f_u, const double* c_x, const double* c_u,
                                               const double* c_xx, const double* c_ux, const double* c_uu, const double* vf_x,
                                               const double* vf_xx, const double* h, const double* uTraj, const zm_inputbox_t* box,
                                               const int32_t* list, int64_t count, const int32_t* active, int shared_hessian, double* l,
                                               double* L, int32_t* qp_capped, int64_t batch, int T, int n, int m, void* stream) {
    const char* who = "zm_ilqr_backward_state_f64";
    int rc;
    if (sweep_prologue(&rc, who, who, list, count, f_x && f_u && c_x && c_u && c_xx && c_ux && c_uu && vf_x && vf_xx && h && l && L, batch,
                       T, n, m))
        return rc;
    if ((box != nullptr) != (uTraj != nullptr)) return zm::set_error(ZM_EINVAL, "%s: box and uTraj go together (both or neither)", who);
    if (box)
        if (const int rb = zm::box_check_constant(box, m, T, who)) return rb;
    const zm::TrajList tl{(const int*)list, (long)count};
    const dim3 grid((unsigned)(tl.list ? tl.count : batch)), block(64);
    hipStream_t st = (hipStream_t)stream;
    const int sh = shared_hessian ? 1 : 0;
    zm::with_ks(n, [&](auto ks) {
        if (box)
            hipLaunchKernelGGL((zm::ilqr_backward_box_pen_t16_f64<decltype(ks)::value>), grid, block, 0, st, f_x, f_u, c_x, c_u, c_xx, c_ux,
                               c_uu, vf_x, vf_xx, h, uTraj, box->lb, box->ub, (long)box->stride, (long)n, (long)n * n, (const int*)active,
                               sh, l, L, (int*)qp_capped, T, n, m, tl);
        else
            hipLaunchKernelGGL((zm::ilqr_backward_pen_t16_f64<decltype(ks)::value>), grid, block, 0, st, f_x, f_u, c_x, c_u, c_xx, c_ux,
                               c_uu, vf_x, vf_xx, h, (long)n, (long)n * n, (const int*)active, sh, l, L, T, n, m, tl);
    });
    ZM_HIP_CHECK(hipGetLastError());
    return ZM_OK;
}

extern "C" int zm_ilqr_backward_state_f64(const double* f_x, const double* f_u, const double* c_x, const double* c_u,
                                          const double* c_xx, const double* c_ux, const double* c_uu, const double* vf_x,
                                          const double* vf_xx, const double* h, const double* uTraj, const zm_inputbox_t* box,
                                          int shared_hessian, double* l, double* L, int32_t* qp_capped, int64_t batch, int T, int n, int m,
                                          void* stream) {
    return zm_ilqr_backward_state_list_f64(f_x, f_u, c_x, c_u, c_xx, c_ux, c_uu, vf_x, vf_xx, h, uTraj, box, nullptr, 0, nullptr,
                                           shared_hessian, l, L, qp_capped, batch, T, n, m, stream);
}

extern "C" int zm_boxqp_f64(const double* H, const double* g, const double* lo, const double* hi, double* d_out, int32_t* clamped_out,
                            int32_t* iters_out, int64_t batch, int m, void* stream) {
    if (batch == 0) return ZM_OK;
    if (!H || !g || !lo || !hi || !d_out) return zm::set_error(ZM_EINVAL, "zm_boxqp_f64: null pointer");
    if (batch < 0 || m < 1) return zm::set_error(ZM_EINVAL, "zm_boxqp_f64: bad size batch=%lld m=%d", (long long)batch, m);
    if (m > 4) return zm::set_error(ZM_EUNSUPPORTED, "zm_boxqp_f64: m=%d not covered (need m<=4)", m);
    hipLaunchKernelGGL(zm::boxqp_kernel, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, (hipStream_t)stream, H, g, lo, hi, d_out,
                       (int*)clamped_out, (int*)iters_out, (long)batch, m);
    ZM_HIP_CHECK(hipGetLastError());
    return ZM_OK;
}

extern "C" int zm_ilqr_backward_ex_f64(const double* f_x, const double* f_u, const double* c_x, const double* c_u,
                                       const double* c_xx, const double* c_ux, const double* c_uu, const double* vf_x,
                                       const double* vf_xx, const int32_t* active, int shared_hessian, double* l,
                                       double* L, int64_t batch, int T, int n, int m, void* stream) {
    return zm_ilqr_backward_list_f64(f_x, f_u, c_x, c_u, c_xx, c_ux, c_uu, vf_x, vf_xx, nullptr, 0, active, shared_hessian, l, L,
                                     batch, T, n, m, stream);
}

extern "C" int zm_ilqr_backward_f64(const double* f_x, const double* f_u, const double* c_x, const double* c_u,
                                    const double* c_xx, const double* c_ux, const double* c_uu, const double* vf_x,
                                    const double* vf_xx, double* l, double* L, int64_t batch, int T, int n, int m,
                                    void* stream) {
    if (batch == 0) return ZM_OK;   /* empty batch: nothing to do (pointers of empty arrays may be NULL) */
    return zm_ilqr_backward_ex_f64(f_x, f_u, c_x, c_u, c_xx, c_ux, c_uu, vf_x, vf_xx, nullptr, 0, l, L, batch, T, n, m,
                                   stream);
}

extern "C" int zm_lqr_backward_affine_f64(const double* A, const double* B, const double* d, const double* Q,
                                          const double* R, const double* H, const double* q, const double* r, double* L,
                                          double* l, int64_t batch, int T, int n, int m, void* stream) {
    if (batch == 0) return ZM_OK;   /* empty batch: nothing to do (pointers of empty arrays may be NULL) */
    if (!A || !B || !d || !Q || !R || !H || !q || !r || !L || !l)
        return zm::set_error(ZM_EINVAL, "zm_lqr_backward_affine_f64: null pointer");
    if (const int rc = zm_check_sweep_args("zm_lqr_backward_affine_f64", batch, T, n, m, true)) return rc;
    // carry (V, v) <- (Q[T-1], q[T-1])   (lqrUtils.py:261): terminal pointers into the last step, trajectory stride T*size
    const double* vf_xx = Q + (int64_t)(T - 1) * n * n;
    const double* vf_x = q + (int64_t)(T - 1) * n;
    if (n > 12 || m > 4)   // large states: fp64 MFMA tile sweep (sweep_tiled_f64.hip)
        return zm::sweep_tiled_f64_dispatch(1, A, B, q, r, Q, H, R, vf_x, vf_xx, d, (long)T * n, (long)T * n * n, nullptr, 0, l, L, batch,
                                            T, n, m, (hipStream_t)stream, nullptr, 0);
    if (zm::ilqr_backward_dma_dispatch<1>(A, B, q, r, Q, H, R, vf_x, vf_xx, d, (long)T * n, (long)T * n * n, nullptr, 0, l, L,
                                          batch, T, n, m, (hipStream_t)stream) == ZM_OK)
        return ZM_OK;
    return zm::launch_ilqr<1>(A, B, q, r, Q, H, R, vf_x, vf_xx, d, (long)T * n, (long)T * n * n, nullptr, 0, l, L, batch, T,
                              n, m, (hipStream_t)stream);
}

extern "C" int zm_ddp_backward_list_f64(const double* f_x, const double* f_u, const double* f_xx, const double* f_ux,
                                        const double* f_uu, const double* c_x, const double* c_u, const double* c_xx,
                                        const double* c_ux, const double* c_uu, const double* vf_x, const double* vf_xx,
                                        const int32_t* list, int64_t count, const int32_t* active, int shared_hessian,
                                        double* l, double* L, int64_t batch, int T, int n, int m, void* stream) {
    int rc;
    if (sweep_prologue(&rc, "zm_ddp_backward_list_f64", "zm_ddp_backward_f64", list, count,
                       f_x && f_u && f_xx && (!f_ux == !f_uu) && c_x && c_u && c_xx && c_ux && c_uu && vf_x && vf_xx && l && L, batch, T, n, m,
                       false, ZM_DDP_NULL_NOTE))
        return rc;
    if ((int64_t)n * n * n >= (int64_t)1 << 31) return zm::set_error(ZM_EUNSUPPORTED, "zm_ddp_backward_f64: n too large");
    return zm::launch_ilqr<2>(f_x, f_u, c_x, c_u, c_xx, c_ux, c_uu, vf_x, vf_xx, nullptr, (long)n, (long)n * n,
                              (const int*)active, shared_hessian ? 1 : 0, l, L, batch, T, n, m, (hipStream_t)stream,
                              zm::DdpTensors{f_xx, f_ux, f_uu}, zm::ValueIO{nullptr, nullptr, nullptr, nullptr, nullptr},
                              zm::TrajList{(const int*)list, (long)count});
}

extern "C" int zm_ddp_backward_pairs_list_f64(const zm_model_t* model, const double* f_x, const double* f_u, const double* H,
                                              const double* c_x, const double* c_u, const double* c_xx, const double* c_ux,
                                              const double* c_uu, const double* vf_x, const double* vf_xx, const int32_t* list,
                                              int64_t count, const int32_t* active, int shared_hessian, double* l, double* L,
                                              int64_t batch, int T, void* stream) {
    const char* who = "zm_ddp_backward_pairs_list_f64";
    const int n = model ? model->n : 0, m = model ? model->m : 0;
    int rc;
    if (sweep_prologue(&rc, who, who, list, count, model && f_x && f_u && H && c_x && c_u && c_xx && c_ux && c_uu && vf_x && vf_xx && l && L,
                       batch, T, n, m))
        return rc;
    const zm::PairTab pt = zm::model_pair_table(model->kind);
    if (pt.n < 1) return zm::set_error(ZM_EUNSUPPORTED, "%s: the model declares no Hessian pairs", who);
    const zm::TrajList tl{(const int*)list, (long)count};
    {   // the LDS-ring kernel where it applies (quadcopter shapes, shared cost Hessians); the register kernel otherwise
        const int rd = zm::ddp_backward_dma_dispatch(f_x, f_u, H, pt, c_x, c_u, c_xx, c_ux, c_uu, vf_x, vf_xx, (long)n, (const int*)active,
                                                     shared_hessian ? 1 : 0, l, L, batch, T, n, m, (hipStream_t)stream, tl);
        if (rd != ZM_EUNSUPPORTED) return rd;
    }
    zm::DdpTensors z{nullptr, nullptr, nullptr, H, pt};
    return zm::launch_ilqr<2>(f_x, f_u, c_x, c_u, c_xx, c_ux, c_uu, vf_x, vf_xx, nullptr, (long)n, (long)n * n, (const int*)active,
                              shared_hessian ? 1 : 0, l, L, batch, T, n, m, (hipStream_t)stream, z,
                              zm::ValueIO{nullptr, nullptr, nullptr, nullptr, nullptr}, tl);
}

// Extension; the reference has no counterpart: the DDP backward pass with input bounds (control-limited DDP with its second-order
// dynamics terms).  One launcher behind the tensor and the pairs entries; every check has run before it.
static int launch_ddp_box(const double* f_x, const double* f_u, const zm::DdpTensors& z, const double* c_x,
                          const double* c_u, const double* c_xx, const double* c_ux, const double* c_uu, const double* vf_x,
                          const double* vf_xx, const double* uTraj, const zm_inputbox_t* box, const zm::TrajList tl, const int32_t* active,
                          int shared_hessian, double* l, double* L, int32_t* qp_capped, int64_t batch, int T, int n, int m, void* stream) {
    const dim3 grid((unsigned)(tl.list ? tl.count : batch)), block(64);
    hipStream_t st = (hipStream_t)stream;
    const int sh = shared_hessian ? 1 : 0;
    zm::with_ks(n, [&](auto ks) {
        if (box->step_stride != 0)
            hipLaunchKernelGGL((zm::ddp_backward_box_t16_f64<decltype(ks)::value, true>), grid, block, 0, st, f_x, f_u, c_x, c_u, c_xx,
                               c_ux, c_uu, vf_x, vf_xx, uTraj, box->lb, box->ub, (long)box->stride, z.f_xx, z.f_ux,
                               z.f_uu, (long)n, (long)n * n, (const int*)active, sh, l, L, (int*)qp_capped, T, n, m, tl, z.Hpk, z.ptab);
        else
            hipLaunchKernelGGL((zm::ddp_backward_box_t16_f64<decltype(ks)::value, false>), grid, block, 0, st, f_x, f_u, c_x, c_u, c_xx,
                               c_ux, c_uu, vf_x, vf_xx, uTraj, box->lb, box->ub, (long)box->stride, z.f_xx, z.f_ux, z.f_uu, (long)n,
                               (long)n * n, (const int*)active, sh, l, L, (int*)qp_capped, T, n, m, tl, z.Hpk, z.ptab);
    });
    ZM_HIP_CHECK(hipGetLastError());
    return ZM_OK;
}

extern "C" int zm_ddp_backward_box_list_f64(const double* f_x, const double* f_u, const double* f_xx, const double* f_ux,
                                            const double* f_uu, const double* c_x, const double* c_u, const double* c_xx,
                                            const double* c_ux, const double* c_uu, const double* vf_x, const double* vf_xx,
                                            const double* uTraj, const zm_inputbox_t* box, const int32_t* list, int64_t count,
                                            const int32_t* active, int shared_hessian, double* l, double* L, int32_t* qp_capped,
                                            int64_t batch, int T, int n, int m, void* stream) {
    const char* who = "zm_ddp_backward_box_list_f64";
    int rc;
    if (sweep_prologue(&rc, who, who, list, count,
                       f_x && f_u && f_xx && (!f_ux == !f_uu) && c_x && c_u && c_xx && c_ux && c_uu && vf_x && vf_xx && uTraj && l && L, batch,
                       T, n, m, false, ZM_DDP_NULL_NOTE))
        return rc;
    if ((int64_t)n * n * n >= (int64_t)1 << 31) return zm::set_error(ZM_EUNSUPPORTED, "%s: n too large", who);
    if (const int rb = zm::box_check(box, m, T, who)) return rb;
    return launch_ddp_box(f_x, f_u, zm::DdpTensors{f_xx, f_ux, f_uu}, c_x, c_u, c_xx, c_ux, c_uu, vf_x, vf_xx,
                          uTraj, box, zm::TrajList{(const int*)list, (long)count}, active, shared_hessian, l, L, qp_capped, batch, T, n,
                          m, stream);
}

extern "C" int zm_ddp_backward_box_f64(const double* f_x, const double* f_u, const double* f_xx, const double* f_ux,
                                       const double* f_uu, const double* c_x, const double* c_u, const double* c_xx,
                                       const double* c_ux, const double* c_uu, const double* vf_x, const double* vf_xx,
                                       const double* uTraj, const zm_inputbox_t* box, int shared_hessian, double* l, double* L,
                                       int32_t* qp_capped, int64_t batch, int T, int n, int m, void* stream) {
    return zm_ddp_backward_box_list_f64(f_x, f_u, f_xx, f_ux, f_uu, c_x, c_u, c_xx, c_ux, c_uu, vf_x, vf_xx, uTraj, box, nullptr, 0,
                                        nullptr, shared_hessian, l, L, qp_capped, batch, T, n, m, stream);
}

extern "C" int zm_ddp_backward_pairs_box_list_f64(const zm_model_t* model, const double* f_x, const double* f_u, const double* H,
                                                  const double* c_x, const double* c_u, const double* c_xx, const double* c_ux,
                                                  const double* c_uu, const double* vf_x, const double* vf_xx, const double* uTraj,
                                                  const zm_inputbox_t* box, const int32_t* list, int64_t count, const int32_t* active,
                                                  int shared_hessian, double* l, double* L, int32_t* qp_capped, int64_t batch, int T,
                                                  void* stream) {
    const char* who = "zm_ddp_backward_pairs_box_list_f64";
    const int n = model ? model->n : 0, m = model ? model->m : 0;
    int rc;
    if (sweep_prologue(&rc, who, who, list, count,
                       model && f_x && f_u && H && c_x && c_u && c_xx && c_ux && c_uu && vf_x && vf_xx && uTraj && l && L, batch, T, n, m))
        return rc;
    const zm::PairTab pt = zm::model_pair_table(model->kind);
    if (pt.n < 1) return zm::set_error(ZM_EUNSUPPORTED, "%s: the model declares no Hessian pairs", who);
    if (const int rb = zm::box_check(box, m, T, who)) return rb;
    return launch_ddp_box(f_x, f_u, zm::DdpTensors{nullptr, nullptr, nullptr, H, pt}, c_x, c_u,
                          c_xx, c_ux, c_uu, vf_x, vf_xx, uTraj, box, zm::TrajList{(const int*)list, (long)count}, active,
                          shared_hessian, l, L, qp_capped, batch, T, n, m, stream);
}

extern "C" int zm_ddp_backward_f64(const double* f_x, const double* f_u, const double* f_xx, const double* f_ux,
                                   const double* f_uu, const double* c_x, const double* c_u, const double* c_xx,
                                   const double* c_ux, const double* c_uu, const double* vf_x, const double* vf_xx,
                                   const int32_t* active, int shared_hessian, double* l, double* L, int64_t batch, int T,
                                   int n, int m, void* stream) {
    return zm_ddp_backward_list_f64(f_x, f_u, f_xx, f_ux, f_uu, c_x, c_u, c_xx, c_ux, c_uu, vf_x, vf_xx, nullptr, 0, active,
                                    shared_hessian, l, L, batch, T, n, m, stream);
}

extern "C" int zm_riccati_value_f64(const double* f_x, const double* f_u, const double* f_xx, const double* f_ux,
                                    const double* f_uu, const double* c, const double* c_x, const double* c_u,
                                    const double* c_xx, const double* c_ux, const double* c_uu, const double* vf,
                                    const double* vf_x, const double* vf_xx, double* l, double* L, double* v_out,
                                    double* vx_out, double* vxx_out, int64_t batch, int T, int n, int m, void* stream) {
    if (batch == 0) return ZM_OK;   /* empty batch: nothing to do (pointers of empty arrays may be NULL) */
    if (!f_x || !f_u || !c_x || !c_u || !c_xx || !c_ux || !c_uu || !vf_x || !vf_xx || !l || !L)
        return zm::set_error(ZM_EINVAL, "zm_riccati_value_f64: null pointer");
    const bool ddp = f_xx || f_ux || f_uu;
    if (ddp && (!f_xx || (!f_ux != !f_uu)))
        return zm::set_error(ZM_EINVAL, "zm_riccati_value_f64: f_xx goes with f_ux and f_uu (the latter two may be NULL together: zero)");
    const int rc = zm_check_sweep_args("zm_riccati_value_f64", batch, T, n, m, !ddp);
    if (rc) return rc;
    if (!ddp && (n > 12 || m > 4)) {   // large states: the tile sweep with its value-function outputs (sweep_tiled_f64.hip)
        if (!v_out || !vx_out || !vxx_out) return zm::set_error(ZM_EINVAL, "zm_riccati_value_f64: the value outputs are required at n > 12 or m > 4");
        return zm::sweep_tiled_f64_dispatch(0, f_x, f_u, c_x, c_u, c_xx, c_ux, c_uu, vf_x, vf_xx, nullptr, (long)n, (long)n * n, nullptr, 0,
                                            l, L, batch, T, n, m, (hipStream_t)stream, nullptr, 0, c, vf, v_out, vx_out, vxx_out);
    }
    const zm::ValueIO v{c, vf, v_out, vx_out, vxx_out};
    if (ddp)
        return zm::launch_ilqr<2>(f_x, f_u, c_x, c_u, c_xx, c_ux, c_uu, vf_x, vf_xx, nullptr, (long)n, (long)n * n, nullptr, 0, l,
                                  L, batch, T, n, m, (hipStream_t)stream, zm::DdpTensors{f_xx, f_ux, f_uu}, v);
    return zm::launch_ilqr<0>(f_x, f_u, c_x, c_u, c_xx, c_ux, c_uu, vf_x, vf_xx, nullptr, (long)n, (long)n * n, nullptr, 0, l, L,
                              batch, T, n, m, (hipStream_t)stream, zm::DdpTensors{nullptr, nullptr, nullptr}, v);
}

#ifdef ZM_SWEEP_LAB
extern "C" int zm_lab_sweep_stamps(unsigned long long* out, int reset) {
    ZM_HIP_CHECK(hipDeviceSynchronize());
    ZM_HIP_CHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(zm::zm_sweep_stamps), sizeof(unsigned long long) * 10));
    if (reset) {
        unsigned long long z[10] = {0};
        ZM_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(zm::zm_sweep_stamps), z, sizeof(z)));
    }
    return ZM_OK;
}
#endif
