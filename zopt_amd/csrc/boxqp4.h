// Box-constrained QP in at most four unknowns, on registers (the backward step of control-limited DDP: Tassa, Mansard, Todorov 2014).
//
//     d = argmin  1/2 d^T sym(H) d + g^T d      subject to      lo <= d <= hi                (H positive definite: the minimiser is unique)
//
// Extension; the reference has no counterpart (its backward pass solves the unconstrained system, ilqrUtils.py:167-168).
//
// Method: the primal active-set iteration.  d starts at clip(0, lo, hi), its clamped set at the components that sit on a bound with
// the gradient pushing outward.  Every pass solves the 4 x 4 system whose clamped rows and columns are the identity's (so the sweep's
// lu_solve4_nopivot / lu_solve4 serve), then either
//   * the solution y is feasible: d <- y; a clamped component whose multiplier has the wrong sign is released (the largest one),
//     and if there is none d is the minimiser; or
//   * it is not: d moves along y - d up to the first bound it meets, and that component joins the clamped set.
// The cost never increases and d is feasible after every pass.  Everything is unrolled over the four components with selects, the
// sets are bit masks: no runtime-indexed array, nothing goes to scratch.  The sweep kernel runs it wave-uniform (every lane on the
// same numbers), the test entry zm_boxqp_f64 one problem per lane.  At most BOXQP_CAP passes: inputs with a NaN end after one (every
// comparison is false, nothing is blocked, nothing is released) and return NaN.  lo == hi fixes a component: it is clamped and never
// released.  Components with lo = -inf, hi = +inf (also the padding beyond m: identity row, zero gradient) are never clamped.
#pragma once
#include "input_box.h"
#include "tile16_f64.h"

namespace zm {

constexpr int BOXQP_CAP = 24;

// S <- H with the rows and columns of the components in `mask` replaced by the identity's
__device__ __forceinline__ void boxqp_mask(double (&S)[4][4], const double (&H)[4][4], const int mask) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool cl = (((mask >> i) | (mask >> j)) & 1) != 0;
            S[i][j] = cl ? (i == j ? 1.0 : 0.0) : H[i][j];
        }
    }
}

// returns the number of passes; `clamped`: bit i set where d[i] sits on a bound with a multiplier of the right sign; `capped`: the
// cap was reached (d is then the last feasible iterate, clamped the set it was computed with)
__device__ __forceinline__ int boxqp4(const double (&Hin)[4][4], const double (&g)[4], const double (&lo)[4], const double (&hi)[4],
                                      double (&d)[4], int& clamped, bool& capped) {
    double H[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) H[i][j] = (i == j) ? Hin[i][i] : 0.5 * (Hin[i][j] + Hin[j][i]);
    }
    int atlo = 0, athi = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) d[i] = clip_nan(0.0, lo[i], hi[i]);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double gr = g[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) gr = __builtin_fma(H[i][j], d[j], gr);
        const bool fixed = lo[i] == hi[i];
        const bool l = d[i] == lo[i] && (gr > 0.0 || fixed);
        const bool h = !l && d[i] == hi[i] && gr < 0.0;
        atlo |= l ? (1 << i) : 0;
        athi |= h ? (1 << i) : 0;
    }
    int it = 0;
    bool done = false;
    for (; it < BOXQP_CAP && !done; ++it) {
        const int cm = atlo | athi;
        double S[4][4], b[4], y[4];
        boxqp_mask(S, H, cm);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            double r = g[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) r = ((cm >> j) & 1) ? __builtin_fma(H[i][j], d[j], r) : r;
            b[i] = ((cm >> i) & 1) ? d[i] : -r;
        }
        if (!lu_solve4_nopivot(S, b, y)) lu_solve4_fallback(S, b, y);
        bool blocked = false;
        double tmin = __builtin_inf(), bnd = 0.0;
        int blk = 0;
        bool blow = false;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            y[i] = ((cm >> i) & 1) ? d[i] : y[i];   // (a NaN elsewhere reaches the identity rows through 0 * NaN)
            const bool below = !((cm >> i) & 1) && y[i] < lo[i], above = !((cm >> i) & 1) && y[i] > hi[i];
            const double bi = below ? lo[i] : hi[i];
            const double ti = (bi - d[i]) / (y[i] - d[i]);
            const bool first = (below || above) && (ti < tmin || !blocked);
            tmin = first ? ti : tmin;
            bnd = first ? bi : bnd;
            blk = first ? i : blk;
            blow = first ? below : blow;
            blocked |= below || above;
        }
        if (!blocked) {
            double worst = 0.0;
            int rel = -1;
#pragma unroll
            for (int i = 0; i < 4; ++i) d[i] = y[i];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                double gr = g[i];
#pragma unroll
                for (int j = 0; j < 4; ++j) gr = __builtin_fma(H[i][j], d[j], gr);
                const bool fixed = lo[i] == hi[i];
                const bool wrong = !fixed && ((((atlo >> i) & 1) && gr < 0.0) || (((athi >> i) & 1) && gr > 0.0));
                const double mag = __builtin_fabs(gr);
                const bool take = wrong && (rel < 0 || mag > worst);
                worst = take ? mag : worst;
                rel = take ? i : rel;
            }
            if (rel < 0) {
                done = true;
            } else {
                atlo &= ~(1 << rel);
                athi &= ~(1 << rel);
            }
        } else {
            const double t = tmin < 0.0 ? 0.0 : (tmin > 1.0 ? 1.0 : tmin);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const double moved = clip_nan(__builtin_fma(t, y[i] - d[i], d[i]), lo[i], hi[i]);
                d[i] = (i == blk) ? bnd : (((cm >> i) & 1) ? d[i] : moved);
            }
            atlo |= blow ? (1 << blk) : 0;
            athi |= blow ? 0 : (1 << blk);
        }
    }
    clamped = atlo | athi;
    capped = !done;
    return it;
}

}  // namespace zm
