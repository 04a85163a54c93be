// Body of the lane-per-instance MPC solve kernel (mpc.hip).
// A function BODY, not a header: #included verbatim inside mpc_solve_kernel and mpc_solve_batched_kernel (mpc.hip), so that the
// kernel that existed before the per-problem variant compiles from the very same tokens (same ISA; tools/isa_identity.py checks
// it).  The per-problem kernel reaches it with its parameters already offset to its problem (see there).
// The ZM_TRK_* hooks are the reference-tracking variant (mpc.hip: mpc_solve_track_kernel); they expand to nothing in the kernels
// without a reference.
    constexpr int W = NS + MC;
    const long inst = (long)blockIdx.x * 64 + threadIdx.x;
    // Lanes beyond the batch leave at once: the sweeps below store unconditionally (no branch per store), so no lane may
    // alias another instance's slots; the wave-level votes (__all / __any) only count the lanes that are still here.
    if (inst >= g.batch) return;
    constexpr bool live = true;
    const long ii = inst;
    const long bt = g.batch;
    const int N = g.N;
    const double rho = g.rho;
    // workspace, batch-minor: y[k][i][inst], lam[k][i][inst], kf[k][j][inst] (+ spare), rv[k][i][inst]
    double* y = g.ws;
    double* lam = g.ws + (long)N * W * bt;
    double* kf = g.ws + 2L * N * W * bt;
    double* rv = g.ws + 3L * N * W * bt;

    double x0[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) x0[i] = g.x0[ii * NS + i];
    bool x0_ok = true;
#pragma unroll
    for (int i = 0; i < NS; ++i) x0_ok &= (x0[i] >= x_lb[i]) && (x0[i] <= x_ub[i]);  // x_0 = x0 is box-constrained too (:56,:58)

    // warm start is per instance: only iterates of a solve that ended "optimal" are reused (the flag lives in the spare
    // part of the kf block); an instance that was infeasible / hit the limit last time starts cold
    double* okflag = g.ws + 2L * N * W * bt + (long)N * MC * bt;
    const bool lane_warm = g.warm && okflag[ii] == 1.0;
    for (int k = 0; k < N; ++k) {
#pragma unroll
        for (int i = 0; i < W; ++i) {
            if (!lane_warm) {
                y[((long)k * W + i) * bt + ii] = 0.0;
                lam[((long)k * W + i) * bt + ii] = 0.0;
            } else if (g.warm == 2 && k + 1 < N) {   // receding horizon: the old plan advanced by one step (tail repeated)
                y[((long)k * W + i) * bt + ii] = y[((long)(k + 1) * W + i) * bt + ii];
                lam[((long)k * W + i) * bt + ii] = lam[((long)(k + 1) * W + i) * bt + ii];
            }
            rv[((long)k * W + i) * bt + ii] = 0.0;
        }
#pragma unroll
        for (int j = 0; j < MC; ++j) kf[((long)k * MC + j) * bt + ii] = 0.0;
    }

    ZM_TRK_SETUP
    int status = x0_ok ? 0 : ZM_MPC_INFEASIBLE;
    int it = 0;  // this lane's ADMM iterations
    double rp = 0.0, rd = 0.0;
    bool near_ok = false;   // the last iterate's residuals are within 10x the tolerances (OSQP's "solved inaccurate" test at the cap)
    bool done = !live || status != 0;
    for (int gi = 0; gi < g.max_iter; ++gi) {  // gi is wave-uniform
        if (__all(done)) break;
        const bool chk = ((gi + 1) % ZM_MPC_CHK) == 0;  // infeasibility certificate on this iteration
        // ---- backward affine sweep.  Costate of x_{k+1}: p = -rho z(x_{k+1}) + (A^T p - K^T Qu)_{k+1};
        //      Qu = -rho z(u_k) + B^T p;  kf_k = Suu_k^-1 Qu.  Stage k touches only block k of (y, lam) (its states are the copy
        //      of x_{k+1}), and block k-1 is fetched while stage k computes: no load is predicated, no store is conditional
        //      (a finished lane rewrites the values it read), so the loop has no branch and one memory latency
        //      per stage is hidden behind ~500 FMAs.
        double p[NS];
#pragma unroll
        for (int i = 0; i < NS; ++i) p[i] = 0.0;
        double yb[W], lb[W];
#pragma unroll
        for (int i = 0; i < W; ++i) {
            const long e = ((long)(N - 1) * W + i) * bt + ii;
            yb[i] = y[e];
            lb[i] = lam[e];
        }
        ZM_TRK_FIRST
#pragma unroll 1
        for (int k = N - 1; k >= 0; --k) {
            const double* Kk = Ktab + (long)k * MC * NS;
            const double* Mk = Mtab + (long)k * MC * MC;
            double yq[W], lq[W], kfo[MC];
            {
                const int kp = k > 0 ? k - 1 : 0;
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    const long e = ((long)kp * W + i) * bt + ii;
                    yq[i] = y[e];
                    lq[i] = lam[e];
                }
#pragma unroll
                for (int j = 0; j < MC; ++j) kfo[j] = kf[((long)k * MC + j) * bt + ii];
            }
            ZM_TRK_PREFETCH(k)
#pragma unroll
            for (int i = 0; i < NS; ++i) p[i] = __builtin_fma(-rho, yb[i] - lb[i], p[i]);
            ZM_TRK_PX
            double qu[MC];
#pragma unroll
            for (int j = 0; j < MC; ++j) {
                double sacc = -rho * (yb[NS + j] - lb[NS + j]) ZM_TRK_QU(j);
#pragma unroll
                for (int i = 0; i < NS; ++i) sacc = __builtin_fma(B[i * MC + j], p[i], sacc);
                qu[j] = sacc;
            }
#pragma unroll
            for (int j = 0; j < MC; ++j) {
                double sacc = 0.0;
#pragma unroll
                for (int l = 0; l < MC; ++l) sacc = __builtin_fma(Mk[j * MC + l], qu[l], sacc);
                kf[((long)k * MC + j) * bt + ii] = done ? kfo[j] : sacc;   // a finished lane keeps the kf of its last iterate
            }
            double pn[NS];
#pragma unroll
            for (int i = 0; i < NS; ++i) {
                double sacc = 0.0;
#pragma unroll
                for (int l = 0; l < NS; ++l) sacc = __builtin_fma(A[l * NS + i], p[l], sacc);
#pragma unroll
                for (int j = 0; j < MC; ++j) sacc = __builtin_fma(-Kk[j * NS + i], qu[j], sacc);
                pn[i] = sacc;
            }
#pragma unroll
            for (int i = 0; i < NS; ++i) p[i] = pn[i];
#pragma unroll
            for (int i = 0; i < W; ++i) {
                yb[i] = yq[i];
                lb[i] = lq[i];
            }
            ZM_TRK_ROTATE
        }
        // ---- forward rollout w, projection y, dual update lam, residual norms (and r = w - y, support function on chk)
        double x[NS];
#pragma unroll
        for (int i = 0; i < NS; ++i) x[i] = x0[i];
        double nrp = 0.0, nrd = 0.0, nw = 0.0, ny = 0.0, nl = 0.0, sup = 0.0, ndl = 0.0;
        auto forward = [&](auto chk_c) {
            constexpr bool CHK = decltype(chk_c)::value;
            double kfc[MC];
#pragma unroll
            for (int i = 0; i < W; ++i) {
                const long e = (long)i * bt + ii;
                yb[i] = y[e];
                lb[i] = lam[e];
            }
#pragma unroll
            for (int j = 0; j < MC; ++j) kfc[j] = kf[(long)j * bt + ii];
#pragma unroll 1
            for (int k = 0; k < N; ++k) {
                const double* Kk = Ktab + (long)k * MC * NS;
                double yq[W], lq[W], kfq[MC];
                {
                    const int kn = k + 1 < N ? k + 1 : N - 1;
#pragma unroll
                    for (int i = 0; i < W; ++i) {
                        const long e = ((long)kn * W + i) * bt + ii;
                        yq[i] = y[e];
                        lq[i] = lam[e];
                    }
#pragma unroll
                    for (int j = 0; j < MC; ++j) kfq[j] = kf[((long)kn * MC + j) * bt + ii];
                }
                double u[MC], xn[NS];
#pragma unroll
                for (int j = 0; j < MC; ++j) {
                    double sacc = -kfc[j];
#pragma unroll
                    for (int i = 0; i < NS; ++i) sacc = __builtin_fma(-Kk[j * NS + i], x[i], sacc);
                    u[j] = sacc;
                }
#pragma unroll
                for (int i = 0; i < NS; ++i) {
                    double sacc = 0.0;
#pragma unroll
                    for (int l = 0; l < NS; ++l) sacc = __builtin_fma(A[i * NS + l], x[l], sacc);
#pragma unroll
                    for (int j = 0; j < MC; ++j) sacc = __builtin_fma(B[i * MC + j], u[j], sacc);
                    xn[i] = sacc;
                }
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    const double wv = (i < NS) ? xn[i < NS ? i : 0] : u[i >= NS ? i - NS : 0];
                    const double lo = (i < NS) ? x_lb[i < NS ? i : 0] : u_lb[i >= NS ? i - NS : 0];
                    const double hi = (i < NS) ? x_ub[i < NS ? i : 0] : u_ub[i >= NS ? i - NS : 0];
                    const long e = ((long)k * W + i) * bt + ii;
                    const double lold = lb[i], yold = yb[i];
                    const double wh = __builtin_fma(g.alpha, wv, (1.0 - g.alpha) * yold);   // relaxed iterate (alpha = 1: wv exactly)
                    double yn = wh + lold;
                    yn = yn < lo ? lo : (yn > hi ? hi : yn);
                    const double r = wv - yn, dl = wh - yn;   // primal residual; dual step
                    const double ln = lold + dl;
                    y[e] = done ? yold : yn;       // a finished lane keeps its iterate
                    lam[e] = done ? lold : ln;
                    if constexpr (CHK) {
                        rv[e] = dl;                // only read back by lanes that are not finished
                        sup += (dl > 0.0) ? dl * hi : ((dl < 0.0) ? dl * lo : 0.0);  // support function of the box at v = dl
                        ndl = __builtin_fmax(ndl, __builtin_fabs(dl));
                    }
                    nrp = __builtin_fmax(nrp, __builtin_fabs(r));
                    nrd = __builtin_fmax(nrd, __builtin_fabs(yn - yold));
                    nw = __builtin_fmax(nw, __builtin_fabs(wv));
                    ny = __builtin_fmax(ny, __builtin_fabs(yn));
                    nl = __builtin_fmax(nl, __builtin_fabs(ln));
                }
#pragma unroll
                for (int i = 0; i < NS; ++i) x[i] = xn[i];
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    yb[i] = yq[i];
                    lb[i] = lq[i];
                }
#pragma unroll
                for (int j = 0; j < MC; ++j) kfc[j] = kfq[j];
            }
        };
        if (chk)
            forward(std::true_type{});
        else
            forward(std::false_type{});
        bool need_cert = false;
        if (!done) {
            ++it;
            rp = nrp;
            rd = rho * nrd;
            const double ep = g.eps_abs + g.eps_rel * __builtin_fmax(nw, ny);
            double ed = g.eps_abs + g.eps_rel * rho * nl;
            ZM_TRK_ED(ed, rho * nl)
            near_ok = (rp <= 10.0 * ep) && (rd <= 10.0 * ed);
            if (rp <= ep && rd <= ed) {
                status = ZM_MPC_OPTIMAL;
                done = true;
            } else if (!(rp == rp)) {
                done = true;  // NaN iterates (non-finite data): stop with the limit status
            } else {
                need_cert = chk;
            }
        }
        // ---- primal infeasibility certificate (see file header)
        if (chk && __any(need_cert)) {
            double sv[NS];
            {
                const long o = (long)(N - 1) * W;
#pragma unroll
                for (int i = 0; i < NS; ++i) sv[i] = rv[(o + i) * bt + ii];
            }
            double gmax = 0.0;
            for (int k = N - 1; k >= 0; --k) {
#pragma unroll
                for (int j = 0; j < MC; ++j) {
                    double sacc = rv[((long)k * W + NS + j) * bt + ii];
#pragma unroll
                    for (int i = 0; i < NS; ++i) sacc = __builtin_fma(B[i * MC + j], sv[i], sacc);
                    gmax = __builtin_fmax(gmax, __builtin_fabs(sacc));  // (G^T r)_k = ru_k + B^T s
                }
                double sn[NS];
#pragma unroll
                for (int i = 0; i < NS; ++i) {
                    double sacc = (k >= 1) ? rv[((long)(k - 1) * W + i) * bt + ii] : 0.0;
#pragma unroll
                    for (int l = 0; l < NS; ++l) sacc = __builtin_fma(A[l * NS + i], sv[l], sacc);
                    sn[i] = sacc;
                }
#pragma unroll
                for (int i = 0; i < NS; ++i) sv[i] = sn[i];
            }
            double vw0 = 0.0;  // v^T w(u = 0) = s^T x0   (s = sum_j (A^j)^T vx_j after the sweep)
#pragma unroll
            for (int i = 0; i < NS; ++i) vw0 = __builtin_fma(sv[i], x0[i], vw0);
            if (need_cert && gmax <= g.eps_pinf * ndl && (vw0 - sup) > g.eps_pinf * ndl) {
                status = ZM_MPC_INFEASIBLE;
                done = true;
            }
        }
    }
    // final trajectory: the dynamics-exact rollout w of the last iterate
    if (live) {
        double x[NS];
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            x[i] = x0[i];
            g.xTraj[(ii * (N + 1)) * NS + i] = x[i];
        }
        for (int k = 0; k < N; ++k) {
            const double* Kk = Ktab + (long)k * MC * NS;
            double u[MC], xn[NS];
#pragma unroll
            for (int j = 0; j < MC; ++j) {
                double sacc = -kf[((long)k * MC + j) * bt + ii];
#pragma unroll
                for (int i = 0; i < NS; ++i) sacc = __builtin_fma(-Kk[j * NS + i], x[i], sacc);
                u[j] = sacc;
                g.uTraj[(ii * N + k) * MC + j] = sacc;
            }
#pragma unroll
            for (int i = 0; i < NS; ++i) {
                double sacc = 0.0;
#pragma unroll
                for (int l = 0; l < NS; ++l) sacc = __builtin_fma(A[i * NS + l], x[l], sacc);
#pragma unroll
                for (int j = 0; j < MC; ++j) sacc = __builtin_fma(B[i * MC + j], u[j], sacc);
                xn[i] = sacc;
            }
#pragma unroll
            for (int i = 0; i < NS; ++i) {
                x[i] = xn[i];
                g.xTraj[(ii * (N + 1) + k + 1) * NS + i] = x[i];
            }
        }
        g.status[ii] = status ? status : (near_ok ? ZM_MPC_OPTIMAL_INACCURATE : ZM_MPC_USER_LIMIT);
        okflag[ii] = (status == ZM_MPC_OPTIMAL) ? 1.0 : 0.0;
        if (g.iters) g.iters[ii] = it;
        if (g.resid) {
            g.resid[ii * 2] = rp;
            g.resid[ii * 2 + 1] = rd;
        }
    }
