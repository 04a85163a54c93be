// Body of the 16-lanes-per-instance MPC solve kernel (mpc_wave.hip).
// A function BODY, not a header: #included verbatim inside mpc_solve_wave_kernel and mpc_solve_wave_batched_kernel (mpc_wave.hip), so that the
// kernel that existed before the per-problem variant compiles from the very same tokens (same ISA; tools/isa_identity.py checks
// it).  The per-problem kernel reaches it with its parameters already offset to its problem (see there).
// The ZM_TRK_* hooks are the reference-tracking variant (mpc_wave.hip: mpc_solve_wave_track_kernel); they expand to nothing in the
// kernels without a reference.
// The ZM_SOFT_* hooks are the soft-box variant (mpc_wave.hip: mpc_solve_wave_soft_kernel, mpc_closed_loop_wave_soft_kernel); in every other
// kernel they expand to nothing, or to the tokens that stood in their place before there were hooks.
    static_assert(NS + MC <= 16, "the stacked index must fit the 16 lanes of a group");
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int W = NS + MC;
    const int lane = threadIdx.x, grp = lane >> 4, li = lane & 15;
    const long inst_raw = (long)blockIdx.x * 4 + grp;
    const bool live = inst_raw < g.batch;          // uniform over the 16-lane group
    const long inst = live ? inst_raw : g.batch - 1;   // idle groups shadow the last instance and never store
    const int N = g.N;
    double rho = g.rho;        // penalty of this group (changes with adaptive levels)
    int lvl = g.level0;
    const bool sx = li < NS, su = (li >= NS) && (li < W), sw = li < W;   // this lane owns a state / a control / any component
    const int ix = sx ? li : 0, iu = su ? li - NS : 0, iw = sw ? li : 0;
    double* base = lds + (long)grp * N * WS_STAGE;
    double* yw = base + li;                        // + k * WS_STAGE
    double* lw = base + 16 + li;
    double* rw = base + 32 + li;
    double* kf = base + 48 + li;                   // (control lanes)

    // the lane's column of [A | B] (the adjoint products over the state lanes), its row of A (state lanes; the control lanes' row of
    // [A ; K_k] comes from the stage's table) and its row of B (zero outside the state lanes)
    double ABcol[NS], Arow[NS], Brow[MC];
#pragma unroll
    for (int l = 0; l < NS; ++l) {
        const double ac = A[l * NS + ix], bc = B[l * MC + iu], ar = A[ix * NS + l];
        ABcol[l] = sx ? ac : (su ? bc : 0.0);
        Arow[l] = sx ? ar : 0.0;
    }
#pragma unroll
    for (int j = 0; j < MC; ++j) {
        const double br = B[ix * MC + j];
        Brow[j] = sx ? br : 0.0;
    }
    const double inf = __builtin_inf();
    const double lo = sx ? x_lb[ix] : (su ? u_lb[iu] : -inf), hi = sx ? x_ub[ix] : (su ? u_ub[iu] : inf);
    ZM_SOFT_SETUP
    const double x0 = sx ? g.x0[inst * NS + ix] : 0.0;
    // x_0 = x0 is box-constrained too (mpcUtils.py:56,58): group-wide AND over the state lanes
    const double viol = (sx ZM_SOFT_X0 && !(x0 >= lo && x0 <= hi)) ? 1.0 : 0.0;
    const bool x0_in = row_max(viol) == 0.0;

    // per-instance block of the caller's workspace: [y (N,W) | lam (N,W) | kf (N,MC), ok flag, spare | unused]
    double* wsi = g.ws + inst * (4L * N * W);
    double* okflag = wsi + 2L * N * W + (long)N * MC;
    const bool warm = g.warm && (*okflag == 1.0);
    if (warm && g.n_levels > 1) {   // the stored lam is scaled by the penalty the previous solve ended with
        const int l = (int)okflag[1];
        if (l >= 0 && l < g.n_levels) {
            lvl = l;
            rho = g.rho * pow(g.rho_step, (double)(lvl - g.level0));
        }
    }
    ZM_SOFT_RHO
    for (int k = 0; k < N; ++k) {
        const int ks = (g.warm == 2 && k + 1 < N) ? k + 1 : k;    // shifted warm start: iterate k <- iterate k+1
        const double wy = warm ? wsi[(long)ks * W + iw] : 0.0, wl = warm ? wsi[(long)N * W + (long)ks * W + iw] : 0.0;
        yw[k * WS_STAGE] = sw ? wy : 0.0;
        lw[k * WS_STAGE] = sw ? wl : 0.0;
        rw[k * WS_STAGE] = 0.0;
        kf[k * WS_STAGE] = 0.0;
    }

    // Table slices of one stage, by lane role, and the lane's own iterates of that stage from LDS (y, lam, kf: stage-local, so reading
    // them stages ahead of their use is safe in both sweeps: no LDS round trip at the head of a stage's dependency chain):
    //     fwd[l]  the lane's row of [A ; K_k]          (state lanes: row of A, kept; control lanes: row of K_k, loaded under their mask)
    //     adj[j]  the lane's row of [K_k^T ; Suu_k^-1]  (state lanes: column of K_k; control lanes: row of Suu_k^-1)
    // No masking: a lane outside every role (shapes with NS + MC < 16) loads the finite entries of row / column 0 and computes finite
    // values nobody reads -- only lanes < NS of p / x and lanes NS .. W-1 of qu / u are ever broadcast, only lanes < W are stored or
    // enter a norm.  Stage indices are clamped into [0, N).
    struct Tab {
        double fwd[NS], adj[MC];
        double y, lam, kf;
        ZM_TRK_TAB
    };
    // Table addresses: a per-lane base (role and penalty level: set at the top of every ADMM iteration) plus stage index x a per-lane
    // stage stride -- one v_mad per table and stage; the elements of a slice sit at compile-time offsets on either side of the role mask.
    // (Computed from lvl and k inside the stage, the addresses were a third of a backward stage's vector instructions.)
    const char *adj_base = nullptr, *fwd_base = nullptr;
    const unsigned adj_stride = (su ? MC * MC : MC * NS) * (unsigned)sizeof(double);
    auto set_level_bases = [&]() {
        adj_base = su ? (const char*)(Mtab + ((long)lvl * N * MC + iu) * MC) : (const char*)(Ktab + (long)lvl * N * MC * NS + ix);
        fwd_base = (const char*)(Ktab + (long)lvl * N * MC * NS + iu * NS);
    };
    auto load_tab = [&](int k, Tab& t) {
        k = k < 0 ? 0 : (k >= N ? N - 1 : k);
        t.y = yw[k * WS_STAGE];
        t.lam = lw[k * WS_STAGE];
        t.kf = kf[k * WS_STAGE];
        const double* pa = (const double*)(adj_base + (unsigned long long)(unsigned)k * adj_stride);
        if (su) {   // (only the control lanes' rows change with the stage: the state lanes keep their row of A, set once per sweep)
            const double* pf = (const double*)(fwd_base + (unsigned long long)(unsigned)k * (unsigned)(MC * NS * sizeof(double)));
#pragma unroll
            for (int i = 0; i < NS; ++i) t.fwd[i] = pf[i];
#pragma unroll
            for (int j = 0; j < MC; ++j) t.adj[j] = pa[j];           // row of Suu_k^-1
        } else {
#pragma unroll
            for (int j = 0; j < MC; ++j) t.adj[j] = pa[j * NS];      // column of K_k
        }
    };
    auto init_tab = [&](Tab& t) {
#pragma unroll
        for (int i = 0; i < NS; ++i) t.fwd[i] = Arow[i];
    };

    ZM_TRK_SETUP
    const double alpha = g.alpha, om_alpha = 1.0 - g.alpha;
    int status = x0_in ? 0 : ZM_MPC_INFEASIBLE;
    int it = 0;
    double rp = 0.0, rd = 0.0;
    bool near_ok = false;   // the last iterate's residuals are within 10x the tolerances (OSQP's "solved inaccurate" test at the cap)
    bool done = !live || status != 0;              // group-uniform
    for (int gi = 0; gi < g.max_iter; ++gi) {
        if (__all(done)) break;
        const bool chk = ((gi + 1) % ZM_MPC_CHK) == 0;
        set_level_bases();
        // ---- backward affine sweep.  The table slices come from L2 (~500+ cycles) and a stage is shorter than that, so they are
        //      fetched THREE stages ahead into a rotating set of registers (the loop is unrolled by three: no copies).
        double pp = 0.0;   // (A^T p - K^T Qu) of the stage above (state lanes)
        {
            auto bstage = [&](const int k, const Tab& t) {
                const double z = -rho * (t.y - t.lam);    // -rho z_x (state lanes), -rho z_u (control lanes)
                const double kfo = t.kf;
                const double p = pp + z ZM_TRK_G(t);      // costate of x_{k+1} (state lanes)
                double q = sx ? 0.0 : z ZM_TRK_G(t);
                mv<NS>(ABcol, p, q);                      // A^T p (state lanes);  Qu = -rho z_u + B^T p (control lanes)
                double r = 0.0;
                mv<MC, NS>(t.adj, q, r);                  // K^T Qu (state lanes);  kf = Suu^-1 Qu (control lanes)
                if (su) kf[k * WS_STAGE] = done ? kfo : r;
                pp = q - r;
            };
            Tab t0, t1, t2;
            load_tab(N - 1, t0);
            load_tab(N - 2, t1);
            load_tab(N - 3, t2);
            ZM_TRK_LOAD(N - 1, t0)
            ZM_TRK_LOAD(N - 2, t1)
            ZM_TRK_LOAD(N - 3, t2)
            int k = N - 1;
#pragma unroll 1
            for (; k >= 2; k -= 3) {
                bstage(k, t0);
                load_tab(k - 3, t0);
                ZM_TRK_LOAD(k - 3, t0)
                bstage(k - 1, t1);
                load_tab(k - 4, t1);
                ZM_TRK_LOAD(k - 4, t1)
                bstage(k - 2, t2);
                load_tab(k - 5, t2);
                ZM_TRK_LOAD(k - 5, t2)
            }
            if (k >= 0) bstage(k, t0);
            if (k >= 1) bstage(k - 1, t1);
        }
        // ---- forward rollout, projection, dual update, residuals
        double x = x0;
        double nrp = 0.0, nrd = 0.0, nw = 0.0, ny = 0.0, nl = 0.0, sup = 0.0, ndl = 0.0;
        {
            auto fstage = [&](const int k, const Tab& t) {
                double ax = 0.0;
                mv<NS>(t.fwd, x, ax);                 // A x (state lanes), K x (control lanes)
                const double u = -t.kf - ax;          // (control lanes; only their u is ever broadcast, stored or projected)
                double xn = ax;
                mv_seq<MC, NS>(Brow, u, xn);          // + B u (state lanes)
                const double w = sx ? xn : u;         // the stacked iterate [x_{k+1} ; u_k]
                const double lold = t.lam, yold = t.y;
                const double wh = __builtin_fma(alpha, w, om_alpha * yold);   // relaxed iterate (alpha = 1: w exactly)
                double yn = wh + lold;
                ZM_SOFT_PROJECT(yn)
                const double r = w - yn, dl = wh - yn, ln = lold + dl;        // primal residual; dual step
                yw[k * WS_STAGE] = (done || !sw) ? yold : yn;
                lw[k * WS_STAGE] = (done || !sw) ? lold : ln;
                if (chk) rw[k * WS_STAGE] = sw ? dl : 0.0;
                if (sw) {
                    if (chk) {
                        sup += (dl > 0.0) ? dl * ZM_SOFT_SUP_HI : ((dl < 0.0) ? dl * ZM_SOFT_SUP_LO : 0.0);
                        amax(ndl, dl);
                    }
                    amax(nrp, r);
                    amax(nrd, yn - yold);
                    amax(nw, w);
                    amax(ny, yn);
                    amax(nl, ln);
                }
                x = xn;                               // (only the state lanes' x is ever broadcast)
            };
            Tab t0, t1, t2;
            init_tab(t0);
            init_tab(t1);
            init_tab(t2);
            load_tab(0, t0);
            load_tab(1, t1);
            load_tab(2, t2);
            int k = 0;
#pragma unroll 1
            for (; k + 2 < N; k += 3) {
                fstage(k, t0);
                load_tab(k + 3, t0);
                fstage(k + 1, t1);
                load_tab(k + 4, t1);
                fstage(k + 2, t2);
                load_tab(k + 5, t2);
            }
            if (k < N) fstage(k, t0);
            if (k + 1 < N) fstage(k + 1, t1);
        }
        nrp = row_max(nrp);
        nrd = row_max(nrd);
        nw = row_max(nw);
        ny = row_max(ny);
        nl = row_max(nl);
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
                done = true;   // NaN iterates (non-finite data): stop with the limit status
            } else {
                need_cert = chk;
            }
        }
        // ---- adaptive penalty (OSQP adaptive_rho): rho <- rho sqrt(normalised primal / normalised dual residual), taken in
        //      whole steps of the tabulated levels: to the level nearest the wanted penalty on the log scale (so a move happens
        //      when the penalty is off by at least sqrt(rho_step)); the scaled dual lam = mu / rho is rescaled so that the
        //      unscaled multiplier mu is unchanged.  Not at the last iteration the cap allows: no iteration follows it, and the final
        //      rollout below pairs the kf of the last iterate with the level's K_k, so a move there returned a trajectory that is no iterate
        if (g.n_levels > 1 && chk && !done && gi + 1 < g.max_iter) {
            const double tiny = 1e-300;
            const double rpn = rp / __builtin_fmax(__builtin_fmax(nw, ny), tiny);
            const double rdn = rd / __builtin_fmax(rho * nl, tiny);
            const double want = __builtin_sqrt(rpn / __builtin_fmax(rdn, tiny));
            int dl = 0;
            if (want == want && want > 0.0) dl = (int)lrint(log(want) / log(g.rho_step));   // the NEAREST tabulated level
            int nl_ = lvl + dl;
            nl_ = nl_ < 0 ? 0 : (nl_ >= g.n_levels ? g.n_levels - 1 : nl_);
            ZM_TRK_LEVEL(nl_)
            if (nl_ != lvl) {
                const double rnew = g.rho * pow(g.rho_step, (double)(nl_ - g.level0));
                const double sc = rho / rnew;
                for (int k = 0; k < N; ++k) lw[k * WS_STAGE] *= sc;
                rho = rnew;
                lvl = nl_;
                ZM_SOFT_RHO
            }
        }
        // ---- primal infeasibility certificate (mpc.hip header): adjoint sweep over r = w - y
        if (chk && __any(need_cert)) {
            sup = row_sum(sup);
            double sv = sx ? rw[(N - 1) * WS_STAGE] : 0.0;
            double gmax = 0.0;
#pragma unroll 1
            for (int k = N - 1; k >= 0; --k) {
                const double rk = rw[k * WS_STAGE], rkm = (k >= 1) ? rw[(k - 1) * WS_STAGE] : 0.0;
                double gs = su ? rk : (sx ? rkm : 0.0);
                mv<NS>(ABcol, sv, gs);                // (G^T r)_k = r_u,k + B^T s (control lanes);   s <- r_x,k-1 + A^T s (state lanes)
                if (su) gmax = __builtin_fmax(gmax, __builtin_fabs(gs));
                sv = sx ? gs : 0.0;
            }
            gmax = row_max(gmax);
            const double vw0 = row_sum(sv * x0);
            const double dn = row_max(ndl);          // |dual step|: the certificate's scale (= rp without relaxation)
            if (need_cert && gmax <= g.eps_pinf * dn && (vw0 - sup) > g.eps_pinf * dn) {
                status = ZM_MPC_INFEASIBLE;
                done = true;
            }
        }
    }
    // ---- final trajectory (the dynamics-exact rollout of the last iterate) and the iterates for a later warm start
    if (live) {
        set_level_bases();
        double x = x0;
        if (sx) g.xTraj[(inst * (N + 1)) * NS + ix] = x;
        Tab tf;
        init_tab(tf);
#pragma unroll 1
        for (int k = 0; k < N; ++k) {
            load_tab(k, tf);
            double ax = 0.0;
            mv<NS>(tf.fwd, x, ax);
            const double u = su ? -kf[k * WS_STAGE] - ax : 0.0;
            double xn = ax;
            mv_seq<MC, NS>(Brow, u, xn);
            if (su) g.uTraj[(inst * N + k) * MC + iu] = u;
            x = sx ? xn : 0.0;
            if (sx) g.xTraj[(inst * (N + 1) + k + 1) * NS + ix] = x;
            if (sw) {
                wsi[(long)k * W + iw] = yw[k * WS_STAGE];
                wsi[(long)N * W + (long)k * W + iw] = lw[k * WS_STAGE];
            }
        }
        if (li == 0) {
            g.status[inst] = status ? status : (near_ok ? ZM_MPC_OPTIMAL_INACCURATE : ZM_MPC_USER_LIMIT);
            *okflag = (status == ZM_MPC_OPTIMAL) ? 1.0 : 0.0;
            okflag[1] = (double)lvl;
            if (g.iters) g.iters[inst] = it;
            if (g.resid) {
                g.resid[inst * 2] = rp;
                g.resid[inst * 2 + 1] = rd;
            }
        }
    }
