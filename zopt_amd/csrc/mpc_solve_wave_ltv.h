// K9-W, stage-varying dynamics (zm_mpc_solve_ltv_f64):  x_{k+1} = A_k x_k + B_k u_k + c_k  in the 16-lanes-per-instance ADMM.
// Included by mpc_wave.hip after the kernels it is modelled on (their mat-vecs, norms and LDS layout are used as they are); a kernel of
// its own rather than more hooks on mpc_solve_wave_body.h, because what that body keeps in registers for the whole solve -- the lane's
// column of [A | B], its row of A and of B -- is per-stage data here, and the stage tables change type with it:
//     backward (TabB): the lane's column of [A_k | B_k] (NS), its row of [K_k^T ; Suu_k^-1] (MC), g_k, D_k = P_{k+1} c_k (state lanes)
//     forward  (TabF): the lane's row of [A_k ; K_k] (NS), its row of B_k (MC, state lanes), c_k (state lanes)
// (both branches of a load write every member they differ in: a member written under one lane role only became a stack slot)
// The two sweeps do not overlap, so the three rotating sets of the three-stage prefetch hold NS + MC doubles plus the stage's scalars
// each, as in the body; nothing of the dynamics is resident.  The columns of [A_k | B_k] are strided in the caller's layout: the setup
// kernel (mpc.hip: mpc_setup_ltv_kernel) writes them once per problem as contiguous rows (ABt), the rows of A_k and B_k are contiguous
// as the caller gives them.
// Always per-problem and always with the linear term g (a zero block without a reference).  The algorithm is the body's, with
//     backward:  p = p' + z_x + g_x + D_k;  Qu = z_u + g_u + B_k^T p;  kf = Suu_k^-1 Qu;  p' = A_k^T p - K_k^T Qu
//     forward :  u = -K_k x - kf;  x+ = A_k x + B_k u + c_k
//     certificate: v^T w(u=0) = s_0 . x0 + sum_k sigma_k . c_k   (sigma_k: the adjoint vector on entering stage k of the adjoint sweep)
// The dual tolerance scales with max(rho |lam|_inf, |g|_inf) as in the tracking kernels (c sits in the constraints, not in the cost);
// the cycle guard of the adaptive penalty (ZM_TRK_LEVEL) is on when g != 0 or the problem's c != 0 -- offsets drive the same ping-pong
// between adjacent levels as a reference outside the box does.  With constant A_k, B_k, c = 0 the sums are those of
// mpc_solve_wave_track_kernel<NS, MC, true> in the same order.
// Included twice by mpc_wave.hip, which sets the ZM_LTV_* hooks before each: first with one box per problem (x_lb, x_ub (P,n), u_lb, u_ub
// (P,m), resident in the lane's lo / hi; every hook expands to the tokens this file had before it had hooks), then as
// mpc_solve_wave_ltv_stage_kernel (zm_mpc_solve_ltv_stage_f64) with the STAGE's box: x_lb, x_ub are the box of x_0 (P,n), read for the x0
// test only, and u_lb, u_ub carry lo, hi (P,N,n+m) in the stacked stage layout, row k = [bound of x_{k+1} ; bound of u_k].  The lane's
// lo_k, hi_k ride in the forward prefetch set (TabF), 16 consecutive doubles per group and stage like g; they enter the projection and the
// support term of the certificate, nothing else.  Lanes outside every role keep -inf / +inf.  The weights never enter this kernel.
// A third time as mpc_solve_wave_ltv_soft_kernel (zm_mpc_solve_ltv_soft_f64): the stage form with soft box constraints, a penalty
// l1 d + l2 d^2 on the distance d of a component from its box, weights per problem and component (P,n+m) in one more argument block
// (ZM_LTV_ARGS; MpcSoft).  The lane keeps l1, l2 and, of the penalty it runs at, t = l1 / rho and a = rho / (rho + 2 l2) (ZM_LTV_RHO: at
// entry and after every level move).  Three places differ: a soft component of x0 is not tested against row 0 (ZM_LTV_BOX gives it
// -inf / +inf there), the projection is the proximal map of the penalty (ZM_LTV_PROJECT), and the support term of the certificate takes
// -inf / +inf for a soft component, whose y ranges over the whole line (ZM_LTV_SUP_LO / _HI).  The cycle guard is also on when the
// problem has a soft component (ZM_LTV_GUARD).  l1 = +inf is a hard component: t = inf, and every one of these is the stage kernel's.
template <int NS, int MC>
__global__ __launch_bounds__(64) void ZM_LTV_KERNEL(const double* __restrict__ A, const double* __restrict__ B,
                                                                const double* __restrict__ Ktab, const double* __restrict__ Mtab,
                                                                const double* __restrict__ x_lb, const double* __restrict__ x_ub,
                                                                const double* __restrict__ u_lb, const double* __restrict__ u_ub,
                                                                const MpcArgs g, const MpcProb pb, const MpcTrack trk, const MpcLtv lv ZM_LTV_ARGS) {
    static_assert(NS + MC <= 16, "the stacked index must fit the 16 lanes of a group");
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int W = NS + MC;
    const int lane = threadIdx.x, grp = lane >> 4, li = lane & 15;
    const long inst_raw = (long)blockIdx.x * 4 + grp;
    const bool live = inst_raw < g.batch;          // uniform over the 16-lane group
    const long inst = live ? inst_raw : g.batch - 1;   // idle groups shadow the last instance and never store
    const int N = g.N;
    const long p = pb.prob[inst];                  // the group's problem (checked against P on the host)
    double rho = pb.rho[p];
    const double rho0 = rho;
    int lvl = g.level0;
    const bool sx = li < NS, su = (li >= NS) && (li < W), sw = li < W;   // this lane owns a state / a control / any component
    const int ix = sx ? li : 0, iu = su ? li - NS : 0, iw = sw ? li : 0;
    double* base = lds + (long)grp * N * WS_STAGE;
    double* yw = base + li;                        // + k * WS_STAGE
    double* lw = base + 16 + li;
    double* rw = base + 32 + li;
    double* kf = base + 48 + li;                   // (control lanes)

    const double inf = __builtin_inf();
    ZM_LTV_BOX
    const double x0 = sx ? g.x0[inst * NS + ix] : 0.0;
    const double viol = (sx && !(x0 >= ZM_LTV_X0_LO && x0 <= ZM_LTV_X0_HI)) ? 1.0 : 0.0;
    const bool x0_in = row_max(viol) == 0.0;

    // per-instance block of the caller's workspace, as in the body: [y (N,W) | lam (N,W) | kf (N,MC), ok flag, level | unused]
    double* wsi = g.ws + inst * (4L * N * W);
    double* okflag = wsi + 2L * N * W + (long)N * MC;
    const bool warm = g.warm && (*okflag == 1.0);
    if (warm && g.n_levels > 1) {   // the stored lam is scaled by the penalty the previous solve ended with
        const int l = (int)okflag[1];
        if (l >= 0 && l < g.n_levels) {
            lvl = l;
            rho = rho0 * pow(g.rho_step, (double)(lvl - g.level0));
        }
    }
    ZM_LTV_RHO
    for (int k = 0; k < N; ++k) {
        const int ks = (g.warm == 2 && k + 1 < N) ? k + 1 : k;    // shifted warm start: iterate k <- iterate k+1
        const double wy = warm ? wsi[(long)ks * W + iw] : 0.0, wl = warm ? wsi[(long)N * W + (long)ks * W + iw] : 0.0;
        yw[k * WS_STAGE] = sw ? wy : 0.0;
        lw[k * WS_STAGE] = sw ? wl : 0.0;
        rw[k * WS_STAGE] = 0.0;
        kf[k * WS_STAGE] = 0.0;
    }

    // Per-lane bases of the stage data; a stage's slice is base + stage index x stride.  A lane outside every role (NS + MC < 16) reads
    // the finite entries of row / column 0 and computes finite values nobody reads, as in the body.  Stage indices are clamped into [0, N).
    const double* abt_base = lv.ABt + (p * N * W + iw) * NS;                  // + k * W * NS: column iw of [A_k | B_k], contiguous
    const double* arow_base = A + (p * N * NS + ix) * NS;                     // + k * NS * NS: row ix of A_k
    const double* brow_base = B + (p * N * NS + ix) * MC;                     // + k * NS * MC: row ix of B_k
    const double* c_base = lv.c + p * N * NS + ix;                            // + k * NS
    const double* gw = trk.g + inst * ((long)N * W) + iw;                     // + k * W
    const double *adj_base = nullptr, *fwd_base = nullptr, *d_base = nullptr;
    const int adj_stride = su ? MC * MC : MC * NS;
    auto set_level_bases = [&]() {
        const long pl = p * g.n_levels + lvl;
        adj_base = su ? Mtab + (pl * N * MC + iu) * MC : Ktab + pl * N * MC * NS + ix;
        fwd_base = Ktab + pl * N * MC * NS + iu * NS;
        d_base = lv.D + pl * N * NS + ix;
    };
    struct TabB {
        double col[NS], adj[MC];
        double y, lam, kf, g, d;
    };
    struct TabF {
        double fwd[NS], brow[MC];
        double y, lam, kf, c;
        ZM_LTV_TABF
    };
    auto load_b = [&](int k, TabB& t) {
        k = k < 0 ? 0 : (k >= N ? N - 1 : k);
        t.y = yw[k * WS_STAGE];
        t.lam = lw[k * WS_STAGE];
        t.kf = kf[k * WS_STAGE];
        t.g = gw[(long)k * W];
        const double* pc = abt_base + (long)k * (W * NS);
#pragma unroll
        for (int i = 0; i < NS; ++i) t.col[i] = pc[i];
        const double* pa = adj_base + (long)k * adj_stride;
        if (su) {
#pragma unroll
            for (int j = 0; j < MC; ++j) t.adj[j] = pa[j];           // row of Suu_k^-1
            t.d = 0.0;
        } else {
#pragma unroll
            for (int j = 0; j < MC; ++j) t.adj[j] = pa[j * NS];      // column of K_k
            t.d = d_base[(long)k * NS];
        }
    };
    auto load_f = [&](int k, TabF& t) {
        k = k < 0 ? 0 : (k >= N ? N - 1 : k);
        t.y = yw[k * WS_STAGE];
        t.lam = lw[k * WS_STAGE];
        t.kf = kf[k * WS_STAGE];
        ZM_LTV_LOAD_BOX(k, t)
        if (su) {
            const double* pf = fwd_base + (long)k * (MC * NS);
#pragma unroll
            for (int i = 0; i < NS; ++i) t.fwd[i] = pf[i];           // row of K_k
#pragma unroll
            for (int j = 0; j < MC; ++j) t.brow[j] = 0.0;
            t.c = 0.0;
        } else {
            const double* pa = arow_base + (long)k * (NS * NS);
            const double* pbr = brow_base + (long)k * (NS * MC);
#pragma unroll
            for (int i = 0; i < NS; ++i) t.fwd[i] = pa[i];           // row of A_k
#pragma unroll
            for (int j = 0; j < MC; ++j) t.brow[j] = pbr[j];         // row of B_k
            t.c = c_base[(long)k * NS];
        }
    };

    // |g|_inf of the instance and |c|_inf of its problem, once at entry
    double gnorm = 0.0, cnorm = 0.0;
    for (int k = 0; k < N; ++k) {
        const double gk = gw[(long)k * W];
        if (sw) amax(gnorm, gk);
        const double ck = c_base[(long)k * NS];
        if (sx) amax(cnorm, ck);
    }
    gnorm = row_max(gnorm);
    cnorm = row_max(cnorm);
    const bool guard = gnorm > 0.0 || cnorm > 0.0 ZM_LTV_GUARD;
    int trk_last = 0, trk_rev = 0;   // the last level move; consecutive reversals of it
    bool trk_locked = false;

    const double alpha = g.alpha, om_alpha = 1.0 - g.alpha;
    int status = x0_in ? 0 : ZM_MPC_INFEASIBLE;
    int it = 0;
    double rp = 0.0, rd = 0.0;
    bool near_ok = false;
    bool done = !live || status != 0;              // group-uniform
    for (int gi = 0; gi < g.max_iter; ++gi) {
        if (__all(done)) break;
        const bool chk = ((gi + 1) % ZM_MPC_CHK) == 0;
        set_level_bases();
        // ---- backward affine sweep, the stage data fetched three stages ahead
        double pp = 0.0;   // (A_k^T p - K_k^T Qu) of the stage above (state lanes)
        {
            auto bstage = [&](const int k, const TabB& t) {
                const double z = -rho * (t.y - t.lam);    // -rho z_x (state lanes), -rho z_u (control lanes)
                const double kfo = t.kf;
                const double pk = pp + z + t.g + t.d;     // costate of x_{k+1} (state lanes), the offset's share included
                double q = sx ? 0.0 : z + t.g;
                mv<NS>(t.col, pk, q);                     // A_k^T p (state lanes);  Qu = z_u + g_u + B_k^T p (control lanes)
                double r = 0.0;
                mv<MC, NS>(t.adj, q, r);                  // K_k^T Qu (state lanes);  kf = Suu_k^-1 Qu (control lanes)
                if (su) kf[k * WS_STAGE] = done ? kfo : r;
                pp = q - r;
            };
            TabB t0, t1, t2;
            load_b(N - 1, t0);
            load_b(N - 2, t1);
            load_b(N - 3, t2);
            int k = N - 1;
#pragma unroll 1
            for (; k >= 2; k -= 3) {
                bstage(k, t0);
                load_b(k - 3, t0);
                bstage(k - 1, t1);
                load_b(k - 4, t1);
                bstage(k - 2, t2);
                load_b(k - 5, t2);
            }
            if (k >= 0) bstage(k, t0);
            if (k >= 1) bstage(k - 1, t1);
        }
        // ---- forward rollout, projection, dual update, residuals
        double x = x0;
        double nrp = 0.0, nrd = 0.0, nw = 0.0, ny = 0.0, nl = 0.0, sup = 0.0, ndl = 0.0;
        {
            auto fstage = [&](const int k, const TabF& t) {
                double ax = 0.0;
                mv<NS>(t.fwd, x, ax);                 // A_k x (state lanes), K_k x (control lanes)
                const double u = -t.kf - ax;          // (control lanes; only their u is ever broadcast, stored or projected)
                double xn = ax;
                mv_seq<MC, NS>(t.brow, u, xn);        // + B_k u (state lanes)
                xn += t.c;                            // + c_k
                const double w = sx ? xn : u;         // the stacked iterate [x_{k+1} ; u_k]
                const double lold = t.lam, yold = t.y;
                const double wh = __builtin_fma(alpha, w, om_alpha * yold);   // relaxed iterate (alpha = 1: w exactly)
                double yn = wh + lold;
                ZM_LTV_PROJECT(yn, t)
                const double r = w - yn, dl = wh - yn, ln = lold + dl;        // primal residual; dual step
                yw[k * WS_STAGE] = (done || !sw) ? yold : yn;
                lw[k * WS_STAGE] = (done || !sw) ? lold : ln;
                if (chk) rw[k * WS_STAGE] = sw ? dl : 0.0;
                if (sw) {
                    if (chk) {
                        sup += (dl > 0.0) ? dl * ZM_LTV_SUP_HI(t) : ((dl < 0.0) ? dl * ZM_LTV_SUP_LO(t) : 0.0);
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
            TabF t0, t1, t2;
            load_f(0, t0);
            load_f(1, t1);
            load_f(2, t2);
            int k = 0;
#pragma unroll 1
            for (; k + 2 < N; k += 3) {
                fstage(k, t0);
                load_f(k + 3, t0);
                fstage(k + 1, t1);
                load_f(k + 4, t1);
                fstage(k + 2, t2);
                load_f(k + 5, t2);
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
            if (gnorm > rho * nl) ed = g.eps_abs + g.eps_rel * gnorm;
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
        // ---- adaptive penalty: the level rule of the body, then the cycle guard of the tracking kernels (mpc_wave.hip: ZM_TRK_LEVEL)
        if (g.n_levels > 1 && chk && !done && gi + 1 < g.max_iter) {
            const double tiny = 1e-300;
            const double rpn = rp / __builtin_fmax(__builtin_fmax(nw, ny), tiny);
            const double rdn = rd / __builtin_fmax(rho * nl, tiny);
            const double want = __builtin_sqrt(rpn / __builtin_fmax(rdn, tiny));
            int dl = 0;
            if (want == want && want > 0.0) dl = (int)lrint(log(want) / log(g.rho_step));   // the NEAREST tabulated level
            int nl_ = lvl + dl;
            nl_ = nl_ < 0 ? 0 : (nl_ >= g.n_levels ? g.n_levels - 1 : nl_);
            if (guard) {
                const int mvd = nl_ - lvl;
                if (trk_locked) {
                    nl_ = lvl;
                } else if (mvd != 0 && trk_last != 0 && ((mvd > 0) != (trk_last > 0))) {
                    if (++trk_rev >= ZM_TRK_REVERSALS) {
                        trk_locked = true;
                        nl_ = lvl;
                    }
                } else {
                    trk_rev = 0;
                }
                trk_last = nl_ - lvl;
            }
            if (nl_ != lvl) {
                const double rnew = rho0 * pow(g.rho_step, (double)(nl_ - g.level0));
                const double sc = rho / rnew;
                for (int k = 0; k < N; ++k) lw[k * WS_STAGE] *= sc;
                rho = rnew;
                lvl = nl_;
                ZM_LTV_RHO
            }
        }
        // ---- primal infeasibility certificate: adjoint sweep over r = w - y with the stage's own A_k^T, B_k^T; the free response
        //      w(u=0) contains the offsets.  The columns of stage k - 1 are fetched while stage k is computed.
        if (chk && __any(need_cert)) {
            sup = row_sum(sup);
            double sv = sx ? rw[(N - 1) * WS_STAGE] : 0.0;
            double gmax = 0.0, vc = 0.0;
            double col[NS], ck = 0.0;
            {
                const double* pc = abt_base + (long)(N - 1) * (W * NS);
#pragma unroll
                for (int i = 0; i < NS; ++i) col[i] = pc[i];
                ck = c_base[(long)(N - 1) * NS];
            }
#pragma unroll 1
            for (int k = N - 1; k >= 0; --k) {
                double coln[NS], ckn = 0.0;
                {
                    const int kn = k >= 1 ? k - 1 : 0;
                    const double* pc = abt_base + (long)kn * (W * NS);
#pragma unroll
                    for (int i = 0; i < NS; ++i) coln[i] = pc[i];
                    ckn = c_base[(long)kn * NS];
                }
                const double rk = rw[k * WS_STAGE], rkm = (k >= 1) ? rw[(k - 1) * WS_STAGE] : 0.0;
                vc = __builtin_fma(sv, ck, vc);       // sigma_k . c_k, the lane's term (sv is zero outside the state lanes)
                double gs = su ? rk : (sx ? rkm : 0.0);
                mv<NS>(col, sv, gs);                  // (G^T r)_k = r_u,k + B_k^T s (control lanes);   s <- r_x,k-1 + A_k^T s (state lanes)
                if (su) gmax = __builtin_fmax(gmax, __builtin_fabs(gs));
                sv = sx ? gs : 0.0;
#pragma unroll
                for (int i = 0; i < NS; ++i) col[i] = coln[i];
                ck = ckn;
            }
            gmax = row_max(gmax);
            const double vw0 = row_sum(__builtin_fma(sv, x0, vc));
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
        TabF tf;
#pragma unroll 1
        for (int k = 0; k < N; ++k) {
            load_f(k, tf);
            double ax = 0.0;
            mv<NS>(tf.fwd, x, ax);
            const double u = su ? -kf[k * WS_STAGE] - ax : 0.0;
            double xn = ax;
            mv_seq<MC, NS>(tf.brow, u, xn);
            xn += tf.c;
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
}
