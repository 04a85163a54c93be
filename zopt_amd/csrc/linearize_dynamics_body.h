// Body of the 16-lanes-per-point expansion kernel (linearize.hip).
// A function BODY, not a header: #included verbatim inside linearize_dynamics_kernel and linearize_dynamics_track_kernel, so that the
// kernel that existed before the tracking cost compiles from the very same tokens (same ISA; tools/isa_identity.py checks it -- the
// same text as an inlined function taking the kernel's arguments by reference did not).
// The hooks ZM_TRK_POINT, ZM_CX, ZM_CU, ZM_TRK_TERMINAL, ZM_XT are the tracking cost's (linearize.hip defines them around each
// #include): in the kernels without a reference they expand to nothing resp. to xv[i], uv[i], xT[i].
    // one point's [f_x (n, n) | f_u (n, m)] image per 16-lane group: the columns the lanes computed are transposed here so that the
    // group stores whole 128-byte lines instead of column-strided 8-byte pieces
    __shared__ double tile[4 * LIN_WAVES][MAXN * (MAXN + MAXM)];
    const int lane = threadIdx.x;
    const int j = lane & 15;                                   // seed direction / Jacobian column
    const int q = lane >> 4;                                   // group of this workgroup
    const long gi = (long)blockIdx.x * (4 * LIN_WAVES) + q;    // slot * T + k; slots are the listed trajectories, or all of them
    const long nslot = list ? count : batch;
    if (gi >= nslot * T) return;
    const long slot = gi / T;
    const int k = (int)(gi - slot * T);
    const long traj = list ? (long)list[slot] : slot;
    const int n = QUAD ? 12 : md.n, m = QUAD ? 4 : md.m;   // (compile-time in the quadcopter variant)
    const long pt = traj * T + k;                              // point index
    double xv[MAXN], uv[MAXM];
    const double* xk = xTraj + (traj * (T + 1) + k) * n;
    {   // the point's loads go out together with the mask's
        const double* uk = uTraj + pt * m;
#pragma unroll
        for (int i = 0; i < MAXN; ++i) xv[i] = (i < n) ? xk[i] : 0.0;
#pragma unroll
        for (int i = 0; i < MAXM; ++i) uv[i] = (i < m) ? uk[i] : 0.0;
    }
    if (active && active[traj] == 0) return;
    {
        // (the cost part first: its weight loads leave with the state's, ahead of the LDS exchange below -- a compiler barrier)
        if constexpr (COST) {
            const zm_quadcost_t& cs = ec.cs;
            ZM_TRK_POINT(n, m)
            if (j < n) {
                double g;
                if (cs.diagonal == 1) {
                    double xj = 0.0;
#pragma unroll
                    for (int i = 0; i < MAXN; ++i) xj = (i == j) ? ZM_CX(i) : xj;
                    g = (cs.Q[j * n + j] + cs.Q[j * n + j]) * xj;
                } else {
                    g = 0.0;
#pragma unroll
                    for (int i = 0; i < MAXN; ++i)
                        if (i < n) g = __builtin_fma(cs.Q[j * n + i] + cs.Q[i * n + j], ZM_CX(i), g);
                }
                ec.c_x[pt * n + j] = g;
                if (k == T - 1) {   // terminal gradient from x_T
                    const double* xT = xk + n;
                    ZM_TRK_TERMINAL
                    double gv;
                    if (cs.diagonal == 1) {
                        gv = (cs.Qf[j * n + j] + cs.Qf[j * n + j]) * ZM_XT(j);
                    } else {
                        gv = 0.0;
                        for (int i = 0; i < n; ++i) gv = __builtin_fma(cs.Qf[j * n + i] + cs.Qf[i * n + j], ZM_XT(i), gv);
                    }
                    ec.v_x[traj * n + j] = gv;
                }
            } else if (j < n + m) {
                const int ju = j - n;
                double g;
                if (cs.diagonal == 1) {
                    double uj = 0.0;
#pragma unroll
                    for (int i = 0; i < MAXM; ++i) uj = (i == ju) ? ZM_CU(i) : uj;
                    g = (cs.R[ju * m + ju] + cs.R[ju * m + ju]) * uj;
                } else {
                    g = 0.0;
#pragma unroll
                    for (int i = 0; i < MAXM; ++i)
                        if (i < m) g = __builtin_fma(cs.R[ju * m + i] + cs.R[i * m + ju], ZM_CU(i), g);
                }
                ec.c_u[pt * m + ju] = g;
            }
        }
        if constexpr (PACKED) {
            static_assert(QUAD, "packed Jacobians: the quadcopter's closed forms");
            constexpr int NJ = WIND ? QUAD_NJ_WIND : QUAD_NJ_STILL, NJP = (NJ + 1) & ~1;
            const QuadAtoms a = quad_atoms(md, xv, uv);
            if (NJP != NJ && j == 0) tile[q][NJP - 1] = 0.0;
            quad_jac_column_packed<WIND>(j, a, md.dt, tile[q]);
            wave_lds_sync();
            double* op = f_x + pt * NJP;
            for (int e = j; e < NJP; e += 16) op[e] = tile[q][e];
            return;
        }
        double col[MAXN];                                      // column j of [f_x | f_u] (lanes j >= n + m: unused)
        if constexpr (QUAD) {
            // closed-form column j of d xd / d z (generated, quad_derivs_gen.h): the trigonometric values once, a few operations
            // per entry -- instead of the whole model on dual numbers per column.  x+ = x + dt xd  =>  column of [f_x | f_u] =
            // e_j + dt d xd  (dt = 0: the derivative of xd itself, as model_step defines that case).
            const QuadAtoms a = quad_atoms(md, xv, uv);
            double o[12];
            quad_jac_column<WIND>(j, a, o);
#pragma unroll
            for (int i = 0; i < 12; ++i) col[i] = (md.dt == 0.0) ? o[i] : __builtin_fma(md.dt, o[i], (i == j) ? 1.0 : 0.0);
            if (f && j == 0) {   // model_step's quadcopter branch, spelled out (the generic call drags the linear model's A, B loads
                                 // into this loop as invariants)
                double xd[12];
                quad_inertial_dynamics<double>(xv, uv, md.wind_ned, xd);
#pragma unroll
                for (int i = 0; i < 12; ++i) f[pt * 12 + i] = (md.dt == 0.0) ? xd[i] : xv[i] + md.dt * xd[i];
            }
        } else {
            Dual x[MAXN], u[MAXM], xn[MAXN];
#pragma unroll
            for (int i = 0; i < MAXN; ++i) x[i] = Dual{xv[i], (i == j) ? 1.0 : 0.0};
#pragma unroll
            for (int i = 0; i < MAXM; ++i) u[i] = Dual{uv[i], (n + i == j) ? 1.0 : 0.0};
            model_step<Dual>(md, x, u, xn);
#pragma unroll
            for (int i = 0; i < MAXN; ++i) col[i] = xn[i].d;
            if (f && j == 0) {
#pragma unroll
                for (int i = 0; i < MAXN; ++i)
                    if (i < n) f[pt * n + i] = xn[i].v;
            }
        }
        if (j < n + m) {
            double* t = tile[q] + ((j < n) ? j : n * n + (j - n));
            const int st = (j < n) ? n : m;
#pragma unroll
            for (int i = 0; i < MAXN; ++i)
                if (i < n) t[i * st] = col[i];
        }
        wave_lds_sync();
        {
            double* ox = f_x + pt * n * n;
            double* ou = f_u + pt * n * m;
            for (int e = j; e < n * n; e += 16) ox[e] = tile[q][e];
            for (int e = j; e < n * m; e += 16) ou[e] = tile[q][n * n + e];
        }
    }
