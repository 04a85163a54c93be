// Body of the one-lane-per-point expansion kernel of the quadcopter (linearize.hip).
// A function BODY, not a header: #included verbatim inside expand_quad_points_kernel and expand_quad_points_track_kernel (same tokens,
// same ISA for the kernel that existed before the tracking cost; see linearize_dynamics_body.h for the hooks).
    constexpr int NJ = WIND ? QUAD_NJ_WIND : QUAD_NJ_STILL, NJP = (NJ + 1) & ~1;
    constexpr int LD = NJP + 16 + 1;   // a point's row: packed Jacobians, c_x, c_u; odd, so that the lanes' rows start in different banks
    extern __shared__ __attribute__((aligned(16))) double qp_lds[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double* tile = qp_lds + (long)wv * QP_R * LD;
    const long chunk = (long)blockIdx.x * QP_WAVES + wv;
    if (chunk >= nslot * nchunk) return;
    const long slot = chunk / nchunk;
    const int ch = (int)(chunk - slot * nchunk);
    const long traj = list ? (long)list[slot] : slot;
    if (active && active[traj] == 0) return;   // (whole wave)
    const int k0 = ch * per;
    const int np = (T - k0 < per) ? T - k0 : per;
    const zm_quadcost_t& cs = ec.cs;
    if (lane < np) {
        const int k = k0 + lane;
        const double* xk = xTraj + (traj * (T + 1) + k) * 12;
        const double* uk = uTraj + (traj * T + k) * 4;
        double xv[12], uv[4];
#pragma unroll
        for (int i = 0; i < 12; ++i) xv[i] = xk[i];
#pragma unroll
        for (int i = 0; i < 4; ++i) uv[i] = uk[i];
        double* t = tile + lane * LD;
        ZM_TRK_POINT(12, 4)
        // cost gradients: the expressions of quadratize_cost_kernel / linearize_dynamics_kernel, in their order
#pragma unroll
        for (int j = 0; j < 12; ++j) {
            double g;
            if (cs.diagonal == 1) {
                g = (cs.Q[j * 12 + j] + cs.Q[j * 12 + j]) * ZM_CX(j);
            } else {
                g = 0.0;
#pragma unroll
                for (int i = 0; i < 12; ++i) g = __builtin_fma(cs.Q[j * 12 + i] + cs.Q[i * 12 + j], ZM_CX(i), g);
            }
            t[NJP + j] = g;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double g;
            if (cs.diagonal == 1) {
                g = (cs.R[j * 4 + j] + cs.R[j * 4 + j]) * ZM_CU(j);
            } else {
                g = 0.0;
#pragma unroll
                for (int i = 0; i < 4; ++i) g = __builtin_fma(cs.R[j * 4 + i] + cs.R[i * 4 + j], ZM_CU(i), g);
            }
            t[NJP + 12 + j] = g;
        }
        const QuadAtoms a = quad_atoms(md, xv, uv);
        if (NJP != NJ) t[NJP - 1] = 0.0;
        quad_jac_all_packed<WIND>(a, md.dt, t);
    }
    if (k0 + np == T && lane < 12) {   // terminal gradient from x_T, one lane per component
        const double* xT = xTraj + (traj * (T + 1) + T) * 12;
        const int j = lane;
        ZM_TRK_TERMINAL
        double gv;
        if (cs.diagonal == 1) {
            gv = (cs.Qf[j * 12 + j] + cs.Qf[j * 12 + j]) * ZM_XT(j);
        } else {
            gv = 0.0;
#pragma unroll
            for (int i = 0; i < 12; ++i) gv = __builtin_fma(cs.Qf[j * 12 + i] + cs.Qf[i * 12 + j], ZM_XT(i), gv);
        }
        ec.v_x[traj * 12 + j] = gv;
    }
    wave_lds_sync();
    const long p0 = traj * T + k0;
    tile_copy_out<NJP, 0, LD>(f_x + p0 * NJP, tile, np * NJP, lane);
    tile_copy_out<12, NJP, LD>(ec.c_x + p0 * 12, tile, np * 12, lane);
    tile_copy_out<4, NJP + 12, LD>(ec.c_u + p0 * 4, tile, np * 4, lane);
