// Body of the cost expansion kernel (linearize.hip).
// A function BODY, not a header: #included verbatim inside quadratize_cost_kernel and quadratize_cost_track_kernel (same tokens, same
// ISA for the kernel that existed before the tracking cost).  The hooks ZM_TRK_DIFF_X / ZM_TRK_DIFF_U turn x, u into their
// differences from the reference rows; they expand to nothing in the kernel without a reference.
    const long sid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long nslot = list ? count : batch;
    const long npts = nslot * T;
    if (sid >= npts + nslot) return;
    const bool terminal = sid >= npts;
    const long slot = terminal ? (sid - npts) : (sid / T);
    const long traj = list ? (long)list[slot] : slot;
    if (active && active[traj] == 0) return;
    const int k = terminal ? T : (int)(sid - slot * T);
    const long id = traj * T + k;                              // point index (unused for the terminal expansion)
    const double* xk = xTraj + (traj * (T + 1) + k) * n;
    double x[MAXN], u[MAXM];
#pragma unroll
    for (int i = 0; i < MAXN; ++i) x[i] = (i < n) ? xk[i] : 0.0;
    ZM_TRK_DIFF_X
    const double* Qm = terminal ? cs.Qf : cs.Q;
    double* gx = terminal ? (v_x ? v_x + traj * n : nullptr) : (c_x ? c_x + id * n : nullptr);
    if (gx) {
        if (cs.diagonal == 1) {   // asserted diagonal weights: the n^2 - n vanishing terms of (Q + Q^T) x are not formed
#pragma unroll
            for (int jj = 0; jj < MAXN; ++jj)
                if (jj < n) gx[jj] = (Qm[jj * n + jj] + Qm[jj * n + jj]) * x[jj];
        } else {
#pragma unroll
            for (int jj = 0; jj < MAXN; ++jj) {
                if (jj < n) {
                    double s = 0.0;   // ((Q + Q^T) x)[jj]
#pragma unroll
                    for (int i = 0; i < MAXN; ++i)
                        if (i < n) s = __builtin_fma(Qm[jj * n + i] + Qm[i * n + jj], x[i], s);
                    gx[jj] = s;
                }
            }
        }
    }
    if (terminal) {
        if (v) v[traj] = terminal_cost(cs, n, x);
        return;
    }
    const double* uk = uTraj + id * m;
#pragma unroll
    for (int i = 0; i < MAXM; ++i) u[i] = (i < m) ? uk[i] : 0.0;
    ZM_TRK_DIFF_U
    if (c_u) {
        if (cs.diagonal == 1) {
#pragma unroll
            for (int jj = 0; jj < MAXM; ++jj)
                if (jj < m) c_u[id * m + jj] = (cs.R[jj * m + jj] + cs.R[jj * m + jj]) * u[jj];
        } else {
#pragma unroll
            for (int jj = 0; jj < MAXM; ++jj) {
                if (jj < m) {
                    double s = 0.0;
#pragma unroll
                    for (int i = 0; i < MAXM; ++i)
                        if (i < m) s = __builtin_fma(cs.R[jj * m + i] + cs.R[i * m + jj], u[i], s);
                    c_u[id * m + jj] = s;
                }
            }
        }
    }
    if (c) c[id] = running_cost(cs, n, m, x, u);
