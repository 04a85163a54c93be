// Body of the generic line-search kernel (rollout.hip).
// A function BODY, not a header: #included verbatim inside rollout_linesearch_kernel and rollout_linesearch_track_kernel, so that the
// kernel that existed before the tracking cost compiles from the very same tokens (same ISA; tools/isa_identity.py checks it).
// The hooks ZM_TRK_FLAG / ZM_TRK_ARGS pass the tracking cost's reference on to rollout_one; they expand to nothing in the kernel
// without a reference.  ZM_PEN_STORE_ARGS: further arguments of the store pass (the state box's plain-cost output); nothing elsewhere.
    constexpr int TPW = 64 / NA;  // trajectories per wave
    const int lane = threadIdx.x;
    const int a = lane % NA;
    const long slot = (long)blockIdx.x * TPW + lane / NA;   // slot -> trajectory id (through `list` when given)
    const long nslot = list ? count : batch;
    const long traj = (slot < nslot) ? (list ? (long)list[slot] : slot) : 0;
    const bool live = (slot < nslot) && (a < n_alpha) && (active == nullptr || active[traj] != 0);
    const long t = live ? traj : 0;
    const int n = md.n, m = md.m;
    const zm_quadcost_t* cs = has_cost ? &cost : nullptr;
    const double alpha = alphas[a < n_alpha ? a : 0];
    const double* x0t = x0 + t * n;
    const double* lt = l + t * T * m;
    const double* Lt = L + t * T * m * n;
    const double* xpt = xPrev + t * (T + 1) * n;
    const double* upt = uPrev + t * T * m;
    double* xo = xTraj + t * (T + 1) * n;
    double* uo = uTraj + t * T * m;

    double J = 0.0;
    int best = 0;
    if (NA > 1) {
        if (live) J = rollout_one<false ZM_TRK_FLAG>(md, cs, alpha, x0t, lt, Lt, xpt, upt, nullptr, nullptr, T ZM_TRK_ARGS);
        // argmin over the NA lanes of this trajectory with jnp.argmin semantics: a NaN cost beats every number
        // (also -inf), the first index wins among equals.  Dead lanes carry (+inf, index NA).
        double key = live ? J : __builtin_inf();
        int isn = (live && (J != J)) ? 1 : 0;
        int who = live ? a : NA;
#pragma unroll
        for (int off = NA / 2; off >= 1; off >>= 1) {
            const double ok = __shfl_xor(key, off);
            const int on = __shfl_xor(isn, off);
            const int ow = __shfl_xor(who, off);
            const bool better = (on > isn) || (on == isn && ((on == 0 && ok < key) || ((on == 1 || ok == key) && ow < who)));
            key = better ? ok : key;
            isn = better ? on : isn;
            who = better ? ow : who;
        }
        best = who < NA ? who : 0;
    }
    // every lane of the trajectory re-rolls the winning step size; lane 0 of the group stores
    const double abest = alphas[best];
    if (live) {
        if (a == 0) {
            const double Jb = rollout_one<true ZM_TRK_FLAG>(md, cs, abest, x0t, lt, Lt, xpt, upt, xo, uo, T ZM_TRK_ARGS ZM_PEN_STORE_ARGS);
            if (Jout) Jout[t] = Jb;
            if (idx_out) idx_out[t] = best;
        }
    }
