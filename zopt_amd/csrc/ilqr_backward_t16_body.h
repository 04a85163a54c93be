// Body of the register-prefetch sweep kernel ilqr_backward_t16_f64 (ilqr_backward.hip).
// A function BODY, not a header: #included verbatim inside ilqr_backward_t16_f64, ilqr_backward_box_t16_f64 and (MODE 2 with the box
// hooks) ddp_backward_box_t16_f64, so that the kernel that existed before the input box compiles from the very same tokens (same ISA;
// tools/isa_identity.py checks it).
// The hooks ZM_BOX_SETUP (statements after the lane roles are known), ZM_BOX_FLAGS (further template arguments of ilqr_step) and
// ZM_BOX_ARGS (its further arguments) expand to nothing in the kernel without a box.
// The hooks ZM_PEN_LOAD_FLAG / ZM_PEN_LOAD_ARG (the operand fetch also reads the lane's entry of the diagonal addend h_k) and
// ZM_PEN_TERMINAL (h_T joins the terminal V_xx) expand to nothing in the kernels without a state-box penalty.
    constexpr int NP = 4 * KS;
    const int lane = threadIdx.x;
    const long traj = tl.list ? (long)tl.list[blockIdx.x] : (long)blockIdx.x;
    if (active && active[traj] == 0) return;  // whole wave leaves: this trajectory keeps its previous policy
    const int g = lane >> 4, c = lane & 15;
    __shared__ double sm[ILQR_LDS_DOUBLES];
    __shared__ double jA[MODE == 2 ? NS_LDS_DOUBLES : 1];

    IlqrAddr<KS> a;
    const int nn = n * n, nm = n * m, mm = m * m;
    const bool cA = c < n;
    a.cA = cA;
    const bool cB = (c >= NP) && (c < NP + m);
    const long last = traj * T + (T - 1);
    const double* fxt = f_x + last * nn;
    const double* fut = f_u + last * nm;
    const double* cxt = c_x + last * n;
    const double* cut = c_u + last * m;
    // shared_h: one time-invariant cost Hessian for every trajectory and step (strides 0)
    const double* cxxt = shared_h ? c_xx : c_xx + last * nn;
    const double* cuxt = shared_h ? c_ux : c_ux + last * nm;
    const double* cuut = shared_h ? c_uu : c_uu + last * mm;
    a.sC = shared_h ? 0 : nn;
    const bool row0 = g < n;
    const bool laneA = row0 && cA, laneB = row0 && cB;
    a.dF = laneA ? 4 * n : laneB ? 4 * m : 0;
    a.sF = laneB ? nm : nn;
    a.dC = laneA ? 4 * n : 0;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int row = 4 * s + g;
        a.rowok[s] = row < n;
        a.vF[s] = (row < n) && (cA || cB);
        a.vC[s] = (row < n) && cA;
    }
    a.pF0 = laneA ? (fxt + g * n + c) : laneB ? (fut + g * m + (c - NP)) : fxt;
    a.pC0 = laneA ? (cxxt + g * n + c) : cxxt;
    // row NP+g of the stacked Hessian: c_ux[g][c] under the state columns, c_uu[g][c-NP] under the control columns
    const bool vux = (g < m) && cA, vuu = (g < m) && cB;
    a.vCu = vux || vuu;
    a.pCu = vux ? (cuxt + g * n + c) : vuu ? (cuut + g * m + (c - NP)) : cuxt;
    a.sCu = shared_h ? 0 : (vuu ? mm : nm);
    a.cu_pad = (g >= m && c == NP + g) ? 1.0 : 0.0;
    a.vcv = cA || cB;
    a.pcv = cA ? (cxt + c) : cB ? (cut + (c - NP)) : cxt;
    a.scv = cB ? m : n;
    if constexpr (MODE == 1) {
        const double* dt_ = dvec + last * n;
        a.pdc = cA ? (dt_ + c) : dt_;
        a.pdr0 = row0 ? (dt_ + g) : dt_;
        a.sd = n;
    }
    if constexpr (MODE == 2) {
        const long nnn = (long)nn * n, nmn = (long)nm * n, nmm = (long)nm * m;
        const double* fxxt = f_xx + last * nnn;
        const double* fuxt = f_ux + last * nmn;
        const double* fuut = f_uu + last * nmm;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 4 * r + g;
            const bool rx = row < n, ru = (row >= NP) && (row < NP + m);
            // compact index: states 0..n-1, controls n..n+m-1
            const int ca = rx ? row : (ru ? n + (row - NP) : -1);
            const int cb = cA ? c : (cB ? n + (c - NP) : -1);
            a.zc[r] = (ca >= 0 && cb >= 0) ? ca * 17 + cb : -1;   // 17-wide compact index; only its sign is read (a 0/-1 flag changes the generated code)
            a.zlive[r] = (ca >= 0) && (row == c);
            if (Hpk != nullptr) {
                // packed second derivatives (zm_quadratic_dynamics_pairs_list_f64): element (ca, cb) is pair p = (min, max) of the
                // model's table or structurally zero; H[pt][p][i], i contiguous -> the contraction below runs unchanged with a
                // unit stride over i and the same summation order as over the full tensors
                int pidx = -1;
                if (ca >= 0 && cb >= 0) {
                    const int lo = ca < cb ? ca : cb, hi = ca < cb ? cb : ca;
                    for (int q = 0; q < ptab.n; ++q) pidx = (ptab.ab[q] == (unsigned char)(lo * 16 + hi)) ? q : pidx;
                }
                const double* Hl = Hpk + last * (long)ptab.n * n;
                if (pidx >= 0) {
                    a.pz[r] = Hl + (long)pidx * n;  a.sz[r] = 1;  a.stz[r] = ptab.n * n;
                } else {   // structurally zero (or padding): the lane contracts don't-care data and contributes an exact 0.0
                    a.pz[r] = Hl;  a.sz[r] = 0;  a.stz[r] = ptab.n * n;
                    a.zc[r] = -1;
                }
            } else if (f_ux == nullptr && !(rx && cA)) {   // dynamics affine in the controls: f_ux, f_uu are zero and not materialised
                a.zc[r] = -1;
                a.pz[r] = fxxt;  a.sz[r] = 0;  a.stz[r] = (int)nnn;
            } else if (rx && cA) {     // f_xx[i][row][c]
                a.pz[r] = fxxt + row * n + c;  a.sz[r] = nn;  a.stz[r] = (int)nnn;
            } else if (rx && cB) {     // (vf_ux)^T: f_ux[i][c-NP][row]
                a.pz[r] = fuxt + (c - NP) * n + row;  a.sz[r] = nm;  a.stz[r] = (int)nmn;
            } else if (ru && cA) {     // f_ux[i][row-NP][c]
                a.pz[r] = fuxt + (row - NP) * n + c;  a.sz[r] = nm;  a.stz[r] = (int)nmn;
            } else if (ru && cB) {     // f_uu[i][row-NP][c-NP]
                a.pz[r] = fuut + (row - NP) * m + (c - NP);  a.sz[r] = mm;  a.stz[r] = (int)nmm;
            } else {                   // padding: finite don't-care data, dropped (zc = -1)
                a.pz[r] = fxxt;  a.sz[r] = 0;  a.stz[r] = (int)nnn;
            }
        }
    }
    a.vL = (g < m) && cA;
    const bool vl = (g < m) && (c == NP);
    a.vOut = a.vL || vl;
    a.pOut = a.vL ? (Lout + last * nm + g * n + c) : (lout + last * m + g);
    a.sOut = vl ? m : nm;

    // LDS addresses of this lane's right-hand side: column c of [Q_ux | .] for c < n, the row q (Q_u) for c == NP
    const bool rhs_qu = (c == NP);
    const int ob0 = rhs_qu ? (64 + NP + 0) : (0 * 16 + c);
    const int ob1 = rhs_qu ? (64 + NP + 1) : (1 * 16 + c);
    const int ob2 = rhs_qu ? (64 + NP + 2) : (2 * 16 + c);
    const int ob3 = rhs_qu ? (64 + NP + 3) : (3 * 16 + c);
    // Q_uu[c][g] as A operand (c < 4): tile row c, column NP+g.  Lanes c >= 4 only feed output rows >= 4 of
    // Q_uu L, which are never used: they read their own (finite) tile element.
    const int oqa = (c < 4) ? (c * 16 + NP + g) : (g * 16 + c);

    ZM_BOX_SETUP
    // terminal value function
    double Vxx[KS], vxr[KS];
    {
        const double* vxx = shared_h ? vf_xx : vf_xx + traj * svxx;
        const double* vx = vf_x + traj * svx;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int row = 4 * s + g;
            const bool ok = (row < n) && cA;
            const double t = vxx[ok ? row * n + c : 0];
            Vxx[s] = ok ? t : 0.0;
            const double u = vx[row < n ? row : 0];
            vxr[s] = (row < n) ? u : 0.0;
        }
    }

    ZM_PEN_TERMINAL
    if (g == 0) sm[80 + c] = cA ? (vf_x + traj * svx)[c] : 0.0;  // v_x (column-indexed), read by MODE 2's contraction
    ilqr_lds_sync();
    if constexpr (MODE == 2) {
        // a DDP step is ~100 matrix products long: operand prefetch buys nothing and its registers are needed elsewhere
        for (int k2 = T - 1; k2 >= 0; --k2) {
            IlqrStepRegs<KS> d;
            ilqr_load_step<KS, MODE>(d, a);
            ilqr_step<KS, MODE, false ZM_BOX_FLAGS>(Vxx, vxr, d, a, sm, g, c, ob0, ob1, ob2, ob3, oqa, jA, n, m ZM_BOX_ARGS);
        }
    } else {
    IlqrStepRegs<KS> d0, d1;
    ilqr_load_step<KS, MODE ZM_PEN_LOAD_FLAG>(d0, a ZM_PEN_LOAD_ARG);
    if (T >= 2) ilqr_load_step<KS, MODE ZM_PEN_LOAD_FLAG>(d1, a ZM_PEN_LOAD_ARG);
    int k = T - 1;
    while (k >= 3) {
        ilqr_step<KS, MODE, true ZM_BOX_FLAGS>(Vxx, vxr, d0, a, sm, g, c, ob0, ob1, ob2, ob3, oqa, jA, n, m ZM_BOX_ARGS);
        ilqr_step<KS, MODE, true ZM_BOX_FLAGS>(Vxx, vxr, d1, a, sm, g, c, ob0, ob1, ob2, ob3, oqa, jA, n, m ZM_BOX_ARGS);
        k -= 2;
    }
    if (k == 2) {
        ilqr_step<KS, MODE, true ZM_BOX_FLAGS>(Vxx, vxr, d0, a, sm, g, c, ob0, ob1, ob2, ob3, oqa, jA, n, m ZM_BOX_ARGS);
        ilqr_step<KS, MODE, false ZM_BOX_FLAGS>(Vxx, vxr, d1, a, sm, g, c, ob0, ob1, ob2, ob3, oqa, jA, n, m ZM_BOX_ARGS);
        ilqr_step<KS, MODE, false ZM_BOX_FLAGS>(Vxx, vxr, d0, a, sm, g, c, ob0, ob1, ob2, ob3, oqa, jA, n, m ZM_BOX_ARGS);
    } else if (k == 1) {
        ilqr_step<KS, MODE, false ZM_BOX_FLAGS>(Vxx, vxr, d0, a, sm, g, c, ob0, ob1, ob2, ob3, oqa, jA, n, m ZM_BOX_ARGS);
        ilqr_step<KS, MODE, false ZM_BOX_FLAGS>(Vxx, vxr, d1, a, sm, g, c, ob0, ob1, ob2, ob3, oqa, jA, n, m ZM_BOX_ARGS);
    } else {
        ilqr_step<KS, MODE, false ZM_BOX_FLAGS>(Vxx, vxr, d0, a, sm, g, c, ob0, ob1, ob2, ob3, oqa, jA, n, m ZM_BOX_ARGS);
    }
    }
    // optional: the value function the sweep ends with (riccatiStep_ilqr / _ddp return it: ilqrUtils.py:170, :203)
    if (vxx_out) {
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int row = 4 * s + g;
            if (row < n && cA) vxx_out[traj * nn + row * n + c] = Vxx[s];
        }
    }
    if (vx_out && g == 0 && cA) vx_out[traj * n + c] = sm[80 + c];
    if (v_out) {
        double cs = 0.0;   // sum_k c_k
        if (c_s)
            for (int k2 = lane; k2 < T; k2 += 64) cs += c_s[traj * T + k2];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) cs += __shfl_xor(cs, off, 64);
        if (g == 0 && c == NP) v_out[traj] = ((vf_s ? vf_s[traj] : 0.0) + cs) + a.vsum;
    }
