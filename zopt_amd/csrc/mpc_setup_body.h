// Body of the MPC setup kernel (mpc.hip): the Riccati recursion of one problem at one penalty.
// A function BODY, not a header: #included verbatim inside mpc_setup_kernel and mpc_setup_batched_kernel (mpc.hip), so that the
// kernel that existed before the per-problem variant compiles from the very same tokens (same ISA; tools/isa_identity.py checks
// it).  The per-problem kernel reaches it with its parameters already offset to its problem (see there).
    __shared__ double As[SN * SN], Bs[SN * SM], P[SN * SN], PA[SN * SN], PB[SN * SM], Sux[SM * SN], Suu[SM * SM],
        Mi[SM * SM], K[SM * SN], T1[SN * SN], T2[SN * SN];
    const int t = threadIdx.x;
    for (int e = t; e < n * n; e += blockDim.x) {
        As[e] = A[e];
        P[e] = 2.0 * Qf[e] + ((e / n == e % n) ? rho : 0.0);  // P_N = 2 Qf + rho I   (1/2-form Hessian of x'Qf x + rho/2 |x-z|^2)
    }
    for (int e = t; e < n * m; e += blockDim.x) Bs[e] = B[e];
    __syncthreads();
    for (int k = N - 1; k >= 0; --k) {
        mm_nn(PA, P, As, n, n, n);
        mm_nn(PB, P, Bs, n, n, m);
        mm_tn(Sux, Bs, PA, n, m, n);  // B^T P A
        mm_tn(Suu, Bs, PB, n, m, m);  // B^T P B
        if (t < m * m) Suu[t] += 2.0 * R[t] + ((t / m == t % m) ? rho : 0.0);
        __syncthreads();
        if (t == 0) {  // m x m inverse by Gauss-Jordan with partial pivoting (m <= SM)
            double a[SM][2 * SM];
            for (int i = 0; i < m; ++i)
                for (int j = 0; j < m; ++j) {
                    a[i][j] = Suu[i * m + j];
                    a[i][m + j] = (i == j) ? 1.0 : 0.0;
                }
            for (int c = 0; c < m; ++c) {
                int pv = c;
                for (int i = c + 1; i < m; ++i)
                    if (__builtin_fabs(a[i][c]) > __builtin_fabs(a[pv][c])) pv = i;
                for (int j = 0; j < 2 * m; ++j) {
                    const double tmp = a[c][j];
                    a[c][j] = a[pv][j];
                    a[pv][j] = tmp;
                }
                const double inv = 1.0 / a[c][c];
                for (int j = 0; j < 2 * m; ++j) a[c][j] *= inv;
                for (int i = 0; i < m; ++i)
                    if (i != c) {
                        const double f = a[i][c];
                        for (int j = 0; j < 2 * m; ++j) a[i][j] = __builtin_fma(-f, a[c][j], a[i][j]);
                    }
            }
            for (int i = 0; i < m; ++i)
                for (int j = 0; j < m; ++j) Mi[i * m + j] = a[i][m + j];
        }
        __syncthreads();
        mm_nn(K, Mi, Sux, m, m, n);     // K_k = Suu^-1 B^T P A
        mm_tn(T1, As, PA, n, n, n);     // A^T P A
        mm_tn(T2, Sux, K, m, n, n);     // Sux^T K
        for (int e = t; e < n * n; e += blockDim.x)
            T1[e] = (2.0 * Q[e] + ((e / n == e % n) ? rho : 0.0)) + T1[e] - T2[e];
        __syncthreads();
        // the value matrix is stored symmetrised: the antisymmetric rounding error of the update above is propagated through A . A_cl, not
        // A_cl . A_cl, and grows along the horizon of an open-loop-unstable plant unless it is removed at every stage
        for (int e = t; e < n * n; e += blockDim.x) P[e] = 0.5 * (T1[e] + T1[(e % n) * n + e / n]);
        for (int e = t; e < m * n; e += blockDim.x) Kout[(long)k * m * n + e] = K[e];
        for (int e = t; e < m * m; e += blockDim.x) Minvout[(long)k * m * m + e] = Mi[e];
        __syncthreads();
    }
