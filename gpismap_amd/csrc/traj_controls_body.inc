// The body of traj_controls_kernel and of traj_retime_controls_kernel (traj.hip; DESIGN.md §7p, §7w), included into each with
// TRAJ_SCHED 0 or 1.  It is shared as text and not as a template: with TRAJ_SCHED 0 the compiler sees the plain kernel's
// statements exactly as they were, so the plain kernels' instructions are the ones they had.  TRAJ_SCHED 1: the two positions of
// step k are those of the own slots own(k0 + k) and own(k0 + k + 1) of the trajectory's schedule `sc`, dt is the slot, and a
// schedule of status >= 2 stands still.
    constexpr int NU = DIM == 3 ? 4 : 2;
    __shared__ float st[kTree];
    __shared__ double sh[2][kTree];
    __shared__ int swi[2 * (kBlock / 64)];
    __shared__ int sidx[kTree];
    const int tr = first + blockIdx.x, k = threadIdx.x, nthr = blockDim.x;
    const size_t base = (size_t)tr * N;
    double* Uo = U + (size_t)blockIdx.x * T * NU;
    double* hpo = hp + (size_t)blockIdx.x * 5;

#if TRAJ_SCHED
    if (tint[(size_t)tr * 9] != 0 || sc.res[(size_t)tr * kSchedRes] >= 2) {   // not timed, or no schedule: stand still
#else
    if (tint[(size_t)tr * 9] != 0) {                     // not timed: stand still
#endif
        if (k < T) {
#pragma unroll
            for (int u = 0; u < NU; ++u) Uo[(size_t)k * NU + u] = 0.0;
        }
        if (k == 0) {
            hpo[0] = 1.0; hpo[1] = 0.0;
#pragma unroll
            for (int a = 0; a < DIM; ++a) hpo[2 + a] = (double)x[base * DIM + a];
            if (DIM == 2) hpo[4] = 0.0;
            clamped[blockIdx.x] = 0;
        }
        return;
    }
    for (int i = k; i < N; i += nthr) st[i] = tt[base + i];
    __syncthreads();

    double p[DIM], D[DIM];
    double n = 0.0;
    bool mov = false;
#pragma unroll
    for (int a = 0; a < DIM; ++a) { p[a] = 0.0; D[a] = 0.0; }
    if (k < T) {
        double q[DIM];
#if TRAJ_SCHED
        traj_position<DIM, 1>(x + base * DIM, v + base, st, N, (double)sched_own(sc, tr, sc.k0 + k) * dt, p);
        traj_position<DIM, 1>(x + base * DIM, v + base, st, N, (double)sched_own(sc, tr, sc.k0 + k + 1) * dt, q);
#else
        traj_position<DIM>(x + base * DIM, v + base, st, N, t0 + (double)k * dt, p);
        traj_position<DIM>(x + base * DIM, v + base, st, N, t0 + (double)(k + 1) * dt, q);
#endif
#pragma unroll
        for (int a = 0; a < DIM; ++a) D[a] = q[a] - p[a];
        n = sqrt(D[0] * D[0] + D[1] * D[1]);
        mov = n > min_move;
    }
    if (mov) { sh[0][k] = D[0] / n; sh[1][k] = D[1] / n; }
    int fst;
    int last = block_latest_flag(mov, swi, nthr, &fst);  // (its barriers publish sh)
    if (last < 0) last = fst;
    sidx[k] = last;
    __syncthreads();
    int cl = 0;
    if (k < T) {
        const int nxt = k + 1 < T ? sidx[k + 1] : last;  // h_T = h_{T-1}
        double c = 1.0, s = 0.0, c1 = 1.0, s1 = 0.0;
        if (last >= 0) { c = sh[0][last]; s = sh[1][last]; }
        if (nxt >= 0) { c1 = sh[0][nxt]; s1 = sh[1][nxt]; }
        double* u = Uo + (size_t)k * NU;
        u[0] = (c * D[0] + s * D[1]) / dt;
        if (DIM == 3) {
            u[1] = ((-s) * D[0] + c * D[1]) / dt;
            u[2] = D[DIM - 1] / dt;
        }
        const double num = c * s1 - s * c1, den = 1.0 + (c * c1 + s * s1);
        double w;
        if (den <= 0.0) {
            w = w_limit > 0.0 ? (num >= 0.0 ? w_limit : -w_limit) : 0.0;
            cl = 1;
        } else {
            w = (num / den) / (0.5 * dt);
            if (w_limit > 0.0 && w > w_limit) { w = w_limit; cl = 1; }
            else if (w_limit > 0.0 && w < -w_limit) { w = -w_limit; cl = 1; }
        }
        u[NU - 1] = w;
        if (k == 0) {
            hpo[0] = c; hpo[1] = s;
#pragma unroll
            for (int a = 0; a < DIM; ++a) hpo[2 + a] = p[a];
            if (DIM == 2) hpo[4] = 0.0;
        }
    }
    const int total = block_reduce(cl, OpAdd(), swi, nthr, 0);
    if (k == 0) clamped[blockIdx.x] = total;
