// The body of traj_obst_check_kernel and of traj_retime_check_kernel (traj.hip; DESIGN.md §7q, §7w), included into each with
// TRAJ_SCHED 0 or 1; shared as text for the reason traj_controls_body.inc gives.  TRAJ_SCHED 1: p_k is the position of the own
// slot own(k) of the trajectory's schedule `sc`, the balls are taken at the real slot k (dt is the slot, t0 is 0), and a
// schedule of status >= 2 answers as a trajectory without a timing.
    __shared__ float st[kTree];
    __shared__ double sp[kChunk + 1][DIM];
    __shared__ double shd[kBlock / 64];
    __shared__ unsigned long long shk[kBlock / 64];
    __shared__ int shi[kBlock / 64];
    const int tr = blockIdx.x, tid = threadIdx.x;
    const size_t base = (size_t)tr * N;
#if TRAJ_SCHED
    if (tint[(size_t)tr * 9] != 0 || sc.res[(size_t)tr * kSchedRes] >= 2 || n == 0) {
        if (tid == 0) {
            const bool timed = tint[(size_t)tr * 9] == 0 && sc.res[(size_t)tr * kSchedRes] < 2;
#else
    if (tint[(size_t)tr * 9] != 0 || n == 0) {
        if (tid == 0) {
            const bool timed = tint[(size_t)tr * 9] == 0;
#endif
            out_d[(size_t)tr * 2] = timed ? (double)INFINITY : (double)NAN; out_d[(size_t)tr * 2 + 1] = (double)NAN;
            out_i[(size_t)tr * 3] = -1; out_i[(size_t)tr * 3 + 1] = -1; out_i[(size_t)tr * 3 + 2] = 0;
        }
        return;
    }
    for (int i = tid; i < N; i += kBlock) st[i] = tt[base + i];
    double best = INFINITY, best_s = 0.0;
    int best_k = -1, best_i = -1, hit = 0x7fffffff;
    for (int k0 = 0; k0 < steps; k0 += kChunk) {
        const int cnt = min(kChunk, steps - k0);
        __syncthreads();                                 // (st is written; sp of the previous chunk is read)
        for (int j = tid; j <= cnt; j += kBlock) {
            double p[DIM];
#if TRAJ_SCHED
            traj_position<DIM, 1>(x + base * DIM, v + base, st, N, (double)sched_own(sc, tr, k0 + j) * dt, p);
#else
            traj_position<DIM>(x + base * DIM, v + base, st, N, t0 + (double)(k0 + j) * dt, p);
#endif
#pragma unroll
            for (int a = 0; a < DIM; ++a) sp[j][a] = p[a];
        }
        __syncthreads();
        for (int j = tid; j < cnt; j += kBlock) {
            const int k = k0 + j;
            const double e0 = TB + (t0 + (double)k * dt), e1 = TB + (t0 + (double)(k + 1) * dt);
            double p0[DIM], dp[DIM];
#pragma unroll
            for (int a = 0; a < DIM; ++a) { p0[a] = sp[j][a]; dp[a] = sp[j + 1][a] - p0[a]; }
            const double* __restrict__ row = tab;
            for (int i = 0; i < n; ++i, row += Obstacles::kRow) {
                double A[DIM], B[DIM], bb = 0.0, ab = 0.0;
#pragma unroll
                for (int a = 0; a < DIM; ++a) {
                    const double o0 = row[a] + row[3 + a] * e0, o1 = row[a] + row[3 + a] * e1;
                    A[a] = p0[a] - o0;
                    B[a] = dp[a] - (o1 - o0);
                    bb = a ? bb + B[a] * B[a] : B[a] * B[a];
                    ab = a ? ab + A[a] * B[a] : A[a] * B[a];
                }
                double s = 0.0;
                if (bb > 0.0) {
                    s = (-ab) / bb;
                    s = s > 0.0 ? s : 0.0;
                    s = s < 1.0 ? s : 1.0;
                }
                double s2 = 0.0;
#pragma unroll
                for (int a = 0; a < DIM; ++a) {
                    const double q = A[a] + s * B[a];
                    s2 = a ? s2 + q * q : q * q;
                }
                const double sep = sqrt(s2) - row[6];
                if (sep < best) { best = sep; best_s = s; best_k = k; best_i = i; }
                if (sep < clearance && k < hit) hit = k;
            }
        }
    }
    const double bmin = block_reduce(best, OpMin(), shd, kBlock, (double)INFINITY);
    if (tid == 0) shd[0] = bmin;
    __syncthreads();
    const double least = shd[0];
    unsigned long long key = best_k >= 0 && best == least ? ((unsigned long long)best_k << 8) | (unsigned long long)best_i : ~0ull;
    const unsigned long long kmin = block_reduce(key, OpMin(), shk, kBlock, ~0ull);
    if (tid == 0) shk[0] = kmin;
    __syncthreads();
    const unsigned long long win = shk[0];
    const int fh = block_reduce(hit, OpMin(), shi, kBlock, 0x7fffffff);
    if (tid == 0) {
        out_i[(size_t)tr * 3 + 1] = fh == 0x7fffffff ? -1 : fh;
        out_i[(size_t)tr * 3 + 2] = fh == 0x7fffffff ? 0 : 1;
        if (win == ~0ull) {                              // no separation was a number
            out_d[(size_t)tr * 2] = (double)INFINITY; out_d[(size_t)tr * 2 + 1] = (double)NAN; out_i[(size_t)tr * 3] = -1;
        }
    }
    if (key == win && win != ~0ull) {
        out_d[(size_t)tr * 2] = best;
        out_d[(size_t)tr * 2 + 1] = (t0 + (double)best_k * dt) + best_s * dt;
        out_i[(size_t)tr * 3] = best_i;
    }
