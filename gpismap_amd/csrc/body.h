// The robot's footprint (the contract: tests/body_ref.py): at most 16 balls fixed to the robot (discs in 2-D,
// spheres in 3-D), each an offset b[dim] in the body frame (x forward, y left, z up) and a radius rho >= 0 in double.  The host
// copy is the truth; the device table [16][4] = (b0, b1, b2, rho) is written by set() and read by the kernels of the calls that
// take the footprint, and by nothing between them: no consumer keeps a pointer into it.
// The body rule (body_clearance_at below) is the one statement of "the clearance of a body at a state": the sampling
// controller's rollouts (mppi.hip), the batch query (body.hip) and the trajectory check (traj.hip) share it.
#pragma once
#include <cmath>
#include "dev_common.h"
#include "dfield_sample.h"

namespace gpis {

struct DistanceField;

// what a kernel takes of a footprint
struct BodyArgs {
    const double* tab;               // [m][4]
    int m;
};

// where ball `row` = (b0, b1, b2, rho) of a body at position p with the heading (c, s) (a yaw about z) sits in the world; double,
// left to right
template <int D>
__device__ __forceinline__ void body_ball_at(const double* __restrict__ row, const double* p, double c, double s, double* w) {
    const double b0 = row[0], b1 = row[1];
    w[0] = p[0] + (c * b0 - s * b1);
    w[1] = p[1] + (s * b0 + c * b1);
    if constexpr (D == 3) w[2] = p[2] + row[2];
}

// The body rule.  d_j = (double)(the field's sample at the float32 cast of ball j's position) - rho_j; the result is the
// minimum over j ascending, from +inf, by (d_j < D ? d_j : D), *jmin the first j that attains it; a ball off the lattice (a NaN
// sample) makes the body off: NaN and -1.  L.dim must be D.  The table is walked by a pointer whose index is the same in every
// lane: its rows come through scalar loads, and nothing is indexed per lane.
template <int D>
__device__ __forceinline__ double body_clearance_at(const float* __restrict__ F, const DfLattice& L, const double* __restrict__ tab, int m,
                                                    const double* p, double c, double s, int* jmin = nullptr) {
    const double* __restrict__ row = tab;
    double best = INFINITY;
    int jm = 0;
    bool off = false;
    for (int j = 0; j < m; ++j, row += 4) {
        double w[3] = {0.0, 0.0, 0.0};
        body_ball_at<D>(row, p, c, s, w);
        float o[1 + D];
        df_sample_at(F, L, (float)w[0], (float)w[1], D == 3 ? (float)w[2] : 0.f, o);
        const double d = (double)o[0] - row[3];
        off = off || d != d;
        if (d < best) { best = d; jm = j; }
    }
    if (jmin) *jmin = off ? -1 : jm;
    return off ? (double)NAN : best;
}

struct Footprint {
    static constexpr int kMax = 16, kRow = 4;
    static constexpr long long kMaxStates = 1ll << 24;
    static constexpr int kBlock = 256;

    int device = -1;
    double* d_tab = nullptr;         // [kMax][kRow]
    bool inited = false;             // after the first set()
    int dim = 0, m = 0;
    double b[kMax][3], rho[kMax];

    // grow-only buffers of the batch query, overwritten by every call
    double* d_states = nullptr; size_t cap_states = 0;   // [n][dim + 2]
    double* d_D = nullptr;                               // [n]
    int* d_ball = nullptr;                               // [n]
    size_t cap_n = 0;
    double* d_bmin = nullptr;                            // [blocks] the block's least D (+inf: none)
    int* d_bint = nullptr;                               // [3][blocks] states below the clearance, states off, the least D's index
    size_t cap_b = 0;
    int* d_counts = nullptr;                             // [3]

    Footprint();
    ~Footprint();
    bool ok() const { return d_tab != nullptr; }
    // Arguments are checked by the caller.  Returns with the table on the device.
    int set(int dm, int cnt, const double* offset, const double* radius);
    // D [n], ball [n] and counts [3] of host states [n][dim + 2] on df's dist (df on this device, of this dim; m > 0); host
    // outputs, any may be nullptr.  Arguments are checked by the caller; synchronises `s`
    int clearance(const DistanceField& df, const double* states, long long n, double clr, double* D_out, int* ball_out, int* counts,
                  hipStream_t s);
};

}  // namespace gpis
