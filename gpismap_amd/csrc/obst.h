// Moving obstacles (the contract: tests/obst_ref.py): a set of at most 256 balls (discs in 2-D, spheres in 3-D),
// each a centre, a constant velocity and a radius in double, with one epoch: the absolute time at which the centres hold.  Ball
// i at elapsed time e is at c_a + v_a * e per axis.  The set carries the cost options of its term in the controller's stage
// cost.  The host copy is the truth; the device table [n][8] = (c0, c1, c2, v0, v1, v2, r, 0) is written by set() and read
// by the kernels of the calls that take the set, and by nothing between them: no consumer keeps a pointer into it.
#pragma once
#include "dev_common.h"

namespace gpis {

struct ObstOpts {
    double clearance, margin, w_obs, w_col;
};

// what a kernel takes of a set: the table and the term's constants (band = clearance + margin)
struct ObstArgs {
    const double* tab;
    int n;
    double E0;                       // t_now - epoch
    double clearance, band, margin, w_obs, w_col;
};

struct Obstacles {
    static constexpr int kMax = 256, kRow = 8;

    int device = -1;
    double* d_tab = nullptr;         // [kMax][kRow]
    bool inited = false;             // after the first set()
    int dim = 0, n = 0;
    double epoch = 0.0;
    double c[kMax][3], v[kMax][3], r[kMax];
    ObstOpts opts = {0.0, 0.0, 0.0, 0.0};        // all zero (no cost, a hit below separation 0) until set_opts

    Obstacles();
    ~Obstacles();
    bool ok() const { return d_tab != nullptr; }
    // Arguments are checked by the caller.  Returns with the table on the device.
    int set(int dm, int cnt, const double* centre, const double* velocity, const double* radius, double ep);
    // centres [n][dim] at absolute time t: c_a + v_a * (t - epoch)
    void at(double t, double* out) const;
};

void obst_default_opts(int dim, float step, ObstOpts* o);
// GPIS_OK or GPIS_ERR_ARG: a non-finite option, a negative weight, clearance or margin
int obst_check_opts(const ObstOpts& o);

}  // namespace gpis
