// The set of moving balls (obst.h): host state and the upload of its device table.  The kernels that read the
// table are the controller's (mppi.hip).
#include <cmath>
#include <cstring>
#include "obst.h"

namespace gpis {

void obst_default_opts(int dim, float step, ObstOpts* o) {
    (void)dim;
    const double st = (double)step;
    o->clearance = st; o->margin = 4.0 * st; o->w_obs = 1.0; o->w_col = 100.0;
}

int obst_check_opts(const ObstOpts& o) {
    const double all[4] = {o.clearance, o.margin, o.w_obs, o.w_col};
    for (double v : all) if (!std::isfinite(v) || v < 0.0) return GPIS_ERR_ARG;
    return GPIS_OK;
}

Obstacles::Obstacles() {
    if (hipGetDevice(&device) != hipSuccess) { device = -1; return; }
    if (hipMalloc((void**)&d_tab, sizeof(double) * kMax * kRow) != hipSuccess) d_tab = nullptr;
    std::memset(c, 0, sizeof(c)); std::memset(v, 0, sizeof(v)); std::memset(r, 0, sizeof(r));
}

Obstacles::~Obstacles() {
    if (!d_tab) return;
    DeviceScope ds(device);
    (void)hipDeviceSynchronize();
    (void)hipFree(d_tab);
}

int Obstacles::set(int dm, int cnt, const double* centre, const double* velocity, const double* radius, double ep) {
    double tab[kMax][kRow];
    for (int i = 0; i < cnt; ++i) {
        for (int a = 0; a < 3; ++a) {
            tab[i][a] = a < dm ? centre[(size_t)i * dm + a] : 0.0;
            tab[i][3 + a] = a < dm ? velocity[(size_t)i * dm + a] : 0.0;
        }
        tab[i][6] = radius[i]; tab[i][7] = 0.0;
    }
    if (cnt > 0) {
        DeviceScope ds(device);
        GPIS_HIP(hipMemcpy(d_tab, tab, sizeof(double) * (size_t)cnt * kRow, hipMemcpyHostToDevice));      // (returns when it is there)
    }
    for (int i = 0; i < cnt; ++i) {
        for (int a = 0; a < 3; ++a) { c[i][a] = tab[i][a]; v[i][a] = tab[i][3 + a]; }
        r[i] = tab[i][6];
    }
    dim = dm; n = cnt; epoch = ep; inited = true;
    return GPIS_OK;
}

void Obstacles::at(double t, double* out) const {
    const double e = t - epoch;
    for (int i = 0; i < n; ++i)
        for (int a = 0; a < dim; ++a) out[(size_t)i * dim + a] = c[i][a] + v[i][a] * e;
}

}  // namespace gpis
