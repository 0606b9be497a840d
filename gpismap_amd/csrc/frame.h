// One sensor frame as every entry that takes one sees it: a depth image with its pinhole camera, or a laser scan
// with its beam angles and the sensor offset.  The two builders below are the only place where a frame is checked and the beam
// directions are computed; the trackers, the renderers, the locator and the particle filter all start from their result.
// Host code only: no HIP header, so the checks can be compiled and run on their own.
#pragma once
#include <cmath>
#include <vector>
#include "../../include/gpismap_amd.h"

namespace gpis {

// the sensor of one call (3-D: camera, depth image [width * height] column-major; 2-D: beams with host-double cos / sin, the
// map's sensor offset)
struct TrackGeom {
    int dim, width, height;
    float fx, fy, cx, cy;
    float off[2];
};

constexpr long long kMaxFramePoints = 1ll << 26;   // pixels / beams of one frame (Tracker::kMaxPoints, Renderer::kMaxRays)

struct SensorFrame {
    TrackGeom geo;
    long long n;               // pixels (width * height) / beams
    std::vector<double> cs;    // 2-D: cos, sin of beam k at [2k], [2k + 1]
    const double* cs_or_null() const { return geo.dim == 2 ? cs.data() : nullptr; }   // (a 3-D frame has no directions)
};

// A depth frame of camera (fx, fy, cx, cy) and (width, height).  GPIS_ERR_ARG: a size below 1, a focal length that is not finite
// or zero, a centre that is not finite; GPIS_ERR_LIMIT: more than kMaxFramePoints pixels.
inline int frame_from_camera(const float cam4[4], const int wh[2], SensorFrame* f) {
    f->geo = TrackGeom{3, wh[0], wh[1], cam4[0], cam4[1], cam4[2], cam4[3], {0.f, 0.f}};
    f->n = (long long)wh[0] * wh[1];
    f->cs.clear();
    if (wh[0] < 1 || wh[1] < 1 || !std::isfinite(cam4[0]) || !std::isfinite(cam4[1]) || cam4[0] == 0.f || cam4[1] == 0.f ||
        !std::isfinite(cam4[2]) || !std::isfinite(cam4[3]))
        return GPIS_ERR_ARG;
    return f->n > kMaxFramePoints ? GPIS_ERR_LIMIT : GPIS_OK;
}

// A scan frame of n beams and sensor offset off2.  The beam count is checked against kMaxFramePoints before one angle is read and
// before anything is allocated, so a count above it never reads past a short array.  GPIS_ERR_ARG: no angles, n < 1, an offset or
// an angle that is not finite; GPIS_ERR_LIMIT; GPIS_ERR_STATE: the direction table could not be allocated.  Nothing throws.
inline int frame_from_scan(const float* thetas, long long n, const float off2[2], SensorFrame* f) try {
    if (!thetas || n < 1) return GPIS_ERR_ARG;
    if (n > kMaxFramePoints) return GPIS_ERR_LIMIT;
    if (!std::isfinite(off2[0]) || !std::isfinite(off2[1])) return GPIS_ERR_ARG;
    f->geo = TrackGeom{2, 0, 0, 0.f, 0.f, 0.f, 0.f, {off2[0], off2[1]}};
    f->n = n;
    f->cs.resize((size_t)2 * n);
    for (long long k = 0; k < n; ++k) {
        if (!std::isfinite(thetas[k])) return GPIS_ERR_ARG;
        f->cs[2 * (size_t)k] = std::cos((double)thetas[k]);
        f->cs[2 * (size_t)k + 1] = std::sin((double)thetas[k]);
    }
    return GPIS_OK;
} catch (...) { return GPIS_ERR_STATE; }

}  // namespace gpis
