// The world point of a sensor's local point at a float pose: a bit contract shared by the tracker (track.hip), the locator
// (locate.hip) and, through the locator's launch, the particle filter -- a pose scores against the very point the tracker
// samples for it.  Next to dfield_sample.h, which fixes the sample taken there.
#pragma once
#include <hip/hip_runtime.h>

namespace gpis {

// x = R l + t left to right in float (no FMA: -ffp-contract=off); R column-major (3-D R[0..8], t[0..2]; 2-D R[0..3], t[0..1])
template <int D>
__device__ __forceinline__ void world_point(const float* __restrict__ R, const float* __restrict__ t, const float4 l,
                                            float* __restrict__ x) {
    if constexpr (D == 3) {
        x[0] = R[0] * l.x + R[3] * l.y + R[6] * l.z + t[0];
        x[1] = R[1] * l.x + R[4] * l.y + R[7] * l.z + t[1];
        x[2] = R[2] * l.x + R[5] * l.y + R[8] * l.z + t[2];
    } else {
        x[0] = R[0] * l.x + R[2] * l.y + t[0];
        x[1] = R[1] * l.x + R[3] * l.y + t[1];
    }
}

}  // namespace gpis
