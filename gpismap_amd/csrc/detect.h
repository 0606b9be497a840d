// Moving obstacles from a frame's residual against a distance field (the contract: tests/detect_ref.py).  The
// tracker's set-up turns the frame into local points; one kernel takes each valid sample's world point (world_point.h) and the
// field's distance there (dfield_sample.h) and flags the sample as foreign where the field holds free space; the foreign samples
// are compacted (compact.h), linked to their neighbours on the sensor's own grid and labelled by min-label propagation with
// pointer jumping; every component gets a box, a centre and a squared radius by integer atomics.  The host (detect_host.h)
// selects the balls, associates them with those of the previous call and hands them to an Obstacles set.  Every device value is
// a minimum, a maximum or an integer sum, so the bits do not depend on the schedule.
#pragma once
#include <cstdint>
#include <vector>
#include "dev_common.h"
#include "components.h"
#include "detect_host.h"
#include "frame.h"
#include "track.h"

namespace gpis {

struct DistanceField;
struct Coverage;
struct Obstacles;

struct Detector {
    static constexpr int kBlock = 256;

    int device = -1;
    Tracker trk;                                 // the frame's set-up (its stream is the detector's own)
    bool profile = false;                        // synchronise at every stage's end, so that the stage times are the stages'

    // grow-only device buffers over the sample grid (beams; 3-D: W / stride x H / stride, column-major) ...
    float* d_x = nullptr;                        // world points [g][dim]
    float* d_d = nullptr;                        // the sampled distance (NaN: not valid, or off the lattice)
    unsigned char* d_flag = nullptr;             // 1: foreign
    int* d_rank = nullptr;                       // position in the list, -1 elsewhere
    int* d_limg = nullptr;        size_t cap_g = 0;   // the label image: the component's smallest grid index, -1 elsewhere
    // ... and over the foreign samples (comp.d_list: grid indices), their components and the table (components.h), per component
    // the words count, centre bits (3), r2 bits, label, unused (2) and the keys of the least and greatest coordinates; the
    // schedule is comp.check_every
    Components<unsigned> comp;

    // the last result
    bool valid = false;
    int dim = 0;
    long long grid = 0, gw = 0, gh = 0, samples = 0, foreign = 0, ncomp = 0, rounds = 0;
    long long noise = 0, large = 0, dropped = 0;
    double t_last = 0.0;
    double ms = 0.0, setup_ms = 0.0, flag_ms = 0.0, compact_ms = 0.0, label_ms = 0.0, table_ms = 0.0;
    // the component table in label order
    std::vector<int> c_label, c_count, c_flag;
    std::vector<float> c_box;                    // [c][6]: least, greatest
    std::vector<double> c_centre, c_r2;          // [c][3], [c]
    std::vector<DetBall> balls;                  // the current balls (detect_associate's order)
    DetTracks tracks;

    Detector();
    ~Detector();
    void clear_result() {
        valid = false; dim = 0; grid = gw = gh = samples = foreign = ncomp = rounds = noise = large = dropped = 0;
        c_label.clear(); c_count.clear(); c_flag.clear(); c_box.clear(); c_centre.clear(); c_r2.clear(); balls.clear();
    }
    int bind(int dev);
    // The checks of a call, all before anything is touched: GPIS_ERR_ARG, GPIS_ERR_STATE or GPIS_ERR_LIMIT (detect.hip).
    int check(const DistanceField& df, const Coverage* cover, const TrackGeom& geo, long long n, const double* pose, const DetectOpts& o,
              double t) const;
    // The whole call (after check): synchronises `s`.  The previous result is dropped at its start, so a failure from here on --
    // GPIS_ERR_LIMIT: max_rounds exceeded; GPIS_ERR_HIP: an allocation, a copy or a launch failed -- leaves no result; the
    // tracks stay as they were (they are updated last).
    int detect(const DistanceField& df, const Coverage* cover, const TrackGeom& geo, const float* in, const double* cs, long long n,
               const double* pose, const DetectOpts& o, double t, hipStream_t s);
    int to_obstacles(Obstacles& ob) const;
};

}  // namespace gpis
