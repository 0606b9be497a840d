// The host side of the coverage mask (csrc/cover_host.h with csrc/frame.h) on its own: the diamond pseudo-angle, the sector table
// of a scan and the option checks.  Needs no GPU; meant to be compiled with -fsanitize=address,undefined and run directly.  Prints
// "FAILED: ..." per failed expectation, the sector table of a fixed 365-beam scan as "T <q bits> <lim bits> <narrow>" lines for the
// numpy reference to compare, and the number of failures last.
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
#include "frame.h"
#include "cover_host.h"
using namespace gpis;

static int bad = 0;
static void expect(bool ok, const char* what) { if (!ok) { std::printf("FAILED: %s\n", what); ++bad; } }
static uint64_t bits(double v) { uint64_t u; std::memcpy(&u, &v, 8); return u; }

static void table(const std::vector<float>& th, const std::vector<float>& r, float back_off, float max_gap, SectorTable* t) {
    const float off[2] = {0.f, 0.f};
    SensorFrame f;
    expect(frame_from_scan(th.data(), (long long)th.size(), off, &f) == GPIS_OK, "frame_from_scan");
    sector_table(f.cs.data(), r.data(), f.n, back_off, max_gap, t);
}

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const double pi = 3.14159265358979323846;
    // the pseudo-angle: its fixed points, and monotone in the angle all the way round
    expect(pseudo_angle(1, 0) == 0.0 && pseudo_angle(0, 1) == 1.0 && pseudo_angle(-1, 0) == 2.0 && pseudo_angle(0, -1) == 3.0, "axes");
    expect(pseudo_angle(1, 1) == 0.5 && pseudo_angle(-2, 2) == 1.5 && pseudo_angle(-3, -3) == 2.5 && pseudo_angle(0.5, -0.5) == 3.5, "diagonals");
    expect(pseudo_angle(1, -0.0) == 0.0, "s = -0");
    expect(std::isnan(pseudo_angle(0, 0)), "the origin");
    double prev = -1.0;
    bool mono = true, range = true;
    for (int k = 0; k < 100000; ++k) {
        const double a = 2 * pi * k / 100000.0, q = pseudo_angle(std::cos(a), std::sin(a));
        mono = mono && q > prev;
        range = range && q >= 0.0 && q < 4.0;
        prev = q;
    }
    expect(mono, "monotone in the angle");
    expect(range, "in [0, 4)");
    expect(pseudo_angle(1.0, -1e-300) <= 4.0 && pseudo_angle(1.0, -1e-300) > 3.9, "just below a full turn");

    // the sector search
    {
        const double q[4] = {0.5, 1.0, 1.0, 3.0};
        expect(sector_of(q, 4, 0.25) == 3 && sector_of(q, 4, 0.5) == 0 && sector_of(q, 4, 0.75) == 0, "before the first, on it, after it");
        expect(sector_of(q, 4, 1.0) == 2 && sector_of(q, 4, 2.0) == 2, "duplicates: the last of them");
        expect(sector_of(q, 4, 3.0) == 3 && sector_of(q, 4, 3.9) == 3, "the wrapping sector");
        expect(sector_of(q, 1, 0.1) == 0 && sector_of(q, 1, 0.9) == 0, "one beam");
    }

    // the option checks
    CoverOpts o;
    expect(cover_default_opts(2, 0.02f, &o) == GPIS_OK && o.back_off == 0.02f && o.clearance == 3.f * 0.02f && o.min_size == 8 &&
           o.max_rounds == 0 && o.max_gap == (float)(2.0 * (pi / 180.0)) && cover_check_opts(o) == GPIS_OK, "defaults");
    expect(cover_default_opts(4, 0.02f, &o) == GPIS_ERR_ARG && cover_default_opts(3, 0.f, &o) == GPIS_ERR_ARG &&
           cover_default_opts(3, nan, &o) == GPIS_ERR_ARG && cover_default_opts(3, 0.1f, nullptr) == GPIS_ERR_ARG, "bad default arguments");
    (void)cover_default_opts(3, 0.05f, &o);
    { CoverOpts b = o; b.clearance = b.back_off; expect(cover_check_opts(b) == GPIS_ERR_ARG, "clearance == back_off"); }
    { CoverOpts b = o; b.clearance = 0.f; expect(cover_check_opts(b) == GPIS_ERR_ARG, "clearance < back_off"); }
    { CoverOpts b = o; b.clearance = nan; expect(cover_check_opts(b) == GPIS_ERR_ARG, "clearance NaN"); }
    { CoverOpts b = o; b.clearance = inf; expect(cover_check_opts(b) == GPIS_ERR_ARG, "clearance inf"); }
    { CoverOpts b = o; b.back_off = -0.01f; expect(cover_check_opts(b) == GPIS_ERR_ARG, "back_off < 0"); }
    { CoverOpts b = o; b.back_off = 0.f; expect(cover_check_opts(b) == GPIS_OK, "back_off 0"); }
    { CoverOpts b = o; b.max_gap = 0.f; expect(cover_check_opts(b) == GPIS_ERR_ARG, "max_gap 0"); }
    { CoverOpts b = o; b.max_gap = (float)(pi / 2); expect(cover_check_opts(b) == GPIS_ERR_ARG, "max_gap 90 degrees"); }
    { CoverOpts b = o; b.max_gap = 1.5f; expect(cover_check_opts(b) == GPIS_OK, "max_gap 86 degrees"); }
    { CoverOpts b = o; b.max_gap = nan; expect(cover_check_opts(b) == GPIS_ERR_ARG, "max_gap NaN"); }
    { CoverOpts b = o; b.min_size = 0; expect(cover_check_opts(b) == GPIS_ERR_ARG, "min_size 0"); }
    { CoverOpts b = o; b.max_rounds = -1; expect(cover_check_opts(b) == GPIS_ERR_ARG, "max_rounds -1"); }

    // sector tables
    SectorTable t;
    const float gap = (float)(2.0 * (pi / 180.0));
    table({0.f, 0.01f, 0.02f}, {0.f, 0.1f, 40.f}, 0.01f, gap, &t);
    expect(t.size() == 0, "no valid beam");
    table({0.f, 0.01f, 0.02f}, {nan, 1.f, inf}, 0.01f, gap, &t);
    expect(t.size() == 1 && !t.narrow[0] && t.lim[0] == 1.0 - (double)0.01f && t.lim_eff[0] == 0.0, "one valid beam: its sector is a full turn");
    table({(float)(0.5 * pi / 180), (float)(359.5 * pi / 180)}, {2.f, 3.f}, 0.01f, gap, &t);
    expect(t.size() == 2 && t.q[0] < t.q[1] && !t.narrow[0] && t.narrow[1] && t.lim_eff[0] == 0.0 && t.lim_eff[1] == 2.0 - (double)0.01f,
           "two beams a degree apart across the turn");
    table({0.f, 0.01f}, {0.25f, 0.3f}, 0.5f, gap, &t);
    expect(t.size() == 2 && t.narrow[0] && t.lim[0] < 0.0 && t.lim_eff[0] == 0.0, "a sector that ends at the sensor");
    table({1.f, 1.f, 1.f}, {1.f, 2.f, 3.f}, 0.f, gap, &t);
    expect(t.size() == 3 && t.q[0] == t.q[2] && t.lim[0] == 1.0 && t.lim[1] == 2.0 && t.lim[2] == 1.0 && t.narrow[0] && t.narrow[1] && !t.narrow[2],
           "three beams of one direction keep their input order; the wrap is a full turn");

    // the table the reference compares: 365 beams in scrambled order with invalid ranges and a duplicate direction
    std::vector<float> th(365), rg(365);
    for (int k = 0; k < 365; ++k) {
        th[k] = (float)(-3.1 + 6.2 * ((k * 37) % 365) / 364.0);
        rg[k] = (float)(1.0 + 0.5 * ((k * 53) % 101) / 100.0);
        if (k % 11 == 3) rg[k] = 0.f;
    }
    rg[100] = 40.f;
    th[200] = th[17];
    table(th, rg, 0.02f, gap, &t);
    bool sorted = true;
    for (long long k = 1; k < t.size(); ++k) sorted = sorted && t.q[k - 1] <= t.q[k];
    expect(sorted && t.size() > 300, "sorted");
    for (long long k = 0; k < t.size(); ++k)
        std::printf("T %016" PRIx64 " %016" PRIx64 " %d\n", bits(t.q[k]), bits(t.lim[k]), (int)t.narrow[k]);
    std::printf("%d\n", bad);
    return bad != 0;
}
