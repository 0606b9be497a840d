// The host half of the detector (csrc/detect_host.h) on its own, to be built with -fsanitize=address,undefined and run directly:
// the option checks, the selection of 300 components with a cap of 256, and a dozen hand-made frames through the tracks.
// Prints every ball of every frame ("B frame id age missed comp c0 c1 v0 v1 r", doubles as hex bits) for
// tests/test_detect_host.py, which holds them against tests/detect_ref.py; the last line is the number of failed checks.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include "detect_host.h"

using namespace gpis;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { ++fails; printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); } } while (0)

static unsigned long long bits(double v) { unsigned long long b; std::memcpy(&b, &v, sizeof b); return b; }

// the frames' centres: a small linear congruential generator, the same in the test
static unsigned lcg(unsigned& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

int main() {
    DetectOpts o;
    CHECK(detect_default_opts(2, 0.1f, &o) == GPIS_OK && o.stride == 1 && o.min_points == 3 && o.alpha == 0.5);
    CHECK(o.min_dist == (double)(2.f * 0.1f) && o.link == (double)(3.f * 0.1f) && o.gate == (double)(4.f * 0.1f));
    CHECK(detect_default_opts(3, 0.1f, &o) == GPIS_OK && o.stride == 2);
    CHECK(detect_default_opts(4, 0.1f, &o) == GPIS_ERR_ARG && detect_default_opts(2, 0.f, &o) == GPIS_ERR_ARG);
    CHECK(detect_default_opts(2, 0.1f, nullptr) == GPIS_ERR_ARG && detect_default_opts(2, NAN, &o) == GPIS_ERR_ARG);
    CHECK(detect_check_opts(o) == GPIS_OK);
    { DetectOpts b = o; b.link = -1.0; CHECK(detect_check_opts(b) == GPIS_ERR_ARG); }
    { DetectOpts b = o; b.min_dist = NAN; CHECK(detect_check_opts(b) == GPIS_ERR_ARG); }
    { DetectOpts b = o; b.pad = INFINITY; CHECK(detect_check_opts(b) == GPIS_ERR_ARG); }
    { DetectOpts b = o; b.alpha = 0.0; CHECK(detect_check_opts(b) == GPIS_ERR_ARG); b.alpha = 1.0; CHECK(detect_check_opts(b) == GPIS_OK); }
    { DetectOpts b = o; b.alpha = 1.0000001; CHECK(detect_check_opts(b) == GPIS_ERR_ARG); }
    { DetectOpts b = o; b.stride = 0; CHECK(detect_check_opts(b) == GPIS_ERR_ARG); }
    { DetectOpts b = o; b.min_points = 0; CHECK(detect_check_opts(b) == GPIS_ERR_ARG); }
    { DetectOpts b = o; b.max_rounds = -1; CHECK(detect_check_opts(b) == GPIS_ERR_ARG); }

    // selection: 300 components; counts 1 but for a few, one of them too large, two below min_points = 1 never
    {
        std::vector<int> count(300, 1), flag, sel;
        std::vector<double> r2(300, 0.01);
        count[299] = 5; count[270] = 2; count[271] = 2; r2[3] = 4.0;
        DetectOpts s = o;
        s.min_points = 1; s.max_radius = 1.0;
        detect_select(300, count.data(), r2.data(), s, &flag, &sel);
        CHECK(sel.size() == 256 && flag[3] == kDetLarge && flag[299] == kDetBall && flag[270] == kDetBall && flag[271] == kDetBall);
        int dropped = 0;
        for (int c = 0; c < 300; ++c) dropped += flag[c] == kDetDropped;
        CHECK(dropped == 43 && flag[253] == kDetBall && flag[254] == kDetDropped && sel.front() == 0 && sel.back() == 299);
        for (size_t k = 1; k < sel.size(); ++k) CHECK(sel[k - 1] < sel[k]);
        s.min_points = 2;
        detect_select(300, count.data(), r2.data(), s, &flag, &sel);
        CHECK(sel.size() == 3 && flag[0] == kDetNoise);
        detect_select(0, nullptr, nullptr, s, &flag, &sel);
        CHECK(sel.empty() && flag.empty());
    }

    // tracks: 12 frames of 0 .. 7 balls
    DetectOpts to = o;
    (void)detect_default_opts(2, 0.1f, &to);
    to.gate = 0.5; to.max_missed = 3;
    DetTracks tr;
    unsigned seed = 12345u;
    double t = 0.0;
    for (int f = 0; f < 12; ++f) {
        t += 0.25;
        const int n = (int)(lcg(seed) % 8u);
        std::vector<DetBall> det((size_t)n);
        for (int j = 0; j < n; ++j) {
            det[j].c[0] = (double)(lcg(seed) % 2001u) / 1000.0 - 1.0;
            det[j].c[1] = (double)(lcg(seed) % 2001u) / 1000.0 - 1.0;
            det[j].r = 0.1; det[j].comp = j;
        }
        const std::vector<DetBall> out = detect_associate(2, det, t, to, &tr);
        CHECK(out.size() == tr.balls.size() && tr.held && tr.t_prev == t && (int)out.size() <= kDetectMaxBalls);
        for (const DetBall& b : out)
            printf("B %d %d %d %d %d %016llx %016llx %016llx %016llx %016llx\n", f, b.id, b.age, b.missed, b.comp, bits(b.c[0]), bits(b.c[1]),
                   bits(b.v[0]), bits(b.v[1]), bits(b.r));
    }
    tr.reset();
    CHECK(!tr.held && tr.balls.empty());

    // the cap holds with coasting balls: 250 old ones coast, 20 new ones arrive
    {
        DetTracks big;
        std::vector<DetBall> first(250), second(20);
        for (int j = 0; j < 250; ++j) { first[j].c[0] = 10.0 * j; first[j].comp = j; }
        for (int j = 0; j < 20; ++j) { second[j].c[0] = -100.0 - 10.0 * j; second[j].comp = j; }
        (void)detect_associate(2, first, 1.0, to, &big);
        const std::vector<DetBall> out = detect_associate(2, second, 2.0, to, &big);
        CHECK(out.size() == 256 && out[19].comp == 19 && out[20].comp == -1 && out[20].id == 0 && out[255].id == 235 && out[20].missed == 1);
    }
    printf("%d\n", fails);
    return fails ? 1 : 0;
}
