// The host side of the view scorer (csrc/view_host.h with csrc/frame.h) on its own: the option tail and its checks, the limits of
// a batch, and the order table of a scan's beams against cover_host.h's sector_table.  Needs no GPU; meant to be compiled with
// -fsanitize=address,undefined and run directly.  Prints "FAILED: ..." per failed expectation and the number of failures last.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
#include "frame.h"
#include "view_host.h"
using namespace gpis;

static int bad = 0;
static void expect(bool ok, const char* what) { if (!ok) { std::printf("FAILED: %s\n", what); ++bad; } }
static uint64_t bits(double v) { uint64_t u; std::memcpy(&u, &v, 8); return u; }

// the sector table of `ranges` built the way the device builds it -- the valid beams picked out of the order table, then
// sector_table's expressions -- against sector_table itself
static void compare(const SensorFrame& f, const std::vector<double>& q, const std::vector<int>& ord, const std::vector<float>& r,
                    float back_off, float max_gap, const char* what) {
    SectorTable t;
    sector_table(f.cs.data(), r.data(), f.n, back_off, max_gap, &t);
    std::vector<int> sel;
    for (long long j = 0; j < f.n; ++j) {
        const double rr = (double)r[ord[j]];
        if (rr > 0.2 && rr < 30.0) sel.push_back(ord[j]);
    }
    bool same = (long long)sel.size() == t.size();
    const size_t mv = sel.size();
    const double cg = std::cos((double)max_gap), bo = (double)back_off;
    for (size_t e = 0; same && e < mv; ++e) {
        const int a = sel[e], b = sel[e + 1 < mv ? e + 1 : 0];
        const double dq = e + 1 < mv ? q[b] - q[a] : (q[b] + 4.0) - q[a];
        const double dot = f.cs[2 * a] * f.cs[2 * b] + f.cs[2 * a + 1] * f.cs[2 * b + 1];
        const double ra = (double)r[a], rb = (double)r[b];
        const double l = (rb < ra ? rb : ra) - bo;
        const double le = (dq < 2.0 && dot >= cg && l > 0.0) ? l : 0.0;
        same = bits(q[a]) == bits(t.q[e]) && bits(le) == bits(t.lim_eff[e]);
    }
    expect(same, what);
}

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const double pi = 3.14159265358979323846;

    // the option tail
    gpis_view_opts o;
    std::memset(&o, 0, sizeof o);
    o.march.tfar = 30.f;
    expect(view_default_tail(2, 0.02f, &o) == GPIS_OK && o.back_off == 0.02f && o.max_gap == (float)(2.0 * (pi / 180.0)) &&
           o.miss == 30.f - 0.02f && o.min_dist == -inf && view_check_tail(o) == GPIS_OK, "defaults 2-D");
    o.march.tfar = 4.f;
    expect(view_default_tail(3, 0.05f, &o) == GPIS_OK && o.miss == 4.f - 0.05f && o.back_off == 0.05f, "defaults 3-D");
    expect(view_default_tail(4, 0.05f, &o) == GPIS_ERR_ARG && view_default_tail(3, 0.f, &o) == GPIS_ERR_ARG &&
           view_default_tail(3, nan, &o) == GPIS_ERR_ARG && view_default_tail(3, 0.05f, nullptr) == GPIS_ERR_ARG, "bad default arguments");
    { gpis_view_opts b = o; b.min_dist = nan; expect(view_check_tail(b) == GPIS_ERR_ARG, "min_dist NaN"); }
    { gpis_view_opts b = o; b.min_dist = inf; expect(view_check_tail(b) == GPIS_OK, "min_dist +inf"); }
    { gpis_view_opts b = o; b.min_dist = 0.1f; expect(view_check_tail(b) == GPIS_OK, "min_dist finite"); }
    { gpis_view_opts b = o; b.miss = nan; expect(view_check_tail(b) == GPIS_OK, "miss NaN"); }
    { gpis_view_opts b = o; b.miss = 0.f; expect(view_check_tail(b) == GPIS_OK, "miss 0"); }
    { gpis_view_opts b = o; b.miss = -inf; expect(view_check_tail(b) == GPIS_OK, "miss -inf"); }
    { gpis_view_opts b = o; b.back_off = -0.01f; expect(view_check_tail(b) == GPIS_ERR_ARG, "back_off < 0"); }
    { gpis_view_opts b = o; b.back_off = inf; expect(view_check_tail(b) == GPIS_ERR_ARG, "back_off inf"); }
    { gpis_view_opts b = o; b.back_off = 0.f; expect(view_check_tail(b) == GPIS_OK, "back_off 0"); }
    { gpis_view_opts b = o; b.max_gap = 0.f; expect(view_check_tail(b) == GPIS_ERR_ARG, "max_gap 0"); }
    { gpis_view_opts b = o; b.max_gap = (float)(pi / 2); expect(view_check_tail(b) == GPIS_ERR_ARG, "max_gap 90 degrees"); }
    { gpis_view_opts b = o; b.max_gap = nan; expect(view_check_tail(b) == GPIS_ERR_ARG, "max_gap NaN"); }

    // the limits of a batch
    expect(view_check_batch(0, 100) == GPIS_ERR_ARG && view_check_batch(-3, 100) == GPIS_ERR_ARG, "m < 1");
    expect(view_check_batch(1, 1) == GPIS_OK && view_check_batch(65536, 1024) == GPIS_OK && view_check_batch(1, 1ll << 26) == GPIS_OK, "at the limits");
    expect(view_check_batch(65537, 1) == GPIS_ERR_LIMIT && view_check_batch(65536, 1025) == GPIS_ERR_LIMIT &&
           view_check_batch(2, (1ll << 25) + 1) == GPIS_ERR_LIMIT && view_check_batch(1 << 30, 1ll << 40) == GPIS_ERR_LIMIT, "past the limits");

    // the order table: 365 beams in scrambled order with a duplicate direction
    std::vector<float> th(365);
    for (int k = 0; k < 365; ++k) th[k] = (float)(-3.1 + 6.2 * ((k * 37) % 365) / 364.0);
    th[200] = th[17];
    const float off[2] = {0.f, 0.f};
    SensorFrame f;
    expect(frame_from_scan(th.data(), (long long)th.size(), off, &f) == GPIS_OK, "frame_from_scan");
    std::vector<double> q;
    std::vector<int> ord;
    view_order_table(f.cs.data(), f.n, &q, &ord);
    bool sorted = q.size() == 365 && ord.size() == 365, perm = true;
    std::vector<int> hit(365, 0);
    for (size_t j = 0; j < ord.size(); ++j) {
        perm = perm && ord[j] >= 0 && ord[j] < 365 && !hit[ord[j]]++;
        if (j) sorted = sorted && (q[ord[j - 1]] < q[ord[j]] || (q[ord[j - 1]] == q[ord[j]] && ord[j - 1] < ord[j]));
    }
    expect(sorted, "ordered by q, equal q by index");
    expect(perm, "a permutation");
    for (int k = 0; k < 365; ++k) expect(bits(q[k]) == bits(pseudo_angle(f.cs[2 * k], f.cs[2 * k + 1])), "q bits");
    // the tables of several measurements over the one order: all valid, some invalid, one valid, none
    const float gap = (float)(2.0 * (pi / 180.0));
    std::vector<float> r(365);
    for (int k = 0; k < 365; ++k) r[k] = (float)(1.0 + 0.5 * ((k * 53) % 101) / 100.0);
    compare(f, q, ord, r, 0.02f, gap, "all beams valid");
    for (int k = 0; k < 365; ++k) if (k % 11 == 3) r[k] = 0.f;
    r[100] = 40.f; r[17] = 0.1f; r[250] = nan; r[251] = 29.98f;
    compare(f, q, ord, r, 0.02f, gap, "some beams invalid");
    compare(f, q, ord, r, 2.0f, 1.5f, "a back-off past every range, a wide gap");
    std::vector<float> one(365, 0.f);
    one[42] = 1.f;
    compare(f, q, ord, one, 0.02f, gap, "one valid beam");
    compare(f, q, ord, std::vector<float>(365, nan), 0.02f, gap, "no valid beam");
    // one beam
    const float t1[1] = {0.3f};
    expect(frame_from_scan(t1, 1, off, &f) == GPIS_OK, "one beam");
    view_order_table(f.cs.data(), f.n, &q, &ord);
    expect(q.size() == 1 && ord.size() == 1 && ord[0] == 0, "the order of one beam");
    std::printf("%d\n", bad);
    return bad != 0;
}
