// simulate_host_check.cpp — the host-only bracket rule of the simulated light curves (magprop_amd/csrc/mp_simulate.h obs_bracket,
// which mp_set_dataset digests a light curve with, and sim_bracket, which mp_simulate takes) under the address and
// undefined-behaviour sanitizers, on a machine without a GPU: on a geometric grid and on the smallest one, every knot, the
// neighbours of every knot, points inside every interval, with vectors of exactly the grid's size.  No HIP call is made; the
// argument checks of mp_simulate sit behind a handle and are tested on the device (tests/test_gpu_simulate.py).  From the
// repository root:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tools/simulate_host_check.cpp -o /tmp/simulate_host_check && /tmp/simulate_host_check
#include <cmath>
#include <cstdio>
#include <vector>

#include "../magprop_amd/csrc/mp_simulate.h"

static int n_failed = 0;

static void expect(bool ok, const char *what, double x) {
    if (!ok) { std::printf("FAILED: %s at x = %.17g\n", what, x); ++n_failed; }
}

static void check_point(const std::vector<double> &t, double x) {
    const int n = (int)t.size();
    int32_t g, gs;
    double dx, idt, dxs, idts;
    mp::obs_bracket(t, x, g, dx, idt);
    mp::sim_bracket(t, x, gs, dxs, idts);
    expect(g >= 0 && g <= n - 2, "obs_bracket keeps g inside the intervals", x);
    expect(t[g] <= x && (x < t[g + 1] || (g == n - 2 && x == t[n - 1])), "obs_bracket brackets x", x);
    expect(dx == x - t[g] && idt == 1.0 / (t[g + 1] - t[g]), "obs_bracket's dx and idt", x);
    expect(gs >= 0 && gs <= n - 1 && t[gs] <= x && (gs == n - 1 || x < t[gs + 1]), "sim_bracket: the largest knot at or below x", x);
    if (x == t[n - 1]) expect(gs == n - 1 && dxs == 0.0 && idts == 0.0, "sim_bracket puts the last point on its knot", x);
    else expect(gs == g && dxs == dx && idts == idt, "sim_bracket is obs_bracket off the last knot", x);
    expect((dxs == 0.0) == (x == t[gs]), "dx == 0 exactly on a knot", x);
}

static void check_grid(const std::vector<double> &t) {
    const int n = (int)t.size();
    for (int i = 0; i < n; ++i) {
        check_point(t, t[i]);
        if (i > 0) check_point(t, std::nextafter(t[i], -INFINITY));
        if (i < n - 1) {
            check_point(t, std::nextafter(t[i], INFINITY));
            check_point(t, 0.5 * (t[i] + t[i + 1]));
            check_point(t, t[i] + 0.001 * (t[i + 1] - t[i]));
        }
    }
}

int main() {
    std::vector<double> geo(10001);
    for (size_t i = 0; i < geo.size(); ++i) geo[i] = std::pow(10.0, 6.0 * (double)i / 10000.0);
    check_grid(geo);
    check_grid({1.0, 2.0});
    check_grid({-3.0, -1.0, 0.0, 1.0e-300, 5.0});
    std::printf(n_failed ? "%d checks FAILED\n" : "all checks passed\n", n_failed);
    return n_failed ? 1 : 0;
}
