// reweight_host_check.cpp — the host-only rules of the importance reweighting (magprop_amd/csrc/mp_reweight.h
// reweight_bad_alternative and reweight_bad_weight, which mp_model_reweight judges its alternatives and observation weights with,
// and the constants its kernels rely on: whole groups of alternatives, and a tail row that fits the select kernel's LDS sort for
// every n the entry takes) under the address and undefined-behaviour sanitizers, on a machine without a GPU, with tables of
// exactly the stated sizes.  No HIP call is made; the order of the entry's refusals behind a handle is tested on the device
// (tests/test_gpu_reweight.py).  From the repository root:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tools/reweight_host_check.cpp -o /tmp/reweight_host_check && /tmp/reweight_host_check
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../magprop_amd/csrc/mp_reweight.h"

static int n_failed = 0;

static void expect(bool ok, const char *what) {
    if (!ok) { std::printf("FAILED: %s\n", what); ++n_failed; }
}

// the judgement of one alternative placed at `at` of a table of n_alt good ones
static int judge(int n_alt, int at, int32_t kind, double scale, double jitter, double nu) {
    std::vector<int32_t> k((size_t)n_alt);
    std::vector<double> a((size_t)n_alt * 3);
    for (int i = 0; i < n_alt; ++i) {
        k[(size_t)i] = i % 2 ? MP_REWEIGHT_STUDENT : MP_REWEIGHT_GAUSS;
        a[3 * (size_t)i] = 1.0 + 0.01 * i;
        a[3 * (size_t)i + 1] = 0.1 * (i % 3);
        a[3 * (size_t)i + 2] = 0.5 + i;
    }
    k[(size_t)at] = kind;
    a[3 * (size_t)at] = scale;
    a[3 * (size_t)at + 1] = jitter;
    a[3 * (size_t)at + 2] = nu;
    return mp::reweight_bad_alternative(n_alt, k.data(), a.data());
}

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double tiny = std::numeric_limits<double>::denorm_min(), huge = std::numeric_limits<double>::max();
    for (int n_alt : {1, 7, 8, 9, MP_REWEIGHT_MAX_ALT})
        for (int at : {0, n_alt / 2, n_alt - 1}) {
            expect(judge(n_alt, at, MP_REWEIGHT_GAUSS, 1.0, 0.0, 0.0) == -1, "a Gaussian of scale 1 and jitter 0 passes");
            expect(judge(n_alt, at, MP_REWEIGHT_GAUSS, tiny, huge, nan) == -1, "a Gaussian's nu is ignored, NaN included");
            expect(judge(n_alt, at, MP_REWEIGHT_GAUSS, 1.0, 0.0, -inf) == -1, "a Gaussian's nu is ignored, -inf included");
            expect(judge(n_alt, at, MP_REWEIGHT_STUDENT, huge, 0.0, tiny) == -1, "a Student-t of any finite nu > 0 passes");
            expect(judge(n_alt, at, 2, 1.0, 0.0, 1.0) == at, "kind 2 is refused");
            expect(judge(n_alt, at, -1, 1.0, 0.0, 1.0) == at, "kind -1 is refused");
            for (double bad : {0.0, -0.0, -1.0, inf, -inf, nan}) {
                expect(judge(n_alt, at, MP_REWEIGHT_GAUSS, bad, 0.0, 1.0) == at, "a scale not finite or not > 0 is refused");
                expect(judge(n_alt, at, MP_REWEIGHT_STUDENT, 1.0, 0.0, bad) == at, "a Student-t's nu not finite or not > 0 is refused");
            }
            for (double bad : {-tiny, -1.0, inf, -inf, nan})
                expect(judge(n_alt, at, MP_REWEIGHT_STUDENT, 1.0, bad, 1.0) == at, "a jitter not finite or < 0 is refused");
            expect(judge(n_alt, at, MP_REWEIGHT_GAUSS, 1.0, -0.0, 1.0) == -1, "a jitter of -0.0 passes");
        }
    // the first bad one is named
    {
        int32_t k[3] = {0, 5, 7};
        double a[9] = {1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0};
        expect(mp::reweight_bad_alternative(3, k, a) == 1, "the first refused alternative is the one named");
    }
    for (int64_t count : {(int64_t)1, (int64_t)50, (int64_t)MP_REWEIGHT_MAX_ALT * 1944}) {
        std::vector<double> w((size_t)count, 0.75);
        w[0] = 0.0;
        w[(size_t)count - 1] = huge;
        expect(mp::reweight_bad_weight(w.data(), count) == -1, "finite weights >= 0 pass, 0 included");
        for (double bad : {-tiny, -1.0, inf, -inf, nan}) {
            for (int64_t at : {(int64_t)0, count / 2, count - 1}) {
                const double keep = w[(size_t)at];
                w[(size_t)at] = bad;
                expect(mp::reweight_bad_weight(w.data(), count) == at, "a weight not finite or < 0 is refused where it stands");
                w[(size_t)at] = keep;
            }
        }
    }
    // the constants
    expect(MP_REWEIGHT_MAX_ALT % mp::kReweightGroup == 0, "the alternatives come in whole groups");
    expect(mp::kReweightThreads == mp::kPointwiseThreads, "the reductions are workgroups of the pointwise size");
    int longest = 0;
    for (int64_t n = 1; n <= MP_POINTWISE_MAX_SAMPLES; ++n) longest = std::max(longest, mp::pointwise_tail_len(n));
    expect(longest == mp::kPointwiseMaxTail && longest <= mp::kPointwiseSortCap, "every tail row fits the select kernel's sort");
    std::printf(n_failed ? "%d checks FAILED\n" : "all checks passed\n", n_failed);
    return n_failed ? 1 : 0;
}
