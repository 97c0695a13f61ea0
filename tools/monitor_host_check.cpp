// monitor_host_check.cpp — the host-only parts of the chain monitors' interface (magprop_amd/csrc/mp_monitor.h) under the address
// and undefined-behaviour sanitizers, on a machine without a GPU: the eight messages that MonitorNames::off and
// ChainMonitor::run_only build, the two forms of check_discard, ready's refusal of a bad ensemble, and capped / take / start_over.
// It compiles mp_monitor.cpp itself for the host, defines the `fail` that mp_capi.cpp defines in the library, and stands in for
// the kernel launchers, none of which it reaches; no HIP call is made.  From the repository root:
//
//   hipcc -x hip --offload-host-only -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tools/monitor_host_check.cpp -o /tmp/monitor_host_check && /tmp/monitor_host_check
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../magprop_amd/csrc/mp_monitor.cpp"

static std::string g_msg;

int fail(int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_msg = buf;
    return code;
}

namespace mp {
static int unreachable() { std::abort(); }
int launch_acf_accumulate(const AcfArgs &, void *) { return unreachable(); }
int launch_acf_finalise(const AcfArgs &, void *) { return unreachable(); }
int launch_post_reset(const PostArgs &, void *) { return unreachable(); }
int launch_post_accumulate(const PostArgs &, void *) { return unreachable(); }
int launch_thermo(const ThermoArgs &, void *) { return unreachable(); }
int launch_res_filter(const ResArgs &, void *) { return unreachable(); }
int launch_res_merge(const ResArgs &, void *) { return unreachable(); }
}  // namespace mp

static int n_failed = 0;

static void expect(bool ok, const char *what) {
    if (!ok) { std::printf("FAILED: %s (last message: %s)\n", what, g_msg.c_str()); ++n_failed; }
}
static void expect_msg(int rc, int code, const std::string &msg) {
    if (rc != code || g_msg != msg) { std::printf("FAILED: code %d, message \"%s\"; expected %d, \"%s\"\n", rc, g_msg.c_str(), code, msg.c_str()); ++n_failed; }
}

template <class M>
static void messages(const char *what, const char *setter) {
    const std::string w = what, s = setter;
    expect_msg(M::kNames.off("mp_get"), MP_ESTATE, "mp_get: " + w + " is off (" + s + ")");
    const M m(M::kNames, 8, 3, 2, 5, 100);
    const ChainMonitor &base = m;
    expect_msg(base.run_only("mp_sampler_step_apply"), MP_ESTATE,
               "mp_sampler_step_apply: " + w + " (" + s + ") is fed by mp_sampler_run only; turn it off first");
    expect_msg(base.ready("mp_get", 3, nullptr), MP_EINVAL, "mp_get: ensemble must be in [0, 3), got 3");
    expect_msg(base.ready("mp_get", -1, nullptr), MP_EINVAL, "mp_get: ensemble must be in [0, 3), got -1");
    expect(m.n_total == 24 && m.chunk_cap == 100 && m.discard == 5 && m.skip == 0 && m.n == 0, "the constructor's fields");
}

int main() {
    messages<AcfMonitor>("the autocorrelation monitor", "mp_sampler_set_autocorr");
    messages<PostMonitor>("the posterior monitor", "mp_sampler_set_posterior");
    messages<ThermoMonitor>("the thermodynamic monitor", "mp_sampler_set_thermo");
    messages<ResMonitor>("the sample reservoir", "mp_sampler_set_reservoir");

    expect(ChainMonitor::check_discard("f", 0) == MP_OK && ChainMonitor::check_discard("f", 1ll << 40) == MP_OK, "discard >= 0 passes");
    expect_msg(ChainMonitor::check_discard("f", -2), MP_EINVAL, "f: discard must be >= 0, got -2");
    expect_msg(ChainMonitor::check_discard("f", -2, " (-1 turns the monitor off)"), MP_EINVAL,
               "f: discard must be >= 0 (-1 turns the monitor off), got -2");
    expect_msg(AcfMonitor::check("f", 4, -1), MP_EINVAL, "f: discard must be >= 0, got -1");
    expect(AcfMonitor::check("f", 0, 0) == MP_OK && AcfMonitor::check("f", -1, -1) == MP_EINVAL && g_msg.find("max_lag") != std::string::npos,
           "max_lag is checked before discard");

    // capped: 8 walkers x 2 dimensions are 128 bytes a step, so 64 MB hold 524 288 steps; a step of 128 MB still gets a chunk of 1
    ThermoMonitor small(ThermoMonitor::kNames, 8, 1, 2, 3, (size_t)1 << 30), large(ThermoMonitor::kNames, 1 << 20, 1, 16, 0, 7);
    expect(small.capped(100) == 100 && small.capped(524288) == 524288 && small.capped(524289) == 524288 && small.chunk_cap == 524288, "capped, small rows");
    expect(small.capped(0) == 1 && large.capped(100) == 1 && large.chunk_cap == 1, "capped is 1 at least");

    // take: discard 3, chunks of 2, 4 and 5 steps; then the same again behind start_over
    for (int pass = 0; pass < 2; ++pass) {
        small.n = 99;
        small.start_over();
        int first = -1;
        expect(small.n == 0 && small.skip == 3, "start_over");
        expect(small.take(2, &first) == 0 && first == 2 && small.skip == 1, "a chunk inside the discard");
        expect(small.take(4, &first) == 3 && first == 1 && small.skip == 0, "the chunk the discard ends in");
        expect(small.take(5, &first) == 5 && first == 0 && small.skip == 0, "a chunk behind the discard");
        expect(small.take(0, &first) == 0 && first == 0, "an empty chunk");
    }
    if (n_failed) return 1;
    std::printf("monitor_host_check ok\n");
    return 0;
}
