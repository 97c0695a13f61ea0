// mp_probe_bufs.h — test infrastructure only: the device copies of one call of a probe library (mp_probe.hip, mp_probe_select.hip,
// mp_probe_acf.hip, mp_probe_post.hip, mp_probe_derive.hip, mp_probe_pointwise.hip, mp_probe_commit.hip, mp_probe_flows.hip,
// mp_probe_dense.hip, mp_probe_libm.hip, mp_probe_smc.hip, mp_probe_ladder.hip, mp_probe_reservoir.hip, mp_probe_bridge.hip, mp_probe_simulate.hip, mp_probe_reweight.hip).  Nothing here is part of libmagprop_amd.so.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

namespace mp {

namespace {

// the device copies of one call: every buffer uploaded at construction, the writable ones downloaded by finish()
struct Bufs {
    struct Out { void *host, *dev; size_t bytes; };
    std::vector<void *> all;
    std::vector<Out> outs;
    hipError_t err = hipSuccess;

    template <class T>
    const T *in(const T *host, size_t count) {
        return static_cast<const T *>(put(host, count * sizeof(T)));
    }
    template <class T>
    T *io(T *host, size_t count) {
        void *d = put(host, count * sizeof(T));
        if (d) outs.push_back({host, d, count * sizeof(T)});
        return static_cast<T *>(d);
    }
    // a device buffer that somebody else owns: the caller's bytes go into it now and come back with finish()
    template <class T>
    void adopt(T *host, T *dev, size_t count) {
        if (err != hipSuccess || !count) return;
        err = hipMemcpy(dev, host, count * sizeof(T), hipMemcpyHostToDevice);
        if (err == hipSuccess) outs.push_back({host, dev, count * sizeof(T)});
    }
    void *put(const void *host, size_t bytes) {
        if (err != hipSuccess) return nullptr;
        void *d = nullptr;
        err = hipMalloc(&d, bytes ? bytes : 1);
        if (err != hipSuccess) return nullptr;
        all.push_back(d);
        if (bytes) err = hipMemcpy(d, host, bytes, hipMemcpyHostToDevice);
        return err == hipSuccess ? d : nullptr;
    }
    bool ready() const { return err == hipSuccess; }
    int finish(int launch_rc) {   // after the launch
        if (err == hipSuccess) err = (hipError_t)launch_rc;
        if (err == hipSuccess) err = hipDeviceSynchronize();
        for (const Out &o : outs)
            if (err == hipSuccess && o.bytes) err = hipMemcpy(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost);
        return (int)err;
    }
    ~Bufs() {
        for (void *d : all) (void)hipFree(d);
    }
};

}  // namespace

}  // namespace mp
