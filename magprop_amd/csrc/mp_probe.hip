// mp_probe.hip — test infrastructure only: the device primitives of mp_math.hpp, one at a time, behind trivial kernels and
// extern "C" host functions mpp_* (tests/test_gpu_math.py).  Builds into its own libmp_probe.so; nothing here is part of
// libmagprop_amd.so, of include/magprop_amd.h or of the product's ABI.
//
// Every mpp_* function takes HOST pointers, allocates, copies, launches, synchronises and frees on the current device and
// returns 0, a hipError_t, or -1 for arguments it refuses (nothing is launched then).  One workgroup is one wavefront of 64
// lanes; lane l of wave w owns the elements (w * 64 + l) * N .. + N - 1 of every array, so the caller decides what every
// wavefront sees.  n, the number of elements, must be a positive multiple of 64 * N and at most 1 << 20.
#include <hip/hip_runtime.h>

#include <type_traits>
#include <vector>

#include "mp_device.h"
#include "mp_math.hpp"
#include "mp_probe_bufs.h"

namespace mp {

namespace {

constexpr int kMaxN = 1 << 20;

// first element of this lane, or -1 where the lane has none (never, for sizes the host accepted: n is a multiple of 64 * N)
template <int N>
MP_DEV long lane_base(int n) {
    const long b = ((long)blockIdx.x * 64 + threadIdx.x) * N;
    return b + N <= (long)n ? b : -1;
}
template <int N>
MP_DEV Vd<N> load(const double *p, long base, double fill) {
    Vd<N> v;
    FORN v[i] = base >= 0 ? p[base + i] : fill;
    return v;
}
template <int N>
MP_DEV void store(double *p, long base, const Vd<N> &v, int stride = 1, int off = 0) {
    if (base < 0) return;
    FORN p[(base + i) * stride + off] = v[i];
}

// ---------------------------------------------------------------- elementary functions
enum { kRcp, kRsqrt, kExp, kRcbrt, kPow17, kUnaryCount };

template <int F, int N>
__global__ void __launch_bounds__(64) unary_kernel(const double *x, double *y, int n) {
    ktab_init();
    const long base = lane_base<N>(n);
    const Vd<N> v = load<N>(x, base, 1.0);
    Vd<N> r;
    if constexpr (F == kRcp) r = rcp_fast(v);
    else if constexpr (F == kRsqrt) r = rsqrt_fast(v);
    else if constexpr (F == kExp) r = exp_fast(v);
    else if constexpr (F == kRcbrt) r = rcbrt_fast(v);
    else r = pow_m1_7_fast(v);
    store<N>(y, base, r);
}

__global__ void __launch_bounds__(64) exp10_kernel(const double *x, double *y, int n) {
    ktab_init();
    const long base = lane_base<1>(n);
    if (base >= 0) y[base] = exp10_fast(x[base]);
}

// ---------------------------------------------------------------- phi functions, node weights
// out[e][0 .. 6] = e^z, phi_1 .. phi_6 of element e
template <int N>
__global__ void __launch_bounds__(64) phi_kernel(const double *z, double *out, int n) {
    ktab_init();
    const long base = lane_base<N>(n);
    const Vd<N> v = load<N>(z, base, 0.0);
    const Phi5<N> p = phi12345(v);
    const Vd<N> p6 = phi6(v, p);
    store<N>(out, base, p.e, 7, 0);
    store<N>(out, base, p.p1, 7, 1);
    store<N>(out, base, p.p2, 7, 2);
    store<N>(out, base, p.p3, 7, 3);
    store<N>(out, base, p.p4, 7, 4);
    store<N>(out, base, p.p5, 7, 5);
    store<N>(out, base, p6, 7, 6);
}

// phi_6 next to a Phi5 whose phi_5 is the caller's p5 (the other members are not read by phi6)
template <int N>
__global__ void __launch_bounds__(64) phi6_kernel(const double *z, const double *p5, double *out, int n) {
    ktab_init();
    const long base = lane_base<N>(n);
    const Vd<N> v = load<N>(z, base, 0.0);
    Phi5<N> p;
    p.e = p.p1 = p.p2 = p.p3 = p.p4 = v;
    p.p5 = load<N>(p5, base, 0.0);
    store<N>(out, base, phi6(v, p));
}

// out[e][0 .. 4] = c_0 .. c_4 of element e, from the rows of tile kind `kind` of the caller's table
template <int N, bool PIPELINED>
__global__ void __launch_bounds__(64) weights_kernel(const double *wtab, int kind, const double *z, double *out, int n) {
    ktab_init();
    wtab_init(wtab);
    const long base = lane_base<N>(n);
    const Vd<N> v = load<N>(z, base, 0.0);
    const int wbase = kind * kWtabStride;
    EamW5<N> w;
    if constexpr (PIPELINED) {
        const EamRows2 rows = eam5_rows_begin(wbase);
        const Phi5<N> p = phi12345(v);
        w = eam5_node_weights_pipelined(wbase, p, rows);
    } else {
        const Phi5<N> p = phi12345(v);
        w = eam5_node_weights(wbase, p);
    }
    store<N>(out, base, w.c0, 5, 0);
    store<N>(out, base, w.c1, 5, 1);
    store<N>(out, base, w.c2, 5, 2);
    store<N>(out, base, w.c3, 5, 3);
    store<N>(out, base, w.c4, 5, 4);
}

// ---------------------------------------------------------------- wavefront primitives (one element per lane)
__global__ void __launch_bounds__(64) scan_kernel(const double *a, const double *b, double *oa, double *ob, int n) {
    const long base = lane_base<1>(n);
    double x = base >= 0 ? a[base] : 1.0, y = base >= 0 ? b[base] : 0.0;
    scan_affine(x, y);
    if (base >= 0) { oa[base] = x; ob[base] = y; }
}
__global__ void __launch_bounds__(64) lane_prev_kernel(const double *v, double first, double *out, int n) {
    const long base = lane_base<1>(n);
    const double r = lane_prev(base >= 0 ? v[base] : 0.0, first);
    if (base >= 0) out[base] = r;
}
__global__ void __launch_bounds__(64) lane_prev_map_kernel(const double *a, const double *b, double *pa, double *pb, int n) {
    const long base = lane_base<1>(n);
    double x, y;
    lane_prev_map(base >= 0 ? a[base] : 1.0, base >= 0 ? b[base] : 0.0, x, y);
    if (base >= 0) { pa[base] = x; pb[base] = y; }
}
__global__ void __launch_bounds__(64) lane_bcast_kernel(const double *v, int src, double *out, int n) {
    const long base = lane_base<1>(n);
    const double r = lane_bcast(base >= 0 ? v[base] : 0.0, src);
    if (base >= 0) out[base] = r;
}
__global__ void __launch_bounds__(64) uniform_kernel(const double *v, double *out, int n) {
    const long base = lane_base<1>(n);
    const double r = uniform(base >= 0 ? v[base] : 0.0);
    if (base >= 0) out[base] = r;
}
__global__ void __launch_bounds__(64) wave_sum_kernel(const double *v, double *out, int n) {
    const long base = lane_base<1>(n);
    const double r = wave_sum(base >= 0 ? v[base] : 0.0);
    if (base >= 0) out[base] = r;
}

// ---------------------------------------------------------------- extrema over the N values of a lane: out[n / N]
enum { kMaxAbs, kMinAbs, kMax, kMin, kExtCount };
template <int F, int N>
__global__ void __launch_bounds__(64) lane_ext_kernel(const double *v, double *out, int n) {
    const long base = lane_base<N>(n);
    const Vd<N> x = load<N>(v, base, 0.0);
    double r;
    if constexpr (F == kMaxAbs) r = lane_maxabs(x.v);
    else if constexpr (F == kMinAbs) r = lane_minabs(x.v);
    else if constexpr (F == kMax) r = lane_max(x.v);
    else r = lane_min(x.v);
    if (base >= 0) out[base / N] = r;
}

// ---------------------------------------------------------------- unfused arithmetic, composed as the moves compose it
__global__ void __launch_bounds__(64) unfused_kernel(const double *a, const double *b, const double *c, double *addmul, double *submul,
                                                     int n) {
    const long base = lane_base<1>(n);
    if (base < 0) return;
    addmul[base] = add_rn(mul_rn(a[base], b[base]), c[base]);
    submul[base] = sub_rn(a[base], mul_rn(b[base], c[base]));
}

// ---------------------------------------------------------------- log-sum-exp
// every lane folds its K terms into the empty pair, then the butterfly: m[n / K], s[n / K] hold every lane's pair
__global__ void __launch_bounds__(64) lse_kernel(const double *terms, int K, double *m, double *s, int n) {
    const long lane = (long)blockIdx.x * 64 + threadIdx.x;
    const bool ok = (lane + 1) * K <= (long)n;
    double mm = -INFINITY, ss = 0.0;
    for (int k = 0; k < K; ++k) lse_add(mm, ss, ok ? terms[lane * K + k] : -INFINITY);
    wave_lse(mm, ss);
    if (ok) { m[lane] = mm; s[lane] = ss; }
}
__global__ void __launch_bounds__(64) lse_merge_kernel(const double *m, const double *s, const double *mo, const double *so, double *om,
                                                       double *os, int n) {
    const long base = lane_base<1>(n);
    if (base < 0) return;
    double mm = m[base], ss = s[base];
    lse_merge(mm, ss, mo[base], so[base]);
    om[base] = mm;
    os[base] = ss;
}

// ---------------------------------------------------------------- index draws of the DE and snooker moves
// out[e][0 .. 2] = pick(u, m), pick_skip(u, m, c0), pick_skip2(u, m, c0, c1) of element e; -1 where m is below the draw's
// smallest size (2 for pick_skip, 3 for pick_skip2: what mp_sampler_set_moves enforces)
__global__ void __launch_bounds__(64) pick_kernel(const double *u, const double *m, const double *c0, const double *c1, double *out, int n) {
    const long base = lane_base<1>(n);
    if (base < 0) return;
    const int mm = (int)m[base], a = (int)c0[base], b = (int)c1[base];
    out[3 * base] = (double)pick(u[base], mm);
    out[3 * base + 1] = mm >= 2 ? (double)pick_skip(u[base], mm, a) : -1.0;
    out[3 * base + 2] = mm >= 3 ? (double)pick_skip2(u[base], mm, a, b) : -1.0;
}

// ---------------------------------------------------------------- host side
bool size_ok(int n, int per_lane) { return per_lane >= 1 && n >= 1 && n <= kMaxN && n % (64 * per_lane) == 0; }

// f(std::integral_constant<int, N>) for N in 1 .. 5; false for any other N
template <class F>
bool with_n(int N, F &&f) {
    switch (N) {
        case 1: f(std::integral_constant<int, 1>()); return true;
        case 2: f(std::integral_constant<int, 2>()); return true;
        case 3: f(std::integral_constant<int, 3>()); return true;
        case 4: f(std::integral_constant<int, 4>()); return true;
        case 5: f(std::integral_constant<int, 5>()); return true;
    }
    return false;
}
bool n124(int N) { return N == 1 || N == 2 || N == 4; }

template <int F>
void launch_unary(int N, const double *x, double *y, int n) {
    const dim3 g(n / (64 * N)), b(64);
    if (N == 1) unary_kernel<F, 1><<<g, b>>>(x, y, n);
    else if (N == 2) unary_kernel<F, 2><<<g, b>>>(x, y, n);
    else unary_kernel<F, 4><<<g, b>>>(x, y, n);
}
template <int F>
void launch_ext(int N, const double *x, double *y, int n) {
    with_n(N, [&](auto c) { lane_ext_kernel<F, decltype(c)::value><<<dim3(n / (64 * N)), dim3(64)>>>(x, y, n); });
}

}  // namespace

}  // namespace mp

using namespace mp;

extern "C" {

// func: 0 rcp_fast, 1 rsqrt_fast, 2 exp_fast, 3 rcbrt_fast, 4 pow_m1_7_fast; N = 1, 2, 4 values per lane
int mpp_unary(int func, int N, const double *x, double *y, int n) {
    if (func < 0 || func >= kUnaryCount || !n124(N) || !size_ok(n, N) || !x || !y) return -1;
    Bufs B;
    const double *dx = B.in(x, n);
    double *dy = B.io(y, n);
    if (B.ready()) {
        switch (func) {
            case kRcp: launch_unary<kRcp>(N, dx, dy, n); break;
            case kRsqrt: launch_unary<kRsqrt>(N, dx, dy, n); break;
            case kExp: launch_unary<kExp>(N, dx, dy, n); break;
            case kRcbrt: launch_unary<kRcbrt>(N, dx, dy, n); break;
            default: launch_unary<kPow17>(N, dx, dy, n); break;
        }
    }
    return B.finish((int)hipGetLastError());
}

int mpp_exp10(const double *x, double *y, int n) {
    if (!size_ok(n, 1) || !x || !y) return -1;
    Bufs B;
    const double *dx = B.in(x, n);
    double *dy = B.io(y, n);
    if (B.ready()) exp10_kernel<<<dim3(n / 64), dim3(64)>>>(dx, dy, n);
    return B.finish((int)hipGetLastError());
}

// out[n][7] = e^z, phi_1 .. phi_6
int mpp_phi(int N, const double *z, double *out, int n) {
    if (!n124(N) || !size_ok(n, N) || !z || !out) return -1;
    Bufs B;
    const double *dz = B.in(z, n);
    double *d = B.io(out, (size_t)n * 7);
    if (B.ready()) {
        const dim3 g(n / (64 * N)), b(64);
        if (N == 1) phi_kernel<1><<<g, b>>>(dz, d, n);
        else if (N == 2) phi_kernel<2><<<g, b>>>(dz, d, n);
        else phi_kernel<4><<<g, b>>>(dz, d, n);
    }
    return B.finish((int)hipGetLastError());
}

// out[n] = phi6(z, Phi5 with phi_5 = p5)
int mpp_phi6(int N, const double *z, const double *p5, double *out, int n) {
    if (!n124(N) || !size_ok(n, N) || !z || !p5 || !out) return -1;
    Bufs B;
    const double *dz = B.in(z, n), *dp = B.in(p5, n);
    double *d = B.io(out, n);
    if (B.ready()) {
        const dim3 g(n / (64 * N)), b(64);
        if (N == 1) phi6_kernel<1><<<g, b>>>(dz, dp, d, n);
        else if (N == 2) phi6_kernel<2><<<g, b>>>(dz, dp, d, n);
        else phi6_kernel<4><<<g, b>>>(dz, dp, d, n);
    }
    return B.finish((int)hipGetLastError());
}

// out[n][5] = c_0 .. c_4 from rows of tile kind `kind` of wtab[wtab_len] (wtab_len must be mp::kWtabSize)
int mpp_node_weights(int N, int pipelined, int kind, const double *wtab, int wtab_len, const double *z, double *out, int n) {
    if (!n124(N) || !size_ok(n, N) || kind < 0 || kind >= kKinds || wtab_len != kWtabSize || !wtab || !z || !out) return -1;
    Bufs B;
    const double *dw = B.in(wtab, kWtabSize), *dz = B.in(z, n);
    double *d = B.io(out, (size_t)n * 5);
    if (B.ready()) {
        const dim3 g(n / (64 * N)), b(64);
        if (pipelined) {
            if (N == 1) weights_kernel<1, true><<<g, b>>>(dw, kind, dz, d, n);
            else if (N == 2) weights_kernel<2, true><<<g, b>>>(dw, kind, dz, d, n);
            else weights_kernel<4, true><<<g, b>>>(dw, kind, dz, d, n);
        } else {
            if (N == 1) weights_kernel<1, false><<<g, b>>>(dw, kind, dz, d, n);
            else if (N == 2) weights_kernel<2, false><<<g, b>>>(dw, kind, dz, d, n);
            else weights_kernel<4, false><<<g, b>>>(dw, kind, dz, d, n);
        }
    }
    return B.finish((int)hipGetLastError());
}
int mpp_wtab_size(void) { return kWtabSize; }
int mpp_wtab_stride(void) { return kWtabStride; }

int mpp_scan_affine(const double *a, const double *b, double *oa, double *ob, int n) {
    if (!size_ok(n, 1) || !a || !b || !oa || !ob) return -1;
    Bufs B;
    const double *da = B.in(a, n), *db = B.in(b, n);
    double *xa = B.io(oa, n), *xb = B.io(ob, n);
    if (B.ready()) scan_kernel<<<dim3(n / 64), dim3(64)>>>(da, db, xa, xb, n);
    return B.finish((int)hipGetLastError());
}
int mpp_lane_prev(const double *v, double first, double *out, int n) {
    if (!size_ok(n, 1) || !v || !out) return -1;
    Bufs B;
    const double *dv = B.in(v, n);
    double *d = B.io(out, n);
    if (B.ready()) lane_prev_kernel<<<dim3(n / 64), dim3(64)>>>(dv, first, d, n);
    return B.finish((int)hipGetLastError());
}
int mpp_lane_prev_map(const double *a, const double *b, double *pa, double *pb, int n) {
    if (!size_ok(n, 1) || !a || !b || !pa || !pb) return -1;
    Bufs B;
    const double *da = B.in(a, n), *db = B.in(b, n);
    double *xa = B.io(pa, n), *xb = B.io(pb, n);
    if (B.ready()) lane_prev_map_kernel<<<dim3(n / 64), dim3(64)>>>(da, db, xa, xb, n);
    return B.finish((int)hipGetLastError());
}
int mpp_lane_bcast(const double *v, int src, double *out, int n) {
    if (!size_ok(n, 1) || src < 0 || src > 63 || !v || !out) return -1;
    Bufs B;
    const double *dv = B.in(v, n);
    double *d = B.io(out, n);
    if (B.ready()) lane_bcast_kernel<<<dim3(n / 64), dim3(64)>>>(dv, src, d, n);
    return B.finish((int)hipGetLastError());
}
int mpp_uniform(const double *v, double *out, int n) {
    if (!size_ok(n, 1) || !v || !out) return -1;
    Bufs B;
    const double *dv = B.in(v, n);
    double *d = B.io(out, n);
    if (B.ready()) uniform_kernel<<<dim3(n / 64), dim3(64)>>>(dv, d, n);
    return B.finish((int)hipGetLastError());
}
int mpp_wave_sum(const double *v, double *out, int n) {
    if (!size_ok(n, 1) || !v || !out) return -1;
    Bufs B;
    const double *dv = B.in(v, n);
    double *d = B.io(out, n);
    if (B.ready()) wave_sum_kernel<<<dim3(n / 64), dim3(64)>>>(dv, d, n);
    return B.finish((int)hipGetLastError());
}

// func: 0 lane_maxabs, 1 lane_minabs, 2 lane_max, 3 lane_min; N = 1 .. 5 values per lane; out[n / N]
int mpp_lane_ext(int func, int N, const double *v, double *out, int n) {
    if (func < 0 || func >= kExtCount || N < 1 || N > 5 || !size_ok(n, N) || !v || !out) return -1;
    Bufs B;
    const double *dv = B.in(v, n);
    double *d = B.io(out, n / N);
    if (B.ready()) {
        switch (func) {
            case kMaxAbs: launch_ext<kMaxAbs>(N, dv, d, n); break;
            case kMinAbs: launch_ext<kMinAbs>(N, dv, d, n); break;
            case kMax: launch_ext<kMax>(N, dv, d, n); break;
            default: launch_ext<kMin>(N, dv, d, n); break;
        }
    }
    return B.finish((int)hipGetLastError());
}

// addmul = add_rn(mul_rn(a, b), c), submul = sub_rn(a, mul_rn(b, c))
int mpp_unfused(const double *a, const double *b, const double *c, double *addmul, double *submul, int n) {
    if (!size_ok(n, 1) || !a || !b || !c || !addmul || !submul) return -1;
    Bufs B;
    const double *da = B.in(a, n), *db = B.in(b, n), *dc = B.in(c, n);
    double *x = B.io(addmul, n), *y = B.io(submul, n);
    if (B.ready()) unfused_kernel<<<dim3(n / 64), dim3(64)>>>(da, db, dc, x, y, n);
    return B.finish((int)hipGetLastError());
}

// terms[n], K per lane (1 .. 64); m[n / K], s[n / K]: the pair of every lane after lse_add over its terms and wave_lse
int mpp_lse(int K, const double *terms, double *m, double *s, int n) {
    if (K < 1 || K > 64 || !size_ok(n, K) || !terms || !m || !s) return -1;
    Bufs B;
    const double *dt = B.in(terms, n);
    double *dm = B.io(m, n / K), *ds = B.io(s, n / K);
    if (B.ready()) lse_kernel<<<dim3(n / (64 * K)), dim3(64)>>>(dt, K, dm, ds, n);
    return B.finish((int)hipGetLastError());
}
// (om, os) = lse_merge((m, s), (mo, so)) element by element
int mpp_lse_merge(const double *m, const double *s, const double *mo, const double *so, double *om, double *os, int n) {
    if (!size_ok(n, 1) || !m || !s || !mo || !so || !om || !os) return -1;
    Bufs B;
    const double *a = B.in(m, n), *b = B.in(s, n), *c = B.in(mo, n), *d = B.in(so, n);
    double *x = B.io(om, n), *y = B.io(os, n);
    if (B.ready()) lse_merge_kernel<<<dim3(n / 64), dim3(64)>>>(a, b, c, d, x, y, n);
    return B.finish((int)hipGetLastError());
}

// out[n][3] = pick(u, m), pick_skip(u, m, c0), pick_skip2(u, m, c0, c1) per element, the integers m, c0, c1 and the results as
// doubles; -1 where m < 2 (pick_skip) or m < 3 (pick_skip2).  Refused: u outside [0, 1), m outside 1 .. 2^20, c0 or c1 outside
// [0, m), c0 == c1 where m >= 3
int mpp_pick(const double *u, const double *m, const double *c0, const double *c1, double *out, int n) {
    if (!size_ok(n, 1) || !u || !m || !c0 || !c1 || !out) return -1;
    for (int i = 0; i < n; ++i) {
        if (!(u[i] >= 0.0) || !(u[i] < 1.0) || !(m[i] >= 1.0) || !(m[i] <= (double)kMaxN) || m[i] != (double)(int)m[i]) return -1;
        if (!(c0[i] >= 0.0) || !(c0[i] < m[i]) || c0[i] != (double)(int)c0[i]) return -1;
        if (!(c1[i] >= 0.0) || !(c1[i] < m[i]) || c1[i] != (double)(int)c1[i]) return -1;
        if (m[i] >= 3.0 && c0[i] == c1[i]) return -1;
    }
    Bufs B;
    const double *du = B.in(u, n), *dm = B.in(m, n), *d0 = B.in(c0, n), *d1 = B.in(c1, n);
    double *d = B.io(out, (size_t)n * 3);
    if (B.ready()) pick_kernel<<<dim3(n / 64), dim3(64)>>>(du, dm, d0, d1, d, n);
    return B.finish((int)hipGetLastError());
}

}  // extern "C"
