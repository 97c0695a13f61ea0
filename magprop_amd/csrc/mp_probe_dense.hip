// mp_probe_dense.hip — test infrastructure only: the read-out of a kept tile (mp_eval.hpp hermite, hermite_d, hermite5,
// hermite_mdisc, dense_mdisc_qs through image_state in both of its forms, mdot_fb / mdot_fb_d, tables_init) and the host-built
// tables those functions index (mp_capi.cpp build_tables), behind extern "C" host functions over HOST buffers
// (tests/test_gpu_dense_kernels.py, cases of tests/dense_cases.py).  Builds into its own libmp_probe_dense.so and links no
// product object: the functions under test are header templates, instantiated here from the very headers the kernels include.
// Nothing here is part of libmagprop_amd.so, of include/magprop_amd.h or of the product's ABI.
//
// The tables are never rebuilt here: every function that needs them takes an mp_handle * made by the product's mp_create in the
// same process and reads h->first()->sh, so what it sees is what the product built and uploaded.  Every mpi_* function
// uploads, launches once, synchronises and returns the writable buffers as the device holds them.  It returns 0, a hipError_t,
// or -1 for arguments it refuses; nothing is launched or written then.  Refused: everything outside the domain image_state is
// called on by walker_eval (pos8 <= p8 <= pos8 + keep d8, p8 = pos8 modulo 8 for kinds >= 1, 1 <= keep <= 64 G), so that no
// case can make a kernel leave its arrays.
#include <hip/hip_runtime.h>

#include <cmath>
#include <limits>

#include "mp_eval.hpp"
#include "mp_host.h"
#include "mp_probe_bufs.h"

namespace mp {

namespace {

constexpr int kMaxN = 1 << 16;          // elements / queries of one call
constexpr double kCanary = -777.0;      // what the LDS tables hold before tables_init runs

// every LDS table filled with the canary, so that an entry tables_init leaves uncopied shows
template <int G>
MP_DEV void lds_poison(TimeTable<G> &tt, int nt) {
    constexpr int kN = TimeTable<G>::kN;
    for (int i = threadIdx.x; i < kKtabN; i += nt) g_ktab[i] = kCanary;
    for (int i = threadIdx.x; i < kWtabSize; i += nt) g_wtab[i] = kCanary;
    for (int i = threadIdx.x; i < (kKinds - 1) * kN; i += nt) tt.E[i / kN][i % kN] = kCanary;
    __syncthreads();
}

template <int G, int NT>
__global__ void __launch_bounds__(NT) lds_tables_kernel(const DevShared sh, double *ktab, double *wtab, double *E) {
    __shared__ TimeTable<G> tt;
    constexpr int kN = TimeTable<G>::kN;
    lds_poison<G>(tt, NT);
    tables_init<G, NT>(sh, tt);
    for (int i = threadIdx.x; i < kKtabN; i += NT) ktab[i] = g_ktab[i];
    for (int i = threadIdx.x; i < kWtabSize; i += NT) wtab[i] = g_wtab[i];
    for (int i = threadIdx.x; i < (kKinds - 1) * kN; i += NT) E[i] = tt.E[i / kN][i % kN];
}

// in[9][n]: th, h, z, y0, d0, e0, y1, d1, e1; out[4][n]: hermite, hermite_d, hermite5, hermite_mdisc
__global__ void __launch_bounds__(64) hermite_kernel(const double *in, double *out, int n) {
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= n) return;
    const double th = in[q], h = in[n + q], z = in[2 * n + q], y0 = in[3 * n + q], d0 = in[4 * n + q], e0 = in[5 * n + q];
    const double y1 = in[6 * n + q], d1 = in[7 * n + q], e1 = in[8 * n + q];
    out[q] = hermite(th, h, y0, d0, y1, d1);
    out[n + q] = hermite_d(th, h, y0, d0, y1, d1);
    out[2 * n + q] = hermite5(th, h, y0, d0, e0, y1, d1, e1);
    out[3 * n + q] = hermite_mdisc(th, h, z, y0, d0, e0, y1, d1, e1);
}

// thread q owns the N times t[N q ..] and the constants S_amp[q], inv_tfb[q]; out[4][N nq]: mdot_fb, then mdot_fb_d's S, dS, iu
template <int N>
__global__ void __launch_bounds__(64) fallback_kernel(const double *S_amp, const double *inv_tfb, const double *t, double *out, int nq) {
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= nq) return;
    Walker w{};
    w.S_amp = S_amp[q];
    w.inv_tfb = inv_tfb[q];
    w.m53_inv_tfb = (-5.0 / 3.0) * w.inv_tfb;          // (as fill_walker of mp_eval.hpp forms it)
    Vd<N> tv, dS, iu;
    FORN tv[i] = t[(size_t)q * N + i];
    const Vd<N> a = mdot_fb<N>(w, tv), b = mdot_fb_d<N>(w, tv, dS, iu);
    const size_t n = (size_t)nq * N;
    FORN {
        const size_t e = (size_t)q * N + i;
        out[e] = a[i]; out[n + e] = b[i]; out[2 * n + e] = dS[i]; out[3 * n + e] = iu[i];
    }
}

// img[5][64 G + 1]: W, F, M, D, D2 of the image; out[2][n]: (Mv, Wv) of query p8[q].  Every workgroup of 64 lanes builds its
// own LDS tables and image, as a walker does.
template <int G>
__global__ void __launch_bounds__(64) image_state_kernel(const DevShared sh, const Walker w, int kind, int pos8, int keep, double t_s,
                                                         const double *img, const int32_t *p8, int n, double *out) {
    __shared__ TileImage<G> im;
    __shared__ TimeTable<G> tt;
    constexpr int kN = TileImage<G>::kN;
    lds_poison<G>(tt, 64);
    tables_init<G, 64>(sh, tt);
    const double nan = __builtin_nan("");
    for (int i = threadIdx.x; i < kN; i += 64) {
        im.W[i] = img[i]; im.F[i] = img[kN + i]; im.M[i] = img[2 * kN + i]; im.D[i] = img[3 * kN + i]; im.D2[i] = img[4 * kN + i];
        im.R[i] = nan;
    }
    if (threadIdx.x < 4) im.C[threadIdx.x] = nan;
    __syncthreads();
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= n) return;
    double Mv, Wv;
    image_state<G>(sh, w, im, tt, kind, pos8, keep, t_s, p8[q], Mv, Wv);
    out[q] = Mv;
    out[n + q] = Wv;
}

template <int G>
hipError_t launch_image_state(const DevShared &sh, const Walker &w, int kind, int pos8, int keep, double t_s, const double *img,
                              const int32_t *p8, int n, double *out) {
    image_state_kernel<G><<<(n + 63) / 64, 64>>>(sh, w, kind, pos8, keep, t_s, img, p8, n, out);
    return hipGetLastError();
}

}  // namespace

}  // namespace mp

using namespace mp;

extern "C" {

int mpi_kinds(void) { return kKinds; }
int mpi_wtab_size(void) { return kWtabSize; }
int mpi_wtab_stride(void) { return kWtabStride; }
int mpi_wtab_theta(void) { return kWtabTheta; }
int mpi_wtab_dense(void) { return kWtabDense; }
int mpi_ttab_n(void) { return kTtabN; }
int mpi_ktab_n(void) { return kKtabN; }
int mpi_max_n(void) { return kMaxN; }

// The tables of a handle as the device holds them: sk[kKinds][3] (lnQ, inv_Q, one_m_invQ), wtab[kWtabSize],
// ttab[kKinds - 1][kTtabN], scal[3] = t0, lnq8, pre_fine.
int mpi_tables(mp_handle *h, double *sk, double *wtab, double *ttab, double *scal) {
    if (!h || h->ev.empty() || !sk || !wtab || !ttab || !scal) return -1;
    Held held(h, h->first());
    if (!held.scope.ok) return (int)hipErrorInvalidDevice;
    const DevShared &sh = h->first()->sh;
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(wtab, sh.wtab, sizeof(double) * kWtabSize, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(ttab, sh.ttab, sizeof(double) * (kKinds - 1) * kTtabN, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return (int)e;
    for (int k = 0; k < kKinds; ++k) { sk[3 * k] = sh.sk[k].lnQ; sk[3 * k + 1] = sh.sk[k].inv_Q; sk[3 * k + 2] = sh.sk[k].one_m_invQ; }
    scal[0] = sh.t0; scal[1] = sh.lnq8; scal[2] = (double)sh.pre_fine;
    return 0;
}

// The LDS tables after tables_init<G, NT> in one workgroup of NT threads: ktab[kKtabN], wtab[kWtabSize], E[kKinds - 1][64 G + 1].
// (G, NT) = (2, 64), (4, 64), (4, 128), (4, 256): the instances the kernels use.
int mpi_lds_tables(mp_handle *h, int G, int NT, double *ktab, double *wtab, double *E) {
    if (!h || h->ev.empty() || !ktab || !wtab || !E) return -1;
    const int inst = G == 2 && NT == 64 ? 0 : G == 4 && NT == 64 ? 1 : G == 4 && NT == 128 ? 2 : G == 4 && NT == 256 ? 3 : -1;
    if (inst < 0) return -1;
    Held held(h, h->first());
    if (!held.scope.ok) return (int)hipErrorInvalidDevice;
    const DevShared &sh = h->first()->sh;
    Bufs B;
    double *dk = B.io(ktab, (size_t)kKtabN), *dw = B.io(wtab, (size_t)kWtabSize), *dE = B.io(E, (size_t)(kKinds - 1) * (64 * G + 1));
    if (!B.ready()) return B.finish(0);
    switch (inst) {
    case 0: lds_tables_kernel<2, 64><<<1, 64>>>(sh, dk, dw, dE); break;
    case 1: lds_tables_kernel<4, 64><<<1, 64>>>(sh, dk, dw, dE); break;
    case 2: lds_tables_kernel<4, 128><<<1, 128>>>(sh, dk, dw, dE); break;
    default: lds_tables_kernel<4, 256><<<1, 256>>>(sh, dk, dw, dE); break;
    }
    return B.finish((int)hipGetLastError());
}

// in[9][n] (th, h, z, y0, d0, e0, y1, d1, e1) -> out[4][n] (hermite, hermite_d, hermite5, hermite_mdisc)
int mpi_hermite(const double *in, int n, double *out) {
    if (!in || !out || n < 1 || n > kMaxN) return -1;
    Bufs B;
    const double *di = B.in(in, (size_t)9 * n);
    double *dout = B.io(out, (size_t)4 * n);
    if (!B.ready()) return B.finish(0);
    hermite_kernel<<<(n + 63) / 64, 64>>>(di, dout, n);
    return B.finish((int)hipGetLastError());
}

// mdot_fb<N> and mdot_fb_d<N> of nq threads: S_amp[nq], inv_tfb[nq], t[nq][N] -> out[4][nq N] (S of mdot_fb, S, dS, iu of mdot_fb_d)
int mpi_fallback(int N, const double *S_amp, const double *inv_tfb, const double *t, int nq, double *out) {
    if (!S_amp || !inv_tfb || !t || !out || nq < 1 || nq > kMaxN / 4 || (N != 1 && N != 2 && N != 4)) return -1;
    Bufs B;
    const double *ds = B.in(S_amp, (size_t)nq), *di = B.in(inv_tfb, (size_t)nq), *dt = B.in(t, (size_t)nq * N);
    double *dout = B.io(out, (size_t)4 * nq * N);
    if (!B.ready()) return B.finish(0);
    const int blocks = (nq + 63) / 64;
    if (N == 1) fallback_kernel<1><<<blocks, 64>>>(ds, di, dt, dout, nq);
    else if (N == 2) fallback_kernel<2><<<blocks, 64>>>(ds, di, dt, dout, nq);
    else fallback_kernel<4><<<blocks, 64>>>(ds, di, dt, dout, nq);
    return B.finish((int)hipGetLastError());
}

// image_state<G> (G = 2: the read-as-you-go form, G = 4: the batched one) of a tile of kind `kind` that started at pos8 / time t_s
// and kept `keep` steps, on the image img[5][64 G + 1] (W, F, M, D, D2), for the n queries p8[]: out[2][n] = (Mv, Wv).
// walker[3] = inv_tau, S_amp, inv_tfb.
int mpi_image_state(mp_handle *h, int G, const double *walker, int kind, int pos8, int keep, double t_s, const double *img,
                    const int32_t *p8, int n, double *out) {
    if (!h || h->ev.empty() || !walker || !img || !p8 || !out || (G != 2 && G != 4) || n < 1 || n > kMaxN) return -1;
    if (kind < 0 || kind >= kKinds || keep < 1 || keep > 64 * G || pos8 < 0 || pos8 > (1 << 28) || !(t_s > 0.0) || !std::isfinite(t_s)) return -1;
    const int sh8 = kind == 0 ? 0 : kind + 2, d8 = 1 << sh8;
    for (int q = 0; q < n; ++q) {
        if (p8[q] < pos8 || p8[q] > pos8 + keep * d8) return -1;
        if (kind >= 1 && ((p8[q] - pos8) & 7)) return -1;
    }
    Held held(h, h->first());
    if (!held.scope.ok) return (int)hipErrorInvalidDevice;
    const DevShared &sh = h->first()->sh;
    Walker w{};
    w.inv_tau = walker[0];
    w.S_amp = walker[1];
    w.inv_tfb = walker[2];
    w.m53_inv_tfb = (-5.0 / 3.0) * w.inv_tfb;
    Bufs B;
    const double *dimg = B.in(img, (size_t)5 * (64 * G + 1));
    const int32_t *dp = B.in(p8, (size_t)n);
    double *dout = B.io(out, (size_t)2 * n);
    if (!B.ready()) return B.finish(0);
    const hipError_t rc = G == 2 ? launch_image_state<2>(sh, w, kind, pos8, keep, t_s, dimg, dp, n, dout)
                                 : launch_image_state<4>(sh, w, kind, pos8, keep, t_s, dimg, dp, n, dout);
    return B.finish((int)rc);
}

}  // extern "C"
