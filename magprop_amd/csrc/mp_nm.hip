// mp_nm.hip — gfx950 kernels of the Nelder-Mead simplex search (include/magprop_amd.h mp_simplex_*): scipy's
// minimize(method="Nelder-Mead") with bounds, every iteration of every simplex one speculative launch and one small decision.
//
// nm_eval_kernel: one workgroup per (simplex, candidate), on the shell of mp_point.h.  All ndim + 4 points an iteration of the
// serial algorithm may ask for -- reflection, expansion, outside and inside contraction, the ndim shrunk vertices -- depend on the
// sorted simplex alone, so lane 0 builds its candidate from it in LDS, the workgroup evaluates it (point_eval) and lane 0 writes
// the candidate's row.  Nothing is written that another workgroup of the launch reads.  The initial evaluation runs the same grid
// on the vertices as they are.
// nm_decide_kernel: one workgroup per simplex behind every eval launch: scipy's decision tree on the candidates' values, the stable
// sort of the vertices, the counters and the stop rule for the next iteration.
#include <hip/hip_runtime.h>

#include "mp_nm.h"
#include "mp_point.h"

namespace mp {

namespace {

MP_DEV double nm_clip(const NmArgs &a, int d, double x) {
    x = x < a.lower[d] ? a.lower[d] : x;
    return x > a.upper[d] ? a.upper[d] : x;
}

// Candidate c of simplex s into t[0 .. ndim) (lane 0 only; runtime loops over the coordinates: t is LDS).  c = 0 reflection, 1
// expansion, 2 outside contraction, 3 inside contraction, 4 + (j - 1) the shrink of vertex j; initial: vertex c as it is.
MP_DEV void nm_build(const NmArgs &a, int s, int c, double *t) {
    const int N = a.ndim;
    const double *v = a.sim + (size_t)s * (N + 1) * N, *v0 = v, *vN = v + (size_t)N * N;
    if (a.initial) {
        for (int d = 0; d < N; ++d) t[d] = v[(size_t)c * N + d];
    } else if (c >= 4) {
        const double *vj = v + (size_t)(c - 3) * N;
        for (int d = 0; d < N; ++d) t[d] = nm_clip(a, d, add_rn(v0[d], mul_rn(a.sigma, sub_rn(vj[d], v0[d]))));
    } else {
        for (int d = 0; d < N; ++d) {
            double xbar = v[d];
            for (int j = 1; j < N; ++j) xbar = add_rn(xbar, v[(size_t)j * N + d]);
            xbar = xbar / (double)N;
            const double x = c == 3 ? add_rn(mul_rn(a.one_m_psi, xbar), mul_rn(a.psi, vN[d]))
                                    : sub_rn(mul_rn(a.ca[c], xbar), mul_rn(a.cb[c], vN[d]));
            t[d] = nm_clip(a, d, x);
        }
    }
}

// The builds of mp_point.h for the launch's n_simplex * (ndim + 4) candidates (launch_nm_eval).  Target 2, the terraces of
// point_eval, is this driver's: mp_simplex_create alone accepts it.
template <int SPL, bool LONG, int W = 1, int OCC = 0>
MP_POINT_KERNEL(SPL, W, OCC) void nm_eval_kernel(const DevShared sh, const NmArgs a) {
    const int nc = a.ndim + 4;
    const int k = (int)blockIdx.x, s = k / nc, c = k - s * nc;
    if (a.stopped[s]) return;                // frozen simplex (uniform for the workgroup): nothing to do
    if (a.initial && c > a.ndim) return;     // the initial evaluation has ndim + 1 points
    __shared__ PointLds<SPL, W> ws;
    __shared__ double park[MP_MAX_NDIM];     // the candidate across the evaluation
    tables_init<SPL * W, 64 * W>(sh, ws.tt);
    if (threadIdx.x == 0) nm_build(a, s, c, park);
    __syncthreads();
    double lnp;
    int status;
    point_eval<SPL, LONG, W, OCC>(sh, ws, a.ds_id, a.ndim, a.target, k, park, lnp, status);
    if (threadIdx.x == 0) {
        for (int d = 0; d < a.ndim; ++d) a.cand[(size_t)k * a.ndim + d] = park[d];
        a.cand_lnp[k] = lnp;
        a.cand_st[k] = status;
    }
}

// Behind an eval launch, with f = -lnprob.  An iteration: scipy's tree picks the candidate that replaces the worst vertex, or the
// shrink; then (and behind the initial evaluation, which takes its ndim + 1 candidates as the vertices) the stable sort by f, the
// counters and the stop rule for the next iteration.  Thread 0 decides, all threads move the rows: through LDS, so that the
// vertices are permuted in place.
__global__ __launch_bounds__(64) void nm_decide_kernel(const NmArgs a) {
    const int s = (int)blockIdx.x;
    if (a.stopped[s]) return;
    constexpr int kV = MP_MAX_NDIM + 1;
    const int N = a.ndim, nv = N + 1, nc = N + 4;
    __shared__ double row[kV * MP_MAX_NDIM];   // the new vertices, sorted
    __shared__ double fnew[kV];                // their f
    __shared__ int32_t stnew[kV];
    __shared__ int src[kV];                    // where sorted vertex j comes from: vertex src (< nv) or candidate src - nv
    double *const sim = a.sim + (size_t)s * nv * N;
    double *const lnp = a.lnp + (size_t)s * nv;
    int32_t *const st = a.st + (size_t)s * nv;
    const double *const cand = a.cand + (size_t)s * nc * N;
    const double *const clnp = a.cand_lnp + (size_t)s * nc;
    const int32_t *const cst = a.cand_st + (size_t)s * nc;
    if (threadIdx.x == 0) {
        int from[kV];      // unsorted: vertex j's source
        double f[kV];
        if (a.initial) {
            for (int j = 0; j < nv; ++j) { from[j] = nv + j; f[j] = -clnp[j]; }
            a.nfev[s] += nv;
            a.nit[s] = 1;
        } else {
            for (int j = 0; j < nv; ++j) { from[j] = j; f[j] = -lnp[j]; }
            const double fr = -clnp[0], fe = -clnp[1], fo = -clnp[2], fi = -clnp[3];
            int take = -1, outcome, evals = 2;   // take: the candidate that replaces vertex N (-1: shrink)
            if (fr < f[0]) {
                if (fe < fr) { take = 1; outcome = 1; }
                else { take = 0; outcome = 0; }
            } else if (fr < f[N - 1]) {
                take = 0; outcome = 0; evals = 1;
            } else if (fr < f[N]) {
                if (fo <= fr) { take = 2; outcome = 2; }
                else outcome = 4;
            } else {
                if (fi < f[N]) { take = 3; outcome = 3; }
                else outcome = 4;
            }
            if (take >= 0) {
                from[N] = nv + take;
                f[N] = -clnp[take];
            } else {
                for (int j = 1; j < nv; ++j) { from[j] = nv + 3 + j; f[j] = -clnp[3 + j]; }
                evals = N + 2;
            }
            a.nfev[s] += evals;
            a.nit[s] += 1;
            a.outcomes[(size_t)s * kNmOutcomes + outcome] += 1;
        }
        // stable insertion sort by f ascending: equal values keep their order (a replaced vertex sits last)
        int ord[kV];
        for (int j = 0; j < nv; ++j) {
            int i = j;
            while (i > 0 && f[j] < f[ord[i - 1]]) { ord[i] = ord[i - 1]; --i; }
            ord[i] = j;
        }
        for (int j = 0; j < nv; ++j) {
            const int o = from[ord[j]];
            src[j] = o;
            fnew[j] = f[ord[j]];
            stnew[j] = o < nv ? st[o] : cst[o - nv];
        }
    }
    __syncthreads();
    for (int i = (int)threadIdx.x; i < nv * N; i += 64) {
        const int j = i / N, d = i - j * N, o = src[j];
        row[i] = o < nv ? sim[(size_t)o * N + d] : cand[(size_t)(o - nv) * N + d];
    }
    __syncthreads();
    for (int i = (int)threadIdx.x; i < nv * N; i += 64) sim[i] = row[i];
    for (int j = (int)threadIdx.x; j < nv; j += 64) {
        lnp[j] = -fnew[j];
        st[j] = stnew[j];
    }
    if (threadIdx.x == 0) {
        // scipy's test at the top of its loop, for the next iteration: every term <=, so a NaN difference (inf - inf) means go on
        bool stop = true;
        for (int i = N; i < nv * N; ++i) stop = stop && fabs(sub_rn(row[i], row[i % N])) <= a.xatol;
        for (int j = 1; j < nv; ++j) stop = stop && fabs(sub_rn(fnew[0], fnew[j])) <= a.fatol;
        a.stopped[s] = stop ? 1 : 0;
    }
}

}  // namespace

// One workgroup per (simplex, candidate): n = n_simplex * (ndim + 4), fixed for the whole run, the initial evaluation included,
// stopped simplexes or not.
int launch_nm_eval(const DevShared &sh, const NmArgs &a, void *stream) {
    const int n = a.n_simplex * (a.ndim + 4);
    if (n <= 0) return 0;
    return launch_point_kernel(sh, n, [&](auto build, auto lng) {
        using B = decltype(build);
        hipLaunchKernelGGL((nm_eval_kernel<B::SPL, lng, B::W, B::OCC>), dim3((unsigned)n), dim3(64 * B::W), 0, (hipStream_t)stream, sh, a);
    });
}

int launch_nm_decide(const NmArgs &a, void *stream) {
    if (a.n_simplex <= 0) return 0;
    hipLaunchKernelGGL(nm_decide_kernel, dim3((unsigned)a.n_simplex), dim3(64), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

}  // namespace mp
