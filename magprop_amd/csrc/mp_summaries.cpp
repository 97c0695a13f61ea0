// mp_summaries.cpp — the summaries of model curves over host rows of parameters (mp_model_lc, mp_model_band*, mp_model_derived,
// mp_model_flows, mp_model_flow_band, mp_model_pointwise, mp_model_reweight, mp_simulate).  Kernels: mp_band.hip, mp_derive.hip,
// mp_flows.hip, mp_pointwise.hip, mp_reweight.hip, mp_simulate.hip.
//
// First what the entries share: the curve pass, which builds the curves of the rows on the device chunk by chunk and hands every
// chunk to the entry's own kernels and copies, and the band of curve matrices.  Then the entries, each on the handle's first
// evaluator under the handle's lock.
#include "mp_band.h"
#include "mp_derive.h"
#include "mp_flows.h"
#include "mp_host.h"
#include "mp_pointwise.h"
#include "mp_reweight.h"
#include "mp_simulate.h"

// ---------------------------------------------------------------- the curve pass
// What mp_model_lc, mp_model_band, mp_model_derived, mp_model_pointwise, mp_model_reweight, mp_simulate, mp_model_flows and mp_model_flow_band share: the curves of host rows pars[n][ndim], built on
// the device chunk by chunk and handed to the caller's own kernels and copies.  (The caller holds the evaluator, has validated its
// arguments and has ensured its own workspaces.)
// a set of curves: bit i is curve i of Ltot, Lprop, Ldip, Mdisc, omega
constexpr uint32_t kCurveLtot = 1u, kCurveLprop = 2u, kCurveLdip = 4u, kCurveTraj = 24u /* Mdisc and omega */, kCurveAll = 31u;

struct CurveChunk {
    size_t lo, cnt;          // rows [lo, lo + cnt) of the pass
    double *curve[5];        // [cnt][n_grid] each, in the order of the set's bits; nullptr: not wanted.  The wanted ones lie
                             // one behind the other, a chunk size of rows apart; rows of walkers that did not finish are
                             // NaN-filled by the kernel
    const int32_t *status;   // [cnt] on the device
    hipStream_t st;
};

// (everything that enqueues: curve_pass synchronises behind it whatever it returns)
template <class Consume>
static int curve_pass_enqueue(Evaluator *ev, const double *pars, size_t n, int ndim, int physical, uint32_t curves, size_t chunk,
                              std::vector<int32_t> &stt, Consume &consume) {
    const size_t ng = ev->tgrid.size(), rows = chunk * ng;
    hipStream_t st = ev->stream;
    HIP_TRY(hipMemcpyAsync(ev->w_pars.p, pars, sizeof(double) * n * (size_t)ndim, hipMemcpyHostToDevice, st));
    for (size_t lo = 0; lo < n; lo += chunk) {
        CurveChunk c{lo, std::min(chunk, n - lo), {}, ev->w_status.p + lo, st};
        for (int i = 0, k = 0; i < 5; ++i)
            if (curves & (1u << i)) c.curve[i] = ev->w_curves.p + (size_t)k++ * rows;
        mp::LaunchArgs a{};
        a.pars = ev->w_pars.p + lo * (size_t)ndim;
        a.n = (int32_t)c.cnt;
        a.ndim = ndim;
        a.physical = physical ? 1 : 0;
        a.want_chi2 = 0;                          // curves only: no dataset needed
        a.lnprob = ev->w_lnprob.p;
        a.status = ev->w_status.p + lo;
        a.ltot = c.curve[0];
        a.lprop = c.curve[1];
        a.ldip = c.curve[2];
        a.mdisc = c.curve[3];
        a.omega = c.curve[4];
        int rc;
        if ((rc = launch_lnprob_ordered(ev, a, st)) || (rc = consume(c))) return rc;
    }
    HIP_TRY(hipMemcpyAsync(stt.data(), ev->w_status.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
    return MP_OK;
}

// Uploads the rows once; per chunk of `chunk` rows, in stream order: the curve launch (curves: which of the five), then whatever
// consume(chunk) enqueues -- it returns MP_OK or the code of a failure it has reported; at the end the statuses of all rows, one
// synchronise, status_out (may be NULL) and the number of rows that finished.  Every failure behind the first enqueue
// synchronises the stream before it returns, so that nothing still writes the caller's buffers.
template <class Consume>
static int curve_pass(Evaluator *ev, const double *pars, size_t n, int ndim, int physical, uint32_t curves, size_t chunk,
                      int32_t *status_out, int64_t *n_used, Consume consume) {
    int rc;
    if ((rc = ev->w_pars.ensure(n * (size_t)ndim)) || (rc = ev->w_lnprob.ensure(chunk)) || (rc = ev->w_status.ensure(n)) ||
        (rc = ev->w_curves.ensure((size_t)__builtin_popcount(curves) * chunk * ev->tgrid.size())))
        return rc;
    std::vector<int32_t> stt(n);
    if ((rc = curve_pass_enqueue(ev, pars, n, ndim, physical, curves, chunk, stt, consume))) {
        (void)hipStreamSynchronize(ev->stream);
        return rc;
    }
    HIP_TRY(hipStreamSynchronize(ev->stream));
    if (status_out) std::memcpy(status_out, stt.data(), sizeof(int32_t) * n);
    if (n_used) *n_used = (int64_t)std::count(stt.begin(), stt.end(), (int32_t)MP_STATUS_OK);
    return MP_OK;
}

// ---------------------------------------------------------------- the band of curve matrices
// What mp_model_band, mp_model_band_weighted and mp_model_flow_band share.
// the argument checks (who: the entry's name), in the order they fail
static int check_band_args(const char *who, const mp_handle *h, const double *pars, int n, int ndim, const double *q, int nq,
                           const double *band_out) {
    if (!h || !pars || !q || !band_out) return fail(MP_EINVAL, "%s: NULL argument", who);
    if (n < 1 || n > MP_BAND_MAX_SAMPLES) return fail(MP_EINVAL, "%s: n must be 1..%d (MP_BAND_MAX_SAMPLES), got %d", who, MP_BAND_MAX_SAMPLES, n);
    if (ndim < 6 || ndim > MP_MAX_NDIM) return fail(MP_EINVAL, "%s: ndim must be 6..9, got %d", who, ndim);
    if (nq < 1 || nq > MP_BAND_MAX_Q) return fail(MP_EINVAL, "%s: nq must be 1..%d (MP_BAND_MAX_Q), got %d", who, MP_BAND_MAX_Q, nq);
    for (int j = 0; j < nq; ++j)
        if (!(q[j] >= 0.0 && q[j] <= 1.0)) return fail(MP_EINVAL, "%s: q[%d] = %g is not in [0, 1]", who, j, q[j]);
    return MP_OK;
}

// the workspaces of a band of ncurves curves over n rows (units: a weighted one), and its quantiles as the kernels take them
static int band_prepare(Evaluator *ev, int n, int ncurves, const double *q, int nq, bool units, mp::BandQ &bq) {
    const size_t ng = ev->tgrid.size();
    int rc;
    if ((rc = ev->w_band.ensure((size_t)n * ng)) || (rc = ev->w_band_out.ensure((size_t)ncurves * nq * ng))) return rc;
    if (units && (rc = ev->w_band_units.ensure((size_t)n))) return rc;
    bq = mp::BandQ{};
    for (int j = 0; j < nq; ++j) bq.q[j] = q[j];
    bq.nq = nq;
    return MP_OK;
}

// Enqueues the band of ncurves matrices [n][n_grid] (curve(k): the k-th; all rows are in them): the upload of the units (a
// weighted band; NULL: by rank), per matrix a transpose into point-major columns and the select -- by rank, or with units by
// cumulative units -- and the copy of band_out[ncurves][nq][n_grid].
template <class Curve>
static int band_enqueue(Evaluator *ev, int n, int ncurves, const mp::BandQ &bq, const uint32_t *units, double *band_out,
                        hipStream_t st, Curve curve) {
    const size_t ng = ev->tgrid.size();
    if (units) HIP_TRY(hipMemcpyAsync(ev->w_band_units.p, units, sizeof(uint32_t) * (size_t)n, hipMemcpyHostToDevice, st));
    for (int k = 0; k < ncurves; ++k) {
        double *out = ev->w_band_out.p + (size_t)k * bq.nq * ng;
        int e = mp::launch_band_transpose(curve(k), ev->w_band.p, n, (int)ng, (void *)st);
        if (!e) e = units ? mp::launch_band_wselect(ev->w_band.p, ev->w_band_units.p, n, (int)ng, bq, out, (void *)st)
                          : mp::launch_band_select(ev->w_band.p, n, (int)ng, bq, out, (void *)st);
        if (e) return fail(MP_EHIP, "band kernel launch failed: %s", hipGetErrorString((hipError_t)e));
    }
    HIP_TRY(hipMemcpyAsync(band_out, ev->w_band_out.p, sizeof(double) * (size_t)ncurves * bq.nq * ng, hipMemcpyDeviceToHost, st));
    return MP_OK;
}

extern "C" {

int mp_model_lc(mp_handle *h, const double *pars, int ndim, double *out, double *traj, int32_t *status) {
    if (!h || !pars || !out) return fail(MP_EINVAL, "mp_model_lc: NULL argument");
    if (ndim < 6 || ndim > MP_MAX_NDIM) return fail(MP_EINVAL, "mp_model_lc: ndim must be 6..9, got %d", ndim);
    Evaluator *ev = h->first();   // one walker, one device: the first
    Held held(h, ev);
    const size_t ng = ev->tgrid.size();
    return curve_pass(ev, pars, 1, ndim, 1, kCurveAll, 1, status, nullptr, [&](const CurveChunk &c) {
        std::memcpy(out, ev->tgrid.data(), sizeof(double) * ng);
        // (a chunk of one row: its five curves are one block)
        HIP_TRY(hipMemcpyAsync(out + ng, c.curve[0], sizeof(double) * 3 * ng, hipMemcpyDeviceToHost, c.st));
        if (traj) HIP_TRY(hipMemcpyAsync(traj, c.curve[3], sizeof(double) * 2 * ng, hipMemcpyDeviceToHost, c.st));
        return (int)MP_OK;
    });
}

// mp_model_band and mp_model_band_weighted (who; units[n]: the weighted one, the weights already in integer units): one launch of
// all n rows (the curve build kernel_spl_curves names depends on the launch size), then the band of the wanted components.
static int model_band(const char *who, mp_handle *h, const double *pars, int n, int ndim, int physical, const uint32_t *units,
                      const double *q, int nq, uint32_t components, double *band_out, int32_t *status_out, int32_t *n_used) {
    int rc;
    if ((rc = check_band_args(who, h, pars, n, ndim, q, nq, band_out))) return rc;
    static_assert(MP_BAND_LTOT == kCurveLtot && MP_BAND_LPROP == kCurveLprop && MP_BAND_LDIP == kCurveLdip, "a component mask is a curve set");
    const uint32_t all = MP_BAND_LTOT | MP_BAND_LPROP | MP_BAND_LDIP;
    if (components == 0 || (components & ~all)) return fail(MP_EINVAL, "%s: components 0x%x is not a non-empty mask of MP_BAND_*", who, components);
    Evaluator *ev = h->first();
    Held held(h, ev);
    const int ncomp = __builtin_popcount(components);
    mp::BandQ bq;
    if ((rc = band_prepare(ev, n, ncomp, q, nq, units != nullptr, bq))) return rc;
    int64_t used = 0;
    rc = curve_pass(ev, pars, (size_t)n, ndim, physical, components, (size_t)n, status_out, &used, [&](const CurveChunk &c) {
        const double *wanted[3];
        for (int i = 0, k = 0; i < 3; ++i)
            if (c.curve[i]) wanted[k++] = c.curve[i];
        return band_enqueue(ev, n, ncomp, bq, units, band_out, c.st, [&](int k) { return wanted[k]; });
    });
    if (!rc && n_used) *n_used = (int32_t)used;
    return rc;
}

int mp_model_band(mp_handle *h, const double *pars, int n, int ndim, int physical, const double *q, int nq, uint32_t components,
                  double *band_out, int32_t *status_out, int32_t *n_used) {
    return model_band("mp_model_band", h, pars, n, ndim, physical, nullptr, q, nq, components, band_out, status_out, n_used);
}

int mp_band_weight_units(const double *weights, int n, uint32_t *units_out) {
    if (!weights || !units_out) return fail(MP_EINVAL, "mp_band_weight_units: NULL argument");
    if (n < 1) return fail(MP_EINVAL, "mp_band_weight_units: n must be at least 1, got %d", n);
    if (!mp::band_weight_units(weights, n, units_out))
        return fail(MP_EINVAL, "mp_band_weight_units: the weights must be finite and >= 0 with at least one > 0");
    return MP_OK;
}

int mp_model_band_weighted(mp_handle *h, const double *pars, int n, int ndim, int physical, const double *weights, const double *q,
                           int nq, uint32_t components, double *band_out, int32_t *status_out, int32_t *n_used) {
    // (the weights first: they are judged without a handle)
    if (!weights) return fail(MP_EINVAL, "mp_model_band_weighted: NULL argument");
    if (n < 1 || n > MP_BAND_MAX_SAMPLES)
        return fail(MP_EINVAL, "mp_model_band_weighted: n must be 1..%d (MP_BAND_MAX_SAMPLES), got %d", MP_BAND_MAX_SAMPLES, n);
    std::vector<uint32_t> units((size_t)n);
    if (!mp::band_weight_units(weights, n, units.data()))
        return fail(MP_EINVAL, "mp_model_band_weighted: the weights must be finite and >= 0 with at least one > 0");
    return model_band("mp_model_band_weighted", h, pars, n, ndim, physical, units.data(), q, nq, components, band_out, status_out, n_used);
}

// The rows go through the device in chunks of n_simd rows: five curves of a chunk are the workspace, and every chunk runs the
// curve build kernel_spl_curves names for n <= n_simd, the one mp_model_lc runs for a single row.
int mp_model_derived(mp_handle *h, const double *pars, int64_t n, int ndim, int physical, double *out, int32_t *status_out,
                     int64_t *n_used) {
    // (the sizes first: they can be judged without a handle)
    if (n < 1) return fail(MP_EINVAL, "mp_model_derived: n must be at least 1, got %lld", (long long)n);
    if (ndim < 6 || ndim > MP_MAX_NDIM) return fail(MP_EINVAL, "mp_model_derived: ndim must be 6..9, got %d", ndim);
    if (!h || !pars || !out) return fail(MP_EINVAL, "mp_model_derived: NULL argument");
    Evaluator *ev = h->first();
    Held held(h, ev);
    const size_t chunk = (size_t)std::min<int64_t>(n, std::max(1, ev->sh.n_simd));
    int rc;
    if ((rc = ev->w_derive_out.ensure(chunk * MP_DERIVED_N))) return rc;
    return curve_pass(ev, pars, (size_t)n, ndim, physical, kCurveAll, chunk, status_out, n_used, [&](const CurveChunk &c) {
        mp::DeriveArgs d{};
        for (int i = 0; i < 5; ++i) d.curve[i] = c.curve[i];
        d.status = c.status;
        d.tgrid = ev->d_tgrid.p;
        d.out = ev->w_derive_out.p;
        d.n = (int32_t)c.cnt;
        d.n_grid = (int32_t)ev->tgrid.size();
        const int e = mp::launch_derive(d, (void *)c.st);
        if (e) return fail(MP_EHIP, "derive kernel launch failed: %s", hipGetErrorString((hipError_t)e));
        const hipError_t ce = hipMemcpyAsync(out + c.lo * MP_DERIVED_N, ev->w_derive_out.p, sizeof(double) * c.cnt * MP_DERIVED_N, hipMemcpyDeviceToHost, c.st);
        if (ce != hipSuccess) return fail(MP_EHIP, "mp_model_derived: copy failed: %s", hipGetErrorString(ce));
        return (int)MP_OK;
    });
}

// The cells launch of mp_model_flows and mp_model_flow_band behind a chunk's curve launch: the chunk's Mdisc and omega rows, its
// parameter rows and statuses into the cell curves `mask`, curve c at cells + (its position in the mask) * curve_stride +
// row_lo * n_grid.
static int flow_cells_enqueue(Evaluator *ev, const CurveChunk &c, int ndim, int physical, uint32_t mask, double *cells,
                              size_t curve_stride, size_t row_lo, mp::FlowCellsArgs &f) {
    const size_t ng = ev->tgrid.size();
    f = mp::FlowCellsArgs{};
    f.mdisc = c.curve[3];
    f.omega = c.curve[4];
    f.t = ev->d_tgrid.p;
    f.t_row_stride = 0;
    f.pars = ev->w_pars.p + c.lo * (size_t)ndim;
    f.status = c.status;
    for (int i = 0, k = 0; i < MP_FLOW_NCURVES; ++i)
        if (mask & (1u << i)) f.cell[i] = cells + (size_t)k++ * curve_stride + row_lo * ng;
    f.rows = (int32_t)c.cnt;
    f.n_grid = (int32_t)ng;
    f.ndim = ndim;
    f.physical = physical ? 1 : 0;
    const int e = mp::launch_flow_cells(ev->sh, f, (void *)c.st);
    if (e) return fail(MP_EHIP, "flow cells kernel launch failed: %s", hipGetErrorString((hipError_t)e));
    return MP_OK;
}

// The rows go through the device in chunks of n_simd rows as in mp_model_derived, with the Mdisc and omega curves alone: every
// chunk's curve launch is followed by the cells launch (the curves the reduction reads and the ones the caller wants), the
// reduction launch and the copies.
int mp_model_flows(mp_handle *h, const double *pars, int64_t n, int ndim, int physical, double *out, uint32_t curve_mask,
                   double *curves_out, int32_t *status_out, int64_t *n_used) {
    // (the sizes first: they can be judged without a handle)
    if (n < 1) return fail(MP_EINVAL, "mp_model_flows: n must be at least 1, got %lld", (long long)n);
    if (ndim < 6 || ndim > MP_MAX_NDIM) return fail(MP_EINVAL, "mp_model_flows: ndim must be 6..9, got %d", ndim);
    if (curve_mask & ~mp::kFlowAllMask) return fail(MP_EINVAL, "mp_model_flows: curve_mask 0x%x is not a mask of MP_FLOW_CURVE_* bits", curve_mask);
    if (!h || !pars || !out || (curve_mask && !curves_out)) return fail(MP_EINVAL, "mp_model_flows: NULL argument");
    Evaluator *ev = h->first();
    Held held(h, ev);
    const size_t ng = ev->tgrid.size();
    const size_t chunk = (size_t)std::min<int64_t>(n, std::max(1, ev->sh.n_simd));
    const size_t npick = (size_t)__builtin_popcount(curve_mask);
    int rc;
    if ((rc = ev->w_flow_cells.ensure((size_t)MP_FLOW_NCURVES * chunk * ng)) || (rc = ev->w_flow_out.ensure(chunk * MP_FLOW_N))) return rc;
    return curve_pass(ev, pars, (size_t)n, ndim, physical, kCurveTraj, chunk, status_out, n_used, [&](const CurveChunk &c) {
        mp::FlowCellsArgs f;
        const int frc = flow_cells_enqueue(ev, c, ndim, physical, mp::kFlowReduceMask | curve_mask, ev->w_flow_cells.p, chunk * ng, 0, f);
        if (frc) return frc;
        mp::FlowReduceArgs r{};
        for (int i = 0; i < MP_FLOW_NCURVES; ++i) r.cell[i] = f.cell[i];
        r.status = c.status;
        r.tgrid = ev->d_tgrid.p;
        r.out = ev->w_flow_out.p;
        r.rows = (int32_t)c.cnt;
        r.n_grid = (int32_t)ng;
        const int e = mp::launch_flow_reduce(r, (void *)c.st);
        if (e) return fail(MP_EHIP, "flow reduce kernel launch failed: %s", hipGetErrorString((hipError_t)e));
        hipError_t ce = hipMemcpyAsync(out + c.lo * MP_FLOW_N, ev->w_flow_out.p, sizeof(double) * c.cnt * MP_FLOW_N, hipMemcpyDeviceToHost, c.st);
        // curves_out[row][picked curve][n_grid]: one strided copy per picked curve
        for (int i = 0, k = 0; i < MP_FLOW_NCURVES && ce == hipSuccess; ++i) {
            if (!(curve_mask & (1u << i))) continue;
            ce = hipMemcpy2DAsync(curves_out + (c.lo * npick + (size_t)k) * ng, sizeof(double) * npick * ng, f.cell[i], sizeof(double) * ng,
                                  sizeof(double) * ng, c.cnt, hipMemcpyDeviceToHost, c.st);
            ++k;
        }
        if (ce != hipSuccess) return fail(MP_EHIP, "mp_model_flows: copy failed: %s", hipGetErrorString(ce));
        return (int)MP_OK;
    });
}

// The chunked pass of mp_model_flows with the selected curves only, every chunk's cells at its row offset of an n x n_grid matrix
// per curve; behind the last chunk the band of those matrices, as mp_model_band forms it.  The matrices of a band of several
// curves are given back before the call returns: one matrix is what mp_model_band keeps, nine of 16 384 rows are 11.8 GB.
int mp_model_flow_band(mp_handle *h, const double *pars, int n, int ndim, int physical, const double *weights, const double *q,
                       int nq, uint32_t curve_mask, double *band_out, int32_t *status_out, int32_t *n_used) {
    const char *who = "mp_model_flow_band";
    int rc;
    if ((rc = check_band_args(who, h, pars, n, ndim, q, nq, band_out))) return rc;
    if (curve_mask == 0 || (curve_mask & ~mp::kFlowAllMask) || (curve_mask & (1u << MP_FLOW_CURVE_BRANCH)))
        return fail(MP_EINVAL, "%s: curve_mask 0x%x is not a non-empty mask of MP_FLOW_CURVE_* bits without BRANCH", who, curve_mask);
    std::vector<uint32_t> units;
    if (weights) {
        units.resize((size_t)n);
        if (!mp::band_weight_units(weights, n, units.data()))
            return fail(MP_EINVAL, "%s: the weights must be finite and >= 0 with at least one > 0", who);
    }
    Evaluator *ev = h->first();
    Held held(h, ev);
    const size_t ng = ev->tgrid.size(), nn = (size_t)n;
    const size_t chunk = std::min(nn, (size_t)std::max(1, ev->sh.n_simd));
    const int npick = __builtin_popcount(curve_mask);
    mp::BandQ bq;
    if ((rc = ev->w_flow_band.ensure((size_t)npick * nn * ng)) || (rc = band_prepare(ev, n, npick, q, nq, weights != nullptr, bq))) return rc;
    int64_t used = 0;
    rc = curve_pass(ev, pars, nn, ndim, physical, kCurveTraj, chunk, status_out, &used, [&](const CurveChunk &c) {
        mp::FlowCellsArgs f;
        const int frc = flow_cells_enqueue(ev, c, ndim, physical, curve_mask, ev->w_flow_band.p, nn * ng, c.lo, f);
        if (frc || c.lo + c.cnt < nn) return frc;
        // behind the last chunk
        return band_enqueue(ev, n, npick, bq, weights ? units.data() : nullptr, band_out, c.st,
                            [&](int k) { return ev->w_flow_band.p + (size_t)k * nn * ng; });
    });
    if (npick > 1) ev->w_flow_band.release();              // (curve_pass has synchronised the stream, whatever it returns)
    if (!rc && n_used) *n_used = (int32_t)used;
    return rc;
}

int mp_pointwise_tail_len(int64_t n_used) { return mp::pointwise_tail_len(n_used); }

// The rows go through the device in chunks of n_simd rows as in mp_model_derived, with Ltot alone: every chunk's curve launch is
// followed by the launch that turns its rows into columns [lo, lo + cnt) of the cell matrix.  The select and reduce kernels run
// once behind the last chunk; nothing but the results reaches the host.
int mp_model_pointwise(mp_handle *h, const double *pars, int64_t n, int ndim, int physical, int ds_id, double *obs_out,
                       double *tail_out, double *z_out, int32_t *status_out, int64_t *n_used) {
    // (the sizes first: they can be judged without a handle)
    if (n < 1 || n > MP_POINTWISE_MAX_SAMPLES)
        return fail(MP_EINVAL, "mp_model_pointwise: n must be 1..%d (MP_POINTWISE_MAX_SAMPLES), got %lld", MP_POINTWISE_MAX_SAMPLES, (long long)n);
    if (ndim < 6 || ndim > MP_MAX_NDIM) return fail(MP_EINVAL, "mp_model_pointwise: ndim must be 6..9, got %d", ndim);
    if (ds_id < 0 || ds_id >= MP_MAX_DATASETS) return fail(MP_EINVAL, "mp_model_pointwise: ds_id %d out of range", ds_id);
    if (!h || !pars || !obs_out) return fail(MP_EINVAL, "mp_model_pointwise: NULL argument");
    Evaluator *ev = h->first();
    Held held(h, ev);
    if (!ev->ds[ds_id].set) return fail(MP_ESTATE, "mp_model_pointwise: refers to unset dataset %d", ds_id);
    const mp::DsDesc &dd = ev->desc[(size_t)ds_id];
    const size_t nn = (size_t)n, n_obs = (size_t)dd.n_obs;
    if ((int64_t)nn * (int64_t)n_obs > (int64_t)MP_POINTWISE_MAX_CELLS)
        return fail(MP_EINVAL, "mp_model_pointwise: n * n_obs = %lld * %d exceeds MP_POINTWISE_MAX_CELLS = %lld", (long long)n, dd.n_obs,
                    (long long)MP_POINTWISE_MAX_CELLS);
    const size_t chunk = (size_t)std::min<int64_t>(n, std::max(1, ev->sh.n_simd));
    const size_t tlen = (size_t)mp::pointwise_tail_len(n);
    int rc;
    if ((rc = ev->w_pw_z.ensure(n_obs * nn)) || (rc = ev->w_pw_obs.ensure(n_obs * MP_POINTWISE_N)) || (rc = ev->w_pw_tail.ensure(n_obs * tlen)))
        return rc;
    const mp::PointwiseData pd{ev->d_obs_g.p + dd.obs_off, ev->d_obs_dx.p + dd.obs_off, ev->d_obs_idt.p + dd.obs_off,
                               ev->d_obs_y.p + dd.obs_off, ev->d_obs_yerr.p + dd.obs_off, dd.n_obs};
    return curve_pass(ev, pars, nn, ndim, physical, kCurveLtot, chunk, status_out, n_used, [&](const CurveChunk &k) {
        mp::PointwiseCellsArgs c{};
        c.ltot = k.curve[0];                      // (the rows of walkers that did not finish are not read)
        c.status = k.status;
        c.d = pd;
        c.z = ev->w_pw_z.p;
        c.n = n;
        c.lo = (int64_t)k.lo;
        c.cnt = (int32_t)k.cnt;
        c.n_grid = (int32_t)ev->tgrid.size();
        int e = mp::launch_pointwise_cells(c, (void *)k.st);
        if (e) return fail(MP_EHIP, "pointwise cells kernel launch failed: %s", hipGetErrorString((hipError_t)e));
        if (k.lo + k.cnt < nn) return (int)MP_OK;
        // behind the last chunk
        mp::PointwiseColsArgs r{};
        r.z = ev->w_pw_z.p;
        r.obs = ev->w_pw_obs.p;
        r.tail = ev->w_pw_tail.p;
        r.n = n;
        r.n_obs = dd.n_obs;
        r.tail_stride = (int32_t)tlen;
        e = mp::launch_pointwise_select(r, (void *)k.st);
        if (!e) e = mp::launch_pointwise_reduce(r, (void *)k.st);
        if (e) return fail(MP_EHIP, "pointwise reduction kernel launch failed: %s", hipGetErrorString((hipError_t)e));
        hipError_t ce = hipMemcpyAsync(obs_out, ev->w_pw_obs.p, sizeof(double) * n_obs * MP_POINTWISE_N, hipMemcpyDeviceToHost, k.st);
        if (ce == hipSuccess && tail_out) ce = hipMemcpyAsync(tail_out, ev->w_pw_tail.p, sizeof(double) * n_obs * tlen, hipMemcpyDeviceToHost, k.st);
        if (ce == hipSuccess && z_out) ce = hipMemcpyAsync(z_out, ev->w_pw_z.p, sizeof(double) * n_obs * nn, hipMemcpyDeviceToHost, k.st);
        if (ce != hipSuccess) return fail(MP_EHIP, "mp_model_pointwise: copy failed: %s", hipGetErrorString(ce));
        return (int)MP_OK;
    });
}

// The rows go through the device in chunks of n_simd rows as in mp_model_pointwise, with Ltot alone: every chunk's curve launch is
// followed by the launch that sums its rows' differences into columns [lo, lo + cnt) of lw[n_alt][n].  The alternatives and the
// observation weights go up once, inside the pass (so that every failure behind their enqueue synchronises the stream, as
// curve_pass promises); the select and reduce kernels run once behind the last chunk.
int mp_model_reweight(mp_handle *h, const double *pars, int64_t n, int ndim, int physical, int ds_id, int n_alt,
                      const int32_t *kind, const double *alt, const double *obs_w, double *lw_out, double *alt_out,
                      double *tail_out, int32_t *status_out, int64_t *n_used) {
    // (the sizes and the alternatives first: they can be judged without a handle)
    if (n < 1 || n > MP_POINTWISE_MAX_SAMPLES)
        return fail(MP_EINVAL, "mp_model_reweight: n must be 1..%d (MP_POINTWISE_MAX_SAMPLES), got %lld", MP_POINTWISE_MAX_SAMPLES, (long long)n);
    if (ndim < 6 || ndim > MP_MAX_NDIM) return fail(MP_EINVAL, "mp_model_reweight: ndim must be 6..9, got %d", ndim);
    if (ds_id < 0 || ds_id >= MP_MAX_DATASETS) return fail(MP_EINVAL, "mp_model_reweight: ds_id %d out of range", ds_id);
    if (n_alt < 1 || n_alt > MP_REWEIGHT_MAX_ALT)
        return fail(MP_EINVAL, "mp_model_reweight: n_alt must be 1..%d (MP_REWEIGHT_MAX_ALT), got %d", MP_REWEIGHT_MAX_ALT, n_alt);
    if (!h || !pars || !kind || !alt || !alt_out) return fail(MP_EINVAL, "mp_model_reweight: NULL argument");
    const int bad = mp::reweight_bad_alternative(n_alt, kind, alt);
    if (bad >= 0)
        return fail(MP_EINVAL, "mp_model_reweight: alternative %d (kind %d, scale %g, jitter %g, nu %g) is not a Gaussian or Student-t with "
                    "finite scale > 0, jitter >= 0 and (Student-t) nu > 0", bad, (int)kind[bad], alt[3 * bad], alt[3 * bad + 1], alt[3 * bad + 2]);
    Evaluator *ev = h->first();
    Held held(h, ev);
    if (!ev->ds[ds_id].set) return fail(MP_ESTATE, "mp_model_reweight: refers to unset dataset %d", ds_id);
    const mp::DsDesc &dd = ev->desc[(size_t)ds_id];
    const size_t nn = (size_t)n, n_obs = (size_t)dd.n_obs, na = (size_t)n_alt;
    if (obs_w) {
        const int64_t bw = mp::reweight_bad_weight(obs_w, (int64_t)(na * n_obs));
        if (bw >= 0)
            return fail(MP_EINVAL, "mp_model_reweight: obs_w[%lld][%lld] = %g is not finite and >= 0", (long long)(bw / (int64_t)n_obs),
                        (long long)(bw % (int64_t)n_obs), obs_w[bw]);
    }
    const size_t chunk = (size_t)std::min<int64_t>(n, std::max(1, ev->sh.n_simd));
    const size_t tlen = (size_t)mp::pointwise_tail_len(n);
    int rc;
    if ((rc = ev->w_rw_lw.ensure(na * nn)) || (rc = ev->w_rw_out.ensure(na * MP_REWEIGHT_N)) || (rc = ev->w_rw_tail.ensure(na * tlen)) ||
        (rc = ev->w_rw_alt.ensure(na * (3 + n_obs))) || (rc = ev->w_rw_kind.ensure(na)))
        return rc;
    double *d_w = obs_w ? ev->w_rw_alt.p + 3 * na : nullptr;
    const mp::PointwiseData pd{ev->d_obs_g.p + dd.obs_off, ev->d_obs_dx.p + dd.obs_off, ev->d_obs_idt.p + dd.obs_off,
                               ev->d_obs_y.p + dd.obs_off, ev->d_obs_yerr.p + dd.obs_off, dd.n_obs};
    return curve_pass(ev, pars, nn, ndim, physical, kCurveLtot, chunk, status_out, n_used, [&](const CurveChunk &k) {
        if (k.lo == 0) {                          // the tables go up once, behind the first curve launch and before the first row launch
            hipError_t ue = hipMemcpyAsync(ev->w_rw_kind.p, kind, sizeof(int32_t) * na, hipMemcpyHostToDevice, k.st);
            if (ue == hipSuccess) ue = hipMemcpyAsync(ev->w_rw_alt.p, alt, sizeof(double) * 3 * na, hipMemcpyHostToDevice, k.st);
            if (ue == hipSuccess && obs_w) ue = hipMemcpyAsync(d_w, obs_w, sizeof(double) * na * n_obs, hipMemcpyHostToDevice, k.st);
            if (ue != hipSuccess) return fail(MP_EHIP, "mp_model_reweight: copy failed: %s", hipGetErrorString(ue));
        }
        mp::ReweightRowsArgs c{};
        c.ltot = k.curve[0];                      // (the rows of walkers that did not finish are not read)
        c.status = k.status;
        c.d = pd;
        c.kind = ev->w_rw_kind.p;
        c.alt = ev->w_rw_alt.p;
        c.obs_w = d_w;
        c.lw = ev->w_rw_lw.p;
        c.n = n;
        c.lo = (int64_t)k.lo;
        c.cnt = (int32_t)k.cnt;
        c.n_grid = (int32_t)ev->tgrid.size();
        c.n_alt = n_alt;
        int e = mp::launch_reweight_rows(c, (void *)k.st);
        if (e) return fail(MP_EHIP, "reweight rows kernel launch failed: %s", hipGetErrorString((hipError_t)e));
        if (k.lo + k.cnt < nn) return (int)MP_OK;
        // behind the last chunk
        mp::ReweightColsArgs r{};
        r.lw = ev->w_rw_lw.p;
        r.out = ev->w_rw_out.p;
        r.tail = ev->w_rw_tail.p;
        r.n = n;
        r.n_alt = n_alt;
        r.tail_stride = (int32_t)tlen;
        e = mp::launch_reweight_select(r, (void *)k.st);
        if (!e) e = mp::launch_reweight_reduce(r, (void *)k.st);
        if (e) return fail(MP_EHIP, "reweight reduction kernel launch failed: %s", hipGetErrorString((hipError_t)e));
        hipError_t ce = hipMemcpyAsync(alt_out, ev->w_rw_out.p, sizeof(double) * na * MP_REWEIGHT_N, hipMemcpyDeviceToHost, k.st);
        if (ce == hipSuccess && tail_out) ce = hipMemcpyAsync(tail_out, ev->w_rw_tail.p, sizeof(double) * na * tlen, hipMemcpyDeviceToHost, k.st);
        if (ce == hipSuccess && lw_out) ce = hipMemcpyAsync(lw_out, ev->w_rw_lw.p, sizeof(double) * na * nn, hipMemcpyDeviceToHost, k.st);
        if (ce != hipSuccess) return fail(MP_EHIP, "mp_model_reweight: copy failed: %s", hipGetErrorString(ce));
        return (int)MP_OK;
    });
}

// The rows go through the device in chunks of n_simd rows as in mp_model_pointwise, with Ltot alone: every chunk's curve launch is
// followed by the launch that turns its rows into cells, and the copies of the chunk's cells to the caller's rows [lo, lo + cnt).
// The brackets are formed here, on the host, by the rule mp_set_dataset keeps (mp_simulate.h); shared tables go up once, per-row
// tables chunk by chunk.  A row's noise is drawn under its index in the call (lo + its place in the chunk), so nothing depends
// on the chunking.  Behind the pass the rows the kernel marked (a cell with error 0) get MP_STATUS_ZEROERR and NaN cells.
int mp_simulate(mp_handle *h, const double *pars, int64_t n, int ndim, int physical, const double *x, int n_obs, int64_t x_rows,
                const double *yerr, double frac_err, uint64_t seed, double *y_out, double *yerr_out, double *model_out,
                double *z_out, int32_t *status_out, int64_t *n_ok) {
    // (the sizes first: they can be judged without a handle)
    if (n < 1 || n > MP_SIM_MAX_ROWS) return fail(MP_EINVAL, "mp_simulate: n must be 1..%d (MP_SIM_MAX_ROWS), got %lld", MP_SIM_MAX_ROWS, (long long)n);
    if (ndim < 6 || ndim > MP_MAX_NDIM) return fail(MP_EINVAL, "mp_simulate: ndim must be 6..9, got %d", ndim);
    if (n_obs < 1) return fail(MP_EINVAL, "mp_simulate: n_obs must be at least 1, got %d", n_obs);
    if (n * (int64_t)n_obs > (int64_t)MP_SIM_MAX_CELLS)
        return fail(MP_EINVAL, "mp_simulate: n * n_obs = %lld * %d exceeds MP_SIM_MAX_CELLS = %lld", (long long)n, n_obs, (long long)MP_SIM_MAX_CELLS);
    if (x_rows != 1 && x_rows != n) return fail(MP_EINVAL, "mp_simulate: x_rows must be 1 or n = %lld, got %lld", (long long)n, (long long)x_rows);
    if (!h || !pars || !x || !y_out) return fail(MP_EINVAL, "mp_simulate: NULL argument");
    const size_t nn = (size_t)n, no = (size_t)n_obs, tab = (size_t)x_rows * no;
    if (yerr) {
        for (size_t j = 0; j < tab; ++j)
            if (!(yerr[j] > 0.0) || !std::isfinite(yerr[j])) return fail(MP_EINVAL, "mp_simulate: yerr[%zu] = %g is not finite and > 0", j, yerr[j]);
    } else if (!(frac_err > 0.0) || !std::isfinite(frac_err)) {
        return fail(MP_EINVAL, "mp_simulate: frac_err = %g is not finite and > 0", frac_err);
    }
    Evaluator *ev = h->first();
    Held held(h, ev);
    const std::vector<double> &t = ev->tgrid;
    std::vector<int32_t> g(tab);
    std::vector<double> dx(tab), idt(tab);
    for (size_t j = 0; j < tab; ++j) {
        if (!(x[j] >= t.front()) || !(x[j] <= t.back()))
            return fail(MP_ERANGE, "mp_simulate: x[%zu] = %g is outside the model grid [%g, %g]", j, x[j], t.front(), t.back());
        mp::sim_bracket(t, x[j], g[j], dx[j], idt[j]);
    }
    const size_t chunk = (size_t)std::min<int64_t>(n, std::max(1, ev->sh.n_simd));
    const size_t trows = x_rows == 1 ? 1 : chunk;             // table rows on the device at a time
    const size_t tcells = trows * no, ccells = chunk * no;
    int rc;
    if ((rc = ev->w_sim.ensure(3 * tcells + 4 * ccells)) || (rc = ev->w_sim_g.ensure(tcells + nn))) return rc;
    double *d_dx = ev->w_sim.p, *d_idt = d_dx + tcells, *d_ye_in = d_idt + tcells, *d_out = d_ye_in + tcells;
    int32_t *d_g = ev->w_sim_g.p, *d_zero = d_g + tcells;
    hipStream_t st = ev->stream;
    auto upload = [&](size_t row_lo, size_t rows) {           // table rows [row_lo, row_lo + rows) to the front of the device tables
        const size_t o = row_lo * no, c = rows * no;
        hipError_t e = hipMemcpyAsync(d_g, g.data() + o, sizeof(int32_t) * c, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(d_dx, dx.data() + o, sizeof(double) * c, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(d_idt, idt.data() + o, sizeof(double) * c, hipMemcpyHostToDevice, st);
        if (e == hipSuccess && yerr) e = hipMemcpyAsync(d_ye_in, yerr + o, sizeof(double) * c, hipMemcpyHostToDevice, st);
        return e;
    };
    HIP_TRY(hipMemsetAsync(d_zero, 0, sizeof(int32_t) * nn, st));
    if (x_rows == 1) {
        const hipError_t e = upload(0, 1);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(st);
            return fail(MP_EHIP, "mp_simulate: copy failed: %s", hipGetErrorString(e));
        }
    }
    std::vector<int32_t> stt(nn);
    rc = curve_pass(ev, pars, nn, ndim, physical, kCurveLtot, chunk, stt.data(), nullptr, [&](const CurveChunk &k) {
        hipError_t ce = x_rows == 1 ? hipSuccess : upload(k.lo, k.cnt);
        if (ce != hipSuccess) return fail(MP_EHIP, "mp_simulate: copy failed: %s", hipGetErrorString(ce));
        mp::SimCellsArgs c{};
        c.ltot = k.curve[0];                      // (the rows of walkers that did not finish are not read)
        c.status = k.status;
        c.g = d_g;
        c.dx = d_dx;
        c.idt = d_idt;
        c.yerr = yerr ? d_ye_in : nullptr;
        c.frac_err = frac_err;
        c.seed = seed;
        c.row0 = (int64_t)k.lo;
        c.y = d_out;
        c.ye = yerr_out ? d_out + ccells : nullptr;
        c.mod = model_out ? d_out + 2 * ccells : nullptr;
        c.z = z_out ? d_out + 3 * ccells : nullptr;
        c.zero_err = d_zero + k.lo;
        c.cnt = (int32_t)k.cnt;
        c.n_obs = n_obs;
        c.n_grid = (int32_t)t.size();
        c.tab_rows = x_rows == 1 ? 1 : (int32_t)k.cnt;
        const int e = mp::launch_simulate_cells(c, (void *)k.st);
        if (e) return fail(MP_EHIP, "simulate cells kernel launch failed: %s", hipGetErrorString((hipError_t)e));
        double *const host[4] = {y_out, yerr_out, model_out, z_out};
        for (int i = 0; i < 4 && ce == hipSuccess; ++i)
            if (host[i]) ce = hipMemcpyAsync(host[i] + k.lo * no, d_out + (size_t)i * ccells, sizeof(double) * k.cnt * no, hipMemcpyDeviceToHost, k.st);
        if (ce != hipSuccess) return fail(MP_EHIP, "mp_simulate: copy failed: %s", hipGetErrorString(ce));
        return (int)MP_OK;
    });
    if (rc) return rc;
    // (curve_pass has synchronised the stream)
    std::vector<int32_t> zero(nn);
    HIP_TRY(hipMemcpy(zero.data(), d_zero, sizeof(int32_t) * nn, hipMemcpyDeviceToHost));
    int64_t ok = 0;
    for (size_t i = 0; i < nn; ++i) {
        if (stt[i] == MP_STATUS_OK && zero[i]) {
            stt[i] = MP_STATUS_ZEROERR;
            double *const host[4] = {y_out, yerr_out, model_out, z_out};
            for (double *o : host)
                if (o) std::fill(o + i * no, o + (i + 1) * no, std::nan(""));
        }
        ok += stt[i] == MP_STATUS_OK;
    }
    if (status_out) std::memcpy(status_out, stt.data(), sizeof(int32_t) * nn);
    if (n_ok) *n_ok = ok;
    return MP_OK;
}

}  // extern "C"
