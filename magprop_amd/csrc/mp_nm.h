// mp_nm.h — launch arguments of the Nelder-Mead simplex search (mp_nm.hip; include/magprop_amd.h mp_simplex_*), shared by the
// kernels and their host driver (mp_simplex.cpp).
#pragma once
#include "mp_device.h"

namespace mp {

constexpr int kNmOutcomes = 5;   // reflect, expand, outside contraction, inside contraction, shrink: the columns of NmArgs::outcomes

// Arguments of one iteration.  Simplex s holds ndim + 1 vertices sorted by f = -lnprob ascending (rows s * (ndim + 1) + j of sim,
// lnp, st) and ndim + 4 candidates (rows s * (ndim + 4) + c of cand, cand_lnp, cand_st; ds_id has a row per candidate).  The eval
// launch reads only the vertices and writes only the candidates, the decide launch behind it reads both and writes the vertices:
// no workgroup reads what another one of its launch writes.
struct NmArgs {
    double *sim;             // [n_simplex][ndim + 1][ndim]
    double *lnp;             // [n_simplex][ndim + 1] (NaN stored as -inf)
    int32_t *st;             // [n_simplex][ndim + 1] status of every vertex (MP_STATUS_*)
    double *cand;            // [n_simplex][ndim + 4][ndim]
    double *cand_lnp;        // [n_simplex][ndim + 4]
    int32_t *cand_st;        // [n_simplex][ndim + 4]
    const int32_t *ds_id;    // [n_simplex][ndim + 4] dataset of every candidate
    int32_t *stopped;        // [n_simplex] 1: frozen
    int32_t *nit;            // [n_simplex] scipy's iteration count (1 after the initial evaluation)
    int64_t *nfev;           // [n_simplex] evaluations of the serial algorithm
    int64_t *outcomes;       // [n_simplex][kNmOutcomes]
    double lower[MP_MAX_NDIM], upper[MP_MAX_NDIM];   // the bounds box (sampler coordinates)
    int32_t n_simplex, ndim;
    int32_t target;          // 0: posterior, 1: isotropic unit Gaussian, 2: terraced Gaussian
    int32_t initial;         // 0: an iteration, 1: evaluate the vertices as they are (decide: sort, count and check only)
    double ca[3], cb[3];     // reflection, expansion, outside contraction: clip(ca xbar - cb v_N)
    double one_m_psi, psi;   // inside contraction: clip(one_m_psi xbar + psi v_N)
    double sigma;            // shrink: clip(v_0 + sigma (v_j - v_0))
    double xatol, fatol;
};
// one workgroup per (simplex, candidate), then one per simplex (decision tree, stable sort, counters, stop rule); include/magprop_amd.h
int launch_nm_eval(const DevShared &sh, const NmArgs &a, void *stream);
int launch_nm_decide(const NmArgs &a, void *stream);

}  // namespace mp
