"""The C ABI (include/magprop_amd.h) through ctypes, for the GPU tests that drive it without the Python front end: typed
pointers to numpy buffers, the handle every unit-Gaussian driver runs on, and the one raw driver of mp_sampler_* (mp_sampler_run
and the walker-sharded entry points)."""
import ctypes as C

import numpy as np


def dp(a):
    """double * to the buffer of a (None: NULL); ip: int32_t *, lp: int64_t *."""
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def ip(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))


def lp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int64))


def synth_handle(device=-1, **cfg):
    """A handle of the synthetic-set configuration (cfg: fields to override) on the default time grid."""
    from magprop_amd import _capi, engine
    return _capi.Handle(_capi.cfg_synth(**cfg), engine.grid(None), device=device)


def table_args(table):
    """[(kind, weight, p0, p1)] -> kinds, weights, params[n, 2] as mp_sampler_set_moves takes them."""
    kinds = np.array([t[0] for t in table], dtype=np.int32)
    weights = np.array([t[1] for t in table], dtype=np.float64)
    params = np.ascontiguousarray([[t[2], t[3]] for t in table], dtype=np.float64)
    return kinds, weights, params


def swap_counts(L, sp, n_groups, n_temps):
    """Accepted swaps [n_groups, n_temps - 1] of the tempered sampler sp."""
    from magprop_amd import _capi
    out = np.zeros((n_groups, n_temps - 1), dtype=np.int64)
    assert L.mp_sampler_get_swaps(sp, lp(out)) == _capi.MP_OK, _capi.last_error()
    return out


class RawSampler:
    """One mp_sampler of n_ens ensembles through the C ABI, by default on the unit-Gaussian target (target=1) and a handle of
    its own; handle=: a sampler on that handle (its datasets and prior), which stays the caller's.  Every call is asserted
    MP_OK with the library's message.  Settings go in the order the library wants them: temperatures, whole step, moves and
    monitor before set_positions.  ds: the dataset of every ensemble (mp_sampler_create's ens_ds_id; None: dataset 0)."""

    def __init__(self, n_walkers, n_ens, ndim, seed, a=2.0, target=1, handle=None, ds=None):
        from magprop_amd import _capi
        self.cap, self.L = _capi, _capi.lib()
        self.h = synth_handle() if handle is None else handle
        self.own_handle = handle is None
        self.nw, self.ne, self.ndim, self.nt = n_walkers, n_ens, ndim, n_walkers * n_ens
        ids = None if ds is None else np.ascontiguousarray(ds, dtype=np.int32)
        assert ids is None or ids.shape == (n_ens,)
        self.sp = self.L.mp_sampler_create(self.h._h, n_walkers, n_ens, ndim, ip(ids), C.c_uint64(seed), C.c_double(a), target)
        if not self.sp:
            self.close()
        assert self.sp, _capi.last_error()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _ok(self, rc):
        assert rc == self.cap.MP_OK, self.cap.last_error()

    def set_moves(self, table, check=True):
        """Returns the code; check=False: unasserted, for the tests of the argument codes."""
        kinds, weights, params = table_args(table)
        rc = self.L.mp_sampler_set_moves(self.sp, len(table), ip(kinds), dp(weights), dp(params))
        if check:
            self._ok(rc)
        return rc

    def set_temperatures(self, betas):
        b = np.ascontiguousarray(betas, dtype=np.float64)
        self._ok(self.L.mp_sampler_set_temperatures(self.sp, len(b), dp(b)))

    def set_whole_step(self, flag):
        self._ok(self.L.mp_sampler_set_whole_step(self.sp, int(flag)))

    def set_autocorr(self, max_lag, discard):
        self._ok(self.L.mp_sampler_set_autocorr(self.sp, max_lag, discard))

    def set_positions(self, pos):
        self._ok(self.L.mp_sampler_set_positions(self.sp, dp(np.ascontiguousarray(pos, dtype=np.float64))))

    def run(self, n, store=True):
        """n steps; chain (n, n_total, ndim) and lnprob (n, n_total), or (None, None) with store=False."""
        ch, ln = (np.empty((n, self.nt, self.ndim)), np.empty((n, self.nt))) if store else (None, None)
        self._ok(self.L.mp_sampler_run(self.sp, n, dp(ch), dp(ln)))
        return ch, ln

    def run_chunks(self, runs):
        """Consecutive mp_sampler_run calls of runs[i] steps.  Returns chain, lnprob (concatenated) and n_accepted."""
        parts = [self.run(n) for n in runs]
        return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), self.accepted()

    def accepted(self):
        acc = np.empty(self.nt, dtype=np.int64)
        self._ok(self.L.mp_sampler_get_state(self.sp, None, None, lp(acc), None))
        return acc

    def swaps(self, n_groups, n_temps):
        return swap_counts(self.L, self.sp, n_groups, n_temps)

    def state(self):
        """pos, lnprob, n_accepted."""
        pos, lnp, acc = np.empty((self.nt, self.ndim)), np.empty(self.nt), np.empty(self.nt, dtype=np.int64)
        self._ok(self.L.mp_sampler_get_state(self.sp, dp(pos), dp(lnp), lp(acc), None))
        return pos, lnp, acc

    def bad(self):
        """mp_sampler_get_bad: the count of failed proposals and the logged rows."""
        n_bad, n_logged = C.c_int64(0), C.c_int64(0)
        assert self.L.mp_sampler_get_bad(self.sp, 0, None, 0, C.byref(n_bad), C.byref(n_logged)) >= 0
        rows = np.empty((n_logged.value, self.ndim))
        if n_logged.value:
            assert self.L.mp_sampler_get_bad(self.sp, 0, dp(rows), n_logged.value, None, None) == n_logged.value
        return n_bad.value, rows

    # ---- the walker-sharded entry points, driven in one process on the null stream; rows travel as numpy arrays through a
    # device buffer of the sampler's device (a torch tensor)
    @property
    def n_slots(self):
        return self.L.mp_sampler_n_slots(self.sp)

    @property
    def row_doubles(self):
        return self.L.mp_sampler_row_doubles(self.sp)

    @property
    def step_blocks(self):
        return self.L.mp_sampler_step_blocks(self.sp)

    @property
    def step_row_doubles(self):
        return self.L.mp_sampler_step_row_doubles(self.sp)

    def _dev(self, rows, width):
        import torch
        dev = f"cuda:{self.h.device}"
        if isinstance(rows, int):
            return torch.empty((rows, width), dtype=torch.float64, device=dev)
        assert rows.shape[1] == width
        return torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float64)).to(dev)

    def _host(self, t):
        import torch
        torch.cuda.synchronize(t.device)
        return t.cpu().numpy()

    def halfstep_shard(self, half, lo, hi, check=True):
        """Rows [hi - lo, row_doubles] of slots [lo, hi) of the active half; check=False: the code alone."""
        buf = self._dev(max(hi - lo, 1), self.row_doubles)
        rc = self.L.mp_sampler_halfstep_shard(self.sp, half, lo, hi, C.c_void_p(buf.data_ptr()), None)
        if not check:
            return rc
        self._ok(rc)
        return self._host(buf)[:hi - lo]

    def halfstep_apply(self, half, rows, chain_row=None, lnp_row=None):
        """Commits the gathered rows of the half-step; returns the step's chain row and lnprob row with the entries of this
        half's walkers written into chain_row / lnp_row (None: zeros), so that half 1 completes what half 0 began."""
        buf = self._dev(rows, self.row_doubles)
        ch = self._dev(np.zeros((self.nt, self.ndim)) if chain_row is None else chain_row, self.ndim)
        ln = self._dev(np.zeros((self.nt, 1)) if lnp_row is None else lnp_row.reshape(-1, 1), 1)
        self._ok(self.L.mp_sampler_halfstep_apply(self.sp, half, C.c_void_p(buf.data_ptr()), C.c_void_p(ch.data_ptr()),
                                                  C.c_void_p(ln.data_ptr()), None))
        return self._host(ch), self._host(ln)[:, 0]

    def step_shard(self, lo, hi, check=True):
        """Rows [hi - lo, step_row_doubles] of blocks [lo, hi) of the whole step."""
        buf = self._dev(max(hi - lo, 1), self.step_row_doubles)
        rc = self.L.mp_sampler_step_shard(self.sp, lo, hi, C.c_void_p(buf.data_ptr()), None)
        if not check:
            return rc
        self._ok(rc)
        return self._host(buf)[:hi - lo]

    def step_apply(self, rows):
        buf, ch, ln = self._dev(rows, self.step_row_doubles), self._dev(self.nt, self.ndim), self._dev(self.nt, 1)
        self._ok(self.L.mp_sampler_step_apply(self.sp, C.c_void_p(buf.data_ptr()), C.c_void_p(ch.data_ptr()),
                                              C.c_void_p(ln.data_ptr()), None))
        return self._host(ch), self._host(ln)[:, 0]

    def close(self):
        if self.sp:
            self.L.mp_sampler_destroy(self.sp)
            self.sp = None
        if self.own_handle:
            self.h.close()


def gaussian_run(n_walkers, n_ens, ndim, seed, table, pos, runs, whole=None, betas=None):
    """The unit-Gaussian target through the C ABI: runs = steps of consecutive mp_sampler_run calls; betas (per temperature,
    n_ens a multiple of their number): a tempered sampler; whole: mp_sampler_set_whole_step (None: the library's default).
    Returns chain, chain_lnp, n_accepted."""
    with RawSampler(n_walkers, n_ens, ndim, seed) as r:
        if betas is not None:
            r.set_temperatures(betas)
        if whole is not None:
            r.set_whole_step(whole)
        r.set_moves(table)
        r.set_positions(pos)
        return r.run_chunks(runs)
