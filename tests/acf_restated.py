"""numpy restatement of the sampler's device autocorrelation monitor (include/magprop_amd.h mp_sampler_set_autocorr;
magprop_amd/csrc/mp_acf.hip): the same sums in the same order, every product and sum rounded on its own (numpy never fuses), so
the accumulators agree with the device bit for bit.

Monitor(max_lag) takes the samples of ONE ensemble, (rows, nwalkers, ndim), in any number of feed() calls; finalise(c) is the
estimator.  sums_oneshot() states the accumulators once more, lag by lag over the whole sequence, without any history."""
import numpy as np


class Monitor:
    def __init__(self, max_lag):
        self.K = int(max_lag)
        self.n = 0
        self.S = self.T = self.H = self.pivot = self._buf = None
        self._idx = 0

    def feed(self, x):
        x = np.asarray(x, dtype=np.float64)
        K = self.K
        if self.S is None and len(x):
            shp = x.shape[1:]
            self.pivot = x[0].copy()
            self.S, self.H, self.T = np.zeros((K,) + shp), np.zeros((K,) + shp), np.zeros(shp)
            self._buf = np.zeros((2 * K,) + shp)     # y_t at _idx and _idx + K: _buf[_idx:_idx + K] is y_t, y_{t-1}, ...
            self._tmp = np.empty((K,) + shp)
        for row in x:
            y = row - self.pivot
            self._idx = (self._idx - 1) % K
            self._buf[self._idx] = self._buf[self._idx + K] = y
            np.multiply(y[None], self._buf[self._idx:self._idx + K], out=self._tmp)     # y_t y_{t-k}; zeros before sample 0
            np.add(self.S, self._tmp, out=self.S)
            self.T = self.T + y
            self.n += 1
            if self.n < K:
                self.H[self.n] = self.T
        return self

    @property
    def tail(self):
        """(K, ...): row i is y_{n-K+i}, zeros before sample 0."""
        return self._buf[self._idx:self._idx + self.K][::-1].copy()

    def sums(self):
        """The accumulators as mp_sampler_get_autocorr_sums returns them (H_k = T for k > n)."""
        H = self.H.copy()
        H[min(self.n, self.K - 1) + 1:] = self.T
        return {"S": self.S.copy(), "T": self.T.copy(), "H": H, "tail": self.tail, "pivot": self.pivot.copy(), "n": self.n}

    def finalise(self, c=5.0, with_rho=False):
        """(tau[ndim], window[ndim], f[lim, ndim]) over the walkers (axis 0 of a sample) of the ensemble; with_rho: also
        rho[lim, nwalkers, ndim] of every series."""
        K, n = self.K, self.n
        lim = min(K, n)
        tail = self.tail
        L = np.zeros_like(self.S)
        for off in range(-(K - 1), 0):               # increasing t: L_k takes y_{n+off} for every k >= -off
            L[-off:] = L[-off:] + tail[K + off]
        H = self.sums()["H"]
        m = self.T / float(n)
        nk = (float(n) - np.arange(K, dtype=np.float64)).reshape((K,) + (1,) * self.T.ndim)
        ck = (self.S - m * ((2.0 * self.T - H) - L)) + nk * (m * m)
        c0 = ck[0]
        with np.errstate(invalid="ignore", divide="ignore"):
            rho = np.where(c0 != 0.0, ck / c0, 0.0)[:lim]
        nw = rho.shape[1]
        f = np.cumsum(rho, axis=1)[:, -1] / float(nw)              # walker order, sequential
        taus = 2.0 * np.cumsum(f, axis=0) - 1.0                    # lag order, sequential
        ndim = f.shape[1]
        tau, window = np.empty(ndim), np.empty(ndim, dtype=np.int32)
        for d in range(ndim):
            ok = np.arange(lim) < c * taus[:, d]
            if np.any(~ok):
                window[d] = int(np.argmin(ok))
                tau[d] = taus[window[d], d]
            elif n <= K:
                window[d], tau[d] = lim - 1, taus[lim - 1, d]
            else:
                window[d], tau[d] = -1, np.nan
        return (tau, window, f, rho) if with_rho else (tau, window, f)


def sums_oneshot(x, max_lag):
    """S, T, H of the whole sequence x (n, ...) by their definitions, one lag at a time (np.cumsum adds in index order)."""
    x = np.asarray(x, dtype=np.float64)
    n, K = len(x), int(max_lag)
    y = x - x[0]
    S = np.zeros((K,) + x.shape[1:])
    for k in range(min(K, n)):
        S[k] = np.cumsum(y[k:] * y[:n - k], axis=0)[-1]
    pre = np.cumsum(y, axis=0)
    H = np.zeros_like(S)
    for k in range(1, K):
        H[k] = pre[min(k, n) - 1]
    return {"S": S, "T": pre[-1], "H": H, "pivot": x[0].copy(), "n": n}


def host_tau_window(chain, c=5.0):
    """magprop_amd.mcmc_io.integrated_time's tau together with the window it chose (the function returns tau only)."""
    from magprop_amd.mcmc_io import _autocorr_1d, integrated_time
    x = np.asarray(chain, dtype=float)
    nstep, nwalk, ndim = x.shape
    window = np.empty(ndim, dtype=np.int32)
    for d in range(ndim):
        acf = np.zeros(nstep)
        for k in range(nwalk):
            acf += _autocorr_1d(x[:, k, d])
        acf /= nwalk
        taus = 2.0 * np.cumsum(acf) - 1.0
        m = np.arange(len(taus)) < c * taus
        window[d] = int(np.argmin(m)) if np.any(~m) else len(taus) - 1
    return integrated_time(x, c=c, quiet=True), window


def ar1(rng, rho, nsteps, nwalkers, ndim, mean=0.0, start=None):
    """Seeded AR(1) series of unit stationary variance around `mean`, (nsteps, nwalkers, ndim); start: the first sample
    (default: a stationary draw)."""
    x = np.empty((nsteps, nwalkers, ndim))
    x[0] = rng.standard_normal((nwalkers, ndim)) if start is None else start
    s = np.sqrt(1.0 - rho * rho)
    for t in range(1, nsteps):
        x[t] = rho * x[t - 1] + s * rng.standard_normal((nwalkers, ndim))
    return x + mean
