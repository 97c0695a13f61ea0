"""libmp_probe_dense.so (magprop_amd/csrc/mp_probe_dense.hip: the read-out of a kept tile and the tables of a handle over host
buffers; test infrastructure, no part of the product's ABI) behind numpy arrays, for tests/test_gpu_dense_kernels.py."""
import ctypes as C

import numpy as np

import dense_restated as dr
import probe_lib

_dp, _ip, _i, _vp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_int, C.c_void_p
CANARY = -777.0


def _d(a):
    return a.ctypes.data_as(_dp)


class Probe:
    """libmp_probe_dense.so and one handle of the product per grid (no dataset: the tables are all the probe reads)"""

    def __init__(self):
        from magprop_amd import _capi
        self.capi = _capi
        _capi.lib()                                        # first, so that one HIP runtime is shared
        self.L = L = probe_lib.load("dense")
        for name in ("mpi_kinds", "mpi_wtab_size", "mpi_wtab_stride", "mpi_wtab_theta", "mpi_wtab_dense", "mpi_ttab_n", "mpi_ktab_n", "mpi_max_n"):
            getattr(L, name).restype, getattr(L, name).argtypes = _i, []
        L.mpi_tables.restype, L.mpi_tables.argtypes = _i, [_vp, _dp, _dp, _dp, _dp]
        L.mpi_lds_tables.restype, L.mpi_lds_tables.argtypes = _i, [_vp, _i, _i, _dp, _dp, _dp]
        L.mpi_hermite.restype, L.mpi_hermite.argtypes = _i, [_dp, _i, _dp]
        L.mpi_fallback.restype, L.mpi_fallback.argtypes = _i, [_i, _dp, _dp, _dp, _i, _dp]
        L.mpi_image_state.restype = _i
        L.mpi_image_state.argtypes = [_vp, _i, _dp, _i, _i, _i, C.c_double, _dp, _ip, _i, _dp]
        self.handles = {}

    def handle(self, tgrid):
        key = (float(tgrid[0]), float(tgrid[-1]), int(tgrid.size))
        if key not in self.handles:
            self.handles[key] = self.capi.Handle(self.capi.cfg_synth(), tgrid)
        return self.handles[key]

    def tables(self, h):
        sk, wtab = np.full((dr.KINDS, 3), CANARY), np.full(dr.WTAB_SIZE, CANARY)
        ttab, scal = np.full((dr.KINDS - 1, dr.TTAB_N), CANARY), np.full(3, CANARY)
        rc = self.L.mpi_tables(h._h, _d(sk), _d(wtab), _d(ttab), _d(scal))
        assert rc == 0, f"mpi_tables returned {rc}"
        return dict(sk=sk, wtab=wtab, ttab=ttab, t0=scal[0], lnq8=scal[1], pre_fine=int(scal[2]))

    def lds_tables(self, h, G, NT):
        ktab, wtab, E = np.full(dr.KTAB_N, CANARY), np.full(dr.WTAB_SIZE, CANARY), np.full((dr.KINDS - 1, 64 * G + 1), CANARY)
        rc = self.L.mpi_lds_tables(h._h, G, NT, _d(ktab), _d(wtab), _d(E))
        assert rc == 0, f"mpi_lds_tables returned {rc}"
        return ktab, wtab, E

    def hermite(self, elems):
        """elems[9][n] -> [4][n]: hermite, hermite_d, hermite5, hermite_mdisc"""
        elems = np.ascontiguousarray(elems, dtype=np.float64)
        n = elems.shape[1]
        out = np.full((4, n), CANARY)
        rc = self.L.mpi_hermite(_d(elems), n, _d(out))
        assert rc == 0, f"mpi_hermite returned {rc}"
        return out

    def fallback(self, N, S_amp, inv_tfb, t):
        """-> [4][nq][N]: S of mdot_fb, then S, dS, iu of mdot_fb_d"""
        S_amp, inv_tfb, t = (np.ascontiguousarray(a, dtype=np.float64) for a in (S_amp, inv_tfb, t))
        nq = S_amp.size
        assert t.shape == (nq, N)
        out = np.full((4, nq, N), CANARY)
        rc = self.L.mpi_fallback(N, _d(S_amp), _d(inv_tfb), _d(t), nq, _d(out))
        assert rc == 0, f"mpi_fallback returned {rc}"
        return out

    def image_state_rc(self, h, G, tile, p8=None, out=None):
        walker = np.array(tile["walker"], dtype=np.float64)
        img = np.ascontiguousarray(tile["img"], dtype=np.float64)
        assert img.shape == (5, 64 * G + 1)
        p8 = np.ascontiguousarray(tile["p8"] if p8 is None else p8, dtype=np.int32)
        out = np.full((2, p8.size), CANARY) if out is None else out
        rc = self.L.mpi_image_state(h._h, G, _d(walker), int(tile["kind"]), int(tile["pos8"]), int(tile["keep"]), float(tile["t_s"]),
                                    _d(img), p8.ctypes.data_as(_ip), int(p8.size), _d(out))
        return rc, out

    def image_state(self, h, G, tile):
        """-> (Mv, Wv) of every query of the tile"""
        rc, out = self.image_state_rc(h, G, tile)
        assert rc == 0, f"mpi_image_state returned {rc}"
        return out[0], out[1]
