"""libmp_probe_flows.so (magprop_amd/csrc/mp_probe_flows.hip: the two kernels behind mp_model_flows over host buffers; test
infrastructure, no part of the product's ABI) behind numpy arrays, for tests/test_gpu_flows_kernels.py and tests/test_gpu_flows.py."""
import ctypes as C

import numpy as np

import flows_cases as fc
import flows_restated as fr
import probe_lib

_dp, _ip, _i, _u32 = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_int, C.c_uint32
ALL = (1 << fr.NCURVES) - 1


class Probe:
    """libmp_probe_flows.so behind numpy arrays"""

    def __init__(self):
        from magprop_amd import _capi
        self.capi = _capi
        _capi.lib()                                        # first, so that one HIP runtime is shared
        self.L = probe_lib.load("flows")
        for name in ("mpf_threads", "mpf_lane", "mpf_window", "mpf_curves", "mpf_columns", "mpf_max_rows"):
            getattr(self.L, name).restype = _i
            getattr(self.L, name).argtypes = []
        self.L.mpf_reduce_mask.restype, self.L.mpf_reduce_mask.argtypes = C.c_uint, []
        self.L.mpf_seg.restype, self.L.mpf_seg.argtypes = _i, [_i]
        self.L.mpf_cells.restype = _i
        self.L.mpf_cells.argtypes = [C.POINTER(_capi.ModelCfg), _dp, _dp, _dp, _dp, _ip, _i, _i, _i, _u32, _dp]
        self.L.mpf_reduce.restype = _i
        self.L.mpf_reduce.argtypes = [_dp, _ip, _dp, _i, _i, _dp]

    def cfg(self, preset, **over):
        return (self.capi.cfg_synth if preset == "synth" else self.capi.cfg_lib)(**dict(fc.PRESETS[preset], **over))

    def cells(self, cfg, pars, t, mdisc, omega, status=None, mask=ALL):
        pars = np.ascontiguousarray(np.atleast_2d(pars), dtype=np.float64)
        t, mdisc, omega = (np.ascontiguousarray(np.atleast_2d(a), dtype=np.float64) for a in (t, mdisc, omega))
        rows, G = t.shape
        st = np.zeros(rows, dtype=np.int32) if status is None else np.ascontiguousarray(status, dtype=np.int32)
        out = np.full((bin(mask).count("1"), rows, G), -777.0)     # a canary the kernel must overwrite
        rc = self.L.mpf_cells(C.byref(cfg), t.ctypes.data_as(_dp), mdisc.ctypes.data_as(_dp), omega.ctypes.data_as(_dp),
                              pars.ctypes.data_as(_dp), st.ctypes.data_as(_ip), rows, G, pars.shape[1], mask, out.ctypes.data_as(_dp))
        assert rc == 0, f"mpf_cells returned {rc}"
        return out

    def reduce(self, t, cells, status):
        cells = np.ascontiguousarray(cells, dtype=np.float64)
        status = np.ascontiguousarray(status, dtype=np.int32)
        t = np.ascontiguousarray(t, dtype=np.float64)
        out = np.full((cells.shape[1], fr.N), -777.0)
        rc = self.L.mpf_reduce(cells.ctypes.data_as(_dp), status.ctypes.data_as(_ip), t.ctypes.data_as(_dp), cells.shape[1], t.size,
                               out.ctypes.data_as(_dp))
        assert rc == 0, f"mpf_reduce returned {rc}"
        return out
