"""Where the probe libraries are: load("select") opens libmp_probe_select.so, load() libmp_probe.so, from the package directory
(test infrastructure built next to libmagprop_amd.so by magprop_amd/csrc/Makefile, no part of the product's ABI)."""
import ctypes
import os


def load(name=None):
    from magprop_amd import _capi
    pkg = os.path.dirname(os.path.abspath(_capi.__file__))
    return ctypes.CDLL(os.path.join(pkg, "libmp_probe_" + name + ".so" if name else "libmp_probe.so"))
