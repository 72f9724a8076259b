"""Builds and loads tests/sgm_host_probe.cpp (the host SgmStereo through ctypes) into a directory the caller owns.  Test helper,
not collected."""
import ctypes as C
import os

import numpy as np

from host_class_probe import build

INT_KEYS = ("numberOfDisparities", "sobelCapValue", "censusRadius", "windowRadius", "smoothnessPenaltySmall",
            "smoothnessPenaltyLarge", "consistencyThreshold")
FLOAT_KEYS = ("disparityFactor", "censusWeightFactor")


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class SgmHostProbe:
    def __init__(self, out_dir):
        self.L = C.CDLL(build("sgm_host_probe.cpp", out_dir, openmp=False))

    def parse(self, cfg_text, tmp_dir):
        """-> (dict of the nine keys, whether StereoAlgorithm selects SGM); RuntimeError with the message on a refusal."""
        path = os.path.join(str(tmp_dir), "sgm_probe.cfg")
        with open(path, "w") as f:
            f.write(cfg_text)
        ints, doubles, sel = np.zeros(7, np.int32), np.zeros(2, np.float64), C.c_int32()
        err = C.create_string_buffer(1024)
        if self.L.probe_sgm_parse(path.encode(), _ptr(ints), _ptr(doubles), C.byref(sel), err, 1024):
            raise RuntimeError(err.value.decode())
        cfg = dict(zip(INT_KEYS, ints.tolist()))
        cfg.update(zip(FLOAT_KEYS, doubles.tolist()))
        return cfg, bool(sel.value)

    def compute(self, left, right):
        d = np.empty(left.shape, np.float32)
        err = C.create_string_buffer(1024)
        if self.L.probe_sgm_compute(_ptr(left), _ptr(right), left.shape[0], left.shape[1], _ptr(d), err, 1024):
            raise RuntimeError(err.value.decode())
        return d

    def depth(self, left, right, bf):
        z = np.empty(left.shape, np.float32)
        err = C.create_string_buffer(1024)
        if self.L.probe_sgm_depth(_ptr(left), _ptr(right), left.shape[0], left.shape[1], C.c_float(bf), _ptr(z), err, 1024):
            raise RuntimeError(err.value.decode())
        return z

    def release(self):
        self.L.probe_sgm_release()
