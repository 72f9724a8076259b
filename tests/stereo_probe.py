"""Builds and loads tests/stereo_host_probe.cpp (the host StereoAlgorithm / disparityToDepth through ctypes) into a directory the
caller owns.  Test helper, not collected."""
import ctypes as C
import os

import numpy as np

from host_class_probe import build

PARAM_FIELDS = ("pre_filter_type", "pre_filter_size", "pre_filter_cap", "sad_window_size", "min_disparity",
                "number_of_disparities", "texture_threshold", "uniqueness_ratio", "speckle_window_size", "speckle_range",
                "try_smaller_windows", "disp12_max_diff")


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class HostProbe:
    def __init__(self, out_dir):
        self.L = C.CDLL(build("stereo_host_probe.cpp", out_dir, openmp=False))

    def parse(self, cfg_text, tmp_dir):
        path = os.path.join(str(tmp_dir), "stereo_probe.cfg")
        with open(path, "w") as f:
            f.write(cfg_text)
        params = np.zeros(12, np.int32)
        inv = C.c_float()
        err = C.create_string_buffer(1024)
        rc = self.L.probe_parse(path.encode(), _ptr(params), C.byref(inv), err, 1024)
        if rc:
            raise RuntimeError(err.value.decode())
        return dict(zip(PARAM_FIELDS, params.tolist())), inv.value

    def run(self, left, right):
        d = np.empty(left.shape, np.float32)
        err = C.create_string_buffer(1024)
        if self.L.probe_run(_ptr(left), _ptr(right), left.shape[0], left.shape[1], _ptr(d), err, 1024):
            raise RuntimeError(err.value.decode())
        return d

    def depth(self, left, right, bf):
        z = np.empty(left.shape, np.float32)
        err = C.create_string_buffer(1024)
        if self.L.probe_depth(_ptr(left), _ptr(right), left.shape[0], left.shape[1], C.c_float(bf), _ptr(z), err, 1024):
            raise RuntimeError(err.value.decode())
        return z

    def release(self):
        self.L.probe_release()

    def disparity_to_depth(self, d, bf):
        d = np.ascontiguousarray(d, np.float32)
        z = np.empty(d.shape, np.float32)
        self.L.probe_disparity_to_depth(_ptr(d), d.shape[0], d.shape[1], C.c_float(bf), _ptr(z))
        return z
