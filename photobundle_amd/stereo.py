"""Python mirror of the stereo matcher's C-ABI (include/pba_stereo.h): thin, no compute.  StereoBM(rows, cols, **params)
.compute(left, right, bf) runs XSOBEL prefilter + block matching (+ fused depth) in libpba_hip.so on the GPU; there is no
CPU fallback."""
import ctypes as C

import numpy as np

from . import _lib

PARAM_FIELDS = ("pre_filter_type", "pre_filter_size", "pre_filter_cap", "sad_window_size", "min_disparity",
                "number_of_disparities", "texture_threshold", "uniqueness_ratio", "speckle_window_size", "speckle_range",
                "try_smaller_windows", "disp12_max_diff")


class BMParams(C.Structure):
    _fields_ = [(f, C.c_int32) for f in PARAM_FIELDS]


class StereoError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(message)
        self.status = status


def _stereo_lib():
    L = _lib.lib()
    if not getattr(L, "_stereo_bound", False):
        L.pba_stereo_default_params.argtypes = [C.POINTER(BMParams)]
        L.pba_stereo_default_params.restype = None
        L.pba_stereo_create.argtypes = [C.c_int32, C.c_int32, C.POINTER(BMParams), C.c_int32, C.POINTER(C.c_void_p)]
        L.pba_stereo_compute.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
        L.pba_stereo_last_error.argtypes = [C.c_void_p]
        L.pba_stereo_last_error.restype = C.c_char_p
        L.pba_stereo_destroy.argtypes = [C.c_void_p]
        L.pba_stereo_destroy.restype = None
        L.pba_stereo_get_prefiltered.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.pba_stereo_get_timing.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.pba_stereo_validate_params.argtypes = [C.c_int32, C.c_int32, C.POINTER(BMParams)]
        L._stereo_bound = True
    return L


def default_params(**kw):
    """pba_stereo_default_params (reference src/stereo_algorithm.cc:249-264) with the given fields replaced."""
    p = BMParams()
    _stereo_lib().pba_stereo_default_params(C.byref(p))
    for k, v in kw.items():
        if k not in PARAM_FIELDS:
            raise AttributeError(k)
        setattr(p, k, int(v))
    return p


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class StereoBM:
    """One matcher for rows x cols u8 pairs on HIP device `device`."""

    def __init__(self, rows, cols, device=0, **params):
        self._L = _stereo_lib()
        self.rows, self.cols = int(rows), int(cols)
        self.params = default_params(**params)
        self._h = C.c_void_p()
        rc = self._L.pba_stereo_create(self.rows, self.cols, C.byref(self.params), int(device), C.byref(self._h))
        if rc != 0:
            self._h = None
            raise StereoError(rc, "pba_stereo_create: %s: %s" % (self._L.pba_status_string(rc).decode(),
                                                                 self._L.pba_stereo_last_error(None).decode()))

    @property
    def filtered(self):
        return (self.params.min_disparity - 1) * 16

    def _check(self, rc, what):
        if rc != 0:
            raise StereoError(rc, "%s: %s: %s" % (what, self._L.pba_status_string(rc).decode(),
                                                  self._L.pba_stereo_last_error(self._h).decode()))

    def _image(self, a):
        a = np.ascontiguousarray(a, dtype=np.uint8)
        if a.shape != (self.rows, self.cols):
            raise ValueError("image of shape %s, matcher built for %s" % (a.shape, (self.rows, self.cols)))
        return a

    def compute(self, left, right, bf=1.0, disparity=True, depth=True):
        """-> (int16 disparity with 4 fractional bits or None, fp32 depth or None); only what is asked for is copied back."""
        left, right = self._image(left), self._image(right)
        d = np.empty((self.rows, self.cols), np.int16) if disparity else None
        z = np.empty((self.rows, self.cols), np.float32) if depth else None
        self._check(self._L.pba_stereo_compute(self._h, _ptr(left), _ptr(right), C.c_float(bf),
                                               _ptr(d) if d is not None else None, _ptr(z) if z is not None else None),
                    "pba_stereo_compute")
        return d, z

    def prefiltered(self):
        a = np.empty((self.rows, self.cols), np.uint8)
        b = np.empty((self.rows, self.cols), np.uint8)
        self._check(self._L.pba_stereo_get_prefiltered(self._h, _ptr(a), _ptr(b)), "pba_stereo_get_prefiltered")
        return a, b

    def timing(self):
        """(kernels_ms, total_ms) of the last compute, from device events."""
        k, t = C.c_float(), C.c_float()
        self._check(self._L.pba_stereo_get_timing(self._h, C.byref(k), C.byref(t)), "pba_stereo_get_timing")
        return k.value, t.value

    def close(self):
        if getattr(self, "_h", None):
            self._L.pba_stereo_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
