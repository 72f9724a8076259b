"""Python mirror of the stereo matchers' C-ABI (include/pba_stereo.h, include/pba_sgm.h): thin, no compute.
StereoBM(rows, cols, **params).compute(left, right, bf) runs XSOBEL prefilter + block matching (+ fused depth) and
StereoSGM(rows, cols, **params).compute(left, right, bf) semi-global matching (+ fused depth) in libpba_hip.so on the GPU;
there is no CPU fallback."""
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


# --- semi-global matching (include/pba_sgm.h) ---

SGM_INT_FIELDS = ("number_of_disparities", "sobel_cap_value", "census_radius", "window_radius", "smoothness_penalty_small",
                  "smoothness_penalty_large", "consistency_threshold")
SGM_FLOAT_FIELDS = ("disparity_factor", "census_weight_factor")
SGM_PARAM_FIELDS = SGM_INT_FIELDS + SGM_FLOAT_FIELDS

# name -> (PBA_SGM_STAGE_*, dtype, has a disparity axis)
SGM_STAGES = {
    "sobel_left": (0, np.uint8, False), "sobel_right": (1, np.uint8, False),
    "census_left": (2, np.int32, False), "census_right": (3, np.int32, False),
    "cost_left": (4, np.uint16, True), "sum_left": (5, np.int16, True),
    "disp_left_raw": (6, np.uint16, False), "disp_right_raw": (7, np.uint16, False),
    "disp_left_filtered": (8, np.uint16, False), "disp_right_filtered": (9, np.uint16, False),
}


class SGMParams(C.Structure):
    _fields_ = ([(f, C.c_int32) for f in SGM_INT_FIELDS] + [("reserved", C.c_int32)] +
                [(f, C.c_double) for f in SGM_FLOAT_FIELDS])


def _sgm_lib():
    L = _lib.lib()
    if not getattr(L, "_sgm_bound", False):
        L.pba_sgm_default_params.argtypes = [C.POINTER(SGMParams)]
        L.pba_sgm_default_params.restype = None
        L.pba_sgm_validate_params.argtypes = [C.c_int32, C.c_int32, C.POINTER(SGMParams)]
        L.pba_sgm_create.argtypes = [C.c_int32, C.c_int32, C.POINTER(SGMParams), C.c_int32, C.POINTER(C.c_void_p)]
        L.pba_sgm_compute.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
        L.pba_sgm_last_error.argtypes = [C.c_void_p]
        L.pba_sgm_last_error.restype = C.c_char_p
        L.pba_sgm_destroy.argtypes = [C.c_void_p]
        L.pba_sgm_destroy.restype = None
        L.pba_sgm_get_timing.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.pba_sgm_get_stage.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L._sgm_bound = True
    return L


def sgm_default_params(**kw):
    """pba_sgm_default_params (the reference's SgmStereo::Config) with the given fields replaced."""
    p = SGMParams()
    _sgm_lib().pba_sgm_default_params(C.byref(p))
    for k, v in kw.items():
        if k in SGM_INT_FIELDS:
            setattr(p, k, int(v))
        elif k in SGM_FLOAT_FIELDS:
            setattr(p, k, float(v))
        else:
            raise AttributeError(k)
    return p


def sgm_validate_params(rows, cols, **kw):
    """pba_sgm_validate_params: raises StereoError (PBA_ERR_INVALID, the key named in the message) without touching a device."""
    L = _sgm_lib()
    p = sgm_default_params(**kw)
    rc = L.pba_sgm_validate_params(int(rows), int(cols), C.byref(p))
    if rc != 0:
        raise StereoError(rc, "pba_sgm_validate_params: %s: %s" % (L.pba_status_string(rc).decode(),
                                                                    L.pba_sgm_last_error(None).decode()))
    return p


class StereoSGM:
    """One semi-global matcher for rows x cols u8 pairs on HIP device `device`."""

    def __init__(self, rows, cols, device=0, **params):
        self._L = _sgm_lib()
        self.rows, self.cols = int(rows), int(cols)
        self.params = sgm_default_params(**params)
        self._h = C.c_void_p()
        rc = self._L.pba_sgm_create(self.rows, self.cols, C.byref(self.params), int(device), C.byref(self._h))
        if rc != 0:
            self._h = None
            raise StereoError(rc, "pba_sgm_create: %s: %s" % (self._L.pba_status_string(rc).decode(),
                                                              self._L.pba_sgm_last_error(None).decode()))

    def _check(self, rc, what):
        if rc != 0:
            raise StereoError(rc, "%s: %s: %s" % (what, self._L.pba_status_string(rc).decode(),
                                                  self._L.pba_sgm_last_error(self._h).decode()))

    def _image(self, a):
        a = np.ascontiguousarray(a, dtype=np.uint8)
        if a.shape != (self.rows, self.cols):
            raise ValueError("image of shape %s, matcher built for %s" % (a.shape, (self.rows, self.cols)))
        return a

    def compute_all(self, left, right, bf=1.0, disp_scaled=True, disparity=True, depth=True):
        """-> (uint16 disparity * disparity_factor, fp32 disparity, fp32 depth), None for what is not asked for."""
        left, right = self._image(left), self._image(right)
        shape = (self.rows, self.cols)
        u = np.empty(shape, np.uint16) if disp_scaled else None
        d = np.empty(shape, np.float32) if disparity else None
        z = np.empty(shape, np.float32) if depth else None
        self._check(self._L.pba_sgm_compute(self._h, _ptr(left), _ptr(right), C.c_float(bf),
                                            _ptr(u) if u is not None else None, _ptr(d) if d is not None else None,
                                            _ptr(z) if z is not None else None), "pba_sgm_compute")
        return u, d, z

    def compute(self, left, right, bf=1.0):
        """-> (fp32 disparity, 0 = invalid; fp32 depth = d > 0.01 ? bf / d : -0.1)."""
        _, d, z = self.compute_all(left, right, bf, disp_scaled=False)
        return d, z

    def stage(self, name):
        """One intermediate of the last compute (test hook), by its name in SGM_STAGES."""
        index, dtype, volume = SGM_STAGES[name]
        shape = (self.rows, self.cols, self.params.number_of_disparities) if volume else (self.rows, self.cols)
        a = np.empty(shape, dtype)
        self._check(self._L.pba_sgm_get_stage(self._h, index, _ptr(a)), "pba_sgm_get_stage")
        return a

    def timing(self):
        """(kernels_ms, total_ms) of the last compute, from device events."""
        k, t = C.c_float(), C.c_float()
        self._check(self._L.pba_sgm_get_timing(self._h, C.byref(k), C.byref(t)), "pba_sgm_get_timing")
        return k.value, t.value

    def close(self):
        if getattr(self, "_h", None):
            self._L.pba_sgm_destroy(self._h)
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
