"""Loads tests/point_prior_class_probe.cpp (built with host_class_probe.build) and drives it through ctypes.  Test helper, not collected."""
import ctypes as C

import numpy as np

import host_class_probe


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class PointPriorClassProbe:
    def __init__(self, out_dir):
        self.L = C.CDLL(host_class_probe.build("point_prior_class_probe.cpp", out_dir))
        self.L.pp_probe_config_key.restype = C.c_double
        self.L.pp_probe_config_key.argtypes = [C.c_char_p]
        self.L.pp_probe_print_options.argtypes = [C.c_double, C.c_char_p, C.c_int]
        self.size = None

    def create(self, size, K, window, radius, sigma, baseline=0.5, min_score=0.75, num_constant=1, compute_covariance=False, marginalize=False):
        """(status, text): 0 an instance exists, 1 std::invalid_argument, 2 another exception (no device), with the exception's text."""
        K4 = np.array(K, np.float64)
        what = C.create_string_buffer(1024)
        self.size = size
        rc = self.L.pp_probe_create(int(size[0]), int(size[1]), _ptr(K4), C.c_double(baseline), int(window), int(radius), C.c_double(min_score),
                                    int(num_constant), int(bool(compute_covariance)), int(bool(marginalize)), C.c_double(sigma), what, 1024)
        return rc, what.value.decode()

    def add(self, image, depth, T, max_poses=64):
        """None when no optimisation ran, else dict(initial_cost, final_cost, depth_prior_cost, covariance_ok, message, min_camera_pivot,
        min_point_pivot, n_free, poses)."""
        image = np.ascontiguousarray(image, np.uint8)
        depth = np.ascontiguousarray(depth, np.float32)
        T = np.ascontiguousarray(T, np.float64)
        ints, vals, poses = np.zeros(4, np.int32), np.zeros(5), np.zeros((max_poses, 4, 4))
        msg, err = C.create_string_buffer(1024), C.create_string_buffer(1024)
        if self.L.pp_probe_add(_ptr(image), _ptr(depth), _ptr(T), _ptr(ints), _ptr(vals), _ptr(poses), max_poses, msg, 1024, err, 1024):
            raise RuntimeError(err.value.decode())
        if not ints[0]:
            return None
        return dict(initial_cost=float(vals[0]), final_cost=float(vals[1]), depth_prior_cost=float(vals[2]), covariance_ok=bool(ints[2]),
                    message=msg.value.decode(), min_camera_pivot=float(vals[3]), min_point_pivot=float(vals[4]), n_free=int(ints[3]),
                    poses=poses[:ints[1]].copy())

    def add_frames(self):
        what = C.create_string_buffer(1024)
        rc = self.L.pp_probe_add_frames(int(self.size[0]), int(self.size[1]), what, 1024)
        return rc, what.value.decode()

    def defaults_are_zero(self):
        return bool(self.L.pp_probe_defaults_are_zero())

    def config_key(self, value):
        return float(self.L.pp_probe_config_key(value.encode()))

    def print_options(self, sigma):
        out = C.create_string_buffer(8192)
        self.L.pp_probe_print_options(float(sigma), out, 8192)
        return out.value.decode()

    def release(self):
        self.L.pp_probe_release()
