"""Loads tests/covariance_class_probe.cpp (built with host_class_probe.build) and drives it through ctypes.  Test helper, not collected."""
import ctypes as C

import numpy as np

import host_class_probe


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class CovarianceClassProbe:
    def __init__(self, out_dir):
        self.L = C.CDLL(host_class_probe.build("covariance_class_probe.cpp", out_dir))

    def _call(self, fn, *args):
        err = C.create_string_buffer(1024)
        if fn(*args, err, 1024):
            raise RuntimeError(err.value.decode())

    def create(self, size, K, window, radius, min_score=0.75, num_constant=1, cameras_constant=False, compute_covariance=False):
        K4 = np.array(K, np.float64)
        self._call(self.L.cov_probe_create, int(size[0]), int(size[1]), _ptr(K4), int(window), int(radius), C.c_double(min_score),
                   int(num_constant), int(bool(cameras_constant)), int(bool(compute_covariance)))

    def add(self, image, depth, T, max_poses=64, max_points=1 << 16):
        """None when no optimisation ran, else dict(poses, refined, covariance_ok, message, min_camera_pivot, min_point_pivot, frame_ids,
        pose_cov [n, n], point_cov [m, 3, 3])."""
        image = np.ascontiguousarray(image, np.uint8)
        depth = np.ascontiguousarray(depth, np.float32)
        T = np.ascontiguousarray(T, np.float64)
        ints, piv, ids, n_pc = np.zeros(5, np.int32), np.zeros(2), np.zeros(32, np.int32), C.c_int(0)
        poses, refined = np.zeros((max_poses, 4, 4)), np.zeros((max_points, 3))
        pose_cov, point_cov = np.zeros(192 * 192), np.zeros((max_points, 3, 3))
        msg = C.create_string_buffer(1024)
        self._call(self.L.cov_probe_add, _ptr(image), _ptr(depth), _ptr(T), _ptr(ints), _ptr(poses), max_poses, _ptr(refined), max_points,
                   _ptr(piv), _ptr(ids), _ptr(pose_cov), _ptr(point_cov), C.byref(n_pc), msg, 1024)
        if not ints[0]:
            return None
        assert ints[1] <= max_poses and ints[2] <= max_points
        n = 6 * int(ints[4])
        return dict(poses=poses[:ints[1]].copy(), refined=refined[:ints[2]].copy(), covariance_ok=bool(ints[3]), message=msg.value.decode(),
                    min_camera_pivot=float(piv[0]), min_point_pivot=float(piv[1]), frame_ids=[int(v) for v in ids[:ints[4]]],
                    pose_cov=pose_cov[:n * n].reshape(n, n).copy(), point_cov=point_cov[:n_pc.value].copy())

    def track(self, image, T, compute_covariance):
        image = np.ascontiguousarray(image, np.uint8)
        T = np.ascontiguousarray(T, np.float64)
        out, ints, cov, piv = np.zeros((4, 4)), np.zeros(2, np.int32), np.zeros((6, 6)), C.c_double(0.0)
        self._call(self.L.cov_probe_track, _ptr(image), _ptr(T), int(bool(compute_covariance)), _ptr(out), _ptr(ints), _ptr(cov), C.byref(piv))
        return out, dict(tracked=bool(ints[0]), covariance_ok=bool(ints[1]), covariance=cov, min_pivot=piv.value)

    def defaults(self):
        return int(self.L.cov_probe_defaults())

    def print_options(self, compute_covariance):
        out = C.create_string_buffer(4096)
        self.L.cov_probe_print_options(int(bool(compute_covariance)), out, 4096)
        return out.value.decode()

    def release(self):
        self.L.cov_probe_release()
