"""Builds and loads tests/points_host_probe.cpp (the host class with Options::camerasConstant through ctypes) into a directory the
caller owns.  Test helper, not collected."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "photobundle_amd")


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def build(out_dir):
    so = os.path.join(str(out_dir), "libpoints_host_probe.so")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-fopenmp", "-shared", "-o", so,
                           os.path.join(ROOT, "tests", "points_host_probe.cpp"), "-L" + PKG, "-lphotobundle", "-lpba_hip",
                           "-Wl,-rpath," + PKG])
    return so


class PointsProbe:
    def __init__(self, out_dir):
        self.L = C.CDLL(build(out_dir))

    def _call(self, fn, *args):
        err = C.create_string_buffer(1024)
        if fn(*args, err, 1024):
            raise RuntimeError(err.value.decode())

    def create(self, size, K, window, radius, min_score=0.75, cameras_constant=True):
        K4 = np.array(K, np.float64)
        self._call(self.L.probe_points_create, int(size[0]), int(size[1]), _ptr(K4), int(window), int(radius), C.c_double(min_score),
                   int(bool(cameras_constant)))

    def add(self, image, depth, T, max_poses=64, max_points=1 << 16):
        """None when no optimisation ran, else dict(initial_cost, final_cost, poses [k, 4, 4], refined [m, 3], original [m, 3])."""
        image = np.ascontiguousarray(image, np.uint8)
        depth = np.ascontiguousarray(depth, np.float32)
        T = np.ascontiguousarray(T, np.float64)
        ran, costs, counts = C.c_int(0), np.zeros(2), np.zeros(2, np.int32)
        poses, refined, original = np.zeros((max_poses, 4, 4)), np.zeros((max_points, 3)), np.zeros((max_points, 3))
        self._call(self.L.probe_points_add, _ptr(image), _ptr(depth), _ptr(T), C.byref(ran), _ptr(costs), _ptr(counts), _ptr(poses),
                   max_poses, _ptr(refined), _ptr(original), max_points)
        if not ran.value:
            return None
        assert counts[0] <= max_poses and counts[1] <= max_points
        return dict(initial_cost=float(costs[0]), final_cost=float(costs[1]), poses=poses[:counts[0]].copy(),
                    refined=refined[:counts[1]].copy(), original=original[:counts[1]].copy())

    def print_options(self, cameras_constant):
        out = C.create_string_buffer(4096)
        self.L.probe_points_print_options(int(bool(cameras_constant)), out, 4096)
        return out.value.decode()

    def release(self):
        self.L.probe_points_release()
