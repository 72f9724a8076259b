"""Builds and loads tests/anchors_host_probe.cpp (Options::numConstantFrames of the host classes through ctypes) into a directory the
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
    so = os.path.join(str(out_dir), "libanchors_host_probe.so")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-fopenmp", "-shared", "-o", so,
                           os.path.join(ROOT, "tests", "anchors_host_probe.cpp"), "-L" + PKG, "-lphotobundle", "-lpba_hip",
                           "-Wl,-rpath," + PKG])
    return so


class AnchorsProbe:
    def __init__(self, out_dir):
        self.L = C.CDLL(build(out_dir))

    def _call(self, fn, *args):
        err = C.create_string_buffer(1024)
        if fn(*args, err, 1024):
            raise RuntimeError(err.value.decode())

    def create(self, size, K, window, radius, min_score=0.75, num_constant=None, levels=1):
        K4 = np.array(K, np.float64)
        self._call(self.L.probe_anchors_create, int(levels), int(size[0]), int(size[1]), _ptr(K4), int(window), int(radius),
                   C.c_double(min_score), -1 if num_constant is None else int(num_constant))

    def add(self, image, depth, T, max_poses=64):
        """None when no optimisation ran, else dict(poses [n, 4, 4], fixed_cost)."""
        image = np.ascontiguousarray(image, np.uint8)
        depth = np.ascontiguousarray(depth, np.float32)
        T = np.ascontiguousarray(T, np.float64)
        poses = np.zeros((max_poses, 4, 4))
        n, fixed = C.c_int(0), C.c_double(0.0)
        self._call(self.L.probe_anchors_add, _ptr(image), _ptr(depth), _ptr(T), _ptr(poses), max_poses, C.byref(n), C.byref(fixed))
        return dict(poses=poses[:n.value].copy(), fixed_cost=fixed.value) if n.value else None

    def default(self):
        return int(self.L.probe_anchors_default())

    def print_options(self, num_constant):
        out = C.create_string_buffer(4096)
        self.L.probe_anchors_print_options(int(num_constant), out, 4096)
        return out.value.decode()

    def release(self):
        self.L.probe_anchors_release()
