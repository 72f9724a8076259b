"""Loads tests/cull_class_probe.cpp (built with host_class_probe.build) and drives it through ctypes.  Test helper, not collected."""
import ctypes as C
import os

import numpy as np

import host_class_probe


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class CullClassProbe:
    def __init__(self, out_dir):
        self.dir = str(out_dir)
        self.L = C.CDLL(host_class_probe.build("cull_class_probe.cpp", out_dir))

    def _call(self, fn, *args):
        err = C.create_string_buffer(1024)
        if fn(*args, err, 1024):
            raise RuntimeError(err.value.decode())

    def create(self, size, K, window, radius, min_score=0.75, passes=0, quantile=0.5, factor=3.0, min_cost=0.0, min_observations=2):
        K4 = np.array(K, np.float64)
        o5 = np.array([passes, quantile, factor, min_cost, min_observations], np.float64)
        self._call(self.L.cull_probe_create, int(size[0]), int(size[1]), _ptr(K4), int(window), int(radius), C.c_double(min_score), _ptr(o5))

    def add(self, image, depth, T, max_poses=64):
        """None when no optimisation ran, else dict(poses, n_left, culled_blocks, culled_points, iterations, initial_cost, final_cost)."""
        image = np.ascontiguousarray(image, np.uint8)
        depth = np.ascontiguousarray(depth, np.float32)
        T = np.ascontiguousarray(T, np.float64)
        ints, costs, poses = np.zeros(6, np.int32), np.zeros(2), np.zeros((max_poses, 4, 4))
        self._call(self.L.cull_probe_add, _ptr(image), _ptr(depth), _ptr(T), _ptr(ints), _ptr(costs), _ptr(poses), max_poses)
        if not ints[0]:
            return None
        assert ints[1] <= max_poses
        return dict(poses=poses[:ints[1]].copy(), n_left=int(ints[2]), culled_blocks=int(ints[3]), culled_points=int(ints[4]),
                    iterations=int(ints[5]), initial_cost=float(costs[0]), final_cost=float(costs[1]))

    def track(self, image, T, passes):
        image = np.ascontiguousarray(image, np.uint8)
        T = np.ascontiguousarray(T, np.float64)
        out, ints, costs = np.zeros((4, 4)), np.zeros(4, np.int32), np.zeros(2)
        self._call(self.L.cull_probe_track, _ptr(image), _ptr(T), int(passes), _ptr(out), _ptr(ints), _ptr(costs))
        return out, dict(tracked=bool(ints[0]), num_points=int(ints[1]), culled_blocks=int(ints[2]), culled_points=int(ints[3]),
                         initial_cost=float(costs[0]), final_cost=float(costs[1]))

    def add_frames(self, image, depth, T):
        image = np.ascontiguousarray(image, np.uint8)
        depth = np.ascontiguousarray(depth, np.float32)
        T = np.ascontiguousarray(T, np.float64)
        self._call(self.L.cull_probe_add_frames, _ptr(image), _ptr(depth), _ptr(T))

    def defaults(self):
        """(Options::outlierPasses, outlierQuantile, outlierFactor, outlierMinCost, outlierMinObservations), bits of the non-zero
        defaults among the Result / TrackOptions / TrackResult fields."""
        out = np.zeros(5)
        bits = int(self.L.cull_probe_defaults(_ptr(out)))
        return tuple(out), bits

    def parse_and_print(self, config_text):
        """Options(ConfigFile of config_text) printed as ConfigFile lines."""
        out = C.create_string_buffer(8192)
        self._call(self.L.cull_probe_parse_and_print, config_text.encode(), os.path.join(self.dir, "probe.cfg").encode(), out, 8192)
        return out.value.decode()

    def release(self):
        self.L.cull_probe_release()
