"""Loads tests/admit_class_probe.cpp (built with host_class_probe.build) and drives it through ctypes.  Test helper, not collected."""
import ctypes as C
import os

import numpy as np

import host_class_probe


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class AdmitClassProbe:
    def __init__(self, out_dir):
        self.dir = str(out_dir)
        self.L = C.CDLL(host_class_probe.build("admit_class_probe.cpp", out_dir))

    def _call(self, fn, *args):
        err = C.create_string_buffer(1024)
        rc = fn(*args, err, 1024)
        if rc:
            raise RuntimeError(err.value.decode() or "the probe returned %d" % rc)

    def create(self, size, K, window, radius, min_score=0.75, passes=0, factor=1.0, quantile=0.5, min_cost=0.0, outlier_passes=0):
        K4 = np.array(K, np.float64)
        o4 = np.array([passes, factor, quantile, min_cost], np.float64)
        self._call(self.L.admit_probe_create, int(size[0]), int(size[1]), _ptr(K4), int(window), int(radius), C.c_double(min_score), _ptr(o4),
                   int(outlier_passes))

    def add(self, image, depth, T, max_admitted=1 << 16):
        """None when no optimisation ran, else dict(n_poses, admitted_blocks, admitted [k, 2] = (position in visibility(), frame id),
        culled_blocks, residuals, initial_cost, final_cost)."""
        image = np.ascontiguousarray(image, np.uint8)
        depth = np.ascontiguousarray(depth, np.float32)
        T = np.ascontiguousarray(T, np.float64)
        ints, costs, adm = np.zeros(6, np.int32), np.zeros(2), np.zeros((max_admitted, 2), np.uint32)
        self._call(self.L.admit_probe_add, _ptr(image), _ptr(depth), _ptr(T), _ptr(ints), _ptr(costs), _ptr(adm), max_admitted)
        if not ints[0]:
            return None
        assert ints[3] <= max_admitted
        return dict(n_poses=int(ints[1]), admitted_blocks=int(ints[2]), admitted=adm[:ints[3]].astype(np.int64), culled_blocks=int(ints[4]),
                    residuals=int(ints[5]), initial_cost=float(costs[0]), final_cost=float(costs[1]))

    def visibility(self, max_lists=1 << 16, max_ids=1 << 20):
        """The visibility list of every scene point the instance holds: a list of int arrays."""
        n, begin, ids = C.c_int(0), np.zeros(max_lists + 1, np.int32), np.zeros(max_ids, np.uint32)
        self._call(self.L.admit_probe_visibility, C.byref(n), _ptr(begin), max_lists, _ptr(ids), max_ids)
        return [ids[begin[i]:begin[i + 1]].astype(np.int64) for i in range(n.value)]

    def add_frames(self, image, depth, T):
        image = np.ascontiguousarray(image, np.uint8)
        depth = np.ascontiguousarray(depth, np.float32)
        T = np.ascontiguousarray(T, np.float64)
        self._call(self.L.admit_probe_add_frames, _ptr(image), _ptr(depth), _ptr(T))

    def defaults(self):
        """(Options::reobservePasses, reobserveFactor, reobserveQuantile, reobserveMinCost), Result's admitted count by default."""
        out = np.zeros(4)
        n = int(self.L.admit_probe_defaults(_ptr(out)))
        return tuple(out), n

    def parse_and_print(self, config_text):
        """Options(ConfigFile of config_text) printed as ConfigFile lines."""
        out = C.create_string_buffer(8192)
        self._call(self.L.admit_probe_parse_and_print, config_text.encode(), os.path.join(self.dir, "probe.cfg").encode(), out, 8192)
        return out.value.decode()

    def release(self):
        self.L.admit_probe_release()
