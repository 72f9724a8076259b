"""Builds and loads tests/host_class_probe.cpp (addFrame, trackFrame, Options::numConstantFrames and Options::camerasConstant of the host
classes through ctypes) into a directory the caller owns, the one compile line of every host probe, and the synthetic sequence the host
tests feed the classes.  Test helper, not collected."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "photobundle_amd")


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _flag(v):
    """A field the probe leaves at its default when it is None."""
    return -1 if v is None else int(v)


def build(source, out_dir, openmp=True):
    """Compiles tests/<source> against the host library into out_dir; returns the shared library's path."""
    so = os.path.join(str(out_dir), "lib%s.so" % os.path.splitext(source)[0])
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC"] + (["-fopenmp"] if openmp else []) +
                          ["-shared", "-o", so, os.path.join(ROOT, "tests", source), "-L" + PKG, "-lphotobundle", "-lpba_hip",
                           "-Wl,-rpath," + PKG])
    return so


class HostClassProbe:
    def __init__(self, out_dir):
        self.L = C.CDLL(build("host_class_probe.cpp", out_dir))

    def _call(self, fn, *args):
        err = C.create_string_buffer(1024)
        if fn(*args, err, 1024):
            raise RuntimeError(err.value.decode())

    def create(self, levels, size, K, window, radius, min_score=0.75, num_constant=None, cameras_constant=None):
        K4 = np.array(K, np.float64)
        self._call(self.L.probe_create, int(levels), int(size[0]), int(size[1]), _ptr(K4), int(window), int(radius), C.c_double(min_score),
                   _flag(num_constant), _flag(cameras_constant))

    def add(self, image, depth, T, max_poses=64, max_points=1 << 16):
        """None when no optimisation ran, else dict(poses [k, 4, 4], fixed_cost, initial_cost, final_cost, refined [m, 3],
        original [m, 3])."""
        image = np.ascontiguousarray(image, np.uint8)
        depth = np.ascontiguousarray(depth, np.float32)
        T = np.ascontiguousarray(T, np.float64)
        ran, costs, counts = C.c_int(0), np.zeros(3), np.zeros(2, np.int32)
        poses, refined, original = np.zeros((max_poses, 4, 4)), np.zeros((max_points, 3)), np.zeros((max_points, 3))
        self._call(self.L.probe_add, _ptr(image), _ptr(depth), _ptr(T), C.byref(ran), _ptr(costs), _ptr(counts), _ptr(poses), max_poses,
                   _ptr(refined), _ptr(original), max_points)
        if not ran.value:
            return None
        assert counts[0] <= max_poses and counts[1] <= max_points
        return dict(poses=poses[:counts[0]].copy(), fixed_cost=float(costs[2]), initial_cost=float(costs[0]), final_cost=float(costs[1]),
                    refined=refined[:counts[1]].copy(), original=original[:counts[1]].copy())

    def track(self, image, T, max_iterations=50, min_points=64):
        image = np.ascontiguousarray(image, np.uint8)
        T = np.ascontiguousarray(T, np.float64)
        out, ints, costs = np.zeros((4, 4)), np.zeros(3, np.int32), np.zeros(2)
        msg = C.create_string_buffer(512)
        self._call(self.L.probe_track, _ptr(image), _ptr(T), int(max_iterations), int(min_points), _ptr(out), _ptr(ints), _ptr(costs), msg, 512)
        return out, dict(tracked=bool(ints[0]), num_points=int(ints[1]), num_iterations=int(ints[2]), initial_cost=float(costs[0]),
                         final_cost=float(costs[1]), message=msg.value.decode())

    def track_defaults(self, image, T):
        """trackFrame(image, T) with its default arguments."""
        image = np.ascontiguousarray(image, np.uint8)
        T = np.ascontiguousarray(T, np.float64)
        out = np.zeros((4, 4))
        self._call(self.L.probe_track_defaults, _ptr(image), _ptr(T), _ptr(out))
        return out

    def default_num_constant(self):
        return int(self.L.probe_default_num_constant())

    def print_options(self, num_constant=None, cameras_constant=None):
        """The Options with the given fields set, printed as ConfigFile lines."""
        out = C.create_string_buffer(4096)
        self.L.probe_print_options(_flag(num_constant), _flag(cameras_constant), out, 4096)
        return out.value.decode()

    def release(self):
        self.L.probe_release()


def sequence(n_frames, size, K):
    """Exactly photo-consistent frames with exact depth: (images, depths, ground-truth world poses, ground-truth frame-to-frame poses
    T_i = inv(T_w_i) T_w_(i-1), the argument addFrame takes)."""
    from photobundle_amd import synthetic
    tex = synthetic.Texture()
    T_gt = synthetic.make_trajectory(n_frames)
    imgs, depths = [], []
    for T in T_gt:
        im, z = synthetic.render_frame(T, K, size, tex)
        imgs.append(im)
        depths.append(np.where(np.isfinite(z), z, -1.0).astype(np.float32))
    local = [np.linalg.inv(T_gt[0])] + [np.linalg.inv(T_gt[i]) @ T_gt[i - 1] for i in range(1, n_frames)]
    return imgs, depths, T_gt, local


def local_pose_error(T, T_gt):
    """(rotation angle [rad], translation distance) between two frame-to-frame poses."""
    from scipy.spatial.transform import Rotation
    d = Rotation.from_matrix(T[:3, :3] @ T_gt[:3, :3].T).as_rotvec()
    return float(np.linalg.norm(d)), float(np.linalg.norm(T[:3, 3] - T_gt[:3, 3]))


def write_sequence(tmp, imgs, depths, K, local, n_trajectory_lines=None):
    """The files run_kitti reads: image_%06d.pgm, depth_%06d.bin, calib.txt and init.txt (the first n_trajectory_lines poses)."""
    for i, (im, z) in enumerate(zip(imgs, depths)):
        with open(os.path.join(tmp, "image_%06d.pgm" % i), "wb") as f:
            f.write(b"P5\n%d %d\n255\n" % (im.shape[1], im.shape[0]))
            f.write(im.tobytes())
        z.tofile(os.path.join(tmp, "depth_%06d.bin" % i))
    with open(os.path.join(tmp, "calib.txt"), "w") as f:
        f.write("%r %r %r %r 0.5372\n" % tuple(K))
    with open(os.path.join(tmp, "init.txt"), "w") as f:
        for T in local[:n_trajectory_lines]:
            f.write(" ".join("%.17g" % v for v in T[:3, :].reshape(-1)) + "\n")
