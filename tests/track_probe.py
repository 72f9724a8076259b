"""Builds and loads tests/track_host_probe.cpp (trackFrame of the host classes through ctypes) into a directory the caller owns, and the
synthetic sequence the tracking tests feed it.  Test helper, not collected."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "photobundle_amd")


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def build(out_dir):
    so = os.path.join(str(out_dir), "libtrack_host_probe.so")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-fopenmp", "-shared", "-o", so,
                           os.path.join(ROOT, "tests", "track_host_probe.cpp"), "-L" + PKG, "-lphotobundle", "-lpba_hip",
                           "-Wl,-rpath," + PKG])
    return so


class TrackProbe:
    def __init__(self, out_dir):
        self.L = C.CDLL(build(out_dir))

    def _call(self, fn, *args):
        err = C.create_string_buffer(1024)
        if fn(*args, err, 1024):
            raise RuntimeError(err.value.decode())

    def create(self, levels, size, K, window, radius, min_score=0.75):
        K4 = np.array(K, np.float64)
        self._call(self.L.probe_track_create, int(levels), int(size[0]), int(size[1]), _ptr(K4), int(window), int(radius), C.c_double(min_score))

    def add(self, image, depth, T, max_poses=64):
        image = np.ascontiguousarray(image, np.uint8)
        depth = np.ascontiguousarray(depth, np.float32)
        T = np.ascontiguousarray(T, np.float64)
        poses = np.zeros((max_poses, 4, 4))
        n = C.c_int(0)
        self._call(self.L.probe_track_add, _ptr(image), _ptr(depth), _ptr(T), _ptr(poses), max_poses, C.byref(n))
        return poses[:n.value].copy()

    def track(self, image, T, max_iterations=50, min_points=64):
        image = np.ascontiguousarray(image, np.uint8)
        T = np.ascontiguousarray(T, np.float64)
        out, ints, costs = np.zeros((4, 4)), np.zeros(3, np.int32), np.zeros(2)
        msg = C.create_string_buffer(512)
        self._call(self.L.probe_track_track, _ptr(image), _ptr(T), int(max_iterations), int(min_points), _ptr(out), _ptr(ints), _ptr(costs), msg, 512)
        return out, dict(tracked=bool(ints[0]), num_points=int(ints[1]), num_iterations=int(ints[2]), initial_cost=float(costs[0]),
                         final_cost=float(costs[1]), message=msg.value.decode())

    def release(self):
        self.L.probe_track_release()


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
