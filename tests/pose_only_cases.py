"""The cases of the pose-only mode (pba_set_points_constant): the tracking problem and its bar, and the windows of the device trace tests.
The yardstick they are solved with is lm_yardstick.CameraBlocks."""
import numpy as np


def pose_error(cam, cam_gt):
    """(rotation angle [rad], translation distance |t - t_gt|) between two world->camera parameter vectors [w, t], the form
    meta['cams_gt'] holds."""
    from scipy.spatial.transform import Rotation
    Ra, Rb = Rotation.from_rotvec(cam[:3]), Rotation.from_rotvec(cam_gt[:3])
    return float(np.linalg.norm((Ra * Rb.inv()).as_rotvec())), float(np.linalg.norm(cam[3:] - cam_gt[3:]))


# ---- the tracking case: ONE camera against a map whose points stay put ------------------------------------------------------------
TRACKING_SHAPES = {      # the three shapes of the tracking bar: size, K, radius, depth noise
    "120x160-r1-exact": dict(size=(120, 160), K=(200.0, 200.0, 80.0, 60.0), radius=1, depth_noise=0.0),
    # (scene seed 1: with seed 0 the 1 % depth noise alone puts the minimum of this shape 21-23 mm from the ground truth -- measured on
    # the yardstick, independent of the start and of the tolerances --, i.e. beyond the bar before any solver runs)
    "120x160-r2-noise": dict(size=(120, 160), K=(200.0, 200.0, 80.0, 60.0), radius=2, depth_noise=0.01, seed_offset=1),
    "188x620-r1-noise": dict(size=(188, 620), K=(359.428, 359.428, 303.5964, 92.60785), radius=1, depth_noise=0.01),
}
TRACK_BAR_M, TRACK_BAR_RAD = 0.02, 1.75e-3      # one sigma of make_window's `trans` / `rot_deg` defaults (0.02 m, 0.1 degree)


def tracking_window(shape, n_frames=5, n_points=400, huber=0.05):
    from photobundle_amd import synthetic
    return synthetic.make_window(n_frames=n_frames, n_points=n_points, huber=huber, **TRACKING_SHAPES[shape])


def tracking_problem(p, start, slot=None):
    """The window `p` reduced to the tracking problem of its frame `slot` (default: the last): only that frame's residual blocks, every
    other camera at its ground truth (none of them has a residual block, so none is in the program), the tracked camera at `start`:
    "velocity" = the constant-velocity prediction from the two frames before it, "zero" = zero motion (the previous frame's pose)."""
    from photobundle_amd import se3
    from photobundle_amd.problem import WindowProblem
    slot = p.n_frames - 1 if slot is None else slot
    T = p.meta["T_gt"]
    if start == "velocity":
        T0 = T[slot - 1] @ (np.linalg.inv(T[slot - 2]) @ T[slot - 1])
    elif start == "zero":
        T0 = T[slot - 1]
    else:
        raise KeyError(start)
    keep = np.asarray(p.obs_slot) == slot
    pts = np.unique(p.obs_point[keep])
    remap = -np.ones(p.n_points, np.int64)
    remap[pts] = np.arange(len(pts))
    cams = np.array(p.meta["cams_gt"], dtype=np.float64)
    cams[slot] = se3.pose_to_params(np.linalg.inv(T0))
    return WindowProblem(K=p.K, radius=p.radius, planes=p.planes, cams=cams, xyz=p.xyz[pts].copy(), desc=p.desc[pts],
                         obs_point=remap[p.obs_point[keep]].astype(np.int32), obs_slot=p.obs_slot[keep].astype(np.int32),
                         weights=p.weights, huber=p.huber, fixed_slot=0, images=p.images, meta=dict(p.meta, tracked_slot=slot),
                         channels=p.channels, channel_images=p.channel_images)


# ---- the windows of the device trace tests --------------------------------------------------------------------------------------------
_SMALL = dict(size=(120, 160), K=(200.0, 200.0, 80.0, 60.0))
_LONG = dict(size=(120, 200), K=(250.0, 250.0, 100.0, 60.0))
TRACE_CASES = {
    # name: (make_window arguments, fixed_slot, extras)
    "3-frames-r1-huber": (dict(n_frames=3, n_points=200, radius=1, huber=0.05, seed_offset=1, **_SMALL), 0, ()),
    "5-frames-r2-no-fixed": (dict(n_frames=5, n_points=200, radius=2, seed_offset=2, **_SMALL), -1, ()),
    "8-frames-r1-huber-middle-fixed-causal": (dict(n_frames=8, n_points=200, radius=1, huber=0.05, visibility="causal", seed_offset=3, **_LONG), 3, ()),
    "20-frames-r1-causal": (dict(n_frames=20, n_points=150, radius=1, visibility="causal", seed_offset=2, **_SMALL), 0, ()),
    "4-frames-r2-gaussian-huber": (dict(n_frames=4, n_points=200, radius=2, huber=0.05, gaussian=True, seed_offset=4, **_SMALL), 0, ()),
    "4-frames-r1-3-channels": (dict(n_frames=4, n_points=150, radius=1, seed_offset=5, **_SMALL), 0, ("channels3",)),
    "4-frames-r1-camera-without-blocks": (dict(n_frames=4, n_points=200, radius=1, huber=0.05, seed_offset=6, **_SMALL), 0, ("drop-slot-2",)),
    "4-frames-r2-inverse-depth": (dict(n_frames=4, n_points=200, radius=2, seed_offset=7, **_SMALL), 0, ("inverse-depth",)),
    "tracking-5-frames-r1": (None, 0, ("tracking",)),
}


def trace_case(name):
    """(problem, extras) of a trace case.  "drop-slot-2": slot 2 keeps no residual block (a free camera outside the program);
    "inverse-depth": the engine is given rays + inverse depths (the points the yardstick uses are then the engine's own world points);
    "tracking": the tracking problem of the first tracking shape from the constant-velocity prediction."""
    from photobundle_amd import synthetic
    kw, fixed, extras = TRACE_CASES[name]
    if "tracking" in extras:
        return tracking_problem(tracking_window(sorted(TRACKING_SHAPES)[0]), "velocity"), extras
    if "channels3" in extras:
        kw = dict(kw, channel_fn=synthetic.channel_fn("IntensityAndGradient"))
    p = synthetic.make_window(**kw)
    p.fixed_slot = fixed
    if "drop-slot-2" in extras:
        keep = np.asarray(p.obs_slot) != 2
        p.obs_point, p.obs_slot = p.obs_point[keep], p.obs_slot[keep]
        assert len(np.unique(p.obs_point)) == p.n_points
    return p, extras
