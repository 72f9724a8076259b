"""The cases of the structure-only mode (pba_set_cameras_constant): the windows of the device tests, cameras at the ground truth, points as
make_window leaves them (1 % depth noise).  The yardstick they are solved with is lm_yardstick.PointBlocks."""
import numpy as np

_SMALL = dict(size=(120, 160), K=(200.0, 200.0, 80.0, 60.0))
_LONG = dict(size=(120, 200), K=(250.0, 250.0, 100.0, 60.0))
TRACE_CASES = {
    # name: (make_window arguments, extras)
    "3-frames-r1-huber": (dict(n_frames=3, n_points=200, radius=1, huber=0.05, seed_offset=1, **_SMALL), ()),
    "5-frames-r2": (dict(n_frames=5, n_points=200, radius=2, seed_offset=2, **_SMALL), ()),
    "8-frames-r1-huber-causal": (dict(n_frames=8, n_points=200, radius=1, huber=0.05, visibility="causal", seed_offset=3, **_LONG), ()),
    "20-frames-r1-causal": (dict(n_frames=20, n_points=150, radius=1, visibility="causal", seed_offset=2, **_SMALL), ("one-and-all",)),
    "4-frames-r2-gaussian-huber": (dict(n_frames=4, n_points=200, radius=2, huber=0.05, gaussian=True, seed_offset=4, **_SMALL), ()),
    "4-frames-r1-3-channels": (dict(n_frames=4, n_points=150, radius=1, seed_offset=5, **_SMALL), ("channels3",)),
    # (seed 4: every candidate of the 12 iterations keeps its inverse depths positive, min 0.011.  With seeds 7..12 the first steps send
    # some of them below zero -- a point behind every camera, outside the parameterisation's domain, where the oracle returns some finite
    # cost and the device's sampler a failed evaluation -- and with seed 3 the ninth does; test_points_only_cpu.py asserts the domain)
    "4-frames-r2-inverse-depth": (dict(n_frames=4, n_points=200, radius=2, seed_offset=4, **_SMALL), ("inverse-depth",)),
    "single-observation-5-frames-r1": (None, ("single-observation",)),
}
REF_ITERATIONS = 12      # iteration limit of the yardstick in the trace tests (the device runs the compared ones)
BOUNDARY_WINDOW = dict(n_frames=4, n_points=700, radius=1, seed_offset=8, **_SMALL)      # the 700-point window of the system test
BOUNDARY_COUNTS = (1, 63, 64, 65, 255, 256, 257, 700)       # one fewer than, exactly and one more than a wave / a 256-thread workgroup


def cameras_to_ground_truth(p):
    p.cams = np.array(p.meta["cams_gt"], dtype=np.float64)
    return p


def first_points(p, k):
    """The problem of the first k points of p (their observations are the first ones of the list)."""
    from photobundle_amd.problem import WindowProblem
    keep = np.asarray(p.obs_point) < k
    return WindowProblem(K=p.K, radius=p.radius, planes=p.planes, cams=p.cams, xyz=p.xyz[:k].copy(), desc=p.desc[:k],
                         obs_point=p.obs_point[keep].astype(np.int32), obs_slot=p.obs_slot[keep].astype(np.int32), weights=p.weights,
                         huber=p.huber, fixed_slot=p.fixed_slot, images=p.images, meta=p.meta, channels=p.channels,
                         channel_images=p.channel_images)


def trace_case(name):
    """(problem, extras, rays, rho) of a trace case; rays / rho are None but for "inverse-depth" (what the engine is given too).
    "one-and-all": the first point seen by fewer than all frames keeps its first observation only, and the window must hold a point
    seen by every frame; "single-observation": the tracking problem of pose_only_cases (one residual block per point: every V has rank 2
    and only the damping makes the block solvable)."""
    from photobundle_amd import synthetic
    kw, extras = TRACE_CASES[name]
    if "single-observation" in extras:
        import pose_only_cases as pose
        p = pose.tracking_problem(pose.tracking_window(sorted(pose.TRACKING_SHAPES)[0]), "velocity")
        cameras_to_ground_truth(p)
        assert p.n_obs == p.n_points
        return p, extras, None, None
    if "channels3" in extras:
        kw = dict(kw, channel_fn=synthetic.channel_fn("IntensityAndGradient"))
    p = cameras_to_ground_truth(synthetic.make_window(**kw))
    if "one-and-all" in extras:
        count = np.bincount(p.obs_point, minlength=p.n_points)
        assert count.max() == p.n_frames, "the window must hold a point seen by every frame"
        victim = int(np.nonzero(count < p.n_frames)[0][0])
        first = int(np.searchsorted(p.obs_point, victim))
        keep = (np.asarray(p.obs_point) != victim) | (np.arange(p.n_obs) == first)
        p.obs_point, p.obs_slot = p.obs_point[keep], p.obs_slot[keep]
        count = np.bincount(p.obs_point, minlength=p.n_points)
        assert count.min() == 1 and count.max() == p.n_frames
    rays = rho = None
    if "inverse-depth" in extras:
        rays, rho = synthetic.inverse_depth_rays(p)
    return p, extras, rays, rho
