"""The rule of pba_cull (include/pba.h) restated in numpy, and the occluder window the usefulness tests share.

reference_cull(c, obs_point, ...) is the yardstick of tests/test_cull_cpu.py (hand-written cases) and tests/test_gpu_cull.py (the engine's
verdict, bit for bit).  It is written from the sentences of the contract, one line each, and shares no code with the engine."""
import math

import numpy as np

DEFAULTS = dict(min_cost=0.0, factor=3.0, quantile=0.5, min_observations=2)      # the class defaults (Options::outlier*)


class CullNumericError(ValueError):
    """factor * quantile_cost is not finite (PBA_ERR_NUMERIC)."""


def u64_order_statistic(c, k):
    """The k-th smallest of c (0-based), ordered by IEEE bit pattern read as an unsigned 64-bit integer."""
    bits = np.ascontiguousarray(c, np.float64).view(np.uint64)
    return np.partition(bits, k)[k:k + 1].view(np.float64)[0]


def reference_cull(c, obs_point, min_cost=0.0, factor=0.0, quantile=0.5, min_observations=2):
    """c [n]: block costs in list order; obs_point [n]: the point of every block (grouped, ascending).  Returns
    (block_keep uint8 [n], point_map int32 [n_points], info dict with the fields of pba_cull_info but `applied`)."""
    c = np.ascontiguousarray(c, np.float64)
    obs_point = np.asarray(obs_point, np.int64)
    n = c.shape[0]
    n_points = int(obs_point.max()) + 1
    assert n >= 1 and obs_point.shape == (n,)
    assert min_cost >= 0 and math.isfinite(min_cost) and factor >= 0 and math.isfinite(factor) and 0.0 <= quantile <= 1.0 and min_observations >= 1
    k = int(math.floor(quantile * float(n - 1)))
    quantile_cost = u64_order_statistic(c, k)
    if factor > 0:
        with np.errstate(all="ignore"):
            fq = np.float64(factor) * quantile_cost
        if not np.isfinite(fq):
            raise CullNumericError("factor * quantile_cost = %r" % fq)
        threshold = np.fmax(np.float64(min_cost), fq)
    else:
        threshold = np.float64(min_cost)
    with np.errstate(invalid="ignore"):
        over = ~(c <= threshold)
    not_over = np.bincount(obs_point[~over], minlength=n_points)
    survives = not_over >= min_observations
    keep = ~over & survives[obs_point]
    point_map = np.where(survives, np.cumsum(survives) - 1, -1).astype(np.int32)
    info = dict(n_blocks_before=n, n_blocks_after=int(keep.sum()), n_points_before=n_points, n_points_after=int(survives.sum()),
                n_blocks_over_threshold=int(over.sum()), n_blocks_by_point_rule=int((~over & ~survives[obs_point]).sum()),
                quantile_cost=float(quantile_cost), threshold=float(threshold))
    return keep.astype(np.uint8), point_map, info


def surviving_lists(p_obs_point, p_obs_slot, keep, point_map):
    """The observation lists of the surviving problem."""
    k = np.asarray(keep, bool)
    return point_map[np.asarray(p_obs_point)[k]].astype(np.int32), np.asarray(p_obs_slot)[k].astype(np.int32)


# ---- the occluder window -----------------------------------------------------------------------------------------------------------
OCCLUDER = dict(n_frames=5, n_points=600, radius=1, size=(120, 160), K=(200.0, 200.0, 80.0, 60.0), visibility="causal", huber=0.05)
OCCLUDER_FRAME = 3
# rows r0:r1, columns c0:c1 of frame OCCLUDER_FRAME.  Chosen on the CPU yardstick: with the Huber loss at the class's robustThreshold the
# solve shrugs off rectangles of a quarter of the image (pose error within 1.3 x the clean window's); this one, 44 % of the frame,
# costs it a factor 5.8.  Smooth texture (the scene's own kind, other seed) pulls the poses harder than white noise of the same area
OCCLUDER_RECT = (40, 110, 10, 150)
OCCLUDER_TEXTURE = dict(seed=777, metres_per_pixel=0.15)


def occluder_patch(shape_rc, origin_rc=(0, 0)):
    """u8 texture unrelated to the scene: the generator's sum of sinusoids with another seed, laid out in image coordinates."""
    from photobundle_amd import synthetic
    tex = synthetic.Texture(seed=OCCLUDER_TEXTURE["seed"])
    ys, xs = np.mgrid[origin_rc[0]:origin_rc[0] + shape_rc[0], origin_rc[1]:origin_rc[1] + shape_rc[1]]
    s = OCCLUDER_TEXTURE["metres_per_pixel"]
    return np.clip(np.rint(tex(xs * s, ys * s)), 0, 255).astype(np.uint8)


def pose_error(cams, cams_gt):
    """One number for `closer to the ground truth`: the norm of gpu_util.pose_rmse_gauge_fixed's rotation RMSE [rad] and camera-centre
    RMSE [m] (both fall and rise together on these windows; the centre term dominates)."""
    import gpu_util
    rot, centre, _ = gpu_util.pose_rmse_gauge_fixed(cams, cams_gt)
    return float(np.hypot(rot, centre))


def occluded_window(make_window, replace):
    """(clean window, contaminated window, inside): a rectangle of one frame overwritten with unrelated texture (occluder_patch);
    inside [n_obs]: blocks of that frame whose ground-truth projection lies inside the rectangle by more than the patch radius.
    make_window: photobundle_amd.synthetic.make_window; replace: dataclasses.replace."""
    from photobundle_amd import imgproc, se3, synthetic
    clean = make_window(**OCCLUDER)
    r0, r1, c0, c1 = OCCLUDER_RECT
    images = clean.images.copy()
    images[OCCLUDER_FRAME, r0:r1, c0:c1] = occluder_patch((r1 - r0, c1 - c0), (r0, c0))
    planes = clean.planes.copy()
    planes[OCCLUDER_FRAME] = imgproc.planes_from_u8(images[OCCLUDER_FRAME])
    dirty = replace(clean, images=images, planes=planes)
    # ground-truth positions of the points: the solve of the clean window is not needed, the generator's depths are
    T_cw = se3.params_to_pose(clean.meta["cams_gt"][OCCLUDER_FRAME])
    gt_xyz = ground_truth_points(clean)
    uv, _ = synthetic.project(clean.K, T_cw, gt_xyz[clean.obs_point])
    m = clean.radius
    inside = (clean.obs_slot == OCCLUDER_FRAME) & (uv[:, 0] > c0 + m) & (uv[:, 0] < c1 - 1 - m) & (uv[:, 1] > r0 + m) & (uv[:, 1] < r1 - 1 - m)
    return clean, dirty, inside


def yardstick_block_costs(p, cams, xyz):
    """c_o of every block on the CPU yardstick: rho(|r|^2) / 2 with Ceres' HuberLoss(p.huber) (the identity for huber <= 0)."""
    from oracle import oracle
    _, sq = oracle.cost(p, cams=cams, xyz=xyz)
    a = p.huber
    return 0.5 * (np.where(sq <= a * a, sq, 2.0 * a * np.sqrt(sq) - a * a) if a > 0 else sq)


def surviving_window(p, replace, cams, xyz, keep, point_map):
    """The WindowProblem of the survivors at the state (cams, xyz)."""
    obs_point, obs_slot = surviving_lists(p.obs_point, p.obs_slot, keep, point_map)
    s = point_map >= 0
    return replace(p, cams=cams, xyz=xyz[s], desc=p.desc[s], obs_point=obs_point, obs_slot=obs_slot)


def ground_truth_points(p):
    """World position of every point on the generator's surfaces: the pixel of its first observation back-projected with the ground-truth
    depth map and pose of that frame (the descriptor was cut there)."""
    from photobundle_amd import se3, synthetic
    first = np.searchsorted(p.obs_point, np.arange(p.n_points))
    slot = p.obs_slot[first]
    fx, fy, cx, cy = p.K
    out = np.zeros((p.n_points, 3))
    for s in np.unique(slot):
        m = slot == s
        T_cw_init = se3.params_to_pose(p.cams[s])
        uv, _ = synthetic.project(p.K, T_cw_init, p.xyz[m])
        x, y = np.rint(uv[:, 0]).astype(int), np.rint(uv[:, 1]).astype(int)
        z = p.meta["depths"][s][y, x].astype(np.float64)
        Xc = np.stack([(x - cx) / fx * z, (y - cy) / fy * z, z], 1)
        T_wc = np.asarray(p.meta["T_gt"][s])
        out[m] = Xc @ T_wc[:3, :3].T + T_wc[:3, 3]
    return out
