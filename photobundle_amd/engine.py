"""Python mirror of the engine's C-ABI (include/pba.h): thin, no compute.  The product path is
WindowProblem -> Engine.load() -> Engine.solve(); everything numerical happens in libpba_hip.so on the GPU."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import EngineUnavailable  # noqa: F401


class EngineError(RuntimeError):
    pass


def default_solver_options(**kw):
    o = _lib.SolverOptions()
    _lib.lib().pba_default_solver_options(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Engine:
    """One engine = one GPU = one shard of points (all cameras and frames replicated)."""

    def __init__(self, rows, cols, K, radius, max_frames, huber=0.0, device=0, keep_reduced_system=False, precision="exact",
                 channels=1):
        self._L = _lib.lib()
        cfg = _lib.Config()
        cfg.rows, cfg.cols, cfg.max_frames, cfg.radius = int(rows), int(cols), int(max_frames), int(radius)
        cfg.fx, cfg.fy, cfg.cx, cfg.cy = [float(v) for v in K]
        cfg.huber = float(huber)
        cfg.device = int(device)
        # precision: "exact" (reference-exact sampler, default) | "fp32" | "bf16" (configs[4] tolerance sweep, include/pba.h)
        cfg.flags = (1 if keep_reduced_system else 0) | ({"exact": 0, "fp32": 1, "bf16": 2}[precision] << 1)
        cfg.channels = int(channels)        # descriptor channels (include/pba.h): > 1 takes float channel images per frame
        self._h = C.c_void_p()
        rc = self._L.pba_create(C.byref(cfg), C.byref(self._h))
        if rc != 0:
            self._h = None
            raise EngineError("pba_create: %s" % self._L.pba_status_string(rc).decode())
        self.cfg = cfg
        self.n_points = self.n_obs = self.n_frames = 0
        self._cb = None

    def close(self):
        if getattr(self, "_h", None):
            self._L.pba_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc, what, **attrs):
        """Raises EngineError for a status other than PBA_OK; `attrs` become attributes of the error."""
        if rc != 0:
            err = EngineError("%s: %s (%s)" % (what, self._L.pba_status_string(rc).decode(),
                                               self._L.pba_last_error(self._h).decode()))
            for k, v in attrs.items():
                setattr(err, k, v)
            raise err

    def _check_info(self, rc, what, info, **extras):
        """_check for a call with an info struct: returns its fields; the EngineError of a failure carries `status`, `info` and extras."""
        fields = {f: getattr(info, f) for f, _ in info._fields_}
        self._check(rc, what, status=rc, info=fields, **extras)
        return fields

    # ---- data ------------------------------------------------------------------------------------------
    def set_frame(self, slot, image_u8):
        img = np.ascontiguousarray(image_u8, dtype=np.uint8)
        assert img.shape == (self.cfg.rows, self.cfg.cols)
        self._check(self._L.pba_set_frame_u8(self._h, int(slot), _ptr(img)), "pba_set_frame_u8")

    def set_frame_channels(self, slot, channels_f32):
        ch = np.ascontiguousarray(channels_f32, dtype=np.float32)
        assert ch.shape == (self.cfg.channels, self.cfg.rows, self.cfg.cols)
        self._check(self._L.pba_set_frame_channels_f32(self._h, int(slot), ch.shape[0], _ptr(ch)), "pba_set_frame_channels_f32")

    DESCRIPTORS = {"Intensity": 0, "IntensityAndGradient": 1, "BitPlanes": 2}

    def set_frame_descriptor(self, slot, image_u8, kind, sigma_ct=1.0, sigma_bp=1.5):
        """The descriptor channels of `kind` built on the device from the u8 frame (pba_set_frame_descriptor_u8)."""
        img = np.ascontiguousarray(image_u8, dtype=np.uint8)
        assert img.shape == (self.cfg.rows, self.cfg.cols)
        self._check(self._L.pba_set_frame_descriptor_u8(self._h, int(slot), _ptr(img), self.DESCRIPTORS[kind], float(sigma_ct), float(sigma_bp)),
                    "pba_set_frame_descriptor_u8")

    def get_frame_channels(self, slot):
        """[C, rows, cols] f32: the channel images of a multi-channel slot (pba_get_frame_channels_f32)."""
        out = np.empty((self.cfg.channels, self.cfg.rows, self.cfg.cols), np.float32)
        self._check(self._L.pba_get_frame_channels_f32(self._h, int(slot), _ptr(out)), "pba_get_frame_channels_f32")
        return out

    def set_frame_pyr_down(self, slot, finer, finer_slot, want_image=True):
        """cv::pyrDown of a frame of the finer level's engine into this one, device to device; returns the u8 image."""
        out = np.empty((self.cfg.rows, self.cfg.cols), np.uint8) if want_image else None
        self._check(self._L.pba_set_frame_pyr_down(self._h, int(slot), finer._h, int(finer_slot), _ptr(out) if want_image else None),
                    "pba_set_frame_pyr_down")
        return out

    # ---- device front-end (pba_frontend_*: reference photobundle.cc:505-603 on the frame in the ring) --------------------------
    def frontend_visibility(self, uv, rc, patches26, min_score, mask_radius):
        """ZNCC test of tracked points on the most recently uploaded u8 frame; returns the hit flags [n] (and stamps the mask)."""
        uv = np.ascontiguousarray(uv, dtype=np.float64).reshape(-1, 2)
        rc = np.ascontiguousarray(rc, dtype=np.int32).reshape(-1, 2)
        pt = np.ascontiguousarray(patches26, dtype=np.float32).reshape(-1, 26)
        n = len(uv)
        assert len(rc) == n and len(pt) == n
        hit = np.zeros(n, np.uint8)
        self._check(self._L.pba_frontend_visibility(self._h, n, _ptr(uv), _ptr(rc), _ptr(pt), float(min_score), int(mask_radius), _ptr(hit)),
                    "pba_frontend_visibility")
        return hit

    def frontend_zncc_probe(self, uv, patches26):
        """Test hook: [n, 27] = the new frame's zero-mean 5x5 patch at uv, its norm, the score against patches26."""
        uv = np.ascontiguousarray(uv, dtype=np.float64).reshape(-1, 2)
        pt = np.ascontiguousarray(patches26, dtype=np.float32).reshape(-1, 26)
        out = np.zeros((len(uv), 27), np.float32)
        self._check(self._L.pba_frontend_zncc_probe(self._h, len(uv), _ptr(uv), _ptr(pt), _ptr(out)), "pba_frontend_zncc_probe")
        return out

    def frontend_candidates(self, slot, depth, min_depth, max_depth, nms_radius, border):
        """Candidate scan of the frame in `slot`; returns a structured array (saliency f4, x i4, y i4) in row-major order."""
        depth = np.ascontiguousarray(depth, dtype=np.float32)
        assert depth.shape == (self.cfg.rows, self.cfg.cols)
        n = C.c_int32(0)
        self._check(self._L.pba_frontend_candidates(self._h, int(slot), _ptr(depth), float(min_depth), float(max_depth), int(nms_radius),
                                                    int(border), C.byref(n)), "pba_frontend_candidates")
        out = np.zeros(n.value, dtype=np.dtype([("saliency", np.float32), ("x", np.int32), ("y", np.int32)]))
        self._check(self._L.pba_frontend_get_candidates(self._h, _ptr(out) if n.value else None, n.value), "pba_frontend_get_candidates")
        return out

    def frontend_descriptors(self, slot, xy):
        """Integer-pixel patches at xy [n][2] = (x, y) of the frame in `slot`: [n, C, (2R+1)^2] f32."""
        xy = np.ascontiguousarray(xy, dtype=np.int32).reshape(-1, 2)
        P = (2 * self.cfg.radius + 1) ** 2
        out = np.zeros((len(xy), max(1, self.cfg.channels), P), np.float32)
        self._check(self._L.pba_frontend_descriptors(self._h, int(slot), len(xy), _ptr(xy), _ptr(out)), "pba_frontend_descriptors")
        return out

    def get_frame_channel(self, slot, channel):
        out = np.empty((3, self.cfg.rows, self.cfg.cols), np.float32)
        self._check(self._L.pba_get_frame_channel(self._h, int(slot), int(channel), _ptr(out[0]), _ptr(out[1]), _ptr(out[2])),
                    "pba_get_frame_channel")
        return out

    def sample_frame(self, slot, y, x, channel=0):
        """The engine's sampler at float positions: [n, 3] = value, Gx, Gy (pba_sample_frame)."""
        y = np.ascontiguousarray(y, np.float32).ravel()
        x = np.ascontiguousarray(x, np.float32).ravel()
        assert y.shape == x.shape
        out = np.empty((y.shape[0], 3), np.float32)
        self._check(self._L.pba_sample_frame(self._h, int(slot), int(channel), y.shape[0], _ptr(y), _ptr(x), _ptr(out)), "pba_sample_frame")
        return out

    def get_frame_planes(self, slot):
        out = np.empty((3, self.cfg.rows, self.cfg.cols), np.float32)
        self._check(self._L.pba_get_frame_planes(self._h, int(slot), _ptr(out[0]), _ptr(out[1]), _ptr(out[2])),
                    "pba_get_frame_planes")
        return out

    def set_problem(self, xyz, desc, obs_point, obs_slot, weights):
        xyz = np.ascontiguousarray(xyz, np.float64)
        desc = np.ascontiguousarray(desc, np.float64)
        op = np.ascontiguousarray(obs_point, np.int32)
        os_ = np.ascontiguousarray(obs_slot, np.int32)
        w = np.ascontiguousarray(weights, np.float64)
        self._check(self._L.pba_set_problem(self._h, xyz.shape[0], _ptr(xyz), _ptr(desc), op.shape[0], _ptr(op),
                                            _ptr(os_), _ptr(w)), "pba_set_problem")
        self.n_points, self.n_obs = xyz.shape[0], op.shape[0]

    def set_cameras(self, cams, fixed_slot=0, constant_slots=None):
        """cams [n_frames, 6].  fixed_slot: the one constant camera (-1: none).  constant_slots: an iterable of slots held constant
        (anchor frames, pba_set_cameras_anchored); it overrides fixed_slot."""
        cams = np.ascontiguousarray(cams, np.float64)
        if constant_slots is None:
            self._check(self._L.pba_set_cameras(self._h, _ptr(cams), cams.shape[0], int(fixed_slot)), "pba_set_cameras")
            n_const = 1 if fixed_slot >= 0 else 0
        else:
            slots = sorted({int(s) for s in constant_slots})
            if any(s < 0 or s >= 32 for s in slots):
                raise ValueError("constant_slots: slots are 0..31, got %r" % (slots,))
            mask = 0
            for s in slots:
                mask |= 1 << s
            self._check(self._L.pba_set_cameras_anchored(self._h, _ptr(cams), cams.shape[0], mask), "pba_set_cameras_anchored")
            n_const = len(slots)
        self.n_frames = cams.shape[0]
        self.n_free = self.n_frames - n_const

    def load(self, prob):
        """Uploads a WindowProblem (frames from prob.images)."""
        if self.cfg.channels > 1:
            assert prob.channel_images is not None and prob.channels == self.cfg.channels
            for s in range(prob.n_frames):
                self.set_frame_channels(s, prob.channel_images[s])
        else:
            assert prob.images is not None, "the engine consumes u8 frames (addFrame's input), not float planes"
            for s in range(prob.n_frames):
                self.set_frame(s, prob.images[s])
        self.set_problem(prob.xyz, prob.desc, prob.obs_point, prob.obs_slot, prob.weights)
        self.set_cameras(prob.cams, prob.fixed_slot)
        return self

    def set_inverse_depth(self, rays, rho):
        """Inverse-depth variant (include/pba.h): rays [n_points, 6] = world origin + direction, rho [n_points] > 0."""
        rays = np.ascontiguousarray(rays, np.float64)
        rho = np.ascontiguousarray(rho, np.float64)
        assert rays.shape == (self.n_points, 6) and rho.shape == (self.n_points,)
        self._check(self._L.pba_set_inverse_depth(self._h, _ptr(rays), _ptr(rho)), "pba_set_inverse_depth")

    def set_points_constant(self, on=True):
        """Pose-only mode (include/pba.h): every point is held constant, the free cameras are aligned to them.  Call after
        set_problem / load; set_problem switches it off again."""
        self._check(self._L.pba_set_points_constant(self._h, 1 if on else 0), "pba_set_points_constant")

    def set_cameras_constant(self, on=True):
        """Structure-only mode (include/pba.h): every camera is held constant, the points are refined against them.  Call after
        set_problem / load; set_problem switches it off again."""
        self._check(self._L.pba_set_cameras_constant(self._h, 1 if on else 0), "pba_set_cameras_constant")

    def get_points_world(self):
        xyz = np.zeros((self.n_points, 3))
        self._check(self._L.pba_get_points_world(self._h, _ptr(xyz)), "pba_get_points_world")
        return xyz

    def get_state(self):
        cams = np.zeros((self.n_frames, 6))
        xyz = np.zeros((self.n_points, 3))
        self._check(self._L.pba_get_state(self._h, _ptr(cams), _ptr(xyz)), "pba_get_state")
        return cams, xyz

    # ---- primitive passes --------------------------------------------------------------------------------
    def linearize(self, want_cost=True):
        c = C.c_double(0.0)
        self._check(self._L.pba_linearize(self._h, C.byref(c) if want_cost else None), "pba_linearize")
        return c.value

    def step(self, radius, init_scale=False, options=None):
        o = options or default_solver_options()
        info = _lib.StepInfo()
        self._check(self._L.pba_step(self._h, float(radius), int(bool(init_scale)), C.byref(o), C.byref(info)), "pba_step")
        return {f: getattr(info, f) for f, _ in _lib.StepInfo._fields_}

    def accept(self):
        self._check(self._L.pba_accept(self._h), "pba_accept")

    def reduced_system(self):
        n = C.c_int32(0)
        nn = 6 * self.n_free
        S = np.zeros((nn, nn))
        rhs = np.zeros(nn)
        self._check(self._L.pba_get_reduced_system(self._h, _ptr(S), _ptr(rhs), C.byref(n)), "pba_get_reduced_system")
        assert n.value == nn
        return S, rhs

    def point_system(self):
        """Scaled and damped point blocks V [n, 3, 3] and scaled gradient rhs [n, 3] of the last step in the cameras-constant mode."""
        V = np.zeros((self.n_points, 3, 3))
        rhs = np.zeros((self.n_points, 3))
        self._check(self._L.pba_get_point_system(self._h, _ptr(V), _ptr(rhs)), "pba_get_point_system")
        return V, rhs

    def obs_records(self):
        rec = np.zeros((self.n_obs, 6))
        self._check(self._L.pba_get_obs_records(self._h, _ptr(rec)), "pba_get_obs_records")
        return rec

    # ---- the LM loop ---------------------------------------------------------------------------------------
    def solve(self, options=None, max_iterations_out=512, fetch_state=True):
        res = self.unpack_solve(*self.solve_raw(options, max_iterations_out))
        if fetch_state:
            res["cams"], res["xyz"] = self.get_state()
        return res

    def solve_raw(self, options=None, max_iterations_out=512, buffers=None):
        """pba_solve and nothing else: returns the C structs (summary, iteration array) as filled by the library.
        `buffers` = a (summary, iteration array) pair from an earlier call to reuse (timing loops)."""
        o = options or default_solver_options()
        s, its = buffers if buffers is not None else self.solve_buffers(max_iterations_out)
        self._check(self._L.pba_solve(self._h, C.byref(o), C.byref(s), its, len(its)), "pba_solve")
        return s, its

    @staticmethod
    def solve_buffers(max_iterations_out=512):
        return _lib.SolverSummary(), (_lib.IterationSummary * max_iterations_out)()

    @staticmethod
    def unpack_solve(s, its):
        res = {f: getattr(s, f) for f, _ in _lib.SolverSummary._fields_}
        res["message"] = s.message.decode()
        res["iterations"] = [{f: getattr(its[i], f) for f, _ in _lib.IterationSummary._fields_}
                             for i in range(s.num_iterations)]
        return res

    # ---- covariance output -----------------------------------------------------------------------------------
    def covariance(self, cameras=True, points=True):
        """pba_covariance: blocks of (J^T J)^-1 of the reduced program at the current state (include/pba.h).  Returns a dict with
        cam_cov [n, n] (None when not asked for), point_cov [n_points, 3, 3] (None likewise) and the fields of pba_covariance_info.
        Raises EngineError with the status and message otherwise; its `status` and `info` attributes carry the status code and
        the info fields (after PBA_ERR_NUMERIC: the first offender and the pivots)."""
        info = _lib.CovarianceInfo()
        n_max = 6 * 32
        cam = np.zeros(n_max * n_max) if cameras else None
        pts = np.zeros((self.n_points, 3, 3)) if points else None
        rc = self._L.pba_covariance(self._h, _ptr(cam) if cameras else None, _ptr(pts) if points else None, C.byref(info))
        fields = self._check_info(rc, "pba_covariance", info)
        n = info.n_cam
        out = dict(fields)
        out["cam_cov"] = cam[:n * n].reshape(n, n).copy() if cameras else None
        out["point_cov"] = pts
        return out

    # ---- camera prior and marginalisation ----------------------------------------------------------------------
    def set_camera_prior(self, slots, x0, Lambda, eta, c):
        """pba_set_camera_prior: one extra residual block E(d) = c + eta^T d + d^T Lambda d / 2 on the camera blocks `slots`
        (ascending), d = the cameras of `slots` minus x0 [k, 6]; Lambda [6k, 6k], eta [6k] (include/pba.h)."""
        sl = np.ascontiguousarray(slots, np.int32).ravel()
        k = sl.shape[0]
        x0 = np.ascontiguousarray(x0, np.float64).reshape(k, 6)
        Lm = np.ascontiguousarray(Lambda, np.float64).reshape(6 * k, 6 * k)
        et = np.ascontiguousarray(eta, np.float64).reshape(6 * k)
        self._check(self._L.pba_set_camera_prior(self._h, k, _ptr(sl), _ptr(x0), _ptr(Lm), _ptr(et), float(c)), "pba_set_camera_prior")

    def clear_camera_prior(self):
        self._check(self._L.pba_set_camera_prior(self._h, 0, None, None, None, None, 0.0), "pba_set_camera_prior")

    def set_point_prior(self, x0, Lambda6=None):
        """pba_set_point_prior: one extra residual block E_i = d^T Lambda_i d / 2, d = X_i - x0_i, on every point; x0 [n_points, 3],
        Lambda6 [n_points, 6] = the upper triangle of Lambda_i row by row (00 01 02 11 12 22), zeros for a point without a prior
        (include/pba.h).  set_point_prior(None) clears."""
        if x0 is None and Lambda6 is None:
            self._check(self._L.pba_set_point_prior(self._h, self.n_points, None, None), "pba_set_point_prior")
            return
        x0 = None if x0 is None else np.ascontiguousarray(x0, np.float64).reshape(-1, 3)
        L6 = None if Lambda6 is None else np.ascontiguousarray(Lambda6, np.float64).reshape(-1, 6)
        n = (x0 if x0 is not None else L6).shape[0]
        if x0 is not None and L6 is not None and L6.shape[0] != n:
            raise ValueError("set_point_prior: x0 has %d rows, Lambda6 %d" % (n, L6.shape[0]))
        self._check(self._L.pba_set_point_prior(self._h, n, _ptr(x0) if x0 is not None else None, _ptr(L6) if L6 is not None else None),
                    "pba_set_point_prior")

    def marginalize(self, drop_slots):
        """pba_marginalize: the prior that the cameras of `drop_slots` and every point they see leave on the kept free cameras, at the
        current state (include/pba.h).  Returns a dict with slots [k], x0 [k, 6], Lambda [6k, 6k], eta [6k], c and the fields of
        pba_marginal_info -- the first five are what set_camera_prior takes.  Raises EngineError otherwise; its `status` and `info`
        attributes carry the status code and the info fields (after PBA_ERR_NUMERIC: the first offender and the pivots)."""
        mask = 0
        for s in drop_slots:
            if int(s) < 0 or int(s) >= 32:
                raise ValueError("drop_slots: slots are 0..31, got %r" % (drop_slots,))
            mask |= 1 << int(s)
        info = _lib.MarginalInfo()
        n_max = 6 * 32
        slots = np.zeros(32, np.int32)
        x0 = np.zeros((32, 6))
        Lm = np.zeros(n_max * n_max)
        eta = np.zeros(n_max)
        c = C.c_double(0.0)
        rc = self._L.pba_marginalize(self._h, mask, _ptr(slots), _ptr(x0), _ptr(Lm), _ptr(eta), C.byref(c), C.byref(info))
        fields = self._check_info(rc, "pba_marginalize", info)
        k = info.k
        out = dict(fields)
        out.update(slots=slots[:k].copy(), x0=x0[:k].copy(), Lambda=Lm[:36 * k * k].reshape(6 * k, 6 * k).copy(), eta=eta[:6 * k].copy(), c=c.value)
        return out

    # ---- outlier culling ---------------------------------------------------------------------------------------
    def block_costs(self):
        """pba_get_block_costs: the loss-corrected cost of every residual block at the current state, [n_obs]."""
        c = np.zeros(self.n_obs)
        self._check(self._L.pba_get_block_costs(self._h, _ptr(c)), "pba_get_block_costs")
        return c

    def cull(self, min_cost=0.0, factor=0.0, quantile=0.5, min_observations=2, apply=True):
        """pba_cull: the verdict over the block costs and, with apply, the engine's problem replaced by the survivors (include/pba.h).
        Returns (block_keep [n_obs before] uint8, point_map [n_points before] int32 with -1 for a point that leaves, info dict);
        n_points / n_obs follow an applied cull.  Raises EngineError otherwise; its `status` and `info` attributes carry the status
        code and the info fields, `block_keep` and `point_map` the tables (filled by the "no point would be left" refusal)."""
        o = _lib.CullOptions(float(min_cost), float(factor), float(quantile), int(min_observations), 1 if apply else 0)
        info = _lib.CullInfo()
        keep = np.zeros(self.n_obs, np.uint8)
        pmap = np.zeros(self.n_points, np.int32)
        rc = self._L.pba_cull(self._h, C.byref(o), _ptr(keep), _ptr(pmap), C.byref(info))
        fields = self._check_info(rc, "pba_cull", info, block_keep=keep, point_map=pmap)
        if info.applied:
            self.n_points, self.n_obs = info.n_points_after, info.n_blocks_after
        return keep, pmap, fields

    # ---- re-observation ----------------------------------------------------------------------------------------
    def admit(self, slot_mask=None, min_depth=0.1, border=None, min_cost=0.0, factor=1.0, quantile=0.5, apply=True, capacity=None):
        """pba_admit: the (point, slot) pairs missing from the observation list whose projection at the current state lies inside the
        image, the verdict over their block costs and, with apply, the engine's lists merged with the ones taken (include/pba.h).
        slot_mask None: every slot below n_frames; border None: the patch radius; capacity None: room for every candidate.
        Returns (cand_point int32, cand_slot int32, cand_cost float64, cand_take uint8, info dict), the arrays n_written long; n_obs
        follows an applied admission.  Raises EngineError otherwise; its `status` and `info` attributes carry the status code and the
        info fields."""
        if slot_mask is None:
            slot_mask = (1 << self.n_frames) - 1
        slot_mask = int(slot_mask) & 0xFFFFFFFF
        if border is None:
            border = self.cfg.radius
        o = _lib.AdmitOptions(slot_mask, float(min_depth), int(border), float(min_cost), float(factor), float(quantile), 1 if apply else 0)
        info = _lib.AdmitInfo()
        # (no call reports more candidates than there are (point, slot) pairs; a capacity <= 0 goes with null pointers)
        cap = self.n_points * bin(slot_mask).count("1") if capacity is None else int(capacity)
        room = max(cap, 0)
        out = np.zeros(room, np.int32), np.zeros(room, np.int32), np.zeros(room), np.zeros(room, np.uint8)
        rc = self._L.pba_admit(self._h, C.byref(o), cap, *[_ptr(a) if room else None for a in out], C.byref(info))
        fields = self._check_info(rc, "pba_admit", info)
        if info.applied:
            self.n_obs = info.n_blocks_after
        return tuple(a[:info.n_written].copy() for a in out) + (fields,)

    def select_u64order(self, v, k):
        """Test hook (pba_internal_select_u64order): the k-th smallest of v by 64-bit pattern, through the select kernels of pba_cull."""
        v = np.ascontiguousarray(v, np.float64).ravel()
        out = C.c_double(0.0)
        self._check(self._L.pba_internal_select_u64order(self._h, _ptr(v), v.shape[0], int(k), C.byref(out)), "pba_internal_select_u64order")
        return out.value

    # ---- multi-GPU -------------------------------------------------------------------------------------------
    @staticmethod
    def comm_unique_id():
        buf = (C.c_char * 128)()
        rc = _lib.lib().pba_comm_unique_id(buf)
        if rc != 0:
            raise EngineError("pba_comm_unique_id failed (librccl not loadable?)")
        return bytes(buf)

    def comm_init_rccl(self, unique_id, rank, world):
        buf = (C.c_char * 128).from_buffer_copy(unique_id)
        self._check(self._L.pba_comm_init_rccl(self._h, buf, int(rank), int(world)), "pba_comm_init_rccl")

    def comm_enable_peer_exchange(self):
        """Collective.  Returns the transport name afterwards ("rccl+peer" / "callback+peer" when the device-side exchange is on)."""
        self._check(self._L.pba_comm_enable_peer_exchange(self._h), "pba_comm_enable_peer_exchange")
        return self.comm_transport()

    def solve_driver(self):
        """Which driver ran the last solve: "resident" (one cooperative launch), "pipelined", "host-stepped" or "none"."""
        return self._L.pba_solve_driver(self._h).decode()

    def comm_rank_count(self):
        return int(self._L.pba_comm_rank_count(self._h))

    def comm_transport(self):
        self._L.pba_comm_transport.restype = C.c_char_p
        return self._L.pba_comm_transport(self._h).decode()

    def comm_init_callback(self, fn, rank, world):
        """fn(numpy float64 view, op) must all-reduce in place (op 0 = sum, 1 = max)."""
        def tramp(ptr, n, op, ctx):
            try:
                a = np.ctypeslib.as_array(ptr, shape=(n,))
                fn(a, int(op))
                return 0
            except Exception:
                import traceback
                traceback.print_exc()
                return 1
        self._cb = _lib.ALLREDUCE_FN(tramp)
        self._check(self._L.pba_comm_init_callback(self._h, self._cb, None, int(rank), int(world)), "pba_comm_init_callback")

    # ---- counters ----------------------------------------------------------------------------------------------
    def reset_counters(self):
        self._check(self._L.pba_reset_counters(self._h), "pba_reset_counters")

    def set_profiling(self, mode):
        """0 off, 1 HIP events around every kernel (host-stepped driver), 2 device time stamps in the asynchronous pipeline."""
        self._check(self._L.pba_set_profiling(self._h, int(mode)), "pba_set_profiling")

    def counters(self):
        c = _lib.Counters()
        self._check(self._L.pba_get_counters(self._h, C.byref(c)), "pba_get_counters")
        return {f: getattr(c, f) for f, _ in _lib.Counters._fields_}


def solve_batch(engines, options=None, max_iterations_out=512, fetch_state=True):
    """pba_solve_batch: solves independent windows together, one batched launch per phase of every LM iteration; returns one dict per
    engine in the shape of Engine.solve, each equal to that engine's own solve.  `options`: None, one options object for all, or a list."""
    engines = list(engines)
    n = len(engines)
    if n < 1 or n > _lib.MAX_BATCH:
        raise EngineError("solve_batch: %d engines (1 to %d)" % (n, _lib.MAX_BATCH))
    if options is None:
        opts = [default_solver_options() for _ in range(n)]
    elif isinstance(options, _lib.SolverOptions):
        opts = [options] * n
    else:
        opts = list(options)
        if len(opts) != n:
            raise EngineError("solve_batch: %d option sets for %d engines" % (len(opts), n))
    L = _lib.lib()
    handles = (C.c_void_p * n)(*[e._h for e in engines])
    o_arr = (_lib.SolverOptions * n)(*opts)
    sums = (_lib.SolverSummary * n)()
    m = int(max_iterations_out)
    its = (_lib.IterationSummary * (n * m))()
    rc = L.pba_solve_batch(handles, n, o_arr, sums, its, m)
    if rc != 0:
        raise EngineError("pba_solve_batch: %s (%s)" % (L.pba_status_string(rc).decode(),
                                                         L.pba_last_error(engines[0]._h).decode() if engines[0]._h else ""))
    out = []
    for w, e in enumerate(engines):
        s = sums[w]
        res = {f: getattr(s, f) for f, _ in _lib.SolverSummary._fields_}
        res["message"] = s.message.decode()
        res["iterations"] = [{f: getattr(its[w * m + i], f) for f, _ in _lib.IterationSummary._fields_} for i in range(s.num_iterations)]
        if fetch_state:
            res["cams"], res["xyz"] = e.get_state()
        out.append(res)
    return out
