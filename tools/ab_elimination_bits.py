"""Recorder of elimination bits: the exact results of pba_covariance and pba_marginalize on a fixed list of small windows with the library
named by PBA_LIB (default: the built one).  The sibling of tools/ab_bits.py for the two calls that eliminate the points from the stored
records of a Jacobian pass (csrc/pba_elim.h); both work off the LM loop, so no solve fixture sees them.

    python tools/ab_elimination_bits.py                         prints one line per case
    python tools/ab_elimination_bits.py --out tests/golden/elimination_bits.json --commit <hash of the commit the library was built from>

Per case: the status code, every field of the info struct (doubles as hex floats) and the SHA-1 of each output array -- cam_cov and
point_cov (null: not asked for), or slots, x0, Lambda, eta and c as a hex float.  Every call goes through the C entry point with poisoned
caller buffers; after PBA_ERR_NUMERIC the outputs are null and `poisoned` holds the SHA-1 of those buffers and `kept` whether they kept
their bytes.

The cases (96 x 128 windows of tests/covariance_cases.py and tests/marginal_cases.py, seconds each):
  cov/full/*       dense windows with 3, 64, 65 and 257 points (one free column: lane, wave and workgroup tails), the causal Huber
                   window at the start and after a 6-iteration solve (several pairs, loss-corrected records), the 32-slot window
  cov/pose         points constant, constant slots (0, 3) of the causal window: no elimination, diagonal pairs only
  cov/structure/*  cameras constant, 65 world points and 65 inverse depths
  cov/fail/*       the structure-only window whose point 37 keeps one observation, and the causal window with one anchor (open gauge)
  marg/<name>      every case of marginal_cases.CASES
  marg/chain       the second call of marginal_cases.CHAIN: a prior is set, so k_prior adds into the dense system
  marg/fail/point  the window whose point 37 has a zero block
One child process, the default driver: both calls consume pba_linearize's unfused Jacobian pass whatever the driver."""
import argparse
import copy
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _d in (ROOT, os.path.join(ROOT, "tests")):
    if _d not in sys.path:
        sys.path.insert(0, _d)

DRIVER_VARS = ("PBA_RESIDENT", "PBA_ASYNC", "PBA_FUSE", "PBA_FUSE_FINAL")
PBA_ERR_NUMERIC = -6
_IMG = dict(size=(96, 128), K=(160.0, 160.0, 64.0, 48.0))
CAUSAL = "5x60-causal-huber-anchors-0-4"
DENSE_POINTS = (3, 64, 65, 257)
SOLVE_ITERATIONS = 6
VICTIM = 37

COV_INFO = ("n_cam", "point_dim", "num_residuals", "num_parameters", "cost", "min_cam_pivot", "min_point_pivot", "failed_is_point", "failed_index")
MARG_INFO = ("k", "n_points", "n_blocks", "cost", "min_point_pivot", "min_cam_pivot", "failed_is_point", "failed_index")
FIELDS = {"cov": ("status",) + COV_INFO + ("cam_cov", "point_cov"), "marg": ("status",) + MARG_INFO + ("slots", "x0", "Lambda", "eta", "c")}
FAILURE_FIELDS = ("poisoned", "kept")      # added to a case that ended in PBA_ERR_NUMERIC


def case_names():
    import marginal_cases as mc
    names = ["cov/full/3-dense-%d-points-anchors-0-2" % n for n in DENSE_POINTS]
    names += ["cov/full/" + CAUSAL, "cov/full/%s-after-solve" % CAUSAL, "cov/full/32-slots-anchors-0-31", "cov/pose"]
    names += ["cov/structure/world-points", "cov/structure/inverse-depths", "cov/fail/single-observation", "cov/fail/5x60-causal-huber-anchor-0"]
    names += ["marg/" + n for n in sorted(mc.CASES)] + ["marg/chain", "marg/fail/point"]
    return names


def _sha(*arrays):
    h = hashlib.sha1()
    for a in arrays:
        h.update(a.tobytes())
    return h.hexdigest()


def _info(info):
    return {f: (v.hex() if isinstance(v, float) else v) for f, v in ((f, getattr(info, f)) for f, _ in info._fields_)}


def _engine(p, slots, mode="full", rays=None, rho=None, prior=None):
    from photobundle_amd.engine import Engine
    _, _, rows, cols = p.planes.shape
    e = Engine(rows, cols, p.K, p.radius, p.n_frames, huber=p.huber)
    for s in range(p.n_frames):
        e.set_frame(s, p.images[s])
    e.set_problem(p.xyz, p.desc, p.obs_point, p.obs_slot, p.weights)
    if rays is not None:
        e.set_inverse_depth(rays, rho)
    if mode == "pose":
        e.set_points_constant()
    elif mode == "structure":
        e.set_cameras_constant()
    e.set_cameras(p.cams, constant_slots=slots)
    if prior is not None:
        e.set_camera_prior(**prior)
    return e


def _covariance(e, cameras=True, points=True):
    """One pba_covariance through the C call with poisoned caller buffers."""
    import numpy as np
    from photobundle_amd import _lib
    cam, pts = np.full(192 * 192, 7.25), np.full((e.n_points, 9), -3.5)
    info = _lib.CovarianceInfo()
    ptr = lambda a, on: a.ctypes.data_as(C.c_void_p) if on else None      # noqa: E731
    rc = e._L.pba_covariance(e._h, ptr(cam, cameras), ptr(pts, points), C.byref(info))
    out = dict(_info(info), status=rc, cam_cov=None, point_cov=None)
    if rc == 0:
        n = info.n_cam
        out.update(cam_cov=_sha(cam[:n * n]) if cameras else None, point_cov=_sha(pts) if points else None)
    elif rc == PBA_ERR_NUMERIC:
        out.update(poisoned=_sha(cam, pts), kept=bool((cam == 7.25).all() and (pts == -3.5).all()))
    else:
        raise RuntimeError("pba_covariance: status %d (%s)" % (rc, e._L.pba_last_error(e._h).decode()))
    return out


def _marginalize(e, drop):
    """One pba_marginalize through the C call with poisoned caller buffers."""
    import numpy as np
    from photobundle_amd import _lib
    mask = sum(1 << int(s) for s in drop)
    slots, x0, Lm, eta, c = np.full(32, -7, np.int32), np.full((32, 6), 7.25), np.full(192 * 192, -3.5), np.full(192, 1.5), C.c_double(-9.0)
    info = _lib.MarginalInfo()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    rc = e._L.pba_marginalize(e._h, mask, ptr(slots), ptr(x0), ptr(Lm), ptr(eta), C.byref(c), C.byref(info))
    out = dict(_info(info), status=rc, slots=None, x0=None, Lambda=None, eta=None, c=None)
    if rc == 0:
        k = info.k
        out.update(slots=_sha(slots[:k]), x0=_sha(x0[:k]), Lambda=_sha(Lm[:36 * k * k]), eta=_sha(eta[:6 * k]), c=c.value.hex())
    elif rc == PBA_ERR_NUMERIC:
        kept = (slots == -7).all() and (x0 == 7.25).all() and (Lm == -3.5).all() and (eta == 1.5).all() and c.value == -9.0
        out.update(poisoned=_sha(slots, x0, Lm, eta, np.float64(c.value)), kept=bool(kept))
    else:
        raise RuntimeError("pba_marginalize: status %d (%s)" % (rc, e._L.pba_last_error(e._h).decode()))
    return out


def _dense65():
    from photobundle_amd import synthetic
    return synthetic.make_window(n_frames=3, n_points=65, radius=1, **_IMG)


def _single_observation_window():
    """tests/test_gpu_covariance.py: point 37 keeps its first observation alone, its block has rank 2."""
    p = copy.copy(_dense65())
    keep = p.obs_point != VICTIM
    keep[(p.obs_point == VICTIM).argmax()] = True
    p.obs_point, p.obs_slot = p.obs_point[keep], p.obs_slot[keep]
    return p


def _zero_block_window():
    """tests/test_gpu_marginal.py: point 37 keeps its observation in slot 0 alone, on a flat patch of frame 0: its block is exactly zero."""
    from photobundle_amd import se3, synthetic
    p = _single_observation_window()
    uv, _ = synthetic.project(p.K, se3.params_to_pose(p.cams[0]), p.xyz[VICTIM:VICTIM + 1])
    x, y = int(round(uv[0, 0])), int(round(uv[0, 1]))
    p.images = p.images.copy()
    p.images[0, y - 6:y + 7, x - 6:x + 7] = 128
    p.desc = p.desc.copy()
    p.desc[VICTIM] = 128.0
    return p


def child():
    """Every case in this process: {case name: record}."""
    import covariance_cases as cc
    import marginal_cases as mc
    from photobundle_amd import synthetic
    from photobundle_amd.engine import default_solver_options
    out = {}
    for name in ["3-dense-%d-points-anchors-0-2" % n for n in DENSE_POINTS] + [CAUSAL, "32-slots-anchors-0-31"]:
        with _engine(cc.window(name), cc.slots_of(name)) as e:
            out["cov/full/" + name] = _covariance(e)
    causal = cc.window(CAUSAL)
    with _engine(causal, cc.slots_of(CAUSAL)) as e:
        e.solve(default_solver_options(max_num_iterations=SOLVE_ITERATIONS))
        out["cov/full/%s-after-solve" % CAUSAL] = _covariance(e)
    with _engine(causal, (0, 3), mode="pose") as e:
        out["cov/pose"] = _covariance(e, points=False)
    p65 = _dense65()
    with _engine(p65, (0,), mode="structure") as e:
        out["cov/structure/world-points"] = _covariance(e, cameras=False)
    rays, rho = synthetic.inverse_depth_rays(p65)
    with _engine(p65, (0,), mode="structure", rays=rays, rho=rho) as e:
        out["cov/structure/inverse-depths"] = _covariance(e, cameras=False)
    with _engine(_single_observation_window(), (0,), mode="structure") as e:
        out["cov/fail/single-observation"] = _covariance(e, cameras=False)
    with _engine(causal, (0,)) as e:
        out["cov/fail/5x60-causal-huber-anchor-0"] = _covariance(e)
    for name in sorted(mc.CASES):
        with _engine(mc.window(name), mc.anchors_of(name)) as e:
            out["marg/" + name] = _marginalize(e, mc.drop_of(name))
    first, drop_b, _ = mc.CHAIN
    p, anchors, drop = mc.window(first), mc.anchors_of(first), mc.drop_of(first)
    with _engine(p, anchors) as e:
        prior = mc.as_prior(e.marginalize(drop))
    q, anchors_b = mc.window_b(p, anchors, drop)
    with _engine(q, anchors_b, prior=prior) as e:
        out["marg/chain"] = _marginalize(e, drop_b)
    with _engine(_zero_block_window(), (0,)) as e:
        out["marg/fail/point"] = _marginalize(e, (0,))
    return out


def record(lib=None):
    """{case: record} from a child process of its own, the default driver.  lib: the library (None: the built one)."""
    env = {k: v for k, v in os.environ.items() if k not in DRIVER_VARS + ("PBA_LIB",)}
    if lib:
        env["PBA_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, timeout=600, env=env)
    if r.returncode != 0:
        raise RuntimeError("ab_elimination_bits child failed (%d): %s" % (r.returncode, r.stderr[-3000:]))
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT")][0][6:])


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--child", action="store_true", help="run the cases in this process and print them as one JSON line")
    ap.add_argument("--out", help="write the result as JSON")
    ap.add_argument("--commit", default=None, help="hash of the commit the library was built from (a field of --out)")
    a = ap.parse_args()
    if a.child:
        print("RESULT" + json.dumps(child()))
        return
    cases = record(os.environ.get("PBA_LIB"))
    for name, c in sorted(cases.items()):
        print("%-52s %s" % (name, " ".join("%s %s" % (f, str(v)[:14]) for f, v in c.items())))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(commit=a.commit, cases=cases), f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
