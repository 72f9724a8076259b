"""Test-only CPU restatements of the stereo block matcher (DESIGN.md "Stereo block matching": this project's statement of
OpenCV 2.4 StereoBM, XSOBEL prefilter, generic C path).  Two independent forms:

  * bm_loop / prefilter_loop: the spec read literally, one pixel and one disparity at a time (tiny images only);
  * bm / prefilter: vectorised numpy, a cost volume from summed-area tables, argmin with the tie rule.

Both return the int16 disparity (4 fractional bits, FILTERED = (minD - 1) * 16).  depth_from_disp16 is the spec's
disparity-to-depth in fp32 (two correctly rounded operations)."""
import numpy as np

XSOBEL = 1


def default_params(**kw):
    """pba_stereo_default_params with numberOfDisparities left to the caller (0 = must be set)."""
    p = dict(pre_filter_type=XSOBEL, pre_filter_size=9, pre_filter_cap=31, sad_window_size=15, min_disparity=0,
             number_of_disparities=0, texture_threshold=10, uniqueness_ratio=15, speckle_window_size=0, speckle_range=0,
             try_smaller_windows=0, disp12_max_diff=-1)
    unknown = set(kw) - set(p)
    assert not unknown, unknown
    p.update(kw)
    return p


def filtered_value(p):
    return (p["min_disparity"] - 1) * 16


def valid_region(H, W, p):
    """[x0, x1) x [y0, y1): the spec's region, bounded by W + minD - r so that no window reads beyond the right image."""
    r = p["sad_window_size"] // 2
    min_d = p["min_disparity"]
    max_d = min_d + p["number_of_disparities"] - 1
    return max(0, max_d) + r, min(W, W - min_d, W + min_d) - r, r, H - r


# ---------------------------------------------------------------------------------------------------------- loop form
def prefilter_loop(I, cap):
    H, W = I.shape
    P = np.full((H, W), cap, dtype=np.uint8)
    for y in range(H):
        if H % 2 == 1 and y == H - 1:
            continue
        ym = 1 if y == 0 else y - 1
        yp = H - 2 if y == H - 1 else y + 1
        for x in range(1, W - 1):
            v = (int(I[ym, x + 1]) - int(I[ym, x - 1])) + 2 * (int(I[y, x + 1]) - int(I[y, x - 1])) + \
                (int(I[yp, x + 1]) - int(I[yp, x - 1]))
            P[y, x] = min(max(v, -cap), cap) + cap
    return P


def bm_loop(left, right, p):
    H, W = left.shape
    cap, r = p["pre_filter_cap"], p["sad_window_size"] // 2
    min_d, nd = p["min_disparity"], p["number_of_disparities"]
    max_d = min_d + nd - 1
    PL = prefilter_loop(left, cap).astype(int)
    PR = prefilter_loop(right, cap).astype(int)
    x0, x1, y0, y1 = valid_region(H, W, p)
    out = np.full((H, W), filtered_value(p), dtype=np.int16)
    for y in range(y0, y1):
        for x in range(x0, x1):
            texture = 0
            for j in range(-r, r + 1):
                for i in range(-r, r + 1):
                    texture += abs(PL[y + j, x + i] - cap)
            C = {}
            for D in range(min_d, max_d + 1):
                s = 0
                for j in range(-r, r + 1):
                    for i in range(-r, r + 1):
                        s += abs(PL[y + j, x + i] - PR[y + j, x + i - D])
                C[D] = s
            # OpenCV's scan: cost index d = maxD - D ascending, strict <
            best = None
            for d in range(nd):
                D = max_d - d
                if best is None or C[D] < C[best]:
                    best = D
            cmin = C[best]
            if texture < p["texture_threshold"]:
                continue
            if p["uniqueness_ratio"] > 0:
                thresh = cmin + (cmin * p["uniqueness_ratio"]) // 100
                if any(abs(D - best) > 1 and C[D] <= thresh for D in C):
                    continue
            c_lo = C.get(best - 1)
            c_hi = C.get(best + 1)
            if best == max_d:
                c_hi = c_lo
            if best == min_d:
                c_lo = c_hi
            den = c_lo + c_hi - 2 * cmin + abs(c_lo - c_hi)
            num = (c_lo - c_hi) * 256
            frac = 0 if den == 0 else (abs(num) // den) * (1 if num >= 0 else -1)   # C truncating division
            out[y, x] = (best * 256 + frac + 15) >> 4
    return out


# --------------------------------------------------------------------------------------------------------- numpy form
def prefilter(I, cap):
    I = I.astype(np.int32)
    H, W = I.shape
    up = I[np.r_[1, 0:H - 1]]                       # row y - 1, reflect-101
    dn = I[np.r_[1:H, H - 2]]                       # row y + 1
    v = (up[:, 2:] - up[:, :-2]) + 2 * (I[:, 2:] - I[:, :-2]) + (dn[:, 2:] - dn[:, :-2])
    P = np.full((H, W), cap, dtype=np.int32)
    P[:, 1:-1] = np.clip(v, -cap, cap) + cap
    if H % 2 == 1:
        P[-1, :] = cap
    return P.astype(np.uint8)


def _box(A, w):
    S = np.zeros((A.shape[0] + 1, A.shape[1] + 1), dtype=np.int64)
    S[1:, 1:] = A.cumsum(0).cumsum(1)
    return S[w:, w:] - S[:-w, w:] - S[w:, :-w] + S[:-w, :-w]


def bm(left, right, p):
    H, W = left.shape
    cap, w = p["pre_filter_cap"], p["sad_window_size"]
    r = w // 2
    min_d, nd = p["min_disparity"], p["number_of_disparities"]
    max_d = min_d + nd - 1
    out = np.full((H, W), filtered_value(p), dtype=np.int16)
    x0, x1, y0, y1 = valid_region(H, W, p)
    if x0 >= x1 or y0 >= y1:
        return out
    PL = prefilter(left, cap).astype(np.int32)
    PR = prefilter(right, cap).astype(np.int32)
    Lw = PL[y0 - r:y1 + r, x0 - r:x1 + r]
    texture = _box(np.abs(Lw - cap), w)
    cdt = np.uint16 if w * w * 2 * cap < 65536 else np.int32
    cost = np.empty((nd, y1 - y0, x1 - x0), dtype=cdt)      # index d = maxD - D
    for d in range(nd):
        D = max_d - d
        cost[d] = _box(np.abs(Lw - PR[y0 - r:y1 + r, x0 - r - D:x1 + r - D]), w)
    dmin = np.argmin(cost, axis=0)                           # first minimum = smallest d = largest D
    cmin = np.take_along_axis(cost, dmin[None], 0)[0].astype(np.int64)
    D_star = max_d - dmin.astype(np.int64)
    c_lo = np.take_along_axis(cost, np.minimum(dmin + 1, nd - 1)[None], 0)[0].astype(np.int64)   # C(D* - 1)
    c_hi = np.take_along_axis(cost, np.maximum(dmin - 1, 0)[None], 0)[0].astype(np.int64)        # C(D* + 1)
    c_hi = np.where(dmin == 0, c_lo, c_hi)
    c_lo = np.where(dmin == nd - 1, c_hi, c_lo)
    far = np.full(cmin.shape, np.iinfo(np.int64).max, dtype=np.int64)
    for d in range(nd):
        far = np.where(np.abs(d - dmin) > 1, np.minimum(far, cost[d]), far)
    den = c_lo + c_hi - 2 * cmin + np.abs(c_lo - c_hi)
    num = (c_lo - c_hi) * 256
    frac = np.where(den != 0, np.sign(num) * (np.abs(num) // np.maximum(den, 1)), 0)
    res = (D_star * 256 + frac + 15) >> 4
    bad = texture < p["texture_threshold"]
    if p["uniqueness_ratio"] > 0:
        bad |= far <= cmin + (cmin * p["uniqueness_ratio"]) // 100
    out[y0:y1, x0:x1] = np.where(bad, filtered_value(p), res).astype(np.int16)
    return out


def depth_from_disp16(disp16, bf):
    """d = out * 0.0625 (exact); depth = d > 0.01 ? Bf * (1 / d) : -0.1, in fp32."""
    d = disp16.astype(np.float32) * np.float32(0.0625)
    return disparity_to_depth(d, bf)


def disparity_to_depth(d, bf):
    d = np.asarray(d, dtype=np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        z = np.float32(bf) * (np.float32(1.0) / d)
    return np.where(d > np.float32(0.01), z, np.float32(-0.1)).astype(np.float32)
