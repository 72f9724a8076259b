"""Numpy restatement of the semi-global matcher, written from the algorithm: vectorised over (y, d) or
(x, d), serial along each path; the speckle components through scipy.sparse.csgraph.connected_components on the edge
rule.  It exposes every stage pba_sgm_get_stage does, under the same names.

All volumes are [rows, cols, D].  16-bit saturating arithmetic is carried in int32 and clipped after every operation."""
import numpy as np

I16_MIN, I16_MAX = -32768, 32767

STAGES = ("sobel_left", "sobel_right", "census_left", "census_right", "cost_left", "sum_left", "disp_left_raw",
          "disp_right_raw", "disp_left_filtered", "disp_right_filtered")


def _sat(a):
    return np.clip(a, I16_MIN, I16_MAX)


def _wrap16(a):
    """int -> the int16 a C cast leaves (two's complement truncation)."""
    return ((np.asarray(a, np.int64) + 32768) & 0xFFFF) - 32768


def effective_cap(v):
    return min(max(int(v), 15), 127) | 1


def capped_sobel(img, cap):
    """u8 [H, W]: cap on the border, clamp(sobel_x, -cap, cap) + cap inside."""
    a = img.astype(np.int32)
    out = np.full(a.shape, cap, np.int32)
    if a.shape[0] > 2 and a.shape[1] > 2:
        s = (a[:-2, 2:] + 2 * a[1:-1, 2:] + a[2:, 2:]) - (a[:-2, :-2] + 2 * a[1:-1, :-2] + a[2:, :-2])
        out[1:-1, 1:-1] = np.where(s > cap, 2 * cap, np.where(s < -cap, 0, s + cap))
    return out.astype(np.uint8)


def census(img, radius):
    """int32 [H, W]: one bit per window position, row-major, set when the neighbour is inside and >= the centre."""
    H, W = img.shape
    a = img.astype(np.int32)
    pad = np.full((H + 2 * radius, W + 2 * radius), -1, np.int32)
    pad[radius:radius + H, radius:radius + W] = a
    code = np.zeros((H, W), np.int64)
    for oy in range(-radius, radius + 1):
        for ox in range(-radius, radius + 1):
            nb = pad[radius + oy:radius + oy + H, radius + ox:radius + ox + W]
            code = (code << 1) + (nb >= a)
    return code.astype(np.int32)


def _half_pixel_interval(s):
    """min and max of a Sobel row's value and its two half-pixel neighbours (integer halves, row ends repeat the centre)."""
    c = s.astype(np.int32)
    left = c.copy()
    left[:, 1:] = (c[:, 1:] + c[:, :-1]) // 2
    right = c.copy()
    right[:, :-1] = (c[:, :-1] + c[:, 1:]) // 2
    return c, np.minimum(np.minimum(left, right), c), np.maximum(np.maximum(left, right), c)


def _popcount(a):
    a = a.astype(np.uint32)
    a = a - ((a >> 1) & 0x55555555)
    a = (a & 0x33333333) + ((a >> 2) & 0x33333333)
    a = (a + (a >> 4)) & 0x0F0F0F0F
    return ((a * 0x01010101) >> 24).astype(np.int32) & 0xFF


def pixel_cost(sob_l, sob_r, cen_l, cen_r, ndisp, weight):
    """u8 [H, W, D]: interval cost on the Sobel images + (u8)(hamming * weight), added in u8; d > x repeats d = x."""
    H, W = sob_l.shape
    lc, lmin, lmax = _half_pixel_interval(sob_l)
    rc, rmin, rmax = _half_pixel_interval(sob_r)
    P = np.empty((H, W, ndisp), np.uint8)
    x = np.arange(W)
    for d in range(ndisp):
        xr = np.maximum(x - d, 0)
        l2r = np.maximum(np.maximum(0, lc - rmax[:, xr]), rmin[:, xr] - lc)
        r2l = np.maximum(np.maximum(0, rc[:, xr] - lmax), lmin - rc[:, xr])
        sad = np.minimum(l2r, r2l)
        ham = _popcount(np.bitwise_xor(cen_l, cen_r[:, xr]))
        hw = (ham.astype(np.float64) * float(weight)).astype(np.int64) & 0xFF
        P[:, :, d] = ((sad + hw) & 0xFF).astype(np.uint8)
    return P


def row_aggregate(P, radius):
    """int32 [H, W, D]: sum of P over x - radius .. x + radius, x clamped to the row."""
    H, W, D = P.shape
    idx = np.clip(np.arange(-radius - 1, W + radius), 0, W - 1)
    cs = np.cumsum(P[:, idx, :].astype(np.int32), axis=1)
    A = cs[:, 2 * radius + 1:, :] - cs[:, :W, :]
    assert A.max() <= I16_MAX
    return A


def cost_volume(P, radius):
    """uint16 [H, W, D], the left cost volume: row 0 in wrapping uint16, the rows below it by the saturating int16
    recurrence C[y] = (C[y-1] -s A[max(y-r-1, 0)]) +s A[y+r]; column 0 of rows >= 1 and the bottom `radius` rows stay 0."""
    H, W, D = P.shape
    A = row_aggregate(P, radius)
    C = np.zeros((H, W, D), np.uint16)
    top = (radius + 1) * A[0].astype(np.int64)
    for r in range(1, radius + 1):
        top = top + A[r]
    C[0] = (top & 0xFFFF).astype(np.uint16)
    prev = C[0].view(np.int16).astype(np.int32)
    for y in range(1, H):
        if y + radius >= H:
            break
        cur = _sat(_sat(prev - A[max(y - radius - 1, 0)]) + A[y + radius])
        cur[0, :] = 0
        C[y] = cur.astype(np.int16).view(np.uint16)
        prev = cur
    return C


def right_cost_volume(C):
    """C_R(y, x, d) = C_L(y, x + d, d), the last in-image value repeated beyond."""
    H, W, D = C.shape
    x = np.arange(W)[:, None]
    d = np.arange(D)[None, :]
    dd = np.minimum(d, W - 1 - x)
    return C[:, x + dd, dd]


def _path(C16, S, axis, reverse, p1, p2):
    """One path direction over the whole volume: axis 1 = along the row, axis 0 = along the column.  Adds its costs to S
    (int16, saturating)."""
    n = C16.shape[axis]
    other = C16.shape[1 - axis]
    D = C16.shape[2]
    prev = np.zeros((other, D), np.int32)
    prev_min = np.zeros((other,), np.int64)
    order = range(n - 1, -1, -1) if reverse else range(n)
    big = np.full((other, 1), I16_MAX, np.int32)
    for i in order:
        cost = (C16[:, i, :] if axis == 1 else C16[i, :, :]).astype(np.int32)
        pm = _wrap16(prev_min + p2).astype(np.int32)[:, None]
        lo = _sat(np.concatenate([big, prev[:, :-1]], axis=1) + p1)
        hi = _sat(np.concatenate([prev[:, 1:], big], axis=1) + p1)
        c = np.minimum(np.minimum(prev, lo), np.minimum(hi, pm))
        cur = _sat(_sat(c - pm) + cost)
        if axis == 1:
            S[:, i, :] = _sat(S[:, i, :].astype(np.int32) + cur).astype(np.int16)
        else:
            S[i, :, :] = _sat(S[i, :, :].astype(np.int32) + cur).astype(np.int16)
        prev = cur
        prev_min = cur.min(axis=1).astype(np.int64)


def path_sums(C, p1, p2):
    """int16 [H, W, D]: forward-row, forward-column, backward-row, backward-column path costs, summed in that order."""
    C16 = C.view(np.int16)
    S = np.zeros(C.shape, np.int16)
    _path(C16, S, 1, False, p1, p2)
    _path(C16, S, 0, False, p1, p2)
    _path(C16, S, 1, True, p1, p2)
    _path(C16, S, 0, True, p1, p2)
    return S


def winner(S, factor):
    """uint16 [H, W]: first minimum over d, the sub-pixel step in double, times the disparity factor."""
    H, W, D = S.shape
    factor = float(factor)
    best = np.argmin(S, axis=2)
    inner = (best > 0) & (best < D - 1)
    bi = np.clip(best, 1, D - 2)
    s = S.astype(np.int32)
    c = np.take_along_axis(s, bi[:, :, None], 2)[:, :, 0]
    l = np.take_along_axis(s, (bi - 1)[:, :, None], 2)[:, :, 0]
    r = np.take_along_axis(s, (bi + 1)[:, :, None], 2)[:, :, 0]
    den = np.where(r < l, c - l, c - r)
    den = np.where(inner & (den != 0), den, 1)
    sub = (best * factor + (r - l).astype(np.float64) / den / 2.0 * factor) + 0.5
    out = np.where(inner, sub.astype(np.int64), (best * factor).astype(np.int64))
    return (out & 0xFFFF).astype(np.uint16)


def speckle_filter(disp, max_size, max_diff):
    """Components of non-zero pixels, 4-connected, neighbours differing by <= max_diff; those of <= max_size pixels -> 0."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    H, W = disp.shape
    v = disp.astype(np.int32)
    idx = np.arange(H * W).reshape(H, W)
    eh = (v[:, :-1] != 0) & (v[:, 1:] != 0) & (np.abs(v[:, :-1] - v[:, 1:]) <= max_diff)
    ev = (v[:-1, :] != 0) & (v[1:, :] != 0) & (np.abs(v[:-1, :] - v[1:, :]) <= max_diff)
    a = np.concatenate([idx[:, :-1][eh], idx[:-1, :][ev]])
    b = np.concatenate([idx[:, 1:][eh], idx[1:, :][ev]])
    g = coo_matrix((np.ones(a.size, np.int8), (a, b)), shape=(H * W, H * W))
    _, lab = connected_components(g, directed=False)
    size = np.bincount(lab)[lab].reshape(H, W)
    out = disp.copy()
    out[(v != 0) & (size <= max_size)] = 0
    return out


def left_right_check(dl, dr, factor, threshold):
    H, W = dl.shape
    factor = float(factor)
    lv = (dl.astype(np.float64) / factor + 0.5).astype(np.int64)
    x = np.arange(W)[None, :]
    xr = x - lv
    inside = xr >= 0
    rv = (np.take_along_axis(dr, np.clip(xr, 0, W - 1), axis=1).astype(np.float64) / factor + 0.5).astype(np.int64)
    bad = (~inside) | (rv == 0) | (np.abs(lv - rv) > threshold)
    out = dl.copy()
    out[(dl != 0) & bad] = 0
    return out


def compute(left, right, ndisp, sobelCapValue=15, censusRadius=2, windowRadius=2, smoothnessPenaltySmall=100,
            smoothnessPenaltyLarge=1600, consistencyThreshold=1, disparityFactor=256.0, censusWeightFactor=1.0 / 6.0,
            stages=False):
    """-> dict with disp_scaled (uint16, after the left-right check) and disparity (fp32), plus every stage when asked."""
    cap = effective_cap(sobelCapValue)
    out = {}
    sl, sr = capped_sobel(left, cap), capped_sobel(right, cap)
    cl, cr = census(left, censusRadius), census(right, censusRadius)
    P = pixel_cost(sl, sr, cl, cr, ndisp, censusWeightFactor)
    C = cost_volume(P, windowRadius)
    del P
    S = path_sums(C, smoothnessPenaltySmall, smoothnessPenaltyLarge)
    raw_l = winner(S, disparityFactor)
    if stages:
        out.update(sobel_left=sl, sobel_right=sr, census_left=cl, census_right=cr, cost_left=C, sum_left=S)
    del S
    CR = right_cost_volume(C)
    del C
    raw_r = winner(path_sums(np.ascontiguousarray(CR), smoothnessPenaltySmall, smoothnessPenaltyLarge), disparityFactor)
    del CR
    max_diff = int(2 * float(disparityFactor))
    fl, fr = speckle_filter(raw_l, 100, max_diff), speckle_filter(raw_r, 100, max_diff)
    final = left_right_check(fl, fr, disparityFactor, consistencyThreshold)
    out.update(disp_left_raw=raw_l, disp_right_raw=raw_r, disp_left_filtered=fl, disp_right_filtered=fr, disp_scaled=final,
               disparity=(final.astype(np.float64) / float(disparityFactor)).astype(np.float32))
    return out
