"""Helpers of the wide-window scale tests (test_wide_scale_cpu.py, test_gpu_wide_scale.py): the co-observation structure of a window as
wide_prepare (csrc/pba_engine.hip) cuts it into chunks, and tools that shape a generated window into the structures the pair stage has to
get right -- several chunks per camera pair, a chunk that is exactly full, a second chunk of one entry, camera pairs without a common point."""
import dataclasses
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def wide_chunk():
    """kWideChunk of csrc/pba_wide.h: co-observations per workgroup of the pair stage."""
    src = open(os.path.join(ROOT, "photobundle_amd", "csrc", "pba_wide.h")).read()
    m = re.search(r"constexpr\s+int\s+kWideChunk\s*=\s*(\d+)\s*;", src)
    assert m, "kWideChunk not found in pba_wide.h"
    return int(m.group(1))


def cost_block_stride_obs():
    """The observation count above which the tail workgroup of k_wide_assemble (128 threads) takes a second trip through the cost blocks:
    pba_set_problem launches the sampling pass with sample_grid = ceil(n_obs / (kSampleWaves * 64)) workgroups, one cost block each, so
    sample_grid > 128 <=> n_obs > 128 * kSampleWaves * 64."""
    src = open(os.path.join(ROOT, "photobundle_amd", "csrc", "pba_engine.hip")).read()
    m = re.search(r"constexpr\s+int\s+kSampleWaves\s*=\s*(\d+)\s*;", src)
    assert m and "e->sample_grid = (n_obs + e->sample_waves * 64 - 1) / (e->sample_waves * 64);" in src
    return 128 * int(m.group(1)) * 64


def free_slots(p):
    return [s for s in range(p.n_frames) if s != p.fixed_slot]


def co_observation_counts(p):
    """[n_free, n_free] int64, symmetric: entry (a, b) = points observed by both free cameras a and b (free indices: the slots in
    ascending order without fixed_slot); the diagonal = observations of camera a.  Entry (a, b), a <= b, is the length of the pair's
    list in wide_prepare."""
    free = free_slots(p)
    col = -np.ones(p.n_frames, np.int64)
    col[free] = np.arange(len(free))
    c = col[p.obs_slot]
    m = c >= 0
    V = np.zeros((p.n_points, len(free)), np.int64)
    np.add.at(V, (p.obs_point[m], c[m]), 1)
    assert V.max() <= 1, "a point observed twice by one camera"
    return V.T @ V


def structure(p, chunk=None):
    """The figures the tests assert on: dict(C, n_pairs, multi (pairs with 2+ chunks), empty (pairs without an entry), largest, chunks)."""
    chunk = chunk or wide_chunk()
    C = co_observation_counts(p)
    iu = np.triu_indices(len(C))
    v = C[iu]
    n = -(-v // chunk)
    return dict(C=C, n_pairs=len(v), multi=int((n >= 2).sum()), empty=int((v == 0).sum()), largest=int(v.max()), chunks=int(n.sum()),
                max_chunks=int(n.max()))


def restrict_observations(p, keep):
    """A copy of `p` with the observations keep (bool mask or indices) only, in their order.  Points keep their indices."""
    keep = np.asarray(keep)
    idx = np.nonzero(keep)[0] if keep.dtype == bool else np.sort(keep)
    q = dataclasses.replace(p, cams=p.cams.copy(), xyz=p.xyz.copy(), obs_point=p.obs_point[idx].copy(), obs_slot=p.obs_slot[idx].copy(),
                            meta=dict(p.meta))
    assert len(np.unique(q.obs_point)) == p.n_points, "a point lost every observation"
    return q


def obs_per_point(p):
    return np.bincount(p.obs_point, minlength=p.n_points)


def shape_window(p, band=None, exact=()):
    """Drops observations of `p` (a copy is returned) so that
      * the window is banded: an observation stays only if slot - birth slot <= band (birth = the point's first observation), and
      * every pair named in exact = [((a, b), count), ...] (free indices, a <= b) has exactly `count` co-observations: from evenly
        spread points that see both cameras and keep at least three observations, camera b's observation is removed.  A removal never
        touches a pair named earlier in the list (such points are not candidates), so list diagonal pairs last.
    Every point keeps at least two observations (asserted)."""
    keep = np.ones(p.n_obs, bool)
    if band is not None:
        first = np.searchsorted(p.obs_point, np.arange(p.n_points))
        birth = p.obs_slot[first][p.obs_point]
        keep &= (p.obs_slot - birth) <= band
    q = restrict_observations(p, keep)
    free = free_slots(q)
    frozen = []
    for (a, b), count in exact:
        assert 0 <= a <= b < len(free)
        sa, sb = free[a], free[b]
        V = np.zeros((q.n_points, q.n_frames), bool)
        V[q.obs_point, q.obs_slot] = True
        have = int((V[:, sa] & V[:, sb]).sum())
        assert have >= count, ((a, b), have, count)
        cand = V[:, sa] & V[:, sb] & (V.sum(1) >= 4)
        for (fa, fb) in frozen:          # removing camera b's observation changes every pair (b, x) of a point that sees x
            if fa == b or fb == b:
                other = free[fa if fb == b else fb]
                cand &= ~V[:, other]
        cand = np.nonzero(cand)[0]
        n_drop = have - count
        assert len(cand) >= n_drop, ((a, b), len(cand), n_drop)
        pts = cand[np.unique(np.linspace(0, len(cand) - 1, n_drop).round().astype(int))] if n_drop else cand[:0]
        if len(pts) < n_drop:            # (rounding made two picks coincide)
            rest = np.setdiff1d(cand, pts)
            pts = np.concatenate([pts, rest[:n_drop - len(pts)]])
        drop = np.isin(q.obs_point, pts) & (q.obs_slot == sb)
        assert int(drop.sum()) == n_drop
        q = restrict_observations(q, ~drop)
        frozen.append((a, b))
    assert obs_per_point(q).min() >= 2
    C = co_observation_counts(q)
    for (a, b), count in exact:
        assert C[a, b] == count, ((a, b), int(C[a, b]), count)
    return q


def pick_exact_pairs(C, chunk):
    """Pairs of a banded window to trim (shape_window's `exact`): two different adjacent pairs (a, a + 1) to chunk and chunk + 1 and one
    diagonal pair, of a camera in neither, to 2 * chunk -- each the candidate that loses the fewest observations."""
    n = len(C)
    adj = sorted((int(C[a, a + 1]), a) for a in range(n - 1) if C[a, a + 1] > chunk + 1)
    assert len(adj) >= 2, "no two adjacent pairs above one chunk"
    (_, a0) = adj[0]
    a1 = next(a for _, a in adj[1:] if abs(a - a0) >= 2)
    used = {a0, a0 + 1, a1, a1 + 1}
    dia = sorted((int(C[d, d]), d) for d in range(n) if d not in used and C[d, d] > 2 * chunk)
    assert dia, "no diagonal pair above two chunks"
    d = dia[0][1]
    return [((a0, a0 + 1), chunk), ((a1, a1 + 1), chunk + 1), ((d, d), 2 * chunk)]
