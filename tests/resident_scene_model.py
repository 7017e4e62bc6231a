"""numpy model of the resident scene's gate (include/svgf.h, row f14): the padded box of a triangle, the slab test S(box, ray) and
the ungated triangle loop's winner, float32 with one rounding per operation, written the way the builder and the kernel write them.
The frame itself is tests/scene_model.py's: wherever the ungated winner passes its own gate the resident scene draws that frame.
Test infrastructure only.
"""
import numpy as np

import scene_model as sm

F = np.float32
FLAT = F(2.0 ** -100)


def padded_boxes(tris):
    """(lo, hi) float32[n, 3] of float32[n, 3, 8] (or [n, 24]) triangles."""
    P = np.ascontiguousarray(tris, dtype=F).reshape(-1, 3, 8)[:, :, 0:3]
    mn = np.minimum(np.minimum(P[:, 0], P[:, 1]), P[:, 2])
    mx = np.maximum(np.maximum(P[:, 0], P[:, 1]), P[:, 2])
    ext = (mx - mn).astype(F).max(axis=1, initial=F(0))[:, None]
    m = np.maximum(F(1), np.maximum(np.abs(mn), np.abs(mx)))
    pad = ((ext * F(2.0 ** -8)).astype(F) + (F(2.0 ** -16) * m).astype(F)).astype(F)
    return (mn - pad).astype(F), (mx + pad).astype(F)


def slab(lo, hi, o, d):
    """S(box, ray): (pass, tn).  lo, hi: three scalars or arrays; o: three scalars; d: three arrays (broadcast against lo / hi)."""
    with np.errstate(all="ignore"):
        tn, tf, ok = F(0), F(np.inf), True
        for c in range(3):
            flat = np.abs(d[c]) < FLAT
            inv = (F(1) / d[c]).astype(F)
            t1, t2 = ((lo[c] - o[c]).astype(F) * inv).astype(F), ((hi[c] - o[c]).astype(F) * inv).astype(F)
            ok = ok & np.where(flat, (lo[c] <= o[c]) & (o[c] <= hi[c]), True)
            tn = np.where(flat, tn, np.maximum(tn, np.minimum(t1, t2))).astype(F)
            tf = np.where(flat, tf, np.minimum(tf, np.maximum(t1, t2))).astype(F)
        return ok & (tn <= tf), tn


def hits(tri, o, d):
    """scene_model.render's triangle test on one triangle (24 floats) for direction planes d: (accepted with t > 0, t)."""
    T = np.asarray(tri, dtype=F).reshape(24)
    with np.errstate(all="ignore"):
        e1, e2 = [F(T[8 + c] - T[c]) for c in range(3)], [F(T[16 + c] - T[c]) for c in range(3)]
        pv = [(d[1] * e2[2] - e2[1] * d[2]).astype(F), (d[2] * e2[0] - e2[2] * d[0]).astype(F), (d[0] * e2[1] - e2[0] * d[1]).astype(F)]
        det = sm._dot(e1, pv)
        go = ~(det < sm.EPS)
        f = (F(1) / det).astype(F)
        sv = [F(o[c] - T[c]) for c in range(3)]
        bx = (f * sm._dot(sv, pv)).astype(F)
        go &= ~((bx < 0) | (bx > 1))
        q = [F(sv[1] * e1[2] - e1[1] * sv[2]), F(sv[2] * e1[0] - e1[2] * sv[0]), F(sv[0] * e1[1] - e1[0] * sv[1])]
        by = (f * sm._dot(d, q)).astype(F)
        go &= ~((by < 0) | ((by + bx).astype(F) > 1))
        t = (f * F((e2[0] * q[0] + e2[1] * q[1]) + e2[2] * q[2])).astype(F)
        return go & (t > 0), t


def gate_report(W, H, cam, tris, pixel_length=None):
    """The ungated triangle loop of scene_model.render started from +inf (the winner among the triangles; with primitives in the
    scene the frame's triangle winner is this one or none), and the gate of every accepted (ray, triangle) pair.
    Returns dict(best int[H, W], winner_fails int, pair_fails int, pairs int, flat_rays int)."""
    tris = np.ascontiguousarray(tris, dtype=F).reshape(-1, 24)
    o = [F(c) for c in np.asarray(cam["position"], dtype=F)]
    d = sm.rays(W, H, cam, pixel_length)
    lo, hi = padded_boxes(tris)
    best, bt = np.full((H, W), -1, np.int64), np.full((H, W), np.inf, F)
    best_fails = np.zeros((H, W), bool)
    pairs = pair_fails = 0
    for i in range(len(tris)):
        acc, t = hits(tris[i], o, d)
        if not acc.any():
            continue
        ok, tn = slab(lo[i], hi[i], o, d)
        fails = acc & ~(ok & (t >= tn))
        pairs += int(acc.sum()); pair_fails += int(fails.sum())
        take = acc & (t < bt)
        bt, best, best_fails = np.where(take, t, bt).astype(F), np.where(take, i, best), np.where(take, fails, best_fails)
    flat = (np.abs(d[0]) < FLAT) | (np.abs(d[1]) < FLAT) | (np.abs(d[2]) < FLAT)
    return dict(best=best, winner_fails=int(best_fails.sum()), pair_fails=pair_fails, pairs=pairs, flat_rays=int(flat.sum()))


def leaves_below(nodes, k=0):
    """Triangle positions (indices into `order`) below node k, per the SvgfBvhNode rules."""
    out, todo = [], [k]
    while todo:
        n = nodes[todo.pop()]
        if n["count"] > 0:
            out.extend(range(int(n["first"]), int(n["first"]) + int(n["count"])))
        else:
            todo += [int(n["first"]), int(n["first"]) + 1]
    return out
