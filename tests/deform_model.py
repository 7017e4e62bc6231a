"""numpy model of row f26 (include/svgf_deform.h): the skin of a rig's triangles, their padded boxes, the cur / prev state of a
sequence of bone tables and the previous position of a pixel - float32, one rounding per operation, in the order the header writes
them.  The frame of a deformed scene is tests/scene_model.py's on the deformed triangles; the previous-position plane sits on top of
that frame (its position and id planes) and of a triangle loop of its own that keeps the winner's index and barycentrics.  Test
infrastructure only; it shares no text with the kernels.

NaN: as in scene_pose_model.py - NaNs in the same places count as equal."""
import numpy as np

import resident_scene_model as rm
import scene_model as sm

F = np.float32


def _blend(w, q):
    """((w0 q0 + w1 q1) + w2 q2) + w3 q3 over the last axis of w[..., 4] and q[..., 4]."""
    s = ((w[..., 0] * q[..., 0]).astype(F) + (w[..., 1] * q[..., 1]).astype(F)).astype(F)
    s = (s + (w[..., 2] * q[..., 2]).astype(F)).astype(F)
    return (s + (w[..., 3] * q[..., 3]).astype(F)).astype(F)


def skin(rest, bone, weight, xf):
    """float32[n, 3, 8]: the rig's rest triangles (float32[n, 3, 8]) through the bone table xf (float32[n_bones, 12]): positions by the
    whole map, normals by its linear block, four influences each, uv untouched."""
    rest = np.array(rest, dtype=F).reshape(-1, 3, 8)
    bone, w = np.asarray(bone).reshape(-1, 3, 4).astype(np.int64), np.asarray(weight, F).reshape(-1, 3, 4)
    M = np.asarray(xf, F).reshape(-1, 3, 4)[bone]                       # [n, 3, 4 influences, 3 rows, 4]
    P, N = rest[:, :, None, 0:3], rest[:, :, None, 3:6]                  # broadcast over the influences
    out = rest.copy()
    with np.errstate(all="ignore"):
        for r in range(3):
            q = ((M[..., r, 0] * P[..., 0]).astype(F) + (M[..., r, 1] * P[..., 1]).astype(F)).astype(F)
            q = (q + (M[..., r, 2] * P[..., 2]).astype(F)).astype(F)
            q = (q + M[..., r, 3]).astype(F)
            m = ((M[..., r, 0] * N[..., 0]).astype(F) + (M[..., r, 1] * N[..., 1]).astype(F)).astype(F)
            m = (m + (M[..., r, 2] * N[..., 2]).astype(F)).astype(F)
            out[:, :, r], out[:, :, 3 + r] = _blend(w, q), _blend(w, m)
    return out


def boxes(tris):
    """(lo, hi) float32[n, 3]: row f14's padded boxes of deformed triangles, written as the kernels write the formula - fminf / fmaxf (a NaN
    operand is ignored) and `e > ext ? e : ext` (a NaN extent is skipped) - so that a corner that is not finite has a defined box too.
    On finite triangles this is resident_scene_model.padded_boxes (tests/test_deform_scene.py holds the two to each other)."""
    P = np.ascontiguousarray(tris, dtype=F).reshape(-1, 3, 8)[:, :, 0:3]
    with np.errstate(all="ignore"):
        mn, mx = np.fmin(np.fmin(P[:, 0], P[:, 1]), P[:, 2]), np.fmax(np.fmax(P[:, 0], P[:, 1]), P[:, 2])
        ext = np.zeros(len(P), F)
        for c in range(3):
            e = (mx[:, c] - mn[:, c]).astype(F)
            ext = np.where(e > ext, e, ext).astype(F)
        m = np.fmax(F(1), np.fmax(np.abs(mn), np.abs(mx)))
        pad = ((ext[:, None] * F(2.0 ** -8)).astype(F) + (F(2.0 ** -16) * m).astype(F)).astype(F)
        return (mn - pad).astype(F), (mx + pad).astype(F)


class Rig:
    """The state svgf_deform_create makes and svgf_deform_apply advances, for `drawn` (float32[n_tris, 3, 8], the triangles as drawn at
    creation): slot, cur, prev; apply(xf, drawn) returns the triangles as drawn after the apply (`drawn`: what stands there before it,
    svgf_scene_pose's bytes)."""

    def __init__(self, drawn, tri_index, bone, weight):
        drawn = np.asarray(drawn, F).reshape(-1, 3, 8)
        self.tri_index = np.asarray(tri_index, np.int64).reshape(-1)
        self.bone, self.weight = np.asarray(bone).reshape(-1, 3, 4), np.asarray(weight, F).reshape(-1, 3, 4)
        self.rest = drawn[self.tri_index].copy()
        self.slot = np.full(len(drawn), -1, np.int32)
        self.slot[self.tri_index] = np.arange(len(self.tri_index), dtype=np.int32)
        self.cur, self.prev = self.rest[:, :, 0:3].copy(), self.rest[:, :, 0:3].copy()

    def apply(self, xf, drawn):
        out = np.array(drawn, dtype=F).reshape(-1, 3, 8)
        skinned = skin(self.rest, self.bone, self.weight, xf)
        self.prev, self.cur = self.cur, skinned[:, :, 0:3].copy()
        out[self.tri_index] = skinned
        return out


def winners(W, H, cam, tris, pixel_length=None):
    """The triangle loop of scene_model.render started from +inf, keeping what the frame drops: (best int64[H, W] or -1, bx, by)."""
    tris = np.ascontiguousarray(tris, dtype=F).reshape(-1, 24)
    o = [F(c) for c in np.asarray(cam["position"], dtype=F)]
    best, bt = np.full((H, W), -1, np.int64), np.full((H, W), np.inf, F)
    bbx, bby = np.zeros((H, W), F), np.zeros((H, W), F)
    with np.errstate(all="ignore"):
        d = sm.rays(W, H, cam, pixel_length)
        for i in range(len(tris)):
            T = tris[i]
            e1, e2 = [F(T[8 + c] - T[c]) for c in range(3)], [F(T[16 + c] - T[c]) for c in range(3)]
            pv = [(d[1] * e2[2] - e2[1] * d[2]).astype(F), (d[2] * e2[0] - e2[2] * d[0]).astype(F), (d[0] * e2[1] - e2[0] * d[1]).astype(F)]
            det = sm._dot(e1, pv)
            f = (F(1) / det).astype(F)
            sv = [F(o[c] - T[c]) for c in range(3)]
            bx = (f * sm._dot(sv, pv)).astype(F)
            q = [F(sv[1] * e1[2] - e1[1] * sv[2]), F(sv[2] * e1[0] - e1[2] * sv[0]), F(sv[0] * e1[1] - e1[0] * sv[1])]
            by = (f * sm._dot(d, q)).astype(F)
            t = (f * F((e2[0] * q[0] + e2[1] * q[1]) + e2[2] * q[2])).astype(F)
            go = ~(det < sm.EPS) & ~((bx < 0) | (bx > 1)) & ~((by < 0) | ((by + bx).astype(F) > 1)) & (t > 0) & (t < bt)
            bt, best = np.where(go, t, bt).astype(F), np.where(go, i, best)
            bbx, bby = np.where(go, bx, bbx).astype(F), np.where(go, by, bby).astype(F)
    return best, bbx, bby


def displaced(pos, b0, b1, b2, prev, cur):
    """pos float32[..., 3] moved by d_c = (b0 (prev0 - cur0) + b1 (prev1 - cur1)) + b2 (prev2 - cur2); pos itself where d_c == 0.
    prev, cur: float32[..., 3 corners, 3]."""
    with np.errstate(all="ignore"):
        e = (prev - cur).astype(F)
        d = ((b0[..., None] * e[..., 0, :]).astype(F) + (b1[..., None] * e[..., 1, :]).astype(F)).astype(F)
        d = (d + (b2[..., None] * e[..., 2, :]).astype(F)).astype(F)
        return np.where(d == 0, pos, (pos + d).astype(F)).astype(F)


def prev_positions(gb, W, H, cam, tris, tri_ids, rig, pixel_length=None, geom_ids=()):
    """(plane float32[H, W, 3], id int32[H, W]) of svgf_deform_prev_positions for the frame whose G-buffer is `gb` (scene_model.render
    on `tris`, the triangles as drawn).  A pixel is a triangle's when its id is that triangle's; the ids of triangles and primitives
    must not meet (geom_ids: the primitives' ids), or the frame would have to say which of the two won."""
    tri_ids = np.asarray(tri_ids, np.int32)
    assert not set(tri_ids.tolist()) & set(int(g) for g in geom_ids), "an id is a primitive's and a triangle's"
    gid, pos = gb["geomId"], gb["position"]
    best, bx, by = winners(W, H, cam, tris, pixel_length)
    mesh = (best >= 0) & (gid == tri_ids[np.maximum(best, 0)])
    s = np.where(mesh, rig.slot[np.maximum(best, 0)], -1)
    on = s >= 0
    si = np.maximum(s, 0)
    with np.errstate(all="ignore"):
        b0 = ((F(1) - bx).astype(F) - by).astype(F)
        moved = displaced(pos, b0, bx, by, rig.prev[si], rig.cur[si])
    out = np.where(on[..., None], moved, pos).astype(F)
    out = np.where((gid < 0)[..., None], F(np.nan), out).astype(F)
    return out, np.where(gid < 0, -1, gid).astype(np.int32)
