"""numpy model of libsvgf_restir.so (include/svgf_restir.h, row f27), layered on tests/scene_model.py and tests/scene_shadow_model.py:
both launches of svgf_restir_frame and svgf_lights_draw_all from a G-buffer, float32 throughout, one rounding per operation, every
expression nested the way the kernels nest it.  The shadow rays are scene_shadow_model's brute force over all occluders (every
primitive that does not emit, every triangle with its gate), towards a light that differs per pixel.  A State carries H, T and the
previous planes from frame to frame, as the device state does, and every frame returns per-event counts.  Test infrastructure only.

`alt` names ONE deliberate deviation, in scene_model's manner: the model then computes what a kernel with that mistake would, and a
test counts the pixels on which a case tells the two apart.
"""
import numpy as np

import resident_scene_model as rm
import scene_shadow_model as ssm
from scene_model import F, _dot, _sel, synth

ALTS = ("no_source_pdf", "initial_ray_ignored", "history_phat_as_stored", "no_m_cap", "temporal_no_id_test", "temporal_no_normal_test",
        "tap_rounds_down", "neighbour_phat_as_stored", "spatial_no_id_test", "spatial_no_normal_test", "neighbour_may_be_self", "final_ray_ignored",
        "history_stream_is_4128")
EVENTS = ("initial_occluded", "tap_off_screen", "tap_refused_id", "tap_refused_normal", "tap_accepted", "history_selected", "m_capped",
          "neighbour_refused_id", "neighbour_refused_normal", "neighbour_accepted", "neighbour_selected", "empty_shaded", "final_occluded_after_reuse")
LIGHT_DTYPE = np.dtype([("centre", F, 3), ("edge_u", F, 3), ("edge_v", F, 3), ("power", F, 3)])
RESERVOIR_DTYPE = np.dtype([("j", np.int32), ("u", F), ("v", F), ("M", F), ("W", F), ("phat", F), ("zero", np.int32, 2)])


def params(candidates=8, temporal=1, m_cap=20.0, neighbours=3, radius=30.0, normal_min_dot=0.9):
    return dict(candidates=int(candidates), temporal=int(temporal), m_cap=F(m_cap), neighbours=int(neighbours), radius=F(radius),
                normal_min_dot=F(normal_min_dot))


def lights(centre, edge_u=None, edge_v=None, power=30.0):
    c = np.asarray(centre, F).reshape(-1, 3)
    out = np.zeros(len(c), LIGHT_DTYPE)
    out["centre"] = c
    if edge_u is not None:
        out["edge_u"] = np.asarray(edge_u, F)
    if edge_v is not None:
        out["edge_v"] = np.asarray(edge_v, F)
    pw = np.asarray(power, F)
    out["power"] = np.broadcast_to(pw if pw.ndim != 1 or len(pw) == 3 else pw[:, None], (len(c), 3))
    return out


def lum(Fc):
    """svgf_lum_strict: the denoiser's luminance, in double, rounded once."""
    with np.errstate(all="ignore"):
        l = 0.2126 * Fc[0].astype(np.float64) + 0.7152 * Fc[1].astype(np.float64)
        return (l + 0.0722 * Fc[2].astype(np.float64)).astype(F)


def light_term(lt, j, nrm, pos):
    """(F_j,c as three arrays, lam) at the surface points (nrm, pos: three arrays each) for light indices j (one per point)."""
    with np.errstate(all="ignore"):
        tl = [(lt["centre"][j, c] - pos[c]).astype(F) for c in range(3)]
        dist2 = _dot(tl, tl)
        dl = np.sqrt(dist2)
        lam = _dot([(tl[c] / dl).astype(F) for c in range(3)], nrm)
        lam = _sel(lam > 0, lam, F(0))                                   # fmaxf(x, 0): a NaN gives 0
        return [((lt["power"][j, c] * lam).astype(F) / (F(4.0) + dist2).astype(F)).astype(F) for c in range(3)], lam


class Scene:
    """What the shadow rays and the id table need of a scene dict (tests/scene_harness.py's): primitives, triangles as drawn, their
    padded boxes, and the table from geomId to emittance svgf_restir_create builds."""

    def __init__(self, s, tris=None, geoms=None):
        self.geoms = s["geoms"] if geoms is None else geoms
        t = s["tris"] if tris is None else tris
        self.tris = np.zeros((0, 24), F) if t is None else np.ascontiguousarray(t, dtype=F).reshape(-1, 24)
        self.boxes = rm.padded_boxes(self.tris) if len(self.tris) else (None, None)
        ng = 0 if self.geoms is None else len(self.geoms)
        ids = [int(s["geom_ids"][k]) if s["geom_ids"] is not None else k for k in range(ng)]
        tri_ids = [] if s["tri_ids"] is None or not len(self.tris) else [int(i) for i in s["tri_ids"]]
        self.emit = np.zeros(max(ids + tri_ids + [-1]) + 1, F)
        seen = {}
        for k, i in enumerate(ids):
            e = max(F(self.geoms[k]["emittance"]), F(0))
            assert seen.setdefault(i, e) == e, f"id {i} names surfaces of differing emittance"
            self.emit[i] = e
        for i in tri_ids:
            assert seen.setdefault(i, F(0)) == 0, f"id {i} names surfaces of differing emittance"

    def emittance(self, gid):
        ok = (gid >= 0) & (gid < len(self.emit))
        return np.where(ok, self.emit[np.where(ok, gid, 0)] if len(self.emit) else F(0), F(0)).astype(F)

    def first_primitive_emittance(self, s, gid):
        """svgf_lights_draw_all's rule: the emittance of the first primitive whose id is geomId, 0 where none."""
        out, found = np.zeros(gid.shape, F), np.zeros(gid.shape, bool)
        for k in range(0 if self.geoms is None else len(self.geoms)):
            is_k = ~found & (gid == (int(s["geom_ids"][k]) if s["geom_ids"] is not None else k))
            out, found = _sel(is_k, F(self.geoms[k]["emittance"]), out), found | is_k
        return out


def occluded(sc, lt, j, u, v, pos):
    """bool[n]: row f16's shadow sample from pos (three arrays) towards the point (u, v) of light j - scene_shadow_model.visibility's
    statements with the light per point."""
    n = len(j)
    if n == 0:
        return np.zeros(0, bool)
    with np.errstate(all="ignore"):
        su, sv = (F(2.0) * u - F(1.0)).astype(F), (F(2.0) * v - F(1.0)).astype(F)
        L = [((lt["centre"][j, c] + (su * lt["edge_u"][j, c]).astype(F)).astype(F) + (sv * lt["edge_v"][j, c]).astype(F)).astype(F) for c in range(3)]
        q = [(L[c] - pos[c]).astype(F) for c in range(3)]
        dl = np.sqrt(_dot(q, q))
        ray = dl > 0
        d = [(q[c] / dl).astype(F) for c in range(3)]
        t_lo = (ssm.T_LO * _sel(dl > 1, dl, F(1))).astype(F)
        t_hi = (dl - t_lo).astype(F)
        occ = np.zeros(n, bool)
        for k in range(0 if sc.geoms is None else len(sc.geoms)):
            if F(sc.geoms[k]["emittance"]) != 0:
                continue
            hit, tw = ssm.primitive_test(sc.geoms[k], pos, d)
            occ |= hit & (tw > t_lo) & (tw < t_hi)
        for i in range(len(sc.tris)):
            go, t = ssm.triangle_test(sc.tris[i], pos, d)
            go &= (t > t_lo) & (t < t_hi)
            if not go.any():
                continue
            ok, tn = rm.slab(sc.boxes[0][i], sc.boxes[1][i], pos, d)
            occ |= go & ok & (t >= tn)
        return occ & ray


class _Res:
    def __init__(self, n):
        self.j = np.full(n, -1, np.int32)
        self.u, self.v, self.M, self.W, self.phat, self.w_sum = (np.zeros(n, F) for _ in range(6))

    @classmethod
    def stored(cls, rec):
        r = cls(len(rec))
        r.j, r.u, r.v, r.M, r.W, r.phat = (np.array(rec[k]) for k in ("j", "u", "v", "M", "W", "phat"))
        return r

    def pack(self, shape):
        out, e = np.zeros(len(self.j), RESERVOIR_DTYPE), self.j < 0
        out["j"] = np.where(e, -1, self.j)
        for k in ("u", "v", "W", "phat"):
            out[k] = _sel(e, F(0), getattr(self, k))
        out["M"] = self.M
        return out.reshape(shape)


def _update(r, mask, j, u, v, phat, w, M_s, xi):
    """update() of the header on the pixels of `mask`; returns where the sample was selected."""
    with np.errstate(all="ignore"):
        w = _sel(w > 0, w, F(0))
        before = r.w_sum.copy()
        r.w_sum = _sel(mask, (r.w_sum + w).astype(F), r.w_sum)
        r.M = _sel(mask, (r.M + M_s).astype(F), r.M)
        sel = mask & (w > 0) & ((before == 0) | ((xi * r.w_sum).astype(F) < w))
    r.j = np.where(sel, j, r.j).astype(np.int32)
    r.u, r.v, r.phat = _sel(sel, u, r.u), _sel(sel, v, r.v), _sel(sel, phat, r.phat)
    return sel


def _finish(r):
    with np.errstate(all="ignore"):
        r.W = _sel((r.j >= 0) & (r.phat > 0), (r.w_sum / (r.M * r.phat).astype(F)).astype(F), F(0))


def _take(s, mask, r):
    with np.errstate(all="ignore"):
        return _update(s, mask, r.j, r.u, r.v, r.phat, ((r.phat * r.W).astype(F) * r.M).astype(F), r.M, F(0))


def _phat_at(lt, r, nrm, pos):
    valid = (r.j >= 0) & (r.j < len(lt))
    return _sel(valid, lum(light_term(lt, np.where(valid, r.j, 0), nrm, pos)[0]), F(0))


def _take_at(s, mask, lt, r, Mq, xi, nrm, pos, stored_phat=False):
    with np.errstate(all="ignore"):
        phat = r.phat if stored_phat else _phat_at(lt, r, nrm, pos)
        return _update(s, mask, r.j, r.u, r.v, phat, ((phat * r.W).astype(F) * Mq).astype(F), Mq, xi)


def _planes(gb):
    nrm, pos = ([np.ascontiguousarray(gb[f][..., c]).reshape(-1) for c in range(3)] for f in ("normal", "position"))
    return nrm, pos, np.ascontiguousarray(gb["geomId"]).reshape(-1)


def history_tap(prev_gid, prev_n, motion, W, H, gid, nrm, surf, min_dot, alt=None):
    """The history tap of every pixel, as both libraries' first launch takes it: (q, on, id_ok, n_ok, acc) - the previous pixel the
    motion vector rounds to (0 where it is off the frame), and the masks a caller counts its events from: on a surface and on the frame,
    the id as before, the normal within min_dot, accepted.  alt: tap_rounds_down, temporal_no_id_test, temporal_no_normal_test."""
    with np.errstate(all="ignore"):
        mv = np.ascontiguousarray(motion, dtype=F).reshape(-1, 2)
        half = F(0.0) if alt == "tap_rounds_down" else F(0.5)
        fx, fy = np.floor((mv[:, 0] + half).astype(F)), np.floor((mv[:, 1] + half).astype(F))
        on = (fx >= 0) & (fx < F(W)) & (fy >= 0) & (fy < F(H))
        q = np.where(on, np.where(on, fy, 0).astype(np.int64) * W + np.where(on, fx, 0).astype(np.int64), 0)
        id_ok = prev_gid.reshape(-1)[q] == gid
        pn = prev_n.reshape(-1, 3)[q]
        n_ok = _dot(nrm, [pn[:, c] for c in range(3)]) >= min_dot
    on = on & surf
    return q, on, id_ok, n_ok, on & (id_ok | (alt == "temporal_no_id_test")) & (n_ok | (alt == "temporal_no_normal_test"))


def neighbour_tap(u_x, u_y, radius, W, H, gid, nrm, surf, min_dot, alt=None):
    """The neighbour every pixel picks from the uniforms (u_x, u_y), as both libraries' second launch does: (q, on, id_ok, n_ok, acc) -
    its index (0 where there is none) and the masks a caller counts its events from: on a surface, on the frame and not the pixel
    itself, the same id, the normal within min_dot, accepted.  alt: neighbour_may_be_self, spatial_no_id_test, spatial_no_normal_test."""
    x, y = np.tile(np.arange(W), H), np.repeat(np.arange(H), W)
    with np.errstate(all="ignore"):
        ox, oy = (np.floor(((((F(2.0) * u).astype(F) - F(1.0)).astype(F) * radius).astype(F) + F(0.5)).astype(F)).astype(np.int64) for u in (u_x, u_y))
        qx, qy = x + ox, y + oy
        on = surf & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
        if alt != "neighbour_may_be_self":
            on &= ~((ox == 0) & (oy == 0))
        q = np.where(on, qy * W + qx, 0)
        id_ok = gid[q] == gid
        n_ok = _dot(nrm, [nrm[c][q] for c in range(3)]) >= min_dot
    return q, on, id_ok, n_ok, on & (id_ok | (alt == "spatial_no_id_test")) & (n_ok | (alt == "spatial_no_normal_test"))


class State:
    """svgf_restir's planes for one frame size: H and T (RESERVOIR_DTYPE[H, W]), the previous normals and ids.  reset() is
    svgf_restir_reset; frame() both launches of svgf_restir_frame."""

    def __init__(self, sc, W, H):
        self.sc, self.W, self.Hh = sc, W, H
        self.H, self.T = np.zeros((H, W), RESERVOIR_DTYPE), np.zeros((H, W), RESERVOIR_DTYPE)
        self.prev_n, self.prev_gid = np.zeros((H, W, 3), F), np.zeros((H, W), np.int32)
        self.reset()

    def reset(self):
        self.H = np.zeros((self.Hh, self.W), RESERVOIR_DTYPE)
        self.H["j"] = -1
        self.prev_gid = np.full((self.Hh, self.W), -1, np.int32)

    def copy(self):
        c = State.__new__(State)
        c.sc, c.W, c.Hh = self.sc, self.W, self.Hh
        c.H, c.T, c.prev_n, c.prev_gid = self.H.copy(), self.T.copy(), self.prev_n.copy(), self.prev_gid.copy()
        return c

    def frame(self, gb, lt, rp, frame, seed, ambient=0.15, motion=None, alt=None):
        """(D float32[H, W, 3], counts dict over EVENTS) of one svgf_restir_frame; the state moves on as the device's does."""
        assert alt is None or alt in ALTS, alt
        W, H, sc = self.W, self.Hh, self.sc
        n, N, amb = W * H, len(lt), F(ambient)
        nrm, pos, gid = _planes(gb)
        emit = sc.emittance(gid)
        surf = (gid >= 0) & ~(emit > 0)
        hu = lambda k: synth.hash_uniform(seed, frame, n, k)       # noqa: E731
        cnt = dict.fromkeys(EVENTS, 0)
        with np.errstate(all="ignore"):
            # ---- launch 1 ----
            u, v = hu(8), hu(9)
            r = _Res(n)
            for c in range(rp["candidates"]):
                j = np.minimum((hu(4096 + c) * F(N)).astype(F).astype(np.int32), N - 1)
                phat = lum(light_term(lt, j, nrm, pos)[0])
                w = phat if alt == "no_source_pdf" else (phat * F(N)).astype(F)
                _update(r, surf, j, u, v, phat, w, F(1), hu(4128 + c))
            _finish(r)
            cast = surf & (r.j >= 0) & (r.W > 0)
            occ = np.zeros(n, bool)
            ix = np.flatnonzero(cast)
            occ[ix] = occluded(sc, lt, r.j[ix], r.u[ix], r.v[ix], [pos[c][ix] for c in range(3)])
            cnt["initial_occluded"] = int(occ.sum())
            if alt != "initial_ray_ignored":
                r.W = _sel(occ, F(0), r.W)
            s = _Res(n)
            _take(s, surf, r)
            from_history = np.zeros(n, bool)
            if rp["temporal"] and motion is not None:
                q, on, id_ok, n_ok, acc = history_tap(self.prev_gid, self.prev_n, motion, W, H, gid, nrm, surf, rp["normal_min_dot"], alt)
                cnt["tap_off_screen"] = int((surf & ~on).sum())
                cnt["tap_refused_id"] = int((on & ~id_ok).sum())
                cnt["tap_refused_normal"] = int((on & id_ok & ~n_ok).sum())
                cnt["tap_accepted"] = int(acc.sum())
                h = _Res.stored(self.H.reshape(-1)[q])
                cap = (rp["m_cap"] * r.M).astype(F)
                cnt["m_capped"] = int((acc & (h.M > cap)).sum())
                Mq = h.M if alt == "no_m_cap" else _sel(h.M < cap, h.M, cap)
                had = s.w_sum > 0
                from_history = _take_at(s, acc, lt, h, Mq, hu(4128 if alt == "history_stream_is_4128" else 4160), nrm, pos,
                                        stored_phat=alt == "history_phat_as_stored")
                cnt["history_selected"] = int((from_history & had).sum())
            _finish(s)
            self.T = s.pack((H, W))
            # ---- launch 2 ----
            t = _Res.stored(self.T.reshape(-1))
            s = _Res(n)
            _take(s, surf, t)
            reused = from_history & (t.j >= 0)
            for k in range(rp["neighbours"]):
                base = 4192 + 4 * k
                q, on, id_ok, n_ok, acc = neighbour_tap(hu(base), hu(base + 1), rp["radius"], W, H, gid, nrm, surf, rp["normal_min_dot"], alt)
                cnt["neighbour_refused_id"] += int((on & ~id_ok).sum())
                cnt["neighbour_refused_normal"] += int((on & id_ok & ~n_ok).sum())
                cnt["neighbour_accepted"] += int(acc.sum())
                tq = _Res.stored(self.T.reshape(-1)[q])
                had = s.w_sum > 0
                sel = _take_at(s, acc, lt, tq, tq.M, hu(base + 2), nrm, pos, stored_phat=alt == "neighbour_phat_as_stored")
                cnt["neighbour_selected"] += int((sel & had).sum())
                reused = np.where(sel, True, reused)
            _finish(s)
            lit = surf & (s.j >= 0) & (s.j < N)
            cnt["empty_shaded"] = int((surf & ~lit).sum())
            Fc, _ = light_term(lt, np.where(lit, s.j, 0), nrm, pos)
            cast = lit & (s.W > 0)
            occ = np.zeros(n, bool)
            ix = np.flatnonzero(cast)
            occ[ix] = occluded(sc, lt, s.j[ix], s.u[ix], s.v[ix], [pos[c][ix] for c in range(3)])
            cnt["final_occluded_after_reuse"] = int((occ & reused).sum())
            vis = _sel(occ & (alt != "final_ray_ignored"), F(0), F(1))
            D = [_sel(lit, (amb + (vis * (Fc[c] * s.W).astype(F)).astype(F)).astype(F), _sel(surf, amb, _sel(gid >= 0, emit, F(0)))) for c in range(3)]
        self.H = s.pack((H, W))
        self.prev_n = np.stack(nrm, -1).reshape(H, W, 3).copy()
        self.prev_gid = gid.reshape(H, W).copy()
        return np.ascontiguousarray(np.stack(D, -1).reshape(H, W, 3).astype(F)), cnt


def draw_all(sc, s, gb, lt, samples, frame, seed, ambient=0.15):
    """D float32[H, W, 3] of svgf_lights_draw_all, and vis float32[N, H, W] per light (1 where no ray is cast)."""
    H, W = gb["geomId"].shape
    n, amb = W * H, F(ambient)
    nrm, pos, gid = _planes(gb)
    emit = sc.first_primitive_emittance(s, gid)
    surf = (gid >= 0) & ~(emit > 0)
    acc = [np.zeros(n, F) for _ in range(3)]
    all_vis = np.ones((len(lt), n), F)
    with np.errstate(all="ignore"):
        for j in range(len(lt)):
            jj = np.full(n, j, np.int64)
            Fc, lam = light_term(lt, jj, nrm, pos)
            casts = surf & (lam > 0)                                         # lam == 0: no ray, the term is 0 whatever vis
            ix = np.flatnonzero(casts)
            unocc = np.zeros(len(ix), np.int32)
            for k in range(samples):
                u, v = synth.hash_uniform(seed, frame, n, 8 + 2 * k)[ix], synth.hash_uniform(seed, frame, n, 9 + 2 * k)[ix]
                unocc += ~occluded(sc, lt, jj[ix], u, v, [pos[c][ix] for c in range(3)])
            all_vis[j, ix] = (unocc.astype(F) / F(samples)).astype(F)
            acc = [_sel(casts, (acc[c] + (Fc[c] * all_vis[j]).astype(F)).astype(F), acc[c]) for c in range(3)]
        D = [_sel(surf, (amb + acc[c]).astype(F), _sel(gid >= 0, emit, F(0))) for c in range(3)]
    return np.ascontiguousarray(np.stack(D, -1).reshape(H, W, 3).astype(F)), all_vis.reshape(len(lt), H, W)
