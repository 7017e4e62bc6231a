"""numpy model of libsvgf_restir_gi.so (include/svgf_restir_gi.h, row f28), layered on tests/scene_trace_model.py (the bounce: its
directions, its brute-force nearest hit, the radiance L the hit sends back) and tests/scene_shadow_model.py (the occluder tests of the
visibility ray): both launches of svgf_restir_gi_frame from a G-buffer, float32 throughout, one rounding per operation, every
expression nested the way the kernels nest it.  A State carries H, T and the previous planes from frame to frame, as the device state
does, and every frame returns per-event counts.  Test infrastructure only.

`alt` names ONE deliberate deviation, in scene_model's manner: the model then computes what a kernel with that mistake would, and a
test counts the pixel records on which a case tells the two apart.
"""
import numpy as np

import resident_scene_model as rm
import restir_model as rsm
import scene_shadow_model as ssm
import scene_trace_model as stm
from restir_model import _planes, history_tap, lum, neighbour_tap
from scene_model import F, _dot, _sel, synth

ALTS = ("no_inverse_M", "no_jacobian", "no_jacobian_bounds", "g_as_stored", "refused_adds_M", "candidate_target_needs_g", "no_m_cap",
        "temporal_no_id_test", "temporal_no_normal_test", "tap_rounds_down", "history_stream_is_8192", "spatial_no_id_test",
        "spatial_no_normal_test", "neighbour_may_be_self", "final_ray_ignored", "own_sample_retested")
EVENTS = ("candidate_miss", "candidate_emitter", "tap_off_screen", "tap_refused_id", "tap_refused_normal", "tap_refused_invalid", "tap_refused_g",
          "tap_refused_J_low", "tap_refused_J_high", "tap_accepted", "m_capped", "foreign_selected", "final_ray_cast", "final_ray_occluded")
RESERVOIR_GI_DTYPE = np.dtype([("xs", F, 3), ("M", F), ("ns", F, 3), ("W", F), ("L", F, 3), ("phat", F), ("g", F), ("valid", np.int32),
                               ("zero", np.int32, 2)])


def params(candidates=1, temporal=1, m_cap=20.0, neighbours=3, radius=30.0, normal_min_dot=0.9, jacobian_max=10.0, ambient=0.15, shadow_secondary=1):
    return dict(candidates=int(candidates), temporal=int(temporal), m_cap=F(m_cap), neighbours=int(neighbours), radius=F(radius),
                normal_min_dot=F(normal_min_dot), jacobian_max=F(jacobian_max), ambient=F(ambient), shadow_secondary=int(shadow_secondary))


class Scene(rsm.Scene):
    """restir_model.Scene (occluders, padded boxes, the table from geomId to emittance) and what the bounce's nearest hit reads."""

    def __init__(self, s, tris=None, geoms=None):
        super().__init__(s, tris, geoms)
        self.s = s

    def nearest(self, o, d, t_lo):
        s = self.s
        return stm.nearest(o, d, t_lo, self.geoms, s["geom_ids"], self.tris if len(self.tris) else None, s["tri_ids"], s["tri_albedo"], s["tri_tex"],
                           s["textures"])


def t_lo_of(pos):
    m = np.maximum(np.maximum(np.abs(pos[0]), np.abs(pos[1])), np.abs(pos[2]))
    return (stm.T_LO * _sel(m > 1, m, F(1))).astype(F)


def geometry(xs, ns, nrm, pos):
    """g_p(xs, ns) at the pixels (pos, nrm): three arrays each."""
    with np.errstate(all="ignore"):
        v = [(xs[c] - pos[c]).astype(F) for c in range(3)]
        dist2 = _dot(v, v)
        dl = np.sqrt(dist2)
        wd = [(v[c] / dl).astype(F) for c in range(3)]
        cs = _dot(nrm, wd)
        cs = _sel(cs > 0, cs, F(0))
        cphi = (-_dot(ns, wd)).astype(F)
        cphi = _sel(cphi > 0, cphi, F(0))
        return ((cs * cphi).astype(F) / dist2).astype(F)


def bounce(sc, lt, gp, seed, frame, n_pixels, pix, nrm, pos):
    """Row f17's bounce samples c = 0 .. candidates - 1 of the pixels `pix` (nrm, pos: three arrays [len(pix)]): dict(xs, ns, L: three
    float32[J, n] each, hit, emitter bool[J, n]) - scene_trace_model.render's statements with the hit kept."""
    J, n = gp["candidates"], len(pix)
    with np.errstate(all="ignore"):
        d, _ = stm.directions(seed, frame, n_pixels, pix, nrm, J)
        o = [np.broadcast_to(pos[c][None, :], (J, n)).astype(F) for c in range(3)]
        t_lo = np.broadcast_to(t_lo_of(pos)[None, :], (J, n))
        h2 = sc.nearest(o, d, t_lo)
        hit = h2["gid"] >= 0
        em = hit & (h2["emit"] > 0)
        occ = np.zeros(hit.shape, bool)
        if gp["shadow_secondary"]:
            u = np.stack([synth.hash_uniform(seed, frame, n_pixels, 256 + 16 * j + 8)[pix] for j in range(J)]).astype(F)
            v = np.stack([synth.hash_uniform(seed, frame, n_pixels, 256 + 16 * j + 9)[pix] for j in range(J)]).astype(F)
            occ = stm.occluded(h2["pos"], u, v, sc.geoms, sc.tris if len(sc.tris) else None, lt) & hit & ~em
        lit = (_sel(occ, F(0), F(1)) * stm.direct_term([F(c) for c in lt["centre"]], h2["n"], h2["pos"])).astype(F)
        Lu = _sel(em, h2["emit"], (gp["ambient"] + lit).astype(F))
        L = [_sel(hit, (h2["alb"][c] * Lu).astype(F), F(0)) for c in range(3)]
    return dict(xs=h2["pos"], ns=h2["n"], L=L, hit=hit, emitter=em)


def visible(sc, pos, xs):
    """bool[n]: visible(pos, xs) of the header (three arrays each) - a brute force over every occluder."""
    n = len(pos[0])
    if n == 0:
        return np.zeros(0, bool)
    with np.errstate(all="ignore"):
        q = [(xs[c] - pos[c]).astype(F) for c in range(3)]
        dl = np.sqrt(_dot(q, q))
        ray = dl > 0
        d = [(q[c] / dl).astype(F) for c in range(3)]
        end = (stm.T_LO * _sel(dl > 1, dl, F(1))).astype(F)
        t_lo = t_lo_of(pos)
        t_hi = (dl - end).astype(F)
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
        return ~(occ & ray)


class _Res:
    def __init__(self, n):
        self.xs, self.ns, self.L = ([np.zeros(n, F) for _ in range(3)] for _ in range(3))
        self.g, self.M, self.W, self.phat, self.w_sum = (np.zeros(n, F) for _ in range(5))
        self.valid = np.zeros(n, bool)

    @classmethod
    def stored(cls, rec):
        r = cls(len(rec))
        for k in ("xs", "ns", "L"):
            setattr(r, k, [np.array(rec[k][:, c]) for c in range(3)])
        r.g, r.M, r.W, r.phat = (np.array(rec[k]) for k in ("g", "M", "W", "phat"))
        r.valid = np.array(rec["valid"]) != 0
        return r

    def pack(self, shape):
        out, v = np.zeros(len(self.g), RESERVOIR_GI_DTYPE), self.valid
        for k in ("xs", "ns", "L"):
            for c in range(3):
                out[k][:, c] = _sel(v, getattr(self, k)[c], F(0))
        for k in ("g", "W", "phat"):
            out[k] = _sel(v, getattr(self, k), F(0))
        out["M"], out["valid"] = self.M, v.astype(np.int32)
        return out.reshape(shape)


def _update(r, mask, xs, ns, L, g, phat, w, M_s, xi):
    """update() of the header on the pixels of `mask`; returns where the sample was selected."""
    with np.errstate(all="ignore"):
        w = _sel(w > 0, w, F(0))
        before = r.w_sum.copy()
        r.w_sum = _sel(mask, (r.w_sum + w).astype(F), r.w_sum)
        r.M = _sel(mask, (r.M + M_s).astype(F), r.M)
        sel = mask & (w > 0) & ((before == 0) | ((xi * r.w_sum).astype(F) < w))
    for c in range(3):
        r.xs[c], r.ns[c], r.L[c] = _sel(sel, xs[c], r.xs[c]), _sel(sel, ns[c], r.ns[c]), _sel(sel, L[c], r.L[c])
    r.g, r.phat, r.valid = _sel(sel, g, r.g), _sel(sel, phat, r.phat), r.valid | sel
    return sel


def _finish(r, alt=None):
    with np.errstate(all="ignore"):
        den = r.phat if alt == "no_inverse_M" else (r.M * r.phat).astype(F)
        r.W = _sel(r.valid & (r.phat > 0), (r.w_sum / den).astype(F), F(0))


def _restart(r, mask):
    """s = EMPTY; take(s, r, 0), in r's place (outside `mask` r is EMPTY and stays so)."""
    with np.errstate(all="ignore"):
        w = _sel(r.valid & mask, ((r.phat * r.W).astype(F) * r.M).astype(F), F(0))
        w = _sel(w > 0, w, F(0))
    r.w_sum, r.valid, r.W = w, w > 0, np.zeros(len(w), F)
    r.phat = _sel(r.valid, r.phat, F(0))


def _take_at(s, mask, r, Mq, xi, nrm, pos, gp, cnt, alt):
    """take'() of the header on the taps of `mask`; returns where the sample was selected."""
    with np.errstate(all="ignore"):
        g = geometry(r.xs, r.ns, nrm, pos)
        g_ok = (r.g > 0) & (g > 0)
        J = (g / r.g).astype(F)
        jmin = (F(1.0) / gp["jacobian_max"]).astype(F)
        lo_ok, hi_ok = J >= jmin, J <= gp["jacobian_max"]
        if alt == "no_jacobian_bounds":
            lo_ok, hi_ok = np.ones(len(g), bool), np.ones(len(g), bool)
        cnt["tap_refused_invalid"] += int((mask & ~r.valid).sum())
        cnt["tap_refused_g"] += int((mask & r.valid & ~g_ok).sum())
        cnt["tap_refused_J_low"] += int((mask & r.valid & g_ok & ~lo_ok).sum())
        cnt["tap_refused_J_high"] += int((mask & r.valid & g_ok & lo_ok & ~hi_ok).sum())
        ok = mask & r.valid & g_ok & lo_ok & hi_ok
        cnt["tap_accepted"] += int(ok.sum())
        phat = lum(r.L)
        w = (phat * r.W).astype(F)
        w = w if alt == "no_jacobian" else (w * J).astype(F)
        w = (w * Mq).astype(F)
        if alt == "refused_adds_M":
            s.M = _sel(mask & ~ok, (s.M + Mq).astype(F), s.M)
        return _update(s, ok, r.xs, r.ns, r.L, r.g if alt == "g_as_stored" else g, phat, w, Mq, xi)


class State:
    """svgf_restir_gi's planes for one frame size: H and T (RESERVOIR_GI_DTYPE[H, W]), the previous normals and ids.  reset() is
    svgf_restir_gi_reset; frame() both launches of svgf_restir_gi_frame."""

    def __init__(self, sc, W, H):
        self.sc, self.W, self.Hh = sc, W, H
        self.H, self.T = np.zeros((H, W), RESERVOIR_GI_DTYPE), np.zeros((H, W), RESERVOIR_GI_DTYPE)
        self.prev_n, self.prev_gid = np.zeros((H, W, 3), F), np.zeros((H, W), np.int32)
        self.reset()

    def reset(self):
        self.H = np.zeros((self.Hh, self.W), RESERVOIR_GI_DTYPE)
        self.prev_gid = np.full((self.Hh, self.W), -1, np.int32)

    def frame(self, gb, lt, gp, frame, seed, motion=None, alt=None):
        """(I float32[H, W, 3], counts dict over EVENTS) of one svgf_restir_gi_frame; the state moves on as the device's does.
        lt: scene_shadow_model.light's dict (centre and edges are read)."""
        assert alt is None or alt in ALTS, alt
        W, H, sc = self.W, self.Hh, self.sc
        n = W * H
        nrm, pos, gid = _planes(gb)
        surf = (gid >= 0) & ~(sc.emittance(gid) > 0)
        hu = lambda k: synth.hash_uniform(seed, frame, n, k)       # noqa: E731
        cnt = dict.fromkeys(EVENTS, 0)
        with np.errstate(all="ignore"):
            # ---- launch 1 ----
            pix = np.flatnonzero(surf)
            r = _Res(n)
            if len(pix):
                b = bounce(sc, lt, gp, seed, frame, n, pix, [nrm[c][pix] for c in range(3)], [pos[c][pix] for c in range(3)])
                cnt["candidate_miss"] = int((~b["hit"]).sum())
                cnt["candidate_emitter"] = int(b["emitter"].sum())
                for c in range(gp["candidates"]):
                    full = lambda a: _scatter(n, pix, a[c])          # noqa: E731
                    xs, ns, L = ([full(b[k][j]) for j in range(3)] for k in ("xs", "ns", "L"))
                    g = geometry(xs, ns, nrm, pos)
                    phat = lum(L)
                    w = _sel(g > 0, phat, F(0)) if alt == "candidate_target_needs_g" else phat
                    _update(r, surf, xs, ns, L, g, w, w, F(1), hu(8192 + c))
            _finish(r, alt)
            _restart(r, surf)
            s = r
            foreign1 = np.zeros(n, bool)
            if gp["temporal"] and motion is not None:
                q, on, id_ok, n_ok, acc = history_tap(self.prev_gid, self.prev_n, motion, W, H, gid, nrm, surf, gp["normal_min_dot"], alt)
                cnt["tap_off_screen"] = int((surf & ~on).sum())
                cnt["tap_refused_id"] += int((on & ~id_ok).sum())
                cnt["tap_refused_normal"] += int((on & id_ok & ~n_ok).sum())
                h = _Res.stored(self.H.reshape(-1)[q])
                cap = (gp["m_cap"] * s.M).astype(F)
                cnt["m_capped"] = int((acc & h.valid & (h.M > cap)).sum())
                Mq = h.M if alt == "no_m_cap" else _sel(h.M < cap, h.M, cap)
                foreign1 = _take_at(s, acc, h, Mq, hu(8192 if alt == "history_stream_is_8192" else 8224), nrm, pos, gp, cnt, alt)
            _finish(s, alt)
            self.T = s.pack((H, W))
            # ---- launch 2 ----
            s = _Res.stored(self.T.reshape(-1))
            _restart(s, surf)
            foreign = np.zeros(n, bool)
            for k in range(gp["neighbours"]):
                base = 8256 + 4 * k
                q, on, id_ok, n_ok, acc = neighbour_tap(hu(base), hu(base + 1), gp["radius"], W, H, gid, nrm, surf, gp["normal_min_dot"], alt)
                cnt["tap_refused_id"] += int((on & ~id_ok).sum())
                cnt["tap_refused_normal"] += int((on & id_ok & ~n_ok).sum())
                tq = _Res.stored(self.T.reshape(-1)[q])
                foreign |= _take_at(s, acc, tq, tq.M, hu(base + 2), nrm, pos, gp, cnt, alt)
            _finish(s, alt)
            cnt["foreign_selected"] = int(foreign1.sum()) + int(foreign.sum())
            cast = s.valid & (s.W > 0) & (foreign | (alt == "own_sample_retested"))
            ix = np.flatnonzero(cast)
            occ = np.zeros(n, bool)
            occ[ix] = ~visible(sc, [pos[c][ix] for c in range(3)], [s.xs[c][ix] for c in range(3)])
            cnt["final_ray_cast"], cnt["final_ray_occluded"] = len(ix), int(occ.sum())
            vis = _sel(occ & (alt != "final_ray_ignored"), F(0), F(1))
            I = [_sel(s.valid, (vis * (s.L[c] * s.W).astype(F)).astype(F), F(0)) for c in range(3)]      # noqa: E741
        self.H = s.pack((H, W))
        self.prev_n = np.stack(nrm, -1).reshape(H, W, 3).copy()
        self.prev_gid = gid.reshape(H, W).copy()
        return np.ascontiguousarray(np.stack(I, -1).reshape(H, W, 3).astype(F)), cnt


def _scatter(n, pix, a):
    out = np.zeros(n, F)
    out[pix] = a
    return out
