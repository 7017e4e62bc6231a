"""numpy model of svgf_trace_draw (include/svgf_trace.h, row f17), layered on tests/scene_model.py (the first hit) and
tests/scene_shadow_model.py (its shadow rays): then the header's bounce as a BRUTE FORCE - every primitive and every triangle with
its gate for the nearest hit of each bounce ray, every occluder for its shadow ray, no tree.  float32 throughout, one rounding per
operation, every expression nested the way the kernel nests it.  The (pixel, bounce sample) pairs are flattened into one axis
([J, n] arrays), so a scene costs (primitives + triangles) array passes whatever bounce_samples is.  Test infrastructure only.

`alt` names ONE deliberate deviation, in scene_model's manner: the model then computes what a kernel with that mistake would, and a
test counts the pixels on which a scene tells the two apart.
"""
import numpy as np

import resident_scene_model as rm
import scene_model as sm
import scene_shadow_model as ssm
from scene_model import F, _apply34, _dot, _normalise, _sel, synth

ALTS = ("uniform_hemisphere", "first_try_only", "no_t_lo", "ungated", "nearest_primitive_only", "no_secondary_shadow",
        "no_ambient_at_secondary", "emitter_dark", "streams_from_0")
T_LO = F(2.0 ** -10)
MAX_BOUNCE_SAMPLES = 8


def params(bounce_samples=1, ambient=0.15, shadow_secondary=1):
    return dict(bounce_samples=int(bounce_samples), ambient=float(ambient), shadow_secondary=int(shadow_secondary))


def frame_of(n):
    """The branch-free frame (Duff et al. 2017) of normals n (three arrays): (T, B), three arrays each."""
    with np.errstate(all="ignore"):
        s = np.copysign(F(1), n[2]).astype(F)
        q = (F(-1) / (s + n[2]).astype(F)).astype(F)
        w = ((n[0] * n[1]).astype(F) * q).astype(F)
        T = [(F(1) + (((s * n[0]).astype(F) * n[0]).astype(F) * q).astype(F)).astype(F), (s * w).astype(F), (-(s * n[0]).astype(F)).astype(F)]
        B = [w, (s + ((n[1] * n[1]).astype(F) * q).astype(F)).astype(F), (-n[1]).astype(F)]
    return T, B


def directions(seed, frame, n_pixels, pix, n, J, *, alt=None):
    """Bounce directions of pixels `pix` (flat indices into a frame of n_pixels) with normals n (three arrays [len(pix)]):
    (d: three float32[J, len(pix)], fallback bool[J, len(pix)] = none of the four pairs fell inside the disc)."""
    T, B = frame_of(n)
    d, fb = [[], [], []], []
    with np.errstate(all="ignore"):
        for j in range(J):
            base = (0 if alt == "streams_from_0" else 256) + 16 * j
            da, db, found = np.zeros(len(pix), F), np.zeros(len(pix), F), np.zeros(len(pix), bool)
            for k in range(1 if alt == "first_try_only" else 4):
                ak = (F(2.0) * synth.hash_uniform(seed, frame, n_pixels, base + 2 * k)[pix] - F(1.0)).astype(F)
                bk = (F(2.0) * synth.hash_uniform(seed, frame, n_pixels, base + 2 * k + 1)[pix] - F(1.0)).astype(F)
                take = ~found & (((ak * ak).astype(F) + (bk * bk).astype(F)).astype(F) < F(1.0))
                da, db, found = _sel(take, ak, da), _sel(take, bk, db), found | take
            s2 = ((da * da).astype(F) + (db * db).astype(F)).astype(F)
            one = (F(1.0) - s2).astype(F)
            if alt == "uniform_hemisphere":         # Shirley's uniform map of the disc: the pdf no longer cancels the Lambert factor
                k = np.sqrt((F(2.0) - s2).astype(F))
                da, db, cz = (da * k).astype(F), (db * k).astype(F), one
            else:
                cz = np.sqrt(_sel(one > 0, one, F(0)))                      # fmaxf(0, .) on a number
            v = _normalise([(((da * T[c]).astype(F) + (db * B[c]).astype(F)).astype(F) + (cz * n[c]).astype(F)).astype(F) for c in range(3)])
            for c in range(3):
                d[c].append(v[c])
            fb.append(~found)
    return [np.stack(d[c]) for c in range(3)], np.stack(fb)


def _primitive(g, o, d):
    """scene_primitive_test of csrc/svgf_scene_pixel.inc.h for origins o and directions d (three arrays each): (hit, tw, nw, pw);
    the arithmetic of scene_model.render's primitives loop."""
    inv, xf, invT = (np.asarray(g[f], dtype=F) for f in ("inv", "xf", "invT"))
    shape = d[0].shape
    qo = _apply34(inv, o, 1.0)
    qd = _normalise(_apply34(inv, d, 0.0))
    if int(g["type"]) == sm.CUBE:
        tmin, tmax = np.full(shape, -1e38, F), np.full(shape, 1e38, F)
        amin, amax = np.zeros(shape, np.int32), np.zeros(shape, np.int32)
        for ax in range(3):
            t1, t2 = ((F(-0.5) - qo[ax]) / qd[ax]).astype(F), ((F(0.5) - qo[ax]) / qd[ax]).astype(F)
            ta, tb = _sel(t1 < t2, t1, t2), _sel(t1 > t2, t1, t2)           # glm::min / glm::max, see scene_model's docstring
            up = (ta > 0) & (ta > tmin)
            tmin, amin = _sel(up, ta, tmin), np.where(up, ax, amin)
            dn = tb < tmax
            tmax, amax = _sel(dn, tb, tmax), np.where(dn, ax, amax)
        hit = (tmax >= tmin) & (tmax > 0)
        inside = tmin <= 0
        tt = _sel(inside, tmax, tmin)
        axis = np.where(inside, amax, amin)
        qda = _sel(axis == 0, qd[0], _sel(axis == 1, qd[1], qd[2]))
        sgn = _sel(qda < 0, F(1), F(-1))
        no = [_sel(axis == c, sgn, F(0)) for c in range(3)]
        nw = _normalise(_apply34(xf, no, 0.0))
    else:
        b = _dot(qo, qd)
        rad = (b * b - (_dot(qo, qo) - F(0.25))).astype(F)
        sq = np.sqrt(_sel(rad > 0, rad, F(0)))
        ta, tb = (-b + sq).astype(F), (-b - sq).astype(F)
        both_pos, both_neg = (ta > 0) & (tb > 0), (ta < 0) & (tb < 0)
        tt = _sel(both_pos, _sel(tb < ta, tb, ta), _sel(ta < tb, tb, ta))
        hit = (rad >= 0) & ~both_neg
        po = [(qo[c] + tt * qd[c]).astype(F) for c in range(3)]
        nw = _normalise([((invT[3 * r] * po[0] + invT[3 * r + 1] * po[1]) + invT[3 * r + 2] * po[2]).astype(F) for r in range(3)])
    po = [(qo[c] + tt * qd[c]).astype(F) for c in range(3)]
    pw = _apply34(xf, po, 1.0)
    dv = [(o[c] - pw[c]).astype(F) for c in range(3)]
    return hit, np.sqrt(_dot(dv, dv)), nw, pw


def _triangle(T, o, d):
    """scene_tri_test on one triangle (24 floats): (accepted, bx, by, t); t may be <= 0."""
    e1, e2 = [F(T[8 + c] - T[c]) for c in range(3)], [F(T[16 + c] - T[c]) for c in range(3)]
    pv = [(d[1] * e2[2] - e2[1] * d[2]).astype(F), (d[2] * e2[0] - e2[2] * d[0]).astype(F), (d[0] * e2[1] - e2[0] * d[1]).astype(F)]
    det = _dot(e1, pv)
    go = ~(det < sm.EPS)
    f = (F(1) / det).astype(F)
    sv = [(o[c] - T[c]).astype(F) for c in range(3)]
    bx = (f * _dot(sv, pv)).astype(F)
    go &= ~((bx < 0) | (bx > 1))
    q = [(sv[1] * e1[2] - e1[1] * sv[2]).astype(F), (sv[2] * e1[0] - e1[2] * sv[0]).astype(F), (sv[0] * e1[1] - e1[0] * sv[1]).astype(F)]
    by = (f * _dot(d, q)).astype(F)
    go &= ~((by < 0) | ((by + bx).astype(F) > 1))
    t = (f * _dot(e2, q)).astype(F)
    return go, bx, by, t


def nearest(o, d, t_lo, geoms, geom_ids, tris, tri_ids, tri_albedo, tri_tex, textures, *, ungated=False):
    """The nearest hit beyond t_lo of the rays (o, d) (three arrays each, one shape): dict(gid, n, pos, alb, emit, ungated_differs).
    The primary ray's rule (scene_model.render plus row f14's gate) with t_lo in place of its lower bounds."""
    shape = d[0].shape
    n_geoms = 0 if geoms is None else len(geoms)
    tris = np.zeros((0, 24), F) if tris is None else np.ascontiguousarray(tris, dtype=F).reshape(-1, 24)
    full = lambda v, dt=F: np.full(shape, v, dtype=dt)      # noqa: E731
    with np.errstate(all="ignore"):
        t_best, gid = full(np.inf), full(-1, np.int32)
        n, ph, alb = [full(0) for _ in range(3)], [full(0) for _ in range(3)], [full(0) for _ in range(3)]
        emit = full(0)
        for k in range(n_geoms):
            g = geoms[k]
            hit, tw, nw, pw = _primitive(g, o, d)
            take = hit & (tw > t_lo) & (tw < t_best)
            t_best = _sel(take, tw, t_best)
            gid = np.where(take, np.int32(k if geom_ids is None else geom_ids[k]), gid).astype(np.int32)
            for c in range(3):
                n[c], ph[c], alb[c] = _sel(take, nw[c], n[c]), _sel(take, pw[c], ph[c]), _sel(take, F(g["albedo"][c]), alb[c])
            emit = _sel(take, F(g["emittance"]), emit)
        # two triangle searches side by side, so that the gate's effect can be counted: the contract's and the ungated one
        best, bt, bbx, bby = full(-1, np.int64), t_best.copy(), full(0), full(0)
        best_u, bt_u, bbx_u, bby_u = full(-1, np.int64), t_best.copy(), full(0), full(0)
        lo, hi = rm.padded_boxes(tris) if len(tris) else (None, None)
        for i in range(len(tris)):
            go, bx, by, t = _triangle(tris[i], o, d)
            go &= t > t_lo
            go_u = go & (t < bt_u)
            go_g = go & (t < bt)
            if not (go_u.any() or go_g.any()):
                continue
            bt_u, best_u, bbx_u, bby_u = _sel(go_u, t, bt_u), np.where(go_u, i, best_u), _sel(go_u, bx, bbx_u), _sel(go_u, by, bby_u)
            if go_g.any():
                ok, tn = rm.slab(lo[i], hi[i], o, d)
                go_g &= ok & (t >= tn)
                bt, best, bbx, bby = _sel(go_g, t, bt), np.where(go_g, i, best), _sel(go_g, bx, bbx), _sel(go_g, by, bby)
        differs = int((best != best_u).sum())
        if ungated:
            best, bt, bbx, bby = best_u, bt_u, bbx_u, bby_u
        if len(tris):
            mesh = best >= 0
            bi = np.maximum(best, 0)
            T = [tris[bi, j] for j in range(24)]
            w2 = ((F(1) - bbx) - bby).astype(F)
            wn, wu = (bbx, bby, w2), (w2, bbx, bby)
            nt = _normalise([((T[3 + c] * wn[0] + T[11 + c] * wn[1]) + T[19 + c] * wn[2]).astype(F) for c in range(3)])
            ta_ = np.asarray(tri_albedo, dtype=F).reshape(-1, 3)
            at = [ta_[bi, c] for c in range(3)]
            if tri_tex is not None and textures is not None and len(textures):
                tx = np.asarray(tri_tex, dtype=np.int32)[bi]
                u = ((T[6] * wu[0] + T[14] * wu[1]) + T[22] * wu[2]).astype(F)
                v = ((T[7] * wu[0] + T[15] * wu[1]) + T[23] * wu[2]).astype(F)
                for k, tex in enumerate(textures):
                    tex = np.asarray(tex, dtype=np.uint8)
                    th, tw_ = tex.shape[0], tex.shape[1]
                    fx, fy = ((F(1) * F(tw_)) * u).astype(F), ((F(1) * F(th)) * (F(1) - v)).astype(F)
                    cx, cy = F(F(1) * F(tw_) - F(1)), F(F(1) * F(th) - F(1))
                    fx, fy = _sel(fx < cx, fx, cx), _sel(fy < cy, fy, cy)
                    X, Y = np.trunc(_sel(fx < 0, F(0), fx)).astype(np.int64), np.trunc(_sel(fy < 0, F(0), fy)).astype(np.int64)
                    px = tex[np.clip(Y, 0, th - 1), np.clip(X, 0, tw_ - 1)]
                    for c in range(3):
                        at[c] = _sel(tx == k, F(0.003921568627) * px[..., c].astype(F), at[c])
            for c in range(3):
                n[c], ph[c], alb[c] = _sel(mesh, nt[c], n[c]), _sel(mesh, (o[c] + bt * d[c]).astype(F), ph[c]), _sel(mesh, at[c], alb[c])
            emit = _sel(mesh, F(0), emit)
            gid = np.where(mesh, np.asarray(tri_ids, dtype=np.int32)[bi], gid).astype(np.int32)
    return dict(gid=gid, n=n, pos=ph, alb=alb, emit=emit, ungated_differs=differs)


def occluded(pos, u, v, geoms, tris, lt, *, nearest_primitive_only=False):
    """One shadow ray of svgf_scene_draw_shadowed's rule per element, from pos (three arrays) towards the light point of the hash
    values (u, v): bool array."""
    centre, eu, ev = ([F(c) for c in lt[k]] for k in ("centre", "edge_u", "edge_v"))
    n_geoms = 0 if geoms is None else len(geoms)
    tris = np.zeros((0, 24), F) if tris is None else np.ascontiguousarray(tris, dtype=F).reshape(-1, 24)
    with np.errstate(all="ignore"):
        su, sv = (F(2.0) * u - F(1.0)).astype(F), (F(2.0) * v - F(1.0)).astype(F)
        L = [((centre[c] + (su * eu[c]).astype(F)).astype(F) + (sv * ev[c]).astype(F)).astype(F) for c in range(3)]
        q = [(L[c] - pos[c]).astype(F) for c in range(3)]
        dl = np.sqrt(_dot(q, q))
        d = [(q[c] / dl).astype(F) for c in range(3)]
        t_lo = (T_LO * _sel(dl > 1, dl, F(1))).astype(F)
        t_hi = (dl - t_lo).astype(F)
        occ = np.zeros(dl.shape, bool)
        if nearest_primitive_only:
            tb, eb = np.full(dl.shape, np.inf, F), np.zeros(dl.shape, F)
            for k in range(n_geoms):
                hit, tw = ssm.primitive_test(geoms[k], pos, d)
                take = hit & (tw > F(1e-4)) & (tw < tb)
                tb, eb = _sel(take, tw, tb), _sel(take, F(geoms[k]["emittance"]), eb)
            return np.isfinite(tb) & (eb == 0) & (tb > t_lo) & (tb < t_hi) & (dl > 0)
        for k in range(n_geoms):
            if F(geoms[k]["emittance"]) != 0:
                continue
            hit, tw = ssm.primitive_test(geoms[k], pos, d)
            occ |= hit & (tw > t_lo) & (tw < t_hi)
        lo, hi = rm.padded_boxes(tris) if len(tris) else (None, None)
        for i in range(len(tris)):
            go, t = ssm.triangle_test(tris[i], pos, d)
            go &= (t > t_lo) & (t < t_hi)
            if not go.any():
                continue
            ok, tn = rm.slab(lo[i], hi[i], pos, d)
            occ |= go & ok & (t >= tn)
        return occ & (dl > 0)


def direct_term(centre, n, pos):
    """scene_direct: (30 lam) / (4 + dist2) at pos with normal n towards centre."""
    with np.errstate(all="ignore"):
        tl = [(F(centre[c]) - pos[c]).astype(F) for c in range(3)]
        dist2 = _dot(tl, tl)
        dl = np.sqrt(dist2)
        lam = _dot([(tl[c] / dl).astype(F) for c in range(3)], n)
        lam = _sel(lam > 0, lam, F(0))
        return ((F(30.0) * lam).astype(F) / (F(4.0) + dist2).astype(F)).astype(F)


def render(W, H, frame, cam, geoms, geom_ids, tris, tri_ids, tri_albedo, tri_tex, textures, lt, tp, seed=1, noise=0.6, fireflies=0.02,
           pixel_length=None, *, alt=None, first=None, emitters=None):
    """(color float32[H, W, 3], gbuffer, info) of svgf_trace_draw.  `first` = scene_model.render's result for the same arguments with
    light = lt["centre"] (computed when not given; never written to), `emitters` = scene_shadow_model.emitter_mask's.  info: vis,
    cast, ind float32[H, W, 3] (0 where no bounce is cast), pixels int[n], hit bool[J, n], emitter_hit bool[J, n], fallback
    bool[J, n], ungated_differs int (bounce rays whose nearest triangle the gate changes), d (three float32[J, n])."""
    assert alt is None or alt in ALTS, alt
    J, ambient, sec = int(tp["bounce_samples"]), F(tp["ambient"]), int(tp["shadow_secondary"])
    assert 0 <= J <= MAX_BOUNCE_SAMPLES and sec in (0, 1)
    if first is None:
        first = sm.render(W, H, frame, cam, geoms, geom_ids, tris, tri_ids, tri_albedo, tri_tex, textures, lt["centre"], seed=seed, noise=noise,
                          fireflies=fireflies, pixel_length=pixel_length)
    if emitters is None:
        emitters = ssm.emitter_mask(W, H, cam, geoms, geom_ids, tris, tri_ids, pixel_length)
    col0, gb = first
    cast = (gb["geomId"] >= 0) & ~emitters
    unocc, vinfo = ssm.visibility(W, H, frame, seed, gb["position"], cast, geoms, tris, lt)
    pix = np.flatnonzero(cast.reshape(-1))
    centre = [F(c) for c in lt["centre"]]
    info = dict(cast=cast, pixels=pix, ungated_differs=0)
    with np.errstate(all="ignore"):
        vis = (unocc.astype(F) / F(lt["samples"])).astype(F)
        n, pos, alb = ([gb[f][..., c] for c in range(3)] for f in ("normal", "position", "albedo"))
        shade0 = (ambient + (vis * direct_term(centre, n, pos)).astype(F)).astype(F)
        shade = [shade0, shade0, shade0]
        ind = np.zeros((H, W, 3), F)
        if J > 0 and len(pix):
            np_, pp = [n[c].reshape(-1)[pix] for c in range(3)], [pos[c].reshape(-1)[pix] for c in range(3)]
            d, fallback = directions(seed, frame, W * H, pix, np_, J, alt=alt)
            o = [np.broadcast_to(pp[c][None, :], (J, len(pix))).astype(F) for c in range(3)]
            m = np.maximum(np.maximum(np.abs(pp[0]), np.abs(pp[1])), np.abs(pp[2]))
            t_lo = np.broadcast_to((T_LO * _sel(m > 1, m, F(1))).astype(F)[None, :], (J, len(pix)))
            h2 = nearest(o, d, np.zeros_like(t_lo) if alt == "no_t_lo" else t_lo, geoms, geom_ids, tris, tri_ids, tri_albedo, tri_tex, textures,
                         ungated=alt == "ungated")
            hit = h2["gid"] >= 0
            em = hit & (h2["emit"] > 0)
            occ = np.zeros(hit.shape, bool)
            if sec and alt != "no_secondary_shadow":
                k0 = 0 if alt == "streams_from_0" else 256
                u = np.stack([synth.hash_uniform(seed, frame, W * H, k0 + 16 * j + 8)[pix] for j in range(J)]).astype(F)
                v = np.stack([synth.hash_uniform(seed, frame, W * H, k0 + 16 * j + 9)[pix] for j in range(J)]).astype(F)
                occ = occluded(h2["pos"], u, v, geoms, tris, lt, nearest_primitive_only=alt == "nearest_primitive_only") & hit & ~em
            vis2 = _sel(occ, F(0), F(1))
            lit = (vis2 * direct_term(centre, h2["n"], h2["pos"])).astype(F)
            L = lit if alt == "no_ambient_at_secondary" else (ambient + lit).astype(F)
            L = _sel(em, F(0) if alt == "emitter_dark" else h2["emit"], L)
            shade = []
            for c in range(3):
                acc = np.zeros(len(pix), F)
                for j in range(J):
                    acc = (acc + _sel(hit[j], (h2["alb"][c][j] * L[j]).astype(F), F(0))).astype(F)
                ind_c = (acc / F(J)).astype(F)
                ind.reshape(-1, 3)[pix, c] = ind_c
                full = shade0.copy().reshape(-1)
                full[pix] = (shade0.reshape(-1)[pix] + ind_c).astype(F)
                shade.append(full.reshape(H, W))
            info.update(hit=hit, emitter_hit=em, fallback=fallback, ungated_differs=h2["ungated_differs"], d=d, secondary_occluded=occ,
                        hit_gid=h2["gid"])
        hu = lambda k: synth.hash_uniform(seed, frame, W * H, k).reshape(H, W)              # noqa: E731
        mult = (F(1.0) + F(noise) * (F(2.0) * hu(0) - F(1.0)).astype(F)).astype(F)
        mult = _sel(hu(1) < F(fireflies), (mult * F(6.0)).astype(F), mult)
        amp = F(F(0.1) * F(noise))
        col = [_sel(cast, (((alb[c] * shade[c]).astype(F) * mult).astype(F) * (F(1.0) + amp * (hu(2 + c) - F(0.5)).astype(F)).astype(F)).astype(F),
                    col0[..., c]) for c in range(3)]
    info.update(vis=vis, ind=ind, shadow=vinfo)
    return np.ascontiguousarray(np.stack(col, -1).astype(F)), gb, info
