"""numpy model of svgf_scene_draw_shadowed (include/svgf.h, row f16), layered on tests/scene_model.py: the first-hit planes are
scene_model.render's, then the header's rule as a BRUTE FORCE over all occluders - every primitive that does not emit and every
triangle with its gate (tests/resident_scene_model.py's padded box and slab test), no tree.  float32 throughout, one rounding per
operation, every expression nested the way the kernel nests it.  The (pixel, sample) pairs that cast a ray are flattened into one
axis, so a scene costs (primitives + triangles) array passes whatever `samples` is.  Test infrastructure only.

`alt` names ONE deliberate deviation, in scene_model's manner ("each edge acts"): the model then computes what a kernel with that
mistake would, and a test counts the pixels on which a scene tells the two apart.
"""
import numpy as np

import resident_scene_model as rm
import scene_model as sm
from scene_model import F, _apply34, _dot, _normalise, _sel, synth

ALTS = ("ungated", "no_cull", "nearest_primitive_only", "emitter_occludes", "no_t_lo", "t_hi_is_dl", "hash_streams_0_1",
        "light_from_centre_only")
T_LO = F(2.0 ** -10)


def light(centre, edge_u=(0, 0, 0), edge_v=(0, 0, 0), samples=1):
    return dict(centre=tuple(float(c) for c in centre), edge_u=tuple(float(c) for c in edge_u), edge_v=tuple(float(c) for c in edge_v),
                samples=int(samples))


def primitive_test(g, o, d):
    """scene_primitive_test of csrc/svgf_scene_pixel.inc.h for origins o and directions d (three arrays each): (hit, tw).  The
    arithmetic is scene_model.render's primitives loop; the normal is left out (the shadow rays do not use it)."""
    inv, xf = np.asarray(g["inv"], dtype=F), np.asarray(g["xf"], dtype=F)
    qo = _apply34(inv, o, 1.0)
    qd = _normalise(_apply34(inv, d, 0.0))
    if int(g["type"]) == sm.CUBE:
        tmin, tmax = np.full(o[0].shape, -1e38, F), np.full(o[0].shape, 1e38, F)
        for ax in range(3):
            t1, t2 = ((F(-0.5) - qo[ax]) / qd[ax]).astype(F), ((F(0.5) - qo[ax]) / qd[ax]).astype(F)
            ta, tb = _sel(t1 < t2, t1, t2), _sel(t1 > t2, t1, t2)           # glm::min / glm::max, see scene_model's docstring
            tmin = _sel((ta > 0) & (ta > tmin), ta, tmin)
            tmax = _sel(tb < tmax, tb, tmax)
        hit = (tmax >= tmin) & (tmax > 0)
        tt = _sel(tmin <= 0, tmax, tmin)
    else:
        b = _dot(qo, qd)
        rad = (b * b - (_dot(qo, qo) - F(0.25))).astype(F)
        sq = np.sqrt(_sel(rad > 0, rad, F(0)))
        ta, tb = (-b + sq).astype(F), (-b - sq).astype(F)
        both_pos, both_neg = (ta > 0) & (tb > 0), (ta < 0) & (tb < 0)
        tt = _sel(both_pos, _sel(tb < ta, tb, ta), _sel(ta < tb, tb, ta))
        hit = (rad >= 0) & ~both_neg
    po = [(qo[c] + tt * qd[c]).astype(F) for c in range(3)]
    pw = _apply34(xf, po, 1.0)
    dv = [(o[c] - pw[c]).astype(F) for c in range(3)]
    return hit, np.sqrt(_dot(dv, dv))


def triangle_test(T, o, d, cull=True):
    """scene_tri_test on one triangle (24 floats) for origins o and directions d (three arrays each): (accepted, t); t may be <= 0."""
    e1, e2 = [F(T[8 + c] - T[c]) for c in range(3)], [F(T[16 + c] - T[c]) for c in range(3)]
    pv = [(d[1] * e2[2] - e2[1] * d[2]).astype(F), (d[2] * e2[0] - e2[2] * d[0]).astype(F), (d[0] * e2[1] - e2[0] * d[1]).astype(F)]
    det = _dot(e1, pv)
    go = ~(det < sm.EPS) if cull else ~(np.abs(det) < sm.EPS)
    f = (F(1) / det).astype(F)
    sv = [(o[c] - T[c]).astype(F) for c in range(3)]
    bx = (f * _dot(sv, pv)).astype(F)
    go &= ~((bx < 0) | (bx > 1))
    q = [(sv[1] * e1[2] - e1[1] * sv[2]).astype(F), (sv[2] * e1[0] - e1[2] * sv[0]).astype(F), (sv[0] * e1[1] - e1[0] * sv[1]).astype(F)]
    by = (f * _dot(d, q)).astype(F)
    go &= ~((by < 0) | ((by + bx).astype(F) > 1))
    t = (f * _dot(e2, q)).astype(F)
    return go, t


def emitter_mask(W, H, cam, geoms, geom_ids, tris, tri_ids, pixel_length=None):
    """[H, W] bool: the first hit is a primitive with emittance > 0.  scene_model.render decides the hit; the albedo it returns is
    replaced by a flag (albedo plays no part in which surface wins)."""
    if geoms is None or not len(geoms):
        return np.zeros((H, W), bool)
    flag = np.array(geoms, copy=True)
    flag["albedo"] = (np.asarray(geoms["emittance"]) > 0).astype(F)[:, None]
    n = 0 if tris is None else len(tris)
    _, gb = sm.render(W, H, 0, cam, flag, geom_ids, tris, tri_ids, np.zeros((n, 3), F) if n else None, None, None, (0.0, 0.0, 0.0),
                      pixel_length=pixel_length)
    return gb["albedo"][..., 0] > 0


def visibility(W, H, frame, seed, position, cast, geoms, tris, lt, *, alt=None):
    """unoccluded int[H, W] (samples where no ray is cast) and the per-(pixel, sample) planes the tests look at:
    dict(occluded bool[S, n], ungated_differs int, pixels int[n] (flat pixel index of column j), dl float32[S, n])."""
    assert alt is None or alt in ALTS, alt
    S = int(lt["samples"])
    centre, eu, ev = ([F(c) for c in lt[k]] for k in ("centre", "edge_u", "edge_v"))
    pix = np.flatnonzero(cast.reshape(-1))
    pos = [np.broadcast_to(position.reshape(-1, 3)[pix, c][None, :], (S, len(pix))).astype(F) for c in range(3)]
    n_geoms = 0 if geoms is None else len(geoms)
    tris = np.zeros((0, 24), F) if tris is None else np.ascontiguousarray(tris, dtype=F).reshape(-1, 24)
    with np.errstate(all="ignore"):
        k0 = 0 if alt == "hash_streams_0_1" else 8
        u = np.stack([synth.hash_uniform(seed, frame, W * H, k0 + 2 * s)[pix] for s in range(S)]).astype(F)
        v = np.stack([synth.hash_uniform(seed, frame, W * H, k0 + 1 + 2 * s)[pix] for s in range(S)]).astype(F)
        su, sv = (F(2.0) * u - F(1.0)).astype(F), (F(2.0) * v - F(1.0)).astype(F)
        if alt == "light_from_centre_only":
            L = [np.full(su.shape, centre[c], F) for c in range(3)]
        else:
            L = [((centre[c] + (su * eu[c]).astype(F)).astype(F) + (sv * ev[c]).astype(F)).astype(F) for c in range(3)]
        q = [(L[c] - pos[c]).astype(F) for c in range(3)]
        dl = np.sqrt(_dot(q, q))
        ray = dl > 0
        d = [(q[c] / dl).astype(F) for c in range(3)]
        t_lo_true = (T_LO * _sel(dl > 1, dl, F(1))).astype(F)              # fmaxf(1, dl) on a number
        t_hi = dl if alt == "t_hi_is_dl" else (dl - t_lo_true).astype(F)
        t_lo = np.zeros_like(dl) if alt == "no_t_lo" else t_lo_true
        occ = np.zeros(dl.shape, bool)
        occ_ungated = np.zeros(dl.shape, bool)
        if alt == "nearest_primitive_only":         # what scene_primitives would report: the nearest hit beyond 1e-4, emitters included
            tb, eb = np.full(dl.shape, np.inf, F), np.zeros(dl.shape, F)
            for k in range(n_geoms):
                hit, tw = primitive_test(geoms[k], pos, d)
                take = hit & (tw > F(1e-4)) & (tw < tb)
                tb, eb = _sel(take, tw, tb), _sel(take, F(geoms[k]["emittance"]), eb)
            occ |= np.isfinite(tb) & (eb == 0) & (tb > t_lo) & (tb < t_hi)
        else:
            for k in range(n_geoms):
                if F(geoms[k]["emittance"]) != 0 and alt != "emitter_occludes":
                    continue
                hit, tw = primitive_test(geoms[k], pos, d)
                occ |= hit & (tw > t_lo) & (tw < t_hi)
        occ_ungated |= occ
        lo, hi = rm.padded_boxes(tris) if len(tris) else (None, None)
        for i in range(len(tris)):
            go, t = triangle_test(tris[i], pos, d, cull=alt != "no_cull")
            go &= (t > t_lo) & (t < t_hi)
            if not go.any():
                continue
            occ_ungated |= go
            ok, tn = rm.slab(lo[i], hi[i], pos, d)
            occ |= go & ok & (t >= tn)
        occ &= ray
        occ_ungated &= ray
    use = occ_ungated if alt == "ungated" else occ
    unocc = np.full(W * H, S, np.int32)
    unocc[pix] = (~use).sum(axis=0).astype(np.int32)
    return unocc.reshape(H, W), dict(occluded=use, ungated_differs=int((occ != occ_ungated).sum()), pixels=pix, dl=dl)


def render(W, H, frame, cam, geoms, geom_ids, tris, tri_ids, tri_albedo, tri_tex, textures, lt, seed=1, noise=0.6, fireflies=0.02,
           pixel_length=None, *, alt=None, first=None, emitters=None):
    """(color float32[H, W, 3], gbuffer, info) of svgf_scene_draw_shadowed.  `first` = scene_model.render's result for the same
    arguments with light = lt["centre"] (computed when not given; never written to), `emitters` = emitter_mask's.  info: vis
    float32[H, W], cast bool[H, W] and visibility's dict."""
    if first is None:
        first = sm.render(W, H, frame, cam, geoms, geom_ids, tris, tri_ids, tri_albedo, tri_tex, textures, lt["centre"], seed=seed, noise=noise,
                          fireflies=fireflies, pixel_length=pixel_length)
    if emitters is None:
        emitters = emitter_mask(W, H, cam, geoms, geom_ids, tris, tri_ids, pixel_length)
    col0, gb = first
    cast = (gb["geomId"] >= 0) & ~emitters
    unocc, info = visibility(W, H, frame, seed, gb["position"], cast, geoms, tris, lt, alt=alt)
    with np.errstate(all="ignore"):
        vis = (unocc.astype(F) / F(lt["samples"])).astype(F)
        n, pos, alb = ([gb[f][..., c] for c in range(3)] for f in ("normal", "position", "albedo"))
        centre = [F(c) for c in lt["centre"]]
        tl = [(centre[c] - pos[c]).astype(F) for c in range(3)]
        dist2 = _dot(tl, tl)
        dl = np.sqrt(dist2)
        lam = _dot([(tl[c] / dl).astype(F) for c in range(3)], n)
        lam = _sel(lam > 0, lam, F(0))
        shade = (F(0.15) + (vis * ((F(30.0) * lam).astype(F) / (F(4.0) + dist2).astype(F)).astype(F)).astype(F)).astype(F)
        hu = lambda k: synth.hash_uniform(seed, frame, W * H, k).reshape(H, W)              # noqa: E731
        mult = (F(1.0) + F(noise) * (F(2.0) * hu(0) - F(1.0)).astype(F)).astype(F)
        mult = _sel(hu(1) < F(fireflies), (mult * F(6.0)).astype(F), mult)
        amp = F(F(0.1) * F(noise))
        col = [_sel(cast, (((alb[c] * shade).astype(F) * mult).astype(F) * (F(1.0) + amp * (hu(2 + c) - F(0.5)).astype(F)).astype(F)).astype(F),
                    col0[..., c]) for c in range(3)]
    info.update(vis=vis, cast=cast)
    return np.ascontiguousarray(np.stack(col, -1).astype(F)), gb, info
