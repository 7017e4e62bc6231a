"""numpy model of svgf_virtual_draw and svgf_virtual_draw_split (include/svgf_virtual.h, row f21), layered on tests/scene_gloss_model.py
as that one is on the path model: colour, D, I and the first hit's G-buffer are scene_gloss_model.render's, untouched; what this file adds
is the header's GUIDE chain - scene_gloss_model.vertex with the substituted u, scene_trace_model's brute-force nearest hit, the length
L of the chain - as ONE numpy pass per chain step over the pixels still in the chain, and the texel a virtual hit writes.  float32
throughout, one rounding per operation, every expression nested the way the kernel nests it.  Test infrastructure only.

The nearest-hit rule reports a distance (SceneHit::t_best) that scene_trace_model.nearest does not return, so `hit_distance` below
repeats that function's search for the distance alone, from the same per-primitive and per-triangle functions; `guide` checks on every
ray that the hit it finds is the one `nearest` reports.

`alt` names ONE deliberate deviation, in scene_gloss_model's manner.
"""
import numpy as np

import resident_scene_model as rm
import scene_gloss_model as gm
import scene_model as sm
import scene_trace_model as stm
from scene_model import F, _dot, _sel, synth

ALTS = ("position_not_unfolded", "length_without_t0", "guide_reads_the_paths_stream", "origin_not_moved", "id_offset_ignored",
        "partial_mirrors_followed", "albedo_from_the_virtual_hit")
EVENTS = ("mirror", "transmission", "tir", "end_diffuse", "end_emitter", "miss", "cap")
MAX_CHAIN = 8
MAX_ID_OFFSET = 1 << 24


def params(max_chain=4, id_offset=0):
    return dict(max_chain=int(max_chain), id_offset=int(id_offset))


def hit_distance(o, d, t_lo_prim, t_lo_tri, geoms, tris):
    """(t float32, tri int64) per ray (o, d: three arrays each): the distance of the nearest hit (inf: a miss) as the nearest-hit rule
    reports it - a primitive's world-space distance beyond t_lo_prim, replaced by a nearer gated triangle's t beyond t_lo_tri - and the
    triangle's index (-1: a primitive or a miss).  scene_trace_model.nearest's search, for the distance alone."""
    shape = d[0].shape
    n_geoms = 0 if geoms is None else len(geoms)
    tris = np.zeros((0, 24), F) if tris is None else np.ascontiguousarray(tris, dtype=F).reshape(-1, 24)
    with np.errstate(all="ignore"):
        bt = np.full(shape, np.inf, F)
        for k in range(n_geoms):
            hit, tw, _, _ = stm._primitive(geoms[k], o, d)
            bt = _sel(hit & (tw > t_lo_prim) & (tw < bt), tw, bt)
        best = np.full(shape, -1, np.int64)
        lo, hi = rm.padded_boxes(tris) if len(tris) else (None, None)
        for i in range(len(tris)):
            go, _, _, t = stm._triangle(tris[i], o, d)
            go &= (t > t_lo_tri) & (t < bt)
            if not go.any():
                continue
            ok, tn = rm.slab(lo[i], hi[i], o, d)
            go &= ok & (t >= tn)
            bt, best = _sel(go, t, bt), np.where(go, i, best)
    return bt, best


def guide(W, H, frame, cam, geoms, geom_ids, tris, tri_ids, tri_albedo, tri_tex, textures, tab, gb, w_d, emitter, vp, seed=1, pixel_length=None, *,
          alt=None):
    """The header's guide chain on the first-hit G-buffer `gb` (GBUFFER_DTYPE[H, W]) with the first hits' diffuse share w_d and emitter
    mask: dict(chain int32[H, W], normal, position float32[H, W, 3], geomId int32[H, W] - the fields a virtual hit replaces, the first
    hit's elsewhere -, albedo float32[H, W, 3] of the virtual hit (what `albedo_from_the_virtual_hit` writes), seen float32[H, W, 3]:
    the virtual hit's own world position (NaN without one), length float32[H, W]: L, t0, events: a dict of EVENTS per chain step)."""
    K, off = vp["max_chain"], vp["id_offset"]
    assert 1 <= K <= MAX_CHAIN and 0 <= off <= MAX_ID_OFFSET
    n_pixels = W * H
    tri_id_set = gm.tri_id_set(tri_ids)
    gid0 = gb["geomId"].reshape(-1)
    runs = (gid0 >= 0) & ~emitter.reshape(-1) & ((w_d.reshape(-1) < 1) if alt == "partial_mirrors_followed" else (w_d.reshape(-1) == 0))
    pix = np.flatnonzero(runs)
    out = dict(chain=np.zeros(n_pixels, np.int32), normal=gb["normal"].reshape(-1, 3).copy(), position=gb["position"].reshape(-1, 3).copy(),
               geomId=gid0.copy(), albedo=gb["albedo"].reshape(-1, 3).copy(), seen=np.full((n_pixels, 3), np.nan, F),
               length=np.zeros(n_pixels, F), t0=np.zeros(n_pixels, F), events=[])
    o_cam = [F(c) for c in np.asarray(cam["position"], dtype=F)]
    with np.errstate(all="ignore"):
        d0 = [c.reshape(-1)[pix] for c in sm.rays(W, H, cam, pixel_length)]
        o0 = [np.full(len(pix), c, F) for c in o_cam]
        t0, _ = hit_distance(o0, d0, F(1e-4), F(0), geoms, tris)
        out["t0"][pix] = t0
        L = np.zeros(len(pix), F) if alt == "length_without_t0" else t0.copy()
        x, n, alb = ([gb[f].reshape(-1, 3)[pix, c].copy() for c in range(3)] for f in ("position", "normal", "albedo"))
        d = [c.copy() for c in d0]
        gid = gid0[pix].copy()
        inside = np.zeros(len(pix), bool)
        alive = np.ones(len(pix), bool)
        chain = np.zeros(len(pix), np.int32)
        for v in range(0, K + 1):
            ev = dict.fromkeys(EVENTS, 0)
            out["events"].append(ev)
            idx = np.flatnonzero(alive)
            if not len(idx):
                continue
            xs, ns, ds = ([a[c][idx] for c in range(3)] for a in (x, n, d))
            gs = gid[idx]
            tri = np.isin(gs, tri_id_set)
            reflect, refract, _, _ = gm._surface(tab, gs)
            glass = (refract > 0) & ~tri
            follows = (reflect > 0) if alt == "partial_mirrors_followed" else (reflect >= 1)
            u = _sel(~glass & follows, F(0), F(1))
            if alt == "guide_reads_the_paths_stream":
                u = synth.hash_uniform(seed, frame, n_pixels, 139 + 128 * v)[pix[idx]]
            V = gm.vertex(tab, gs, tri, ds, ns, u, inside[idx])
            spec = V["specular"]
            inside[idx] = V["inside"]
            ends = ~spec                                                 # the virtual hit
            capped = spec & (v == K)
            chain[idx] = np.where(ends, v, np.where(capped, -v, chain[idx]))
            ev["end_diffuse"], ev["cap"] = int(ends.sum()), int(capped.sum())
            go = spec & ~capped
            ev["mirror"], ev["transmission"], ev["tir"] = int((V["mirror"] & go).sum()), int((V["moved"] & go).sum()), int((V["tir"] & go).sum())
            alive[idx] = go
            if not go.any():
                continue
            # the ray that leaves vertex v (computed for every element, used where `go`)
            mx = np.maximum(np.maximum(np.abs(xs[0]), np.abs(xs[1])), np.abs(xs[2]))
            t_lo = (stm.T_LO * _sel(mx > 1, mx, F(1))).astype(F)
            back = (-(gm.ORIGIN_FACTOR * t_lo).astype(F)).astype(F)
            moved = V["moved"] & (alt != "origin_not_moved")
            o = [_sel(moved, (xs[c] + (back * V["nn"][c]).astype(F)).astype(F), xs[c]) for c in range(3)]
            dd = V["dn"]
            h = stm.nearest(o, dd, t_lo, geoms, geom_ids, tris, tri_ids, tri_albedo, tri_tex, textures)
            t, _ = hit_distance(o, dd, t_lo, t_lo, geoms, tris)
            assert ((h["gid"] >= 0) == np.isfinite(t))[go].all(), "hit_distance and scene_trace_model.nearest disagree on a miss"
            hit = go & (h["gid"] >= 0)
            miss = go & ~hit
            em = hit & (h["emit"] > 0)
            on = hit & ~em
            ev["miss"], ev["end_emitter"] = int(miss.sum()), int(em.sum())
            chain[idx] = np.where(miss, -(v + 1), np.where(em, v + 1, chain[idx]))
            L[idx] = _sel(hit, (L[idx] + t).astype(F), L[idx])
            for c in range(3):
                x[c][idx], n[c][idx] = _sel(hit, h["pos"][c], x[c][idx]), _sel(hit, h["n"][c], n[c][idx])
                alb[c][idx], d[c][idx] = _sel(hit, h["alb"][c], alb[c][idx]), _sel(hit, dd[c], d[c][idx])
            gid[idx] = np.where(hit, h["gid"], gid[idx])
            alive[idx] = on
        assert not alive.any()
        virt = chain > 0
        vi = pix[virt]
        out["chain"][pix] = chain
        out["length"][pix] = L
        for c in range(3):
            unfolded = (o_cam[c] + (L * d0[c]).astype(F)).astype(F)
            out["normal"][vi, c] = n[c][virt]
            out["position"][vi, c] = (x[c] if alt == "position_not_unfolded" else unfolded)[virt]
            out["albedo"][vi, c] = alb[c][virt]
            out["seen"][vi, c] = x[c][virt]
        out["geomId"][vi] = gid[virt] + (0 if alt == "id_offset_ignored" else off)
    for k in ("chain", "geomId", "length", "t0"):
        out[k] = out[k].reshape(H, W)
    for k in ("normal", "position", "albedo", "seen"):
        out[k] = out[k].reshape(H, W, 3)
    return out


def render(W, H, frame, cam, geoms, geom_ids, tris, tri_ids, tri_albedo, tri_tex, textures, lt, pp, tab=None, vp=None, seed=1, noise=0.6,
           fireflies=0.02, pixel_length=None, *, alt=None, first=None, emitters=None, emittance=None, base=None):
    """(colour, gbuffer, D, I, chain int32[H, W], info) of svgf_virtual_draw / svgf_virtual_draw_split: `base` (or a fresh
    scene_gloss_model.render with these arguments) with the guide's texels in its G-buffer.  info is the gloss model's plus
    guide = the dict `guide` returns and first_gb = the first hit's G-buffer."""
    assert alt is None or alt in ALTS, alt
    vp = params() if vp is None else vp
    if base is None:
        base = gm.render(W, H, frame, cam, geoms, geom_ids, tris, tri_ids, tri_albedo, tri_tex, textures, lt, pp, tab, seed=seed, noise=noise,
                         fireflies=fireflies, pixel_length=pixel_length, first=first, emitters=emitters, emittance=emittance)
    col, gb0, D, I, ginfo = base                                         # noqa: E741
    g = guide(W, H, frame, cam, geoms, geom_ids, tris, tri_ids, tri_albedo, tri_tex, textures, tab, gb0, ginfo["w_d"], ginfo["emitter"], vp, seed=seed,
              pixel_length=pixel_length, alt=alt)
    gb = gb0.copy()
    gb["normal"], gb["position"], gb["geomId"] = g["normal"], g["position"], g["geomId"]
    if alt == "albedo_from_the_virtual_hit":
        gb["albedo"] = g["albedo"]
    info = dict(ginfo, guide=g, first_gb=gb0)
    return col, gb, D, I, g["chain"], info


def total(g, event):
    return sum(e[event] for e in g["events"])
