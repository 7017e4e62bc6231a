"""numpy model of svgf_gloss_draw and svgf_gloss_draw_split (include/svgf_gloss.h, row f20), layered on tests/scene_path_model.py as
that one is on the trace model: the first hit, its shadow rays and its term are scene_trace_model.render's with no bounce; every ray
behind it is that file's sampler (`directions`), its brute-force nearest hit (`nearest`), its shadow ray (`occluded`) and its light
term (`direct_term`); streams move by scene_path_model.stream_seed.  What the draw adds is the header's vertex: its class (diffuse,
mirror, glass) from the surface table, the direction a specular vertex sends the path on in, the `inside` bit, the moved origin of a
transmitted ray, and the first term weighted by the first hit's diffuse share.  The vertex (`vertex`) and the vertex loop (`paths`) are
tests/scene_vertex_model.py's, shared with the rough and the highlight models; this file holds the surface table and `render`, which
hands that loop its `rough`, `hp`, `alt` and `keep_rays` by argument: a render is a function of its arguments alone.  float32
throughout, one rounding per operation, every expression nested the way the kernel nests it.  Test infrastructure only.

A hit is a TRIANGLE hit when its id is one of tri_ids (an object is a mesh or a primitive, never both).

Events, per vertex in info["events"], counted where a ray leaves the vertex: mirror0 / glass0 (the class of the first hit), mirror
(behind it), enter / exit (a transmitted ray into / out of glass), fresnel_reflect, tir, partial_diffuse / partial_mirror (0 < reflect < 1
decided the class), exit_found (a ray that entered an object found that object again).

`alt` names ONE deliberate deviation, in scene_path_model's manner.
"""
import numpy as np

import scene_model as sm
import scene_path_model as spm
import scene_shadow_model as ssm
import scene_split_model as splm
import scene_trace_model as stm
from scene_model import F, _sel
from scene_vertex_model import GLOSS_EVENTS as EVENTS
from scene_vertex_model import ORIGIN_FACTOR, SURFACE_DTYPE, _surface, paths, tri_id_set, vertex      # noqa: F401  (re-exported)

ALTS = ("inside_from_dot_sign", "eta_not_inverted", "spec_on_transmission", "gather_at_mirror", "first_unweighted",
        "lobe_stream_is_roulette_stream", "origin_not_moved", "glass_on_triangles")


def table(n, **entries):
    """A surface table of n diffuse records (ior 1) with entries {id: (reflect, refract, ior, spec)} set; keys are given as g<id>."""
    t = np.zeros(n, SURFACE_DTYPE)
    t["ior"] = F(1.0)
    for k, (reflect, refract, ior, spec) in entries.items():
        t[int(k[1:])] = (reflect, refract, ior, spec)
    return t


def render(W, H, frame, cam, geoms, geom_ids, tris, tri_ids, tri_albedo, tri_tex, textures, lt, pp, tab=None, seed=1, noise=0.6, fireflies=0.02,
           pixel_length=None, *, alt=None, first=None, emitters=None, emittance=None, keep_rays=False, rough=None, hp=None, alts=ALTS):
    """(colour float32[H, W, 3], gbuffer, D, I, info) of svgf_gloss_draw / svgf_gloss_draw_split with surface table `tab` (SURFACE_DTYPE
    records, or None).  `first`, `emitters` and `emittance` as scene_path_model.render's.  info: cast, vis, pixels, w_d, first
    (first', float32[H, W]), ind, acc, depth, hit_gid, events (a dict of EVENTS per vertex).  `rough` and `hp` are the loop's roughness
    table and highlight block (scene_rough_model.render and scene_highlight_model.render pass theirs, with their own `alts` for the
    names `alt` may take)."""
    assert alt is None or alt in alts, alt
    J, K, R, ambient, sec = pp["paths"], pp["max_depth"], pp["rr_depth"], F(pp["ambient"]), pp["shadow_secondary"]
    assert 0 <= J <= spm.MAX_PATHS and 1 <= K <= spm.MAX_DEPTH and 0 <= R <= spm.MAX_DEPTH and sec in (0, 1)
    if first is None:
        first = sm.render(W, H, frame, cam, geoms, geom_ids, tris, tri_ids, tri_albedo, tri_tex, textures, lt["centre"], seed=seed, noise=noise,
                          fireflies=fireflies, pixel_length=pixel_length)
    if emitters is None:
        emitters = ssm.emitter_mask(W, H, cam, geoms, geom_ids, tris, tri_ids, pixel_length)
    if emittance is None:
        emittance = splm.emittance_plane(W, H, cam, geoms, geom_ids, tris, tri_ids, pixel_length)
    col0, gb, base = stm.render(W, H, frame, cam, geoms, geom_ids, tris, tri_ids, tri_albedo, tri_tex, textures, lt, stm.params(0, ambient, sec),
                                seed=seed, noise=noise, fireflies=fireflies, pixel_length=pixel_length, first=first, emitters=emitters)
    cast, vis, pix = base["cast"], base["vis"], base["pixels"]
    hit = gb["geomId"] >= 0
    emitter = hit & (emittance > 0)
    info = dict(cast=cast, vis=vis, pixels=pix, depth=[], hit_gid=[], events=[dict.fromkeys(EVENTS, 0) for _ in range(K + 1)])
    with np.errstate(all="ignore"):
        nrm, pos, alb = ([gb[f][..., c] for c in range(3)] for f in ("normal", "position", "albedo"))
        reflect, refract, _, _ = _surface(tab, gb["geomId"])
        glass0 = (refract > 0) & ~np.isin(gb["geomId"], tri_id_set(tri_ids))
        w_d = _sel(glass0, F(0), (F(1) - reflect).astype(F))
        if alt == "first_unweighted":
            w_d = np.ones_like(w_d)
        shade0 = (ambient + (vis * stm.direct_term([F(c) for c in lt["centre"]], nrm, pos)).astype(F)).astype(F)
        first_w = _sel(w_d != 0, (w_d * shade0).astype(F), F(0))
        mult, chroma = splm.modulation(W, H, frame, seed, noise, fireflies)
        ind = np.zeros((H, W, 3), F)
        shade = [first_w, first_w, first_w]
        if J > 0 and len(pix):
            flat = lambda a: [a[c].reshape(-1)[pix] for c in range(3)]            # noqa: E731
            d0 = sm.rays(W, H, cam, pixel_length)
            acc, pinfo = paths(W, H, frame, seed, pix, flat(nrm), flat(pos), flat(d0), gb["geomId"].reshape(-1)[pix], flat(alb), tab, geoms, geom_ids,
                               tris, tri_ids, tri_albedo, tri_tex, textures, lt, pp, rough=rough, hp=hp, alt=alt, keep_rays=keep_rays)
            info.update(pinfo, acc=acc)
            shade = []
            for c in range(3):
                s = np.zeros(len(pix), F)
                for j in range(J):
                    s = (s + acc[c][j]).astype(F)
                ind_c = (s / F(J)).astype(F)
                ind.reshape(-1, 3)[pix, c] = ind_c
                sh = first_w.copy().reshape(-1)
                sh[pix] = (first_w.reshape(-1)[pix] + ind_c).astype(F)
                shade.append(sh.reshape(H, W))
        col = [_sel(cast, (((alb[c] * shade[c]).astype(F) * mult).astype(F) * chroma[c]).astype(F), col0[..., c]) for c in range(3)]
        col = np.ascontiguousarray(np.stack(col, -1).astype(F))
        first_term = _sel(emitter, emittance, first_w)
        D = [_sel(hit, ((first_term * mult).astype(F) * chroma[c]).astype(F), F(0)) for c in range(3)]
        bounced = cast & (J > 0)
        I = [_sel(bounced, ((ind[..., c] * mult).astype(F) * chroma[c]).astype(F), F(0)) for c in range(3)]      # noqa: E741
    info.update(ind=ind, w_d=w_d, first=first_w, emit=emittance, emitter=emitter)
    return col, gb, np.ascontiguousarray(np.stack(D, -1)), np.ascontiguousarray(np.stack(I, -1)), info


def total(info, event, from_vertex=0):
    return sum(e[event] for e in info["events"][from_vertex:])
