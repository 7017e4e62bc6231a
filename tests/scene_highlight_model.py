"""numpy model of svgf_highlight_draw and svgf_highlight_draw_split (include/svgf_highlight.h, row f23), layered on
tests/scene_rough_model.py as that one is on the virtual model.  What the draw adds is the header's light term at ROUGH vertices:
`factor` (H, in the header's order) along `light_direction` (the unit direction and the distance of a shadow sample's light point),
gathered at the rough vertices behind the first hit, and the deterministic term of the first hit, which makes first' per channel.
The two functions and the vertex loop that gathers are tests/scene_vertex_model.py's; `render` is scene_rough_model.render handed the
highlight block (it reaches that loop by argument), then rewrites colour and D (nothing else) on the pixels whose first hit is rough.
float32 throughout, one rounding per operation, every expression nested the way the kernel nests it.  Test infrastructure only.

Events, info["highlight"]: first (shadow samples of a rough first hit that the highlight evaluates), deeper (rough vertices behind the
first hit that gather), occluded (such a sample found occluded), backfacing (a formed, unoccluded sample with l_n <= 0), clamped (the
clamp lowered a contributing H), no_ray (!(dl > 0), or without shadow_secondary an l that is not a number).  info["H_max"]: the largest
unclamped contributing H of the frame.

`alt` names ONE deliberate deviation, in scene_rough_model's manner, and shares the loop's namespace with the names of that file and
of scene_gloss_model.
"""
import numpy as np

import scene_gloss_model as gm
import scene_model as sm
import scene_rough_model as rm
import scene_split_model as splm
import scene_trace_model as stm
from scene_model import F, synth
from scene_vertex_model import HIGHLIGHT_EVENTS as EVENTS
from scene_vertex_model import _channel, _contribution, _dot_dt, _norm_dt, _surface, alpha_of, light_direction, tri_id_set
from scene_vertex_model import factor      # noqa: F401  (re-exported)

ALTS = ("light_centre_for_l", "height_correlated_g", "first_highlight_into_indirect", "divided_by_reflect", "shadow_streams_swapped",
        "clamp_per_channel_after_spec")
assert not set(ALTS) & set(rm.ALTS + gm.ALTS), "one vertex loop honours all three files' names"


def params(enable=1, clamp=0.0):
    return dict(enable=int(enable), clamp=float(clamp))


def first_hit(W, H, frame, cam, geoms, tris, tri_ids, lt, tab, rough, hp, gb0, cast, seed=1, pixel_length=None, *, alt=None):
    """The first hit's term: (flat indices of the pixels whose first hit is rough for the highlight, hl: three float32 arrays over
    them = (reflect spec_c) hm, events, H_max)."""
    ev, hmax = dict.fromkeys(EVENTS, 0), [0.0]
    centre = [F(c) for c in lt["centre"]]
    S = int(lt["samples"])
    with np.errstate(all="ignore"):
        gid0 = gb0["geomId"]
        reflect, refract, _, spec = _surface(tab, gid0)
        glass0 = (refract > 0) & ~np.isin(gid0, tri_id_set(tri_ids))
        alpha0 = alpha_of(rough, gid0)
        d0 = sm.rays(W, H, cam, pixel_length)
        nrm, pos = ([gb0[f][..., c] for c in range(3)] for f in ("normal", "position"))
        v_n = _dot_dt([(-d0[c]).astype(F) for c in range(3)], nrm)
        is_rough = cast & ~glass0 & (reflect > 0) & (alpha0 > 0) & (v_n > 0) & bool(hp["enable"])
        p = np.flatnonzero(is_rough.reshape(-1))
        if not len(p):
            return p, [np.zeros(0, F) for _ in range(3)], ev, 0.0
        flat = lambda a: [a[c].reshape(-1)[p] for c in range(3)]            # noqa: E731
        xp, np_, dp, ap = flat(pos), flat(nrm), flat(d0), alpha0.reshape(-1)[p]
        hsum = np.zeros(len(p), F)
        per_channel = [np.zeros(len(p), F) for _ in range(3)]               # alt clamp_per_channel_after_spec only
        for s in range(S):
            u = synth.hash_uniform(seed, frame, W * H, 8 + 2 * s)[p]
            v = synth.hash_uniform(seed, frame, W * H, 9 + 2 * s)[p]
            l, dl = light_direction(xp, u, v, lt)                          # noqa: E741
            occ = stm.occluded(xp, u, v, geoms, tris, lt)
            if alt == "light_centre_for_l":
                l = _norm_dt([(centre[c] - xp[c]).astype(F) for c in range(3)])        # noqa: E741
            c_s, _ = _contribution(ev, hmax, ap, dp, np_, xp, l, dl > 0, occ, centre, hp, alt)
            ev["first"] += len(p)
            hsum = (hsum + c_s).astype(F)
            for c in range(3):
                per_channel[c] = (per_channel[c] + _channel(spec[c].reshape(-1)[p], c_s, hp, alt)).astype(F)
        hm = (hsum / F(S)).astype(F)
        rf = reflect.reshape(-1)[p]
        if alt == "clamp_per_channel_after_spec" and hp["clamp"] > 0:
            hl = [(rf * (per_channel[c] / F(S)).astype(F)).astype(F) for c in range(3)]
        elif alt == "divided_by_reflect":
            hl = [(spec[c].reshape(-1)[p] * hm).astype(F) for c in range(3)]
        else:
            hl = [((rf * spec[c].reshape(-1)[p]).astype(F) * hm).astype(F) for c in range(3)]
    return p, hl, ev, hmax[0]


def render(W, H, frame, cam, geoms, geom_ids, tris, tri_ids, tri_albedo, tri_tex, textures, lt, pp, tab=None, vp=None, rough=None, guide_alpha=0.0, hp=None,
           seed=1, noise=0.6, fireflies=0.02, pixel_length=None, *, alt=None, first=None, emitters=None, emittance=None, keep_rays=False):
    """(colour, gbuffer, D, I, chain int32[H, W], info) of svgf_highlight_draw / svgf_highlight_draw_split with hp = params().  info is
    scene_rough_model.render's plus highlight (EVENTS over the frame), H_max, first_rough (flat pixel indices) and first_hl."""
    assert alt is None or alt in ALTS, alt
    hp = params() if hp is None else hp
    assert hp["enable"] in (0, 1) and np.isfinite(hp["clamp"]) and hp["clamp"] >= 0
    col, gb, D, I, chain, info = rm.render(W, H, frame, cam, geoms, geom_ids, tris, tri_ids, tri_albedo, tri_tex, textures, lt, pp, tab, vp, rough,      # noqa: E741
                                           guide_alpha, seed=seed, noise=noise, fireflies=fireflies, pixel_length=pixel_length, alt=alt, first=first,
                                           emitters=emitters, emittance=emittance, keep_rays=keep_rays, hp=hp, alts=ALTS)
    gb0 = info["first_gb"]
    p, hl, ev, hmax = first_hit(W, H, frame, cam, geoms, tris, tri_ids, lt, tab, rough, hp, gb0, info["cast"], seed, pixel_length, alt=alt)
    total_ev = {e: ev[e] + info.get("highlight", {}).get(e, 0) for e in EVENTS}
    info = dict(info, highlight=total_ev, H_max=max(hmax, info.get("H_max", 0.0)), first_rough=p, first_hl=hl)
    if len(p):
        col, D, I = col.copy(), D.copy(), I.copy()                         # noqa: E741
        J = pp["paths"]
        mult, chroma = splm.modulation(W, H, frame, seed, noise, fireflies)
        mult = mult.reshape(-1)[p]
        with np.errstate(all="ignore"):
            for c in range(3):
                ch = chroma[c].reshape(-1)[p]
                alb = gb0["albedo"][..., c].reshape(-1)[p]
                first_w = info["first"].reshape(-1)[p]
                ind = info["ind"][..., c].reshape(-1)[p]
                if alt == "first_highlight_into_indirect":
                    ind = (ind + hl[c]).astype(F)
                    first_c = first_w
                    if J > 0:
                        I.reshape(-1, 3)[p, c] = ((ind * mult).astype(F) * ch).astype(F)
                else:
                    first_c = (first_w + hl[c]).astype(F)
                    D.reshape(-1, 3)[p, c] = ((first_c * mult).astype(F) * ch).astype(F)
                shade = (first_c + ind).astype(F) if J > 0 else first_c
                col.reshape(-1, 3)[p, c] = (((alb * shade).astype(F) * mult).astype(F) * ch).astype(F)
    return col, gb, D, I, chain, info


def total(info, event):
    if event in EVENTS:
        return info["highlight"][event]
    return rm.total(info, event)
