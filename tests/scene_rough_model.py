"""numpy model of svgf_rough_draw and svgf_rough_draw_split (include/svgf_rough.h, row f22), layered on tests/scene_virtual_model.py as
that one is on the gloss model.  What the draw adds is the header's ROUGH vertex: `lobe` (the visible-normal sample, the reflected
direction, G1, absorption) stands with its direction and weight in the smooth mirror's place where a vertex is rough.  The lobe and
the vertex loop that applies it are tests/scene_vertex_model.py's; `render` is scene_gloss_model.render handed the roughness table (it
passes the table on to that loop), then scene_virtual_model.render on a surface table in which the full mirrors the guide must not
follow are partial ones.  float32 throughout, one rounding per operation, every expression nested the way the kernel nests it.  Test
infrastructure only.

Events, per vertex in info["events"]: rough0 / rough (a rough vertex at the first hit / behind it that a ray leaves), absorbed,
degenerate_tangent (a rough vertex whose Vh has no tangential part).  info["guide_events"]: guide_followed (the guide ran on a first hit
that is a full mirror with 0 < alpha <= guide_alpha), guide_stopped (a guide ended on a full mirror with alpha > guide_alpha: at the first
hit, chain 0, or deeper as the virtual hit; found from the texel's id, so an EMITTER with such an id would be counted too).

`alt` names ONE deliberate deviation, in scene_gloss_model's manner, and shares the loop's namespace with that file's names.
"""
import numpy as np

import scene_gloss_model as gm
import scene_virtual_model as vm
from scene_model import F
from scene_vertex_model import ROUGH_EVENTS as EVENTS
from scene_vertex_model import alpha_of, disc, frame_of, lobe, tri_id_set      # noqa: F401  (re-exported)

ALTS = ("roughness_ignored_on_first_vertex", "g1_dropped", "h_not_normalised", "disc_from_other_streams", "absorbed_paths_continue",
        "guide_alpha_compared_the_wrong_way")
GUIDE_EVENTS = ("guide_followed", "guide_stopped")
assert not set(ALTS) & set(gm.ALTS), "one vertex loop honours both files' names"


def _blocked(tab, rough, guide_alpha, alt):
    """Per record of `tab`: a full mirror the guide does not follow."""
    a = alpha_of(rough, np.arange(len(tab)))
    over = ((a > 0) & ~(a > F(guide_alpha))) if alt == "guide_alpha_compared_the_wrong_way" else (a > F(guide_alpha))
    return over & (np.asarray(tab["reflect"]) >= 1), a


def guide_table(tab, rough, guide_alpha, *, alt=None):
    """The surface table the guide of scene_virtual_model walks: a full mirror with alpha > guide_alpha is a partial one there (its
    class with the guide's u = 1 is then `not specular`, at the first hit and deeper), every other record is tab's.  Glass on a cube or
    a sphere is classified ahead of `reflect`, so a changed record of a glass object changes nothing."""
    if tab is None or rough is None or not len(tab) or not len(rough):
        return tab
    t = np.array(tab, dtype=gm.SURFACE_DTYPE, copy=True)
    blocked, _ = _blocked(t, rough, guide_alpha, alt)
    t["reflect"] = np.where(blocked, F(0.5), t["reflect"])
    return t


def render(W, H, frame, cam, geoms, geom_ids, tris, tri_ids, tri_albedo, tri_tex, textures, lt, pp, tab=None, vp=None, rough=None, guide_alpha=0.0, seed=1,
           noise=0.6, fireflies=0.02, pixel_length=None, *, alt=None, first=None, emitters=None, emittance=None, base=None, keep_rays=False, hp=None,
           alts=ALTS):
    """(colour, gbuffer, D, I, chain int32[H, W], info) of svgf_rough_draw / svgf_rough_draw_split.  `base`: the (colour, gbuffer, D,
    I, info) of an earlier call with the same arguments up to vp, guide_alpha and a guide's alt (they do not depend on those).  `hp` is the
    loop's highlight block (scene_highlight_model.render passes its own, with its `alts` for the names `alt` may take)."""
    assert alt is None or alt in alts, alt
    if base is None:
        base = gm.render(W, H, frame, cam, geoms, geom_ids, tris, tri_ids, tri_albedo, tri_tex, textures, lt, pp, tab, seed=seed, noise=noise,
                         fireflies=fireflies, pixel_length=pixel_length, alt=alt, first=first, emitters=emitters, emittance=emittance,
                         keep_rays=keep_rays, rough=rough, hp=hp, alts=alts)
    tab_g = guide_table(tab, rough, guide_alpha, alt=alt)
    col, gb, D, I, chain, info = vm.render(W, H, frame, cam, geoms, geom_ids, tris, tri_ids, tri_albedo, tri_tex, textures, lt, pp, tab_g, vp, seed=seed,      # noqa: E741
                                           pixel_length=pixel_length, base=base)
    ge = dict.fromkeys(GUIDE_EVENTS, 0)
    if tab_g is not None and rough is not None and len(tab_g):
        blocked, a = _blocked(np.asarray(tab, gm.SURFACE_DTYPE), rough, guide_alpha, alt)
        gid0 = info["first_gb"]["geomId"]
        runs = (gid0 >= 0) & ~info["emitter"] & (info["w_d"] == 0)
        ok0 = runs & (gid0 < len(tab))
        g0 = np.where(ok0, gid0, 0)
        full0 = ok0 & (tab["reflect"][g0] >= 1) & ~((tab["refract"][g0] > 0) & ~np.isin(gid0, tri_id_set(tri_ids)))
        ge["guide_followed"] = int((full0 & (a[g0] > 0) & ~blocked[g0]).sum())
        vg = gb["geomId"] - (vp or vm.params())["id_offset"]
        okv = (chain > 0) & (vg >= 0) & (vg < len(tab))
        ge["guide_stopped"] = int((full0 & blocked[g0]).sum()) + int((okv & blocked[np.where(okv, vg, 0)]).sum())
    info = dict(info, guide_events=ge)
    return col, gb, D, I, chain, info


def total(info, event):
    if event in GUIDE_EVENTS:
        return info["guide_events"][event]
    return sum(e.get(event, 0) for e in info["events"])
