"""numpy model of svgf_trace_draw_split and svgf_trace_compose (include/svgf_split.h, row f18), layered on tests/scene_trace_model.py:
the rays, the visibility and the bounce are scene_trace_model.render's (its `info`: vis, ind, cast); this file forms the two
demodulated terms from them with the header's table - float32, one rounding per operation, the header's nesting - and the
recomposition.  Test infrastructure only.
"""
import numpy as np

import scene_model as sm
import scene_trace_model as stm
from scene_model import F, _sel, synth


def emittance_plane(W, H, cam, geoms, geom_ids, tris, tri_ids, pixel_length=None):
    """float32[H, W]: the emittance of the first hit (0 on a triangle and on a miss).  scene_model.render decides the hit, as in
    scene_shadow_model.emitter_mask: the albedo it returns is replaced by the emittance (albedo plays no part in which surface wins)."""
    if geoms is None or not len(geoms):
        return np.zeros((H, W), F)
    flag = np.array(geoms, copy=True)
    flag["albedo"] = np.asarray(geoms["emittance"], dtype=F)[:, None]
    n = 0 if tris is None else len(tris)
    _, gb = sm.render(W, H, 0, cam, flag, geom_ids, tris, tri_ids, np.zeros((n, 3), F) if n else None, None, None, (0.0, 0.0, 0.0),
                      pixel_length=pixel_length)
    return np.ascontiguousarray(gb["albedo"][..., 0])


def modulation(W, H, frame, seed, noise, fireflies):
    """(mult float32[H, W], chroma: three float32[H, W]): svgf_scene_draw's noise multiplier (fireflies included) and chroma factors."""
    hu = lambda k: synth.hash_uniform(seed, frame, W * H, k).reshape(H, W)              # noqa: E731
    mult = (F(1.0) + F(noise) * (F(2.0) * hu(0) - F(1.0)).astype(F)).astype(F)
    mult = _sel(hu(1) < F(fireflies), (mult * F(6.0)).astype(F), mult)
    amp = F(F(0.1) * F(noise))
    return mult, [(F(1.0) + amp * (hu(2 + c) - F(0.5)).astype(F)).astype(F) for c in range(3)]


def render(W, H, frame, cam, geoms, geom_ids, tris, tri_ids, tri_albedo, tri_tex, textures, lt, tp, seed=1, noise=0.6, fireflies=0.02,
           pixel_length=None, *, first=None, emitters=None, traced=None, emittance=None):
    """(direct float32[H, W, 3], indirect float32[H, W, 3], colour, gbuffer, info) of svgf_trace_draw_split.  colour, gbuffer and info
    are scene_trace_model.render's for the same arguments (`traced`, computed when not given; never written to); `emittance` is
    emittance_plane's.  info gains shade0 (ambient + vis * direct, float32[H, W]) and emit."""
    if traced is None:
        traced = stm.render(W, H, frame, cam, geoms, geom_ids, tris, tri_ids, tri_albedo, tri_tex, textures, lt, tp, seed=seed, noise=noise,
                            fireflies=fireflies, pixel_length=pixel_length, first=first, emitters=emitters)
    if emittance is None:
        emittance = emittance_plane(W, H, cam, geoms, geom_ids, tris, tri_ids, pixel_length)
    col, gb, info = traced
    J, ambient = int(tp["bounce_samples"]), F(tp["ambient"])
    cast, vis, ind = info["cast"], info["vis"], info["ind"]
    hit = gb["geomId"] >= 0
    emitter = hit & (emittance > 0)
    assert np.array_equal(cast, hit & ~emitter)
    centre = [F(c) for c in lt["centre"]]
    with np.errstate(all="ignore"):
        n, pos = ([gb[f][..., c] for c in range(3)] for f in ("normal", "position"))
        shade0 = (ambient + (vis * stm.direct_term(centre, n, pos)).astype(F)).astype(F)
        first_term = _sel(emitter, emittance, shade0)
        mult, chroma = modulation(W, H, frame, seed, noise, fireflies)
        D = [_sel(hit, ((first_term * mult).astype(F) * chroma[c]).astype(F), F(0)) for c in range(3)]
        bounced = cast & (J > 0)
        I = [_sel(bounced, ((ind[..., c] * mult).astype(F) * chroma[c]).astype(F), F(0)) for c in range(3)]      # noqa: E741
    info = dict(info, shade0=shade0, emit=emittance, emitter=emitter)
    return np.ascontiguousarray(np.stack(D, -1)), np.ascontiguousarray(np.stack(I, -1)), col, gb, info


def compose(a, D, I):      # noqa: E741
    """svgf_trace_compose: a * (D + I), one addition then one multiplication in float32."""
    with np.errstate(all="ignore"):
        s = np.add(np.asarray(D, F), np.asarray(I, F), dtype=F)
        return np.multiply(np.asarray(a, F), s, dtype=F)
