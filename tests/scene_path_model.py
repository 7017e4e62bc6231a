"""numpy model of svgf_path_draw and svgf_path_draw_split (include/svgf_path.h, row f19), layered on tests/scene_trace_model.py: the
first hit, its shadow rays and its term are scene_trace_model.render's with no bounce; every bounce of every path is that file's
sampler (`directions`, `frame_of`), its brute-force nearest hit (`nearest`), its shadow ray (`occluded`) and its light term
(`direct_term`); the two demodulated terms are scene_split_model.render's table.  What this file adds is the header's loop: the
(pixel, path) pairs are flattened into one axis and every depth is ONE numpy pass over the pairs still alive.  float32 throughout, one
rounding per operation, every expression nested the way the kernel nests it.  Test infrastructure only.

Streams.  Bounce k of path j reads streams base + 0..10, base = 256 + 128 (k - 1) + 16 j.  scene_trace_model.directions reads
256 + 16 j' + 0..7; the hash's argument is p A + k B + frame C + seed D (mod 2^32) with D odd, so moving every stream by `delta` is
the same hash with a seed moved by delta B / D (mod 2^32): stream_seed() below.  tests/test_path_scene.py checks that identity.

`alt` names ONE deliberate deviation, in scene_trace_model's manner: the model then computes what a kernel with that mistake would,
and a test counts the pixels on which a scene tells the two apart.
"""
import numpy as np

import scene_model as sm
import scene_shadow_model as ssm
import scene_split_model as spm
import scene_trace_model as stm
from scene_model import F, _sel, synth

ALTS = ("thr_not_updated", "ambient_first_vertex_only", "no_roulette_compensation", "roulette_before_throughput",
        "streams_shared_across_depths", "frame_from_first_normal", "t_lo_from_first_pos", "continue_after_emitter", "no_shadow_behind_second")
MAX_PATHS = 8
MAX_DEPTH = 8
COUNTS = ("alive", "hits", "emitter_hits", "misses", "rr_kills", "rr_survivals")
_B, _D = 0x85EBCA77, 0x27D4EB2F
_D_INV = pow(_D, -1, 1 << 32)


def params(paths=1, max_depth=4, rr_depth=2, ambient=0.15, shadow_secondary=1):
    return dict(paths=int(paths), max_depth=int(max_depth), rr_depth=int(rr_depth), ambient=float(ambient), shadow_secondary=int(shadow_secondary))


def stream_seed(seed, delta):
    """The seed under which hash stream k is stream k + delta of `seed`."""
    return (int(seed) + int(delta) * _B * _D_INV) & 0xFFFFFFFF


def paths(W, H, frame, seed, pix, n0, x0, geoms, geom_ids, tris, tri_ids, tri_albedo, tri_tex, textures, lt, pp, *, alt=None):
    """The header's path loop for pixels `pix` (flat indices) with first-hit normals n0 and positions x0 (three arrays [len(pix)]):
    (acc: three float32[paths, len(pix)], info) - info["depth"][k - 1] holds COUNTS of bounce k, info["hit_gid"][k - 1] the geomId of
    every hit of bounce k."""
    J, K, R, ambient, sec = pp["paths"], pp["max_depth"], pp["rr_depth"], F(pp["ambient"]), pp["shadow_secondary"]
    npix, n_pixels = len(pix), W * H
    N = J * npix
    centre = [F(c) for c in lt["centre"]]
    rep = lambda v: np.tile(np.asarray(v, F), J)                        # noqa: E731  index j * npix + i
    jj, ii = np.repeat(np.arange(J), npix), np.tile(np.arange(npix), J)
    thr, acc = [np.ones(N, F) for _ in range(3)], [np.zeros(N, F) for _ in range(3)]
    x, n = [rep(x0[c]) for c in range(3)], [rep(n0[c]) for c in range(3)]
    x_first, n_first = [v.copy() for v in x], [v.copy() for v in n]
    alive = np.ones(N, bool)
    info = dict(depth=[], hit_gid=[])
    with np.errstate(all="ignore"):
        for k in range(1, K + 1):
            idx = np.flatnonzero(alive)
            row = dict.fromkeys(COUNTS, 0)
            row["alive"] = len(idx)
            if not len(idx):
                info["depth"].append(row); info["hit_gid"].append(np.zeros(0, np.int32))
                continue
            depth_off = 0 if alt == "streams_shared_across_depths" else 128 * (k - 1)
            xs = [x[c][idx] for c in range(3)]
            ns = [(n_first if alt == "frame_from_first_normal" else n)[c][idx] for c in range(3)]
            d = [np.zeros(len(idx), F) for _ in range(3)]
            for j in range(J):                                          # one sampler call per path: its own streams
                m = jj[idx] == j
                if not m.any():
                    continue
                dj, _ = stm.directions(stream_seed(seed, depth_off + 16 * j), frame, n_pixels, pix[ii[idx][m]], [ns[c][m] for c in range(3)], 1)
                for c in range(3):
                    d[c][m] = dj[c][0]
            xt = [x_first[c][idx] for c in range(3)] if alt == "t_lo_from_first_pos" else xs
            mx = np.maximum(np.maximum(np.abs(xt[0]), np.abs(xt[1])), np.abs(xt[2]))
            t_lo = (stm.T_LO * _sel(mx > 1, mx, F(1))).astype(F)
            h = stm.nearest(xs, d, t_lo, geoms, geom_ids, tris, tri_ids, tri_albedo, tri_tex, textures)
            hit = h["gid"] >= 0
            em = hit & (h["emit"] > 0)
            occ = np.zeros(len(idx), bool)
            if sec and not (alt == "no_shadow_behind_second" and k >= 2):
                base = 256 + depth_off
                u, v = np.zeros(len(idx), F), np.zeros(len(idx), F)
                for j in range(J):
                    m = jj[idx] == j
                    u[m] = synth.hash_uniform(seed, frame, n_pixels, base + 16 * j + 8)[pix[ii[idx][m]]]
                    v[m] = synth.hash_uniform(seed, frame, n_pixels, base + 16 * j + 9)[pix[ii[idx][m]]]
                occ = stm.occluded(h["pos"], u, v, geoms, tris, lt) & hit & ~em
            lit = (_sel(occ, F(0), F(1)) * stm.direct_term(centre, h["n"], h["pos"])).astype(F)
            L = lit if (alt == "ambient_first_vertex_only" and k >= 2) else (ambient + lit).astype(F)
            L = _sel(em, h["emit"], L)
            thr_s = [thr[c][idx] for c in range(3)]
            for c in range(3):
                add = (acc[c][idx] + (thr_s[c] * (h["alb"][c] * L).astype(F)).astype(F)).astype(F)
                acc[c][idx] = _sel(hit, add, acc[c][idx])
            ends = ~hit | em
            if alt == "continue_after_emitter":
                ends = ~hit
            go = ~ends & (k < K)
            thr_before = thr_s
            if alt != "thr_not_updated":
                thr_s = [(thr_s[c] * h["alb"][c]).astype(F) for c in range(3)]
            kills = np.zeros(len(idx), bool)
            if R > 0 and k >= R:
                tq = thr_before if alt == "roulette_before_throughput" else thr_s
                m3 = np.maximum(np.maximum(tq[0], tq[1]), tq[2])
                q = _sel(m3 < 1, m3, F(1))                                                      # fminf(., 1) on numbers
                xi = np.zeros(len(idx), F)
                for j in range(J):
                    m = jj[idx] == j
                    xi[m] = synth.hash_uniform(seed, frame, n_pixels, 256 + depth_off + 16 * j + 10)[pix[ii[idx][m]]]
                survive = (q > 0) & (xi < q)
                kills = go & ~survive
                row["rr_kills"], row["rr_survivals"] = int(kills.sum()), int((go & survive).sum())
                if alt != "no_roulette_compensation":
                    thr_s = [(thr_s[c] / q).astype(F) for c in range(3)]
            go &= ~kills
            for c in range(3):
                thr[c][idx] = _sel(go, thr_s[c], thr[c][idx])
                x[c][idx] = _sel(go, h["pos"][c], x[c][idx])
                n[c][idx] = _sel(go, h["n"][c], n[c][idx])
            alive[idx] = go
            row["hits"], row["emitter_hits"], row["misses"] = int(hit.sum()), int(em.sum()), int((~hit).sum())
            info["depth"].append(row)
            info["hit_gid"].append(h["gid"][hit])
    return [a.reshape(J, npix) for a in acc], info


def render(W, H, frame, cam, geoms, geom_ids, tris, tri_ids, tri_albedo, tri_tex, textures, lt, pp, seed=1, noise=0.6, fireflies=0.02,
           pixel_length=None, *, alt=None, first=None, emitters=None, emittance=None):
    """(colour float32[H, W, 3], gbuffer, D, I, info) of svgf_path_draw / svgf_path_draw_split.  `first`, `emitters` and `emittance` as
    scene_trace_model.render's and scene_split_model.render's (computed when not given; never written to).  info: cast, vis, pixels,
    ind float32[H, W, 3] (0 where no path starts), acc (three float32[paths, n]), depth (a dict of COUNTS per bounce), hit_gid."""
    assert alt is None or alt in ALTS, alt
    J, K, R, ambient, sec = pp["paths"], pp["max_depth"], pp["rr_depth"], F(pp["ambient"]), pp["shadow_secondary"]
    assert 0 <= J <= MAX_PATHS and 1 <= K <= MAX_DEPTH and 0 <= R <= MAX_DEPTH and sec in (0, 1)
    if first is None:
        first = sm.render(W, H, frame, cam, geoms, geom_ids, tris, tri_ids, tri_albedo, tri_tex, textures, lt["centre"], seed=seed, noise=noise,
                          fireflies=fireflies, pixel_length=pixel_length)
    if emitters is None:
        emitters = ssm.emitter_mask(W, H, cam, geoms, geom_ids, tris, tri_ids, pixel_length)
    col0, gb, base = stm.render(W, H, frame, cam, geoms, geom_ids, tris, tri_ids, tri_albedo, tri_tex, textures, lt, stm.params(0, ambient, sec),
                                seed=seed, noise=noise, fireflies=fireflies, pixel_length=pixel_length, first=first, emitters=emitters)
    cast, vis, pix = base["cast"], base["vis"], base["pixels"]
    info = dict(cast=cast, vis=vis, pixels=pix, shadow=base["shadow"], depth=[], hit_gid=[])
    ind = np.zeros((H, W, 3), F)
    col = col0
    with np.errstate(all="ignore"):
        if J > 0 and len(pix):
            nrm, pos, alb = ([gb[f][..., c] for c in range(3)] for f in ("normal", "position", "albedo"))
            n0, x0 = [nrm[c].reshape(-1)[pix] for c in range(3)], [pos[c].reshape(-1)[pix] for c in range(3)]
            acc, pinfo = paths(W, H, frame, seed, pix, n0, x0, geoms, geom_ids, tris, tri_ids, tri_albedo, tri_tex, textures, lt, pp, alt=alt)
            info.update(pinfo, acc=acc)
            shade0 = (ambient + (vis * stm.direct_term([F(c) for c in lt["centre"]], nrm, pos)).astype(F)).astype(F)
            mult, chroma = spm.modulation(W, H, frame, seed, noise, fireflies)
            out = []
            for c in range(3):
                s = np.zeros(len(pix), F)
                for j in range(J):
                    s = (s + acc[c][j]).astype(F)
                ind_c = (s / F(J)).astype(F)
                ind.reshape(-1, 3)[pix, c] = ind_c
                shade = shade0.copy().reshape(-1)
                shade[pix] = (shade0.reshape(-1)[pix] + ind_c).astype(F)
                shade = shade.reshape(H, W)
                out.append(_sel(cast, (((alb[c] * shade).astype(F) * mult).astype(F) * chroma[c]).astype(F), col0[..., c]))
            col = np.ascontiguousarray(np.stack(out, -1).astype(F))
    info["ind"] = ind
    D, I, _, _, sinfo = spm.render(W, H, frame, cam, geoms, geom_ids, tris, tri_ids, tri_albedo, tri_tex, textures, lt, stm.params(J, ambient, sec),      # noqa: E741
                                   seed=seed, noise=noise, fireflies=fireflies, pixel_length=pixel_length,
                                   traced=(col, gb, dict(cast=cast, vis=vis, ind=ind)), emittance=emittance)
    info.update(shade0=sinfo["shade0"], emit=sinfo["emit"], emitter=sinfo["emitter"])
    return col, gb, D, I, info
