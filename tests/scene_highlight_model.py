"""numpy model of svgf_highlight_draw and svgf_highlight_draw_split (include/svgf_highlight.h, row f23), layered on
tests/scene_rough_model.py as that one is on the virtual model.  What this file adds is the header's light term at ROUGH vertices:
`factor` (H, in the header's order), `light_direction` (the unit direction and the distance of a shadow sample's light point), `paths`
- scene_rough_model.paths' loop with the gather at the rough vertices behind the first hit - and in `render` the deterministic term of
the first hit, which makes first' per channel.  `render` runs scene_rough_model.render with this file's loop swapped in for its own,
then rewrites colour and D (nothing else) on the pixels whose first hit is rough.  float32 throughout, one rounding per operation, every
expression nested the way the kernel nests it.  Test infrastructure only.

`factor` takes the number format as an argument, so that the float64 tests of the BRDF run the very same statements.

Events, info["highlight"]: first (shadow samples of a rough first hit that the highlight evaluates), deeper (rough vertices behind the
first hit that gather), occluded (such a sample found occluded), backfacing (a formed, unoccluded sample with l_n <= 0), clamped (the
clamp lowered a contributing H), no_ray (!(dl > 0), or without shadow_secondary an l that is not a number).  info["H_max"]: the largest
unclamped contributing H of the frame.

`alt` names ONE deliberate deviation, in scene_rough_model's manner.
"""
import functools

import numpy as np

import scene_gloss_model as gm
import scene_model as sm
import scene_path_model as spm
import scene_rough_model as rm
import scene_split_model as splm
import scene_trace_model as stm
from scene_model import F, _sel, synth

ALTS = ("light_centre_for_l", "height_correlated_g", "first_highlight_into_indirect", "divided_by_reflect", "shadow_streams_swapped",
        "clamp_per_channel_after_spec")
EVENTS = ("first", "deeper", "occluded", "backfacing", "clamped", "no_ray")

_dot, _norm = rm._dot, rm._norm


def params(enable=1, clamp=0.0):
    return dict(enable=int(enable), clamp=float(clamp))


def factor(alpha, d, n, x, l, centre, clamp=0.0, dt=F, *, alt=None):      # noqa: E741
    """The header's H for arrays of format dt (alpha: array; d, n, x, l: three arrays each; centre: three numbers):
    dict(H (0 where not l_n > 0), raw (before the clamp), lit (l_n > 0), clamped (lit and the clamp lowered H), l_n, v_n, h_n)."""
    one, two = dt(1), dt(2)
    with np.errstate(all="ignore"):
        l_n = _dot(l, n)
        lit = l_n > 0
        v = [-d[c] for c in range(3)]
        v_n = _dot(v, n)
        h = _norm([v[c] + l[c] for c in range(3)])
        h_n = _dot(h, n)
        a2 = alpha * alpha
        t = (h_n * h_n) * (a2 - one) + one
        tl = [dt(centre[c]) - x[c] for c in range(3)]
        E = dt(30) / (dt(4) + _dot(tl, tl))
        Sl, Sv = np.sqrt(a2 + (one - a2) * (l_n * l_n)), np.sqrt(a2 + (one - a2) * (v_n * v_n))
        if alt == "height_correlated_g":
            raw = ((E * (a2 / (t * t))) * l_n) / (two * (l_n * Sv + v_n * Sl))
        else:
            G = (two * l_n) / (l_n + Sl)
            raw = ((E * (a2 / (t * t))) * G) / (two * (v_n + Sv))
        H = raw
        clamped = np.zeros(np.shape(raw), bool)
        if clamp > 0 and alt != "clamp_per_channel_after_spec":
            H = np.where(raw < dt(clamp), raw, dt(clamp))                # fminf(H, clamp)
            clamped = lit & ~(raw <= dt(clamp))
        H = np.where(lit, H, dt(0))
    assert H.dtype == dt and raw.dtype == dt, "an operation left the number format"
    return dict(H=H, raw=raw, lit=lit, clamped=clamped, l_n=l_n, v_n=v_n, h_n=h_n, E=E)


def light_direction(pos, u, v, lt):
    """The light point of the hash values (u, v), as scene_trace_model.occluded forms it: (l: three arrays, dl)."""
    centre, eu, ev = ([F(c) for c in lt[k]] for k in ("centre", "edge_u", "edge_v"))
    with np.errstate(all="ignore"):
        su, sv = (F(2.0) * u - F(1.0)).astype(F), (F(2.0) * v - F(1.0)).astype(F)
        L = [((centre[c] + (su * eu[c]).astype(F)).astype(F) + (sv * ev[c]).astype(F)).astype(F) for c in range(3)]
        q = [(L[c] - pos[c]).astype(F) for c in range(3)]
        dl = np.sqrt(_dot(q, q))
        return [(q[c] / dl).astype(F) for c in range(3)], dl


def _contribution(ev, hmax, alpha, d, n, x, l, formed, occ, centre, hp, alt):
    """c of the header for the samples given (formed: a ray or a direction exists; occ: it is occluded) and the counts into ev;
    with alt clamp_per_channel_after_spec the clamp is left to the caller.  Returns (c, the factor's dict)."""
    Hd = factor(alpha, d, n, x, l, centre, hp["clamp"], alt=alt)
    use = formed & ~occ
    c = _sel(use & Hd["lit"], Hd["H"], F(0))
    ev["no_ray"] += int((~formed).sum())
    ev["occluded"] += int((formed & occ).sum())
    ev["backfacing"] += int((use & ~Hd["lit"]).sum())
    ev["clamped"] += int((use & Hd["clamped"]).sum())
    r = Hd["raw"][use & Hd["lit"]]
    r = r[np.isfinite(r)]
    if len(r):
        hmax[0] = max(hmax[0], float(r.max()))
    return c, Hd


def _channel(spec_c, c, hp, alt):
    """spec_c * c, the clamp applied here under alt clamp_per_channel_after_spec."""
    t = (spec_c * c).astype(F)
    if alt == "clamp_per_channel_after_spec" and hp["clamp"] > 0:
        t = np.where(t < F(hp["clamp"]), t, F(hp["clamp"])).astype(F)
    return t


def paths(W, H, frame, seed, pix, n0, x0, d0, gid0, alb0, tab, geoms, geom_ids, tris, tri_ids, tri_albedo, tri_tex, textures, lt, pp, *, rough=None,
          ralt=None, hp=None, halt=None, alt=None, keep_rays=False):
    """scene_rough_model.paths (its arguments, its results) with the light's term at the rough vertices behind the first hit:
    `hp` = params(), `halt` this file's deviation.  info gains highlight (a dict of EVENTS) and H_max."""
    assert alt is None and not keep_rays
    alt = ralt
    hp = params(0) if hp is None else hp
    J, K, R, ambient, sec = pp["paths"], pp["max_depth"], pp["rr_depth"], F(pp["ambient"]), pp["shadow_secondary"]
    npix, n_pixels = len(pix), W * H
    N = J * npix
    centre = [F(c) for c in lt["centre"]]
    tri_id_set = np.zeros(0, np.int32) if tri_ids is None else np.unique(np.asarray(tri_ids, np.int32))
    rep = lambda v, dt=F: np.tile(np.asarray(v, dt), J)                  # noqa: E731  index j * npix + i
    jj, ii = np.repeat(np.arange(J), npix), np.tile(np.arange(npix), J)
    thr, acc = [np.ones(N, F) for _ in range(3)], [np.zeros(N, F) for _ in range(3)]
    x, n, d, alb = ([rep(a[c]) for c in range(3)] for a in (x0, n0, d0, alb0))
    gid = rep(gid0, np.int32)
    inside = np.zeros(N, bool)
    alive = np.ones(N, bool)
    hev, hmax = dict.fromkeys(EVENTS, 0), [0.0]
    info = dict(depth=[], hit_gid=[], events=[], rays=[], highlight=hev)
    with np.errstate(all="ignore"):
        for v in range(0, K + 1):
            idx = np.flatnonzero(alive)
            ev = dict.fromkeys(gm.EVENTS + rm.EVENTS, 0)
            row = dict.fromkeys(spm.COUNTS, 0)
            row["alive"] = len(idx)
            info["events"].append(ev)
            if v < K:
                info["depth"].append(row)
            if not len(idx):
                if v < K:
                    info["hit_gid"].append(np.zeros(0, np.int32))
                continue
            pj, pp_ = jj[idx], pix[ii[idx]]
            cb = 139 + 128 * v                                           # + 16 j: the class stream of vertex v
            xs, ns, ds, als = ([a[c][idx] for c in range(3)] for a in (x, n, d, alb))
            gs = gid[idx]
            tri = np.isin(gs, tri_id_set)
            u = gm._hash_per_path(seed, frame, n_pixels, cb, pj, pp_)
            V = gm.vertex(tab, gs, tri, ds, ns, u, inside[idx])
            spec = V["specular"]
            inside[idx] = V["inside"]
            entering = V["moved"] & V["inside"]
            alpha = rm.alpha_of(rough, gs)
            cand = V["mirror"] & (alpha > 0)
            if alt == "roughness_ignored_on_first_vertex" and v == 0:
                cand &= False
            dn, wgt = V["dn"], V["wgt"]
            is_rough = absorbed = degenerate = np.zeros(len(idx), bool)
            if cand.any():
                t1, t2, _ = rm.disc(seed, frame, n_pixels, cb + 117 + (8 if alt == "disc_from_other_streams" else 0), pj, pp_)
                Lb = rm.lobe(alpha, ds, ns, t1, t2, alt=alt)
                is_rough = cand & Lb["faces"]
                absorbed, degenerate = is_rough & Lb["absorbed"], is_rough & Lb["degenerate"]
                dn = [_sel(is_rough, Lb["dn"][c], dn[c]) for c in range(3)]
                wgt = [_sel(is_rough, (wgt[c] * Lb["G1"]).astype(F), wgt[c]) for c in range(3)]
            thr_s = [thr[c][idx] for c in range(3)]
            go = np.ones(len(idx), bool)
            if v >= 1:
                gathers = ~spec
                shines = is_rough & bool(hp["enable"])
                occ_all = np.zeros(len(idx), bool)
                if sec:
                    su = gm._hash_per_path(seed, frame, n_pixels, cb - 3, pj, pp_)
                    sv = gm._hash_per_path(seed, frame, n_pixels, cb - 2, pj, pp_)
                    occ_all = stm.occluded(xs, su, sv, geoms, tris, lt)
                occ = occ_all & gathers
                lit = (_sel(occ, F(0), F(1)) * stm.direct_term(centre, ns, xs)).astype(F)
                L = (ambient + lit).astype(F)
                for c in range(3):
                    add = (acc[c][idx] + (thr_s[c] * (als[c] * L).astype(F)).astype(F)).astype(F)
                    acc[c][idx] = _sel(gathers, add, acc[c][idx])
                if shines.any():
                    m = np.flatnonzero(shines)
                    sub = lambda a: [a[c][m] for c in range(3)]             # noqa: E731
                    xm = sub(xs)
                    if sec:
                        hu, hv = (sv[m], su[m]) if halt == "shadow_streams_swapped" else (su[m], sv[m])
                        lm, dl = light_direction(xm, hu, hv, lt)
                        formed = dl > 0
                        occ_m = stm.occluded(xm, hu, hv, geoms, tris, lt) if halt == "shadow_streams_swapped" else occ_all[m]
                        if halt == "light_centre_for_l":
                            lm = _norm([(centre[c] - xm[c]).astype(F) for c in range(3)])
                    else:
                        lm = _norm([(centre[c] - xm[c]).astype(F) for c in range(3)])
                        formed = np.isfinite(lm[0]) & np.isfinite(lm[1]) & np.isfinite(lm[2])
                        occ_m = np.zeros(len(m), bool)
                    cm, _ = _contribution(hev, hmax, alpha[m], sub(ds), sub(ns), xm, lm, formed, occ_m, centre, hp, halt)
                    hev["deeper"] += len(m)
                    if halt == "divided_by_reflect":
                        cm = (cm / V["reflect"][m]).astype(F)
                    for c in range(3):
                        term = _channel(V["wgt"][c][m], cm, hp, halt)
                        acc[c][idx[m]] = (acc[c][idx[m]] + (thr_s[c][m] * (als[c][m] * term).astype(F)).astype(F)).astype(F)
                if v >= K:
                    alive[idx] = False
                    continue
                thr_s = [(thr_s[c] * (als[c] * wgt[c]).astype(F)).astype(F) for c in range(3)]
                if R > 0 and v >= R:
                    m3 = np.maximum(np.maximum(thr_s[0], thr_s[1]), thr_s[2])
                    q = _sel(m3 < 1, m3, F(1))
                    xi = gm._hash_per_path(seed, frame, n_pixels, cb - 1, pj, pp_)
                    survive = (q > 0) & (xi < q)
                    go = survive
                    info["depth"][v - 1]["rr_kills"], info["depth"][v - 1]["rr_survivals"] = int((~survive).sum()), int(survive.sum())
                    thr_s = [(thr_s[c] / q).astype(F) for c in range(3)]
            else:
                thr_s = [wgt[c].copy() for c in range(3)]
            ev["absorbed"] = int((absorbed & go).sum())
            if alt != "absorbed_paths_continue":
                go = go & ~absorbed
            cnt = lambda m: int((m & go).sum())                          # noqa: E731
            if v == 0:
                ev["mirror0"], ev["glass0"] = cnt(V["mirror"]), cnt(V["glass"])
            else:
                ev["mirror"] = cnt(V["mirror"])
            ev["rough0" if v == 0 else "rough"] = cnt(is_rough)
            ev["degenerate_tangent"] = cnt(degenerate)
            ev["enter"], ev["exit"] = cnt(entering), cnt(V["moved"] & ~V["inside"])
            ev["fresnel_reflect"], ev["tir"] = cnt(V["fresnel"]), cnt(V["tir"])
            ev["partial_diffuse"], ev["partial_mirror"] = cnt(V["partial"] & ~spec), cnt(V["partial"] & spec)
            # the ray that leaves vertex v
            mx = np.maximum(np.maximum(np.abs(xs[0]), np.abs(xs[1])), np.abs(xs[2]))
            t_lo = (stm.T_LO * _sel(mx > 1, mx, F(1))).astype(F)
            dd = [np.zeros(len(idx), F) for _ in range(3)]
            for j in np.unique(pj):
                m = (pj == j) & ~spec
                if not m.any():
                    continue
                dj, _ = stm.directions(spm.stream_seed(seed, 128 * v + 16 * int(j)), frame, n_pixels, pp_[m], [ns[c][m] for c in range(3)], 1)
                for c in range(3):
                    dd[c][m] = dj[c][0]
            back = (-(gm.ORIGIN_FACTOR * t_lo).astype(F)).astype(F)
            moved = V["moved"]
            o = [_sel(moved, (xs[c] + (back * V["nn"][c]).astype(F)).astype(F), xs[c]) for c in range(3)]
            dd = [_sel(spec, dn[c], dd[c]) for c in range(3)]
            h = stm.nearest(o, dd, t_lo, geoms, geom_ids, tris, tri_ids, tri_albedo, tri_tex, textures)
            hit = (h["gid"] >= 0) & go
            em = hit & (h["emit"] > 0)
            ev["exit_found"] = int((entering & hit & (h["gid"] == gs)).sum())
            for c in range(3):
                add = (acc[c][idx] + (thr_s[c] * (h["alb"][c] * h["emit"]).astype(F)).astype(F)).astype(F)
                acc[c][idx] = _sel(em, add, acc[c][idx])
            on = hit & ~em
            for c in range(3):
                thr[c][idx] = _sel(on, thr_s[c], thr[c][idx])
                x[c][idx], n[c][idx] = _sel(on, h["pos"][c], x[c][idx]), _sel(on, h["n"][c], n[c][idx])
                alb[c][idx], d[c][idx] = _sel(on, h["alb"][c], alb[c][idx]), _sel(on, dd[c], d[c][idx])
            gid[idx] = np.where(on, h["gid"], gid[idx])
            alive[idx] = on
            row = info["depth"][v]
            row["hits"], row["emitter_hits"], row["misses"] = int(hit.sum()), int(em.sum()), int((go & ~hit).sum())
            info["hit_gid"].append(h["gid"][hit])
    info["H_max"] = hmax[0]
    return [a.reshape(J, npix) for a in acc], info


def first_hit(W, H, frame, cam, geoms, tris, tri_ids, lt, tab, rough, hp, gb0, cast, seed=1, pixel_length=None, *, alt=None):
    """The first hit's term: (flat indices of the pixels whose first hit is rough for the highlight, hl: three float32 arrays over
    them = (reflect spec_c) hm, events, H_max)."""
    ev, hmax = dict.fromkeys(EVENTS, 0), [0.0]
    tri_id_set = np.zeros(0, np.int32) if tri_ids is None else np.unique(np.asarray(tri_ids, np.int32))
    centre = [F(c) for c in lt["centre"]]
    S = int(lt["samples"])
    with np.errstate(all="ignore"):
        gid0 = gb0["geomId"]
        reflect, refract, _, spec = gm._surface(tab, gid0)
        glass0 = (refract > 0) & ~np.isin(gid0, tri_id_set)
        alpha0 = rm.alpha_of(rough, gid0)
        d0 = sm.rays(W, H, cam, pixel_length)
        nrm, pos = ([gb0[f][..., c] for c in range(3)] for f in ("normal", "position"))
        v_n = _dot([(-d0[c]).astype(F) for c in range(3)], nrm)
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
                l = _norm([(centre[c] - xp[c]).astype(F) for c in range(3)])        # noqa: E741
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
           seed=1, noise=0.6, fireflies=0.02, pixel_length=None, *, alt=None, first=None, emitters=None, emittance=None):
    """(colour, gbuffer, D, I, chain int32[H, W], info) of svgf_highlight_draw / svgf_highlight_draw_split with hp = params().  info is
    scene_rough_model.render's plus highlight (EVENTS over the frame), H_max, first_rough (flat pixel indices) and first_hl."""
    assert alt is None or alt in ALTS, alt
    hp = params() if hp is None else hp
    assert hp["enable"] in (0, 1) and np.isfinite(hp["clamp"]) and hp["clamp"] >= 0
    own = rm.paths
    rm.paths = functools.partial(paths, hp=hp, halt=alt)
    try:
        col, gb, D, I, chain, info = rm.render(W, H, frame, cam, geoms, geom_ids, tris, tri_ids, tri_albedo, tri_tex, textures, lt, pp, tab, vp, rough,      # noqa: E741
                                               guide_alpha, seed=seed, noise=noise, fireflies=fireflies, pixel_length=pixel_length, first=first,
                                               emitters=emitters, emittance=emittance)
    finally:
        rm.paths = own
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
