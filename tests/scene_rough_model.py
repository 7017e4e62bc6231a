"""numpy model of svgf_rough_draw and svgf_rough_draw_split (include/svgf_rough.h, row f22), layered on tests/scene_virtual_model.py as
that one is on the gloss model.  What this file adds is the header's ROUGH vertex: `lobe` (the visible-normal sample, the reflected
direction, G1, absorption) and `paths`, scene_gloss_model.paths' loop - ONE numpy pass per vertex over the (pixel, path) pairs still
alive - with the lobe's direction and weight in the smooth mirror's place where a vertex is rough.  `render` is
scene_gloss_model.render with that loop in its own loop's place (the function is swapped in for the call), then
scene_virtual_model.render on a surface table in which the full mirrors the guide must not follow are partial ones.  float32 throughout,
one rounding per operation, every expression nested the way the kernel nests it.  Test infrastructure only.

`lobe` takes the number format as an argument, so that the float64 tests of the construction run the very same statements.

Events, per vertex in info["events"]: rough0 / rough (a rough vertex at the first hit / behind it that a ray leaves), absorbed,
degenerate_tangent (a rough vertex whose Vh has no tangential part).  info["guide_events"]: guide_followed (the guide ran on a first hit
that is a full mirror with 0 < alpha <= guide_alpha), guide_stopped (a guide ended on a full mirror with alpha > guide_alpha: at the first
hit, chain 0, or deeper as the virtual hit; found from the texel's id, so an EMITTER with such an id would be counted too).

`alt` names ONE deliberate deviation, in scene_gloss_model's manner.
"""
import functools

import numpy as np

import scene_gloss_model as gm
import scene_path_model as spm
import scene_trace_model as stm
import scene_virtual_model as vm
from scene_model import F, _sel

ALTS = ("roughness_ignored_on_first_vertex", "g1_dropped", "h_not_normalised", "disc_from_other_streams", "absorbed_paths_continue",
        "guide_alpha_compared_the_wrong_way")
EVENTS = ("rough0", "rough", "absorbed", "degenerate_tangent")
GUIDE_EVENTS = ("guide_followed", "guide_stopped")


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _norm(v):
    l = np.sqrt(_dot(v, v))
    return [v[0] / l, v[1] / l, v[2] / l]


def frame_of(n, dt=F):
    """scene_trace_model.frame_of in the number format dt."""
    one = dt(1)
    s = np.copysign(one, n[2])
    q = -one / (s + n[2])
    w = (n[0] * n[1]) * q
    return [one + ((s * n[0]) * n[0]) * q, s * w, -(s * n[0])], [w, s + (n[1] * n[1]) * q, -n[1]]


def alpha_of(rough, gid):
    """alpha_g = rough[g] where 0 <= g < n, 0 elsewhere."""
    n = 0 if rough is None else len(rough)
    if n == 0:
        return np.zeros(np.shape(gid), F)
    ok = (gid >= 0) & (gid < n)
    return _sel(ok, np.asarray(rough, F)[np.where(ok, gid, 0)], F(0))


def lobe(alpha, d, n, t1, t2, dt=F, *, alt=None):
    """The header's rough vertex for arrays of format dt (alpha, t1, t2: arrays; d, n: three arrays each): dict(faces (v_n > 0: the
    vertex is rough where alpha > 0 and the class is MIRROR), dn, h (world space), G1, l_n, absorbed, degenerate, Vh)."""
    one, two, half, zero = dt(1), dt(2), dt(0.5), dt(0)
    with np.errstate(all="ignore"):
        T, B = frame_of(n, dt)
        v = [-d[c] for c in range(3)]
        v_t, v_b, v_n = _dot(v, T), _dot(v, B), _dot(v, n)
        Vh = _norm([alpha * v_t, alpha * v_b, v_n])
        q = Vh[0] * Vh[0] + Vh[1] * Vh[1]
        deg = ~(q > 0)
        ln = np.sqrt(q)
        T1x, T1y = np.where(deg, one, -Vh[1] / ln), np.where(deg, zero, Vh[0] / ln)
        T2 = [-(Vh[2] * T1y), Vh[2] * T1x, Vh[0] * T1y - Vh[1] * T1x]
        sh = half * (one + Vh[2])
        w = one - t1 * t1
        t2p = (one - sh) * np.sqrt(w) + sh * t2
        r = w - t2p * t2p
        cz = np.sqrt(np.where(r > 0, r, zero))
        Nh = [(t1 * T1x + t2p * T2[0]) + cz * Vh[0], (t1 * T1y + t2p * T2[1]) + cz * Vh[1], t2p * T2[2] + cz * Vh[2]]
        hl = [alpha * Nh[0], alpha * Nh[1], np.where(Nh[2] > 0, Nh[2], zero)]
        if alt != "h_not_normalised":
            hl = _norm(hl)
        h = [(hl[0] * T[c] + hl[1] * B[c]) + hl[2] * n[c] for c in range(3)]
        f = two * _dot(d, h)
        dn = _norm([d[c] - f * h[c] for c in range(3)])
        l_n = _dot(dn, n)
        a2 = alpha * alpha
        G1 = (two * l_n) / (l_n + np.sqrt(a2 + (one - a2) * (l_n * l_n)))
        if alt == "g1_dropped":
            G1 = np.ones_like(G1)
    out = dict(faces=v_n > 0, dn=dn, h=h, G1=G1, l_n=l_n, absorbed=~(l_n > 0), degenerate=deg, Vh=Vh)
    assert all(a.dtype == dt for a in out["dn"] + out["h"] + [G1, l_n]), "an operation left the number format"
    return out


def disc(seed, frame, n_pixels, base0, jj, pixel):
    """The disc point of the diffuse sampler's bounded rejection on streams base0 + 16 j + 0..7 (scene_trace_model.directions'
    loop, for the point alone): (t1, t2, found)."""
    t1, t2, found = np.zeros(len(jj), F), np.zeros(len(jj), F), np.zeros(len(jj), bool)
    for k in range(4):
        ak = (F(2.0) * gm._hash_per_path(seed, frame, n_pixels, base0 + 2 * k, jj, pixel) - F(1.0)).astype(F)
        bk = (F(2.0) * gm._hash_per_path(seed, frame, n_pixels, base0 + 2 * k + 1, jj, pixel) - F(1.0)).astype(F)
        take = ~found & (((ak * ak).astype(F) + (bk * bk).astype(F)).astype(F) < F(1.0))
        t1, t2, found = _sel(take, ak, t1), _sel(take, bk, t2), found | take
    return t1, t2, found


def paths(W, H, frame, seed, pix, n0, x0, d0, gid0, alb0, tab, geoms, geom_ids, tris, tri_ids, tri_albedo, tri_tex, textures, lt, pp, *, rough=None,
          ralt=None, alt=None, keep_rays=False):
    """scene_gloss_model.paths (its arguments, its results; `alt` and `keep_rays` are that function's and must be unset) with the
    roughness table `rough` (float32 per object id, or None) and this file's deviation `ralt`."""
    assert alt is None and not keep_rays
    alt = ralt
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
    info = dict(depth=[], hit_gid=[], events=[], rays=[])
    with np.errstate(all="ignore"):
        for v in range(0, K + 1):
            idx = np.flatnonzero(alive)
            ev = dict.fromkeys(gm.EVENTS + EVENTS, 0)
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
            # the rough vertices: the lobe's direction and weight in the smooth mirror's place
            alpha = alpha_of(rough, gs)
            cand = V["mirror"] & (alpha > 0)
            if alt == "roughness_ignored_on_first_vertex" and v == 0:
                cand &= False
            dn, wgt = V["dn"], V["wgt"]
            is_rough = absorbed = degenerate = np.zeros(len(idx), bool)
            if cand.any():
                t1, t2, _ = disc(seed, frame, n_pixels, cb + 117 + (8 if alt == "disc_from_other_streams" else 0), pj, pp_)
                Lb = lobe(alpha, ds, ns, t1, t2, alt=alt)
                is_rough = cand & Lb["faces"]
                absorbed, degenerate = is_rough & Lb["absorbed"], is_rough & Lb["degenerate"]
                dn = [_sel(is_rough, Lb["dn"][c], dn[c]) for c in range(3)]
                wgt = [_sel(is_rough, (wgt[c] * Lb["G1"]).astype(F), wgt[c]) for c in range(3)]
            thr_s = [thr[c][idx] for c in range(3)]
            go = np.ones(len(idx), bool)
            if v >= 1:
                gathers = ~spec
                occ = np.zeros(len(idx), bool)
                if sec:
                    su = gm._hash_per_path(seed, frame, n_pixels, cb - 3, pj, pp_)
                    sv = gm._hash_per_path(seed, frame, n_pixels, cb - 2, pj, pp_)
                    occ = stm.occluded(xs, su, sv, geoms, tris, lt) & gathers
                lit = (_sel(occ, F(0), F(1)) * stm.direct_term(centre, ns, xs)).astype(F)
                L = (ambient + lit).astype(F)
                for c in range(3):
                    add = (acc[c][idx] + (thr_s[c] * (als[c] * L).astype(F)).astype(F)).astype(F)
                    acc[c][idx] = _sel(gathers, add, acc[c][idx])
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
            # an absorbed path ends at its vertex (the kernel leaves ahead of the roulette; nothing between the two is stored)
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
    return [a.reshape(J, npix) for a in acc], info


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
           noise=0.6, fireflies=0.02, pixel_length=None, *, alt=None, first=None, emitters=None, emittance=None, base=None):
    """(colour, gbuffer, D, I, chain int32[H, W], info) of svgf_rough_draw / svgf_rough_draw_split.  `base`: the (colour, gbuffer, D,
    I, info) of an earlier call with the same arguments up to vp, guide_alpha and a guide's alt (they do not depend on those)."""
    assert alt is None or alt in ALTS, alt
    if base is None:
        own = gm.paths
        gm.paths = functools.partial(paths, rough=rough, ralt=alt)
        try:
            base = gm.render(W, H, frame, cam, geoms, geom_ids, tris, tri_ids, tri_albedo, tri_tex, textures, lt, pp, tab, seed=seed, noise=noise,
                             fireflies=fireflies, pixel_length=pixel_length, first=first, emitters=emitters, emittance=emittance)
        finally:
            gm.paths = own
    tab_g = guide_table(tab, rough, guide_alpha, alt=alt)
    col, gb, D, I, chain, info = vm.render(W, H, frame, cam, geoms, geom_ids, tris, tri_ids, tri_albedo, tri_tex, textures, lt, pp, tab_g, vp, seed=seed,      # noqa: E741
                                           pixel_length=pixel_length, base=base)
    ge = dict.fromkeys(GUIDE_EVENTS, 0)
    if tab_g is not None and rough is not None and len(tab_g):
        blocked, a = _blocked(np.asarray(tab, gm.SURFACE_DTYPE), rough, guide_alpha, alt)
        tri_id_set = np.zeros(0, np.int32) if tri_ids is None else np.unique(np.asarray(tri_ids, np.int32))
        gid0 = info["first_gb"]["geomId"]
        runs = (gid0 >= 0) & ~info["emitter"] & (info["w_d"] == 0)
        ok0 = runs & (gid0 < len(tab))
        g0 = np.where(ok0, gid0, 0)
        full0 = ok0 & (tab["reflect"][g0] >= 1) & ~((tab["refract"][g0] > 0) & ~np.isin(gid0, tri_id_set))
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
