"""numpy model of svgf_gloss_draw and svgf_gloss_draw_split (include/svgf_gloss.h, row f20), layered on tests/scene_path_model.py as
that one is on the trace model: the first hit, its shadow rays and its term are scene_trace_model.render's with no bounce; every ray
behind it is that file's sampler (`directions`), its brute-force nearest hit (`nearest`), its shadow ray (`occluded`) and its light
term (`direct_term`); streams move by scene_path_model.stream_seed.  What this file adds is the header's vertex: its class (diffuse,
mirror, glass) from the surface table, the direction a specular vertex sends the path on in, the `inside` bit, the moved origin of a
transmitted ray, and the first term weighted by the first hit's diffuse share.  The (pixel, path) pairs are flattened into one axis and
every vertex is ONE numpy pass over the pairs still alive.  float32 throughout, one rounding per operation, every expression nested
the way the kernel nests it.  Test infrastructure only.

A hit is a TRIANGLE hit when its id is one of tri_ids (an object is a mesh or a primitive, never both).

`alt` names ONE deliberate deviation, in scene_path_model's manner.
"""
import numpy as np

import scene_model as sm
import scene_path_model as spm
import scene_shadow_model as ssm
import scene_split_model as splm
import scene_trace_model as stm
from scene_model import F, _dot, _normalise, _sel, synth

ALTS = ("inside_from_dot_sign", "eta_not_inverted", "spec_on_transmission", "gather_at_mirror", "first_unweighted",
        "lobe_stream_is_roulette_stream", "origin_not_moved", "glass_on_triangles")
EVENTS = ("mirror0", "glass0", "mirror", "enter", "exit", "fresnel_reflect", "tir", "partial_diffuse", "partial_mirror", "exit_found")
SURFACE_DTYPE = np.dtype([("reflect", "<f4"), ("refract", "<f4"), ("ior", "<f4"), ("spec", "<f4", 3)])
ORIGIN_FACTOR = F(4.0)


def table(n, **entries):
    """A surface table of n diffuse records (ior 1) with entries {id: (reflect, refract, ior, spec)} set; keys are given as g<id>."""
    t = np.zeros(n, SURFACE_DTYPE)
    t["ior"] = F(1.0)
    for k, (reflect, refract, ior, spec) in entries.items():
        t[int(k[1:])] = (reflect, refract, ior, spec)
    return t


def _surface(tab, gid):
    """S = table[g] where 0 <= g < n, the diffuse surface (all fields 0) elsewhere: (reflect, refract, ior, spec: three arrays)."""
    n = 0 if tab is None else len(tab)
    ok = (gid >= 0) & (gid < n)
    g = np.where(ok, gid, 0)
    if n == 0:
        z = np.zeros(gid.shape, F)
        return z, z.copy(), z.copy(), [z.copy() for _ in range(3)]
    tab = np.asarray(tab, dtype=SURFACE_DTYPE)
    return (_sel(ok, tab["reflect"][g], F(0)), _sel(ok, tab["refract"][g], F(0)), _sel(ok, tab["ior"][g], F(0)),
            [_sel(ok, tab["spec"][g, c], F(0)) for c in range(3)])


def vertex(tab, gid, tri, d, n, u, inside, *, alt=None):
    """gloss_vertex for arrays: dict(specular, glass, dn (three arrays), wgt (three arrays), nn, moved, inside (after), tir, fresnel,
    partial (0 < reflect < 1 decided the class), R, eta)."""
    reflect, refract, ior, spec = _surface(tab, gid)
    with np.errstate(all="ignore"):
        glass = (refract > 0) & (np.ones_like(tri) if alt == "glass_on_triangles" else ~tri)
        dotn = _dot(d, n)
        flip = dotn > 0
        nn = [_sel(flip, (-n[c]).astype(F), n[c]) for c in range(3)]
        ins = flip if alt == "inside_from_dot_sign" else inside
        if alt == "eta_not_inverted":
            ins = ~ins
        eta = _sel(ins, ior, (F(1) / ior).astype(F))
        dnn = _dot(d, nn)
        cs = (-dnn).astype(F)
        r0 = ((F(1) - eta).astype(F) / (F(1) + eta).astype(F)).astype(F)
        R0 = (r0 * r0).astype(F)
        m = (F(1) - cs).astype(F)
        m2 = (m * m).astype(F)
        R = (R0 + ((F(1) - R0).astype(F) * ((m2 * m2).astype(F) * m).astype(F)).astype(F)).astype(F)
        k2 = (F(1) - ((eta * eta).astype(F) * (F(1) - (cs * cs).astype(F)).astype(F)).astype(F)).astype(F)
        tir = glass & ~(k2 >= 0)
        fres = glass & (k2 >= 0) & (u < R)
        g_refl = tir | fres
        trans = glass & ~g_refl
        fg = (F(2) * dnn).astype(F)
        d_gr = [(d[c] - (fg * nn[c]).astype(F)).astype(F) for c in range(3)]
        ft = ((eta * cs).astype(F) - np.sqrt(k2)).astype(F)
        d_tr = [((eta * d[c]).astype(F) + (ft * nn[c]).astype(F)).astype(F) for c in range(3)]
        mirror = ~glass & (u < reflect)
        fm = (F(2) * dotn).astype(F)
        d_mr = [(d[c] - (fm * n[c]).astype(F)).astype(F) for c in range(3)]
        dn = _normalise([_sel(trans, d_tr[c], _sel(g_refl, d_gr[c], d_mr[c])) for c in range(3)])
        specular = glass | mirror
        spec_w = (g_refl | mirror) | (trans if alt == "spec_on_transmission" else False)
        wgt = [_sel(spec_w, spec[c], F(1)) for c in range(3)]
        partial = ~glass & (reflect > 0) & (reflect < 1)
    return dict(specular=specular, glass=glass, mirror=mirror, dn=dn, wgt=wgt, nn=nn, moved=trans, inside=inside ^ trans, tir=tir, fresnel=fres,
                partial=partial, R=R, R0=R0, eta=eta, reflect=reflect)


def _hash_per_path(seed, frame, n_pixels, stream0, jj, pixel):
    """hash(stream0 + 16 j) per element, j = jj, pixel = flat pixel index."""
    out = np.zeros(len(jj), F)
    for j in np.unique(jj):
        m = jj == j
        out[m] = synth.hash_uniform(seed, frame, n_pixels, stream0 + 16 * int(j))[pixel[m]]
    return out


def paths(W, H, frame, seed, pix, n0, x0, d0, gid0, alb0, tab, geoms, geom_ids, tris, tri_ids, tri_albedo, tri_tex, textures, lt, pp, *, alt=None,
          keep_rays=False):
    """The header's vertex loop for pixels `pix` (flat indices) with first-hit normals n0, positions x0, primary directions d0, ids gid0
    and albedos alb0: (acc: three float32[paths, len(pix)], info) - info["events"][v] counts EVENTS at vertex v, info["depth"][v - 1]
    scene_path_model's COUNTS of the ray that arrives at vertex v; with keep_rays info["rays"] lists per vertex the arrays the optics
    tests look at."""
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
            ev = dict.fromkeys(EVENTS, 0)
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
            u = _hash_per_path(seed, frame, n_pixels, cb - 1 if alt == "lobe_stream_is_roulette_stream" else cb, pj, pp_)
            V = vertex(tab, gs, tri, ds, ns, u, inside[idx], alt=alt)
            spec = V["specular"]
            inside[idx] = V["inside"]
            entering = V["moved"] & V["inside"]
            thr_s = [thr[c][idx] for c in range(3)]
            go = np.ones(len(idx), bool)
            if v >= 1:
                gathers = np.ones(len(idx), bool) if alt == "gather_at_mirror" else ~spec
                occ = np.zeros(len(idx), bool)
                if sec:
                    su = _hash_per_path(seed, frame, n_pixels, cb - 3, pj, pp_)
                    sv = _hash_per_path(seed, frame, n_pixels, cb - 2, pj, pp_)
                    occ = stm.occluded(xs, su, sv, geoms, tris, lt) & gathers
                lit = (_sel(occ, F(0), F(1)) * stm.direct_term(centre, ns, xs)).astype(F)
                L = (ambient + lit).astype(F)
                for c in range(3):
                    add = (acc[c][idx] + (thr_s[c] * (als[c] * L).astype(F)).astype(F)).astype(F)
                    acc[c][idx] = _sel(gathers, add, acc[c][idx])
                if v >= K:
                    alive[idx] = False
                    continue
                thr_s = [(thr_s[c] * (als[c] * V["wgt"][c]).astype(F)).astype(F) for c in range(3)]
                if R > 0 and v >= R:
                    m3 = np.maximum(np.maximum(thr_s[0], thr_s[1]), thr_s[2])
                    q = _sel(m3 < 1, m3, F(1))
                    xi = _hash_per_path(seed, frame, n_pixels, cb - 1, pj, pp_)
                    survive = (q > 0) & (xi < q)
                    go = survive
                    info["depth"][v - 1]["rr_kills"], info["depth"][v - 1]["rr_survivals"] = int((~survive).sum()), int(survive.sum())
                    thr_s = [(thr_s[c] / q).astype(F) for c in range(3)]
            else:
                thr_s = [V["wgt"][c].copy() for c in range(3)]
            # events are counted where a ray leaves the vertex (not at vertex max_depth, not on a path the roulette has just ended)
            cnt = lambda m: int((m & go).sum())                          # noqa: E731
            if v == 0:
                ev["mirror0"], ev["glass0"] = cnt(V["mirror"]), cnt(V["glass"])
            else:
                ev["mirror"] = cnt(V["mirror"])
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
            back = (-(ORIGIN_FACTOR * t_lo).astype(F)).astype(F)
            moved = V["moved"] & (alt != "origin_not_moved")
            o = [_sel(moved, (xs[c] + (back * V["nn"][c]).astype(F)).astype(F), xs[c]) for c in range(3)]
            dd = [_sel(spec, V["dn"][c], dd[c]) for c in range(3)]
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
            if keep_rays:
                info["rays"].append(dict(gid=gs, d=ds, n=ns, dn=V["dn"], nn=V["nn"], moved=V["moved"], mirror=V["mirror"], glass=V["glass"], fresnel=V["fresnel"],
                                         tir=V["tir"], eta=V["eta"], R0=V["R0"], u=u, go=go))
    return [a.reshape(J, npix) for a in acc], info


def render(W, H, frame, cam, geoms, geom_ids, tris, tri_ids, tri_albedo, tri_tex, textures, lt, pp, tab=None, seed=1, noise=0.6, fireflies=0.02,
           pixel_length=None, *, alt=None, first=None, emitters=None, emittance=None, keep_rays=False):
    """(colour float32[H, W, 3], gbuffer, D, I, info) of svgf_gloss_draw / svgf_gloss_draw_split with surface table `tab` (SURFACE_DTYPE
    records, or None).  `first`, `emitters` and `emittance` as scene_path_model.render's.  info: cast, vis, pixels, w_d, first
    (first', float32[H, W]), ind, acc, depth, hit_gid, events (a dict of EVENTS per vertex)."""
    assert alt is None or alt in ALTS, alt
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
    tri_id_set = np.zeros(0, np.int32) if tri_ids is None else np.unique(np.asarray(tri_ids, np.int32))
    info = dict(cast=cast, vis=vis, pixels=pix, depth=[], hit_gid=[], events=[dict.fromkeys(EVENTS, 0) for _ in range(K + 1)])
    with np.errstate(all="ignore"):
        nrm, pos, alb = ([gb[f][..., c] for c in range(3)] for f in ("normal", "position", "albedo"))
        reflect, refract, _, _ = _surface(tab, gb["geomId"])
        glass0 = (refract > 0) & ~np.isin(gb["geomId"], tri_id_set)
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
                               tris, tri_ids, tri_albedo, tri_tex, textures, lt, pp, alt=alt, keep_rays=keep_rays)
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
