"""The vertex of k_scene_gloss (include/svgf_scene_gloss.inc.h) in numpy, for the draw families that instantiate that kernel: gloss
(f20), virtual (f21), rough (f22) and highlight (f23).  The device has ONE kernel text with more arguments per library; this file is
its model's counterpart: the per-vertex pieces (`vertex`, `lobe`, `factor` and what they need) and ONE vertex loop, `paths`, that takes
the roughness table and the highlight block as plain arguments.  scene_gloss_model.py, scene_rough_model.py and scene_highlight_model.py
state what their draws mean, own `render`, and re-export from here the names their suites use; scene_virtual_model.py's guide chain is
another loop and calls `vertex`.  This file imports none of them.  float32 throughout, one rounding per operation, every expression
nested the way the kernel nests it.  Test infrastructure only.

`lobe` and `factor` take the number format as an argument, so that the float64 tests of the construction and of the BRDF run the very
same statements.

The event names live here because the loop writes them; each model file publishes its own tuple as EVENTS and says what they count.

`alt` names ONE deliberate deviation; the loop honours the loop-level names of all three model files in one namespace (the three ALTS
tuples are disjoint, scene_highlight_model asserts it), and a name it does not know changes nothing.
"""
import numpy as np

import scene_path_model as spm
import scene_trace_model as stm
from scene_model import F, _dot, _normalise, _sel, synth

GLOSS_EVENTS = ("mirror0", "glass0", "mirror", "enter", "exit", "fresnel_reflect", "tir", "partial_diffuse", "partial_mirror", "exit_found")
ROUGH_EVENTS = ("rough0", "rough", "absorbed", "degenerate_tangent")
HIGHLIGHT_EVENTS = ("first", "deeper", "occluded", "backfacing", "clamped", "no_ray")
SURFACE_DTYPE = np.dtype([("reflect", "<f4"), ("refract", "<f4"), ("ior", "<f4"), ("spec", "<f4", 3)])
ORIGIN_FACTOR = F(4.0)


# scene_model's _dot and _normalise round their result to float32 whatever they are given; this pair nests the same way and stays in
# the number format of its arguments, which `lobe` and `factor` need for their float64 tests.  On float32 arrays the two pairs give the
# same bits (every operation of either is one float32 operation there); on float64 arrays scene_model's would round to float32.
def _dot_dt(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _norm_dt(v):
    l = np.sqrt(_dot_dt(v, v))
    return [v[0] / l, v[1] / l, v[2] / l]


def tri_id_set(tri_ids):
    """The ids that mark a TRIANGLE hit (an object is a mesh or a primitive, never both)."""
    return np.zeros(0, np.int32) if tri_ids is None else np.unique(np.asarray(tri_ids, np.int32))


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


# ---- the rough vertex (row f22) ------------------------------------------------------------------------------------------------------------
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
        v_t, v_b, v_n = _dot_dt(v, T), _dot_dt(v, B), _dot_dt(v, n)
        Vh = _norm_dt([alpha * v_t, alpha * v_b, v_n])
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
            hl = _norm_dt(hl)
        h = [(hl[0] * T[c] + hl[1] * B[c]) + hl[2] * n[c] for c in range(3)]
        f = two * _dot_dt(d, h)
        dn = _norm_dt([d[c] - f * h[c] for c in range(3)])
        l_n = _dot_dt(dn, n)
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
        ak = (F(2.0) * _hash_per_path(seed, frame, n_pixels, base0 + 2 * k, jj, pixel) - F(1.0)).astype(F)
        bk = (F(2.0) * _hash_per_path(seed, frame, n_pixels, base0 + 2 * k + 1, jj, pixel) - F(1.0)).astype(F)
        take = ~found & (((ak * ak).astype(F) + (bk * bk).astype(F)).astype(F) < F(1.0))
        t1, t2, found = _sel(take, ak, t1), _sel(take, bk, t2), found | take
    return t1, t2, found


# ---- the light's term at a rough vertex (row f23) ----------------------------------------------------------------------------------------
def factor(alpha, d, n, x, l, centre, clamp=0.0, dt=F, *, alt=None):      # noqa: E741
    """The header's H for arrays of format dt (alpha: array; d, n, x, l: three arrays each; centre: three numbers):
    dict(H (0 where not l_n > 0), raw (before the clamp), lit (l_n > 0), clamped (lit and the clamp lowered H), l_n, v_n, h_n)."""
    one, two = dt(1), dt(2)
    with np.errstate(all="ignore"):
        l_n = _dot_dt(l, n)
        lit = l_n > 0
        v = [-d[c] for c in range(3)]
        v_n = _dot_dt(v, n)
        h = _norm_dt([v[c] + l[c] for c in range(3)])
        h_n = _dot_dt(h, n)
        a2 = alpha * alpha
        t = (h_n * h_n) * (a2 - one) + one
        tl = [dt(centre[c]) - x[c] for c in range(3)]
        E = dt(30) / (dt(4) + _dot_dt(tl, tl))
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
        dl = np.sqrt(_dot_dt(q, q))
        return [(q[c] / dl).astype(F) for c in range(3)], dl


def _contribution(ev, hmax, alpha, d, n, x, l, formed, occ, centre, hp, alt):      # noqa: E741
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


# ---- the vertex loop -----------------------------------------------------------------------------------------------------------------------
def paths(W, H, frame, seed, pix, n0, x0, d0, gid0, alb0, tab, geoms, geom_ids, tris, tri_ids, tri_albedo, tri_tex, textures, lt, pp, *, rough=None,
          hp=None, alt=None, keep_rays=False):
    """The kernel's vertex loop for pixels `pix` (flat indices) with first-hit normals n0, positions x0, primary directions d0, ids gid0
    and albedos alb0 - ONE numpy pass per vertex over the (pixel, path) pairs still alive: (acc: three float32[paths, len(pix)], info).
    `rough`: the roughness table (float32 per object id) or None - where a mirror vertex has alpha > 0 the lobe's direction and weight
    stand in the smooth mirror's place; `hp`: scene_highlight_model.params() or None - the light's term at the rough vertices behind the
    first hit.  info["events"][v] counts GLOSS_EVENTS at vertex v (and ROUGH_EVENTS where `rough` is given, an empty table too),
    info["depth"][v - 1] scene_path_model's COUNTS of the ray that arrives at vertex v; with keep_rays info["rays"] lists per vertex
    the arrays the optics tests look at; with `hp` info["highlight"] counts HIGHLIGHT_EVENTS over the frame and info["H_max"] is the
    largest unclamped contributing H."""
    J, K, R, ambient, sec = pp["paths"], pp["max_depth"], pp["rr_depth"], F(pp["ambient"]), pp["shadow_secondary"]
    npix, n_pixels = len(pix), W * H
    N = J * npix
    centre = [F(c) for c in lt["centre"]]
    tri_set = tri_id_set(tri_ids)
    rep = lambda v, dt=F: np.tile(np.asarray(v, dt), J)                  # noqa: E731  index j * npix + i
    jj, ii = np.repeat(np.arange(J), npix), np.tile(np.arange(npix), J)
    thr, acc = [np.ones(N, F) for _ in range(3)], [np.zeros(N, F) for _ in range(3)]
    x, n, d, alb = ([rep(a[c]) for c in range(3)] for a in (x0, n0, d0, alb0))
    gid = rep(gid0, np.int32)
    inside = np.zeros(N, bool)
    alive = np.ones(N, bool)
    hev, hmax = dict.fromkeys(HIGHLIGHT_EVENTS, 0), [0.0]
    info = dict(depth=[], hit_gid=[], events=[], rays=[])
    with np.errstate(all="ignore"):
        for v in range(0, K + 1):
            idx = np.flatnonzero(alive)
            ev = dict.fromkeys(GLOSS_EVENTS if rough is None else GLOSS_EVENTS + ROUGH_EVENTS, 0)
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
            tri = np.isin(gs, tri_set)
            u = _hash_per_path(seed, frame, n_pixels, cb - 1 if alt == "lobe_stream_is_roulette_stream" else cb, pj, pp_)
            V = vertex(tab, gs, tri, ds, ns, u, inside[idx], alt=alt)
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
            if rough is not None and cand.any():
                t1, t2, _ = disc(seed, frame, n_pixels, cb + 117 + (8 if alt == "disc_from_other_streams" else 0), pj, pp_)
                Lb = lobe(alpha, ds, ns, t1, t2, alt=alt)
                is_rough = cand & Lb["faces"]
                absorbed, degenerate = is_rough & Lb["absorbed"], is_rough & Lb["degenerate"]
                dn = [_sel(is_rough, Lb["dn"][c], dn[c]) for c in range(3)]
                wgt = [_sel(is_rough, (wgt[c] * Lb["G1"]).astype(F), wgt[c]) for c in range(3)]
            thr_s = [thr[c][idx] for c in range(3)]
            go = np.ones(len(idx), bool)
            if v >= 1:
                gathers = np.ones(len(idx), bool) if alt == "gather_at_mirror" else ~spec
                shines = is_rough & (hp is not None and bool(hp["enable"]))
                occ_all = np.zeros(len(idx), bool)
                if sec:
                    su = _hash_per_path(seed, frame, n_pixels, cb - 3, pj, pp_)
                    sv = _hash_per_path(seed, frame, n_pixels, cb - 2, pj, pp_)
                    occ_all = stm.occluded(xs, su, sv, geoms, tris, lt)
                occ = occ_all & gathers
                lit = (_sel(occ, F(0), F(1)) * stm.direct_term(centre, ns, xs)).astype(F)
                L = (ambient + lit).astype(F)
                for c in range(3):
                    add = (acc[c][idx] + (thr_s[c] * (als[c] * L).astype(F)).astype(F)).astype(F)
                    acc[c][idx] = _sel(gathers, add, acc[c][idx])
                if shines.any():
                    # the light's term where a rough vertex behind the first hit gathers
                    m = np.flatnonzero(shines)
                    sub = lambda a: [a[c][m] for c in range(3)]             # noqa: E731
                    xm = sub(xs)
                    if sec:
                        hu, hv = (sv[m], su[m]) if alt == "shadow_streams_swapped" else (su[m], sv[m])
                        lm, dl = light_direction(xm, hu, hv, lt)
                        formed = dl > 0
                        occ_m = stm.occluded(xm, hu, hv, geoms, tris, lt) if alt == "shadow_streams_swapped" else occ_all[m]
                        if alt == "light_centre_for_l":
                            lm = _norm_dt([(centre[c] - xm[c]).astype(F) for c in range(3)])
                    else:
                        lm = _norm_dt([(centre[c] - xm[c]).astype(F) for c in range(3)])
                        formed = np.isfinite(lm[0]) & np.isfinite(lm[1]) & np.isfinite(lm[2])
                        occ_m = np.zeros(len(m), bool)
                    cm, _ = _contribution(hev, hmax, alpha[m], sub(ds), sub(ns), xm, lm, formed, occ_m, centre, hp, alt)
                    hev["deeper"] += len(m)
                    if alt == "divided_by_reflect":
                        cm = (cm / V["reflect"][m]).astype(F)
                    for c in range(3):
                        term = _channel(V["wgt"][c][m], cm, hp, alt)
                        acc[c][idx[m]] = (acc[c][idx[m]] + (thr_s[c][m] * (als[c][m] * term).astype(F)).astype(F)).astype(F)
                if v >= K:
                    alive[idx] = False
                    continue
                thr_s = [(thr_s[c] * (als[c] * wgt[c]).astype(F)).astype(F) for c in range(3)]
                if R > 0 and v >= R:
                    m3 = np.maximum(np.maximum(thr_s[0], thr_s[1]), thr_s[2])
                    q = _sel(m3 < 1, m3, F(1))
                    xi = _hash_per_path(seed, frame, n_pixels, cb - 1, pj, pp_)
                    survive = (q > 0) & (xi < q)
                    go = survive
                    info["depth"][v - 1]["rr_kills"], info["depth"][v - 1]["rr_survivals"] = int((~survive).sum()), int(survive.sum())
                    thr_s = [(thr_s[c] / q).astype(F) for c in range(3)]
            else:
                thr_s = [wgt[c].copy() for c in range(3)]
            # an absorbed path ends at its vertex (the kernel leaves ahead of the roulette; nothing between the two is stored)
            n_absorbed = int((absorbed & go).sum())
            if alt != "absorbed_paths_continue":
                go = go & ~absorbed
            # events are counted where a ray leaves the vertex (not at vertex max_depth, not on a path the roulette has just ended)
            cnt = lambda m: int((m & go).sum())                          # noqa: E731
            if v == 0:
                ev["mirror0"], ev["glass0"] = cnt(V["mirror"]), cnt(V["glass"])
            else:
                ev["mirror"] = cnt(V["mirror"])
            if rough is not None:
                ev["absorbed"] = n_absorbed
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
            back = (-(ORIGIN_FACTOR * t_lo).astype(F)).astype(F)
            moved = V["moved"] & (alt != "origin_not_moved")
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
            if keep_rays:
                info["rays"].append(dict(gid=gs, d=ds, n=ns, dn=dn, nn=V["nn"], moved=V["moved"], mirror=V["mirror"], glass=V["glass"], fresnel=V["fresnel"],
                                         tir=V["tir"], eta=V["eta"], R0=V["R0"], u=u, go=go))
    if hp is not None:
        info.update(highlight=hev, H_max=hmax[0])
    return [a.reshape(J, npix) for a in acc], info
