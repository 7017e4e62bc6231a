"""numpy model of csrc/svgf_scene.hip (k_scene_frame), every branch: primitives with `geom_ids`, the triangle loop that starts from
the primitives' nearest hit, the two corner-weight orders, the texture lookup with both clamps, the miss position, shading and noise.
float32 throughout, one rounding per operation and no contraction, every dot product written ((a0*b0 + a1*b1) + a2*b2) the way the
kernel writes it; arrays are [H, W] planes per component, so no reduction order is left to numpy.  Test infrastructure only.

min / max.  The reference's slab test calls glm::min / glm::max (src/intersections.h:65-66).  Its own copy of GLM
(external/include/glm/detail/func_common.inl:409-435) defines them as

    min(x, y) = x < y ? x : y            max(x, y) = x > y ? x : y

so a NaN in EITHER argument gives y, here t2: with t2 = NaN the slab is skipped (both tests on it are false), with t1 = NaN the
slab's interval collapses onto t2 = +-inf and the ray misses.  (std::min / std::max would give `y < x ? y : x`, `x < y ? y : x`,
which return the FIRST argument on a NaN; that is not what this GLM does.)  fminf / fmaxf return the operand that is not NaN, and
numpy's minimum / maximum return the NaN: each agrees with GLM on one of the two cases only.
The sphere test (src/intersections.h:104-146) leaves at `radicand < 0` before its sqrt, and picks a root with a plain min / max
(fminf / fmaxf on the device).  There a NaN operand needs a NaN radicand, for which `rad >= 0` is false and the primitive is no
hit, and on numbers the selects below, fminf / fmaxf and GLM's definitions all return the same value; fmaxf(rad, 0) only keeps the
sqrt of a rejected radicand finite.  Texture::getColor's glm::min (src/sceneStructs.h:209-210) has a finite second argument, so
fminf gives the same.  The Lambert term's fmaxf(., 0) is the producer's own shading stub, not the reference's: it maps a NaN
(a mesh without normals) to 0, and is written here as the select that does the same.

`alt` names ONE deliberate deviation (tests/test_scene_model.py, "each edge acts"): the model then computes what a kernel with
that mistake would, so a test can count the pixels on which its scene tells the two apart.
"""
import numpy as np

import __graft_entry__ as ge

_pkg = ge.load_package()
synth = _pkg.synth
F = np.float32
CUBE = 0
EPS = F(1.1920929e-7)

ALTS = ("fminmax_slab", "nan_slab", "std_slab", "tri_le", "no_cull", "normal_uv_weights", "uv_normal_weights", "tri_albedo_shift",
        "tex_x_shift", "tex_y_shift", "no_clamp_low", "no_clamp_high", "tex_ignore", "tex_swap", "geom_ids_identity", "tri_from_inf",
        "lam_nan", "no_inside", "sphere_near_root", "sphere_normal_xf", "cube_normal_unrotated")


def _dot(a, b):
    return ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]).astype(F)


def _normalise(v):
    l = np.sqrt(_dot(v, v))
    return [(v[0] / l).astype(F), (v[1] / l).astype(F), (v[2] / l).astype(F)]


def _apply34(m, v, w):      # 3x4 row-major times (v, w): ((m0*v0 + m1*v1) + m2*v2) + m3*w
    return [(((m[4 * r] * v[0] + m[4 * r + 1] * v[1]) + m[4 * r + 2] * v[2]) + m[4 * r + 3] * F(w)).astype(F) for r in range(3)]


def _sel(c, a, b):
    return np.where(c, a, b).astype(F)


def rays(W, H, cam, pixel_length=None):
    """Primary ray directions as three [H, W] planes, and the pixel lengths used."""
    if pixel_length is None:
        pixel_length = synth._pixel_length(W, H, cam.get("fovy_deg", 45.0))
    plx, ply = F(pixel_length[0]), F(pixel_length[1])
    x = np.broadcast_to(np.arange(W, dtype=F)[None, :], (H, W))
    y = np.broadcast_to(np.arange(H, dtype=F)[:, None], (H, W))
    sx, sy = plx * (x - F(W * 0.5 - 0.5)), ply * (y - F(H * 0.5 - 0.5))
    r, u, v = (np.asarray(cam[k], dtype=F) for k in ("right", "up", "view"))
    return _normalise([((v[c] - r[c] * sx) - u[c] * sy).astype(F) for c in range(3)])


def render(W, H, frame, cam, geoms, geom_ids, tris, tri_ids, tri_albedo, tri_tex, textures, light, seed=1, noise=0.6,
           fireflies=0.02, pixel_length=None, *, alt=None):
    """(color float32[H, W, 3], gbuffer GBUFFER_DTYPE[H, W]) of svgf_scene_render_mesh.  geoms: scene.SCENE_GEOM_DTYPE records (or
    None); geom_ids: None = the primitive's index; tris: float32[n, 3, 8] = pos, normal, uv per corner (or None); tri_tex: None = no
    textures; textures: list of uint8[h, w, 3], rows top to bottom."""
    assert alt is None or alt in ALTS, alt
    n_geoms = 0 if geoms is None else len(geoms)
    tris = np.zeros((0, 24), F) if tris is None else np.ascontiguousarray(tris, dtype=F).reshape(-1, 24)
    tri_albedo = None if tri_albedo is None else np.asarray(tri_albedo, dtype=F).reshape(-1, 3)
    if alt == "geom_ids_identity":
        geom_ids = None
    o = [F(c) for c in np.asarray(cam["position"], dtype=F)]
    shape = (H, W)
    full = lambda v, dt=F: np.full(shape, v, dtype=dt)      # noqa: E731

    with np.errstate(all="ignore"):
        d = rays(W, H, cam, pixel_length)
        t_best = full(np.inf)
        gid = full(-1, np.int32)
        n, ph, alb = [full(0) for _ in range(3)], [full(0) for _ in range(3)], [full(0) for _ in range(3)]
        emit = full(0)

        for k in range(n_geoms):
            g = geoms[k]
            inv, xf, invT = (np.asarray(g[f], dtype=F) for f in ("inv", "xf", "invT"))
            qo = _apply34(inv, [full(c) for c in o], 1.0)
            qd = _normalise(_apply34(inv, d, 0.0))
            if int(g["type"]) == CUBE:      # slab test, entering face (or leaving face when the origin is inside)
                tmin, tmax = full(-1e38), full(1e38)
                amin, amax = full(0, np.int32), full(0, np.int32)
                for ax in range(3):
                    t1, t2 = ((F(-0.5) - qo[ax]) / qd[ax]).astype(F), ((F(0.5) - qo[ax]) / qd[ax]).astype(F)
                    if alt == "fminmax_slab":
                        ta, tb = np.fmin(t1, t2), np.fmax(t1, t2)
                    elif alt == "nan_slab":
                        ta, tb = np.minimum(t1, t2), np.maximum(t1, t2)
                    elif alt == "std_slab":
                        ta, tb = _sel(t2 < t1, t2, t1), _sel(t1 < t2, t2, t1)
                    else:                   # glm::min / glm::max of the reference's GLM, see the module's docstring
                        ta, tb = _sel(t1 < t2, t1, t2), _sel(t1 > t2, t1, t2)
                    up = (ta > 0) & (ta > tmin)
                    tmin, amin = _sel(up, ta, tmin), np.where(up, ax, amin)
                    dn = tb < tmax
                    tmax, amax = _sel(dn, tb, tmax), np.where(dn, ax, amax)
                hit = (tmax >= tmin) & (tmax > 0)
                inside = (tmin <= 0) & (alt != "no_inside")
                tt = _sel(inside, tmax, tmin)
                axis = np.where(inside, amax, amin)
                qda = _sel(axis == 0, qd[0], _sel(axis == 1, qd[1], qd[2]))
                sgn = _sel(qda < 0, F(1), F(-1))                                    # the face normal that looks at the ray
                no = [_sel(axis == c, sgn, F(0)) for c in range(3)]
                nw = no if alt == "cube_normal_unrotated" else _normalise(_apply34(xf, no, 0.0))
            else:                           # unit sphere, radius 0.5
                b = _dot(qo, qd)
                rad = (b * b - (_dot(qo, qo) - F(0.25))).astype(F)
                sq = np.sqrt(_sel(rad > 0, rad, F(0)))
                ta, tb = (-b + sq).astype(F), (-b - sq).astype(F)
                both_pos, both_neg = (ta > 0) & (tb > 0), (ta < 0) & (tb < 0)
                tt = _sel(both_pos, _sel(tb < ta, tb, ta), _sel(ta < tb, tb, ta))
                if alt == "sphere_near_root":
                    tt = _sel(tb < ta, tb, ta)
                hit = (rad >= 0) & ~both_neg
                po = [(qo[c] + tt * qd[c]).astype(F) for c in range(3)]
                if alt == "sphere_normal_xf":
                    nw = _normalise(_apply34(xf, po, 0.0))
                else:
                    nw = _normalise([((invT[3 * r] * po[0] + invT[3 * r + 1] * po[1]) + invT[3 * r + 2] * po[2]).astype(F) for r in range(3)])
            po = [(qo[c] + tt * qd[c]).astype(F) for c in range(3)]
            pw = _apply34(xf, po, 1.0)
            dv = [(o[c] - pw[c]).astype(F) for c in range(3)]
            tw = np.sqrt(_dot(dv, dv))                                              # t is measured in world space
            take = hit & (tw > F(1e-4)) & (tw < t_best)
            t_best = _sel(take, tw, t_best)
            gid = np.where(take, np.int32(k if geom_ids is None else geom_ids[k]), gid).astype(np.int32)
            for c in range(3):
                n[c], ph[c], alb[c] = _sel(take, nw[c], n[c]), _sel(take, pw[c], ph[c]), _sel(take, F(g["albedo"][c]), alb[c])
            emit = _sel(take, F(g["emittance"]), emit)

        # triangles: glm::intersectRayTriangle over every triangle, strictly nearer than the best so far, which starts at the primitives'
        best = full(-1, np.int64)
        bt = full(np.inf) if alt == "tri_from_inf" else t_best.copy()
        bbx, bby = full(0), full(0)
        for i in range(len(tris)):
            T = tris[i]
            e1, e2 = [F(T[8 + c] - T[c]) for c in range(3)], [F(T[16 + c] - T[c]) for c in range(3)]
            pv = [(d[1] * e2[2] - e2[1] * d[2]).astype(F), (d[2] * e2[0] - e2[2] * d[0]).astype(F), (d[0] * e2[1] - e2[0] * d[1]).astype(F)]
            det = _dot(e1, pv)
            go = ~(det < EPS) if alt != "no_cull" else ~(np.abs(det) < EPS)
            f = (F(1) / det).astype(F)
            sv = [F(o[c] - T[c]) for c in range(3)]
            bx = (f * _dot(sv, pv)).astype(F)
            go &= ~((bx < 0) | (bx > 1))
            q = [F(sv[1] * e1[2] - e1[1] * sv[2]), F(sv[2] * e1[0] - e1[2] * sv[0]), F(sv[0] * e1[1] - e1[0] * sv[1])]
            by = (f * _dot(d, q)).astype(F)
            go &= ~((by < 0) | ((by + bx).astype(F) > 1))
            t = (f * F((e2[0] * q[0] + e2[1] * q[1]) + e2[2] * q[2])).astype(F)
            go &= (t > 0) & ((t <= bt) if alt == "tri_le" else (t < bt))
            bt, best, bbx, bby = _sel(go, t, bt), np.where(go, i, best), _sel(go, bx, bbx), _sel(go, by, bby)
        if len(tris):
            mesh = best >= 0
            bi = np.maximum(best, 0)
            T = [tris[bi, j] for j in range(24)]
            w2 = ((F(1) - bbx) - bby).astype(F)
            wn, wu = (bbx, bby, w2), (w2, bbx, bby)             # the reference's normal weights and its uv weights differ (sic)
            if alt == "normal_uv_weights":
                wn = wu
            if alt == "uv_normal_weights":
                wu = wn
            nt = _normalise([((T[3 + c] * wn[0] + T[11 + c] * wn[1]) + T[19 + c] * wn[2]).astype(F) for c in range(3)])
            ai = np.minimum(bi + 1, len(tris) - 1) if alt == "tri_albedo_shift" else bi
            at = [tri_albedo[ai, c] for c in range(3)]
            if tri_tex is not None and textures is not None and len(textures) and alt != "tex_ignore":
                tx = np.asarray(tri_tex, dtype=np.int32)[bi]
                u = ((T[6] * wu[0] + T[14] * wu[1]) + T[22] * wu[2]).astype(F)
                v = ((T[7] * wu[0] + T[15] * wu[1]) + T[23] * wu[2]).astype(F)
                for k, tex in enumerate(textures):              # Texture::getColor at the interpolated uv
                    tex = np.asarray(tex, dtype=np.uint8)
                    if alt == "tex_swap":
                        tex = np.asarray(textures[(k + 1) % len(textures)], dtype=np.uint8)
                    th, tw_ = tex.shape[0], tex.shape[1]
                    fx, fy = ((F(1) * F(tw_)) * u).astype(F), ((F(1) * F(th)) * (F(1) - v)).astype(F)
                    cx, cy = F(F(1) * F(tw_) - F(1)), F(F(1) * F(th) - F(1))
                    if alt != "no_clamp_high":
                        fx, fy = _sel(fx < cx, fx, cx), _sel(fy < cy, fy, cy)
                    # (int) truncates towards zero and X < 0 ? 0 : X follows: the same as truncating max(., 0), which keeps numpy's
                    # cast away from values below INT_MIN
                    X, Y = np.trunc(_sel(fx < 0, F(0), fx)).astype(np.int64), np.trunc(_sel(fy < 0, F(0), fy)).astype(np.int64)
                    if alt in ("no_clamp_low", "no_clamp_high"):    # a missing clamp indexes out of bounds; a wrapped index stands in
                        X, Y = np.trunc(np.nan_to_num(fx)).astype(np.int64), np.trunc(np.nan_to_num(fy)).astype(np.int64)
                        X, Y = (np.maximum(X, 0) if alt == "no_clamp_high" else X) % tw_, (np.maximum(Y, 0) if alt == "no_clamp_high" else Y) % th
                    if alt == "tex_x_shift":
                        X = np.minimum(X + 1, tw_ - 1)
                    if alt == "tex_y_shift":
                        Y = np.minimum(Y + 1, th - 1)
                    px = tex[np.clip(Y, 0, th - 1), np.clip(X, 0, tw_ - 1)]
                    for c in range(3):
                        at[c] = _sel(tx == k, F(0.003921568627) * px[..., c].astype(F), at[c])
            for c in range(3):
                n[c], ph[c], alb[c] = _sel(mesh, nt[c], n[c]), _sel(mesh, (o[c] + bt * d[c]).astype(F), ph[c]), _sel(mesh, at[c], alb[c])
            emit = _sel(mesh, F(0), emit)
            gid = np.where(mesh, np.asarray(tri_ids, dtype=np.int32)[bi], gid).astype(np.int32)

        miss = gid < 0
        pos = [_sel(miss, (o[c] + F(-1.0) * d[c]).astype(F), ph[c]) for c in range(3)]      # t = -1 on a miss
        light = [F(c) for c in np.asarray(light, dtype=F)]
        tl = [(light[c] - pos[c]).astype(F) for c in range(3)]
        dist2 = _dot(tl, tl)
        dl = np.sqrt(dist2)
        lam = _dot([(tl[c] / dl).astype(F) for c in range(3)], n)
        lam = np.maximum(lam, F(0)) if alt == "lam_nan" else _sel(lam > 0, lam, F(0))       # fmaxf(lam, 0): a NaN gives 0
        shade = (F(0.15) + (F(30.0) * lam).astype(F) / (F(4.0) + dist2).astype(F)).astype(F)
        shade = _sel(emit > 0, emit, shade)

        hu = lambda k: synth.hash_uniform(seed, frame, W * H, k).reshape(H, W)              # noqa: E731
        mult = (F(1.0) + F(noise) * (F(2.0) * hu(0) - F(1.0)).astype(F)).astype(F)
        mult = _sel(hu(1) < F(fireflies), (mult * F(6.0)).astype(F), mult)
        amp = F(F(0.1) * F(noise))
        col = [_sel(miss, F(0), (((alb[c] * shade).astype(F) * mult).astype(F) * (F(1.0) + amp * (hu(2 + c) - F(0.5)).astype(F)).astype(F)).astype(F))
               for c in range(3)]

    gb = np.zeros(shape, dtype=synth.GBUFFER_DTYPE)
    gb["normal"], gb["position"], gb["albedo"] = np.stack(n, -1), np.stack(pos, -1), np.stack(alb, -1)
    gb["ialbedo"] = F(1.0)
    gb["geomId"] = gid
    return np.ascontiguousarray(np.stack(col, -1).astype(F)), gb
