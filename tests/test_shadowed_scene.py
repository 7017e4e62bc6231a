"""The shadowed resident scene (include/svgf.h row f16: svgf_scene_draw_shadowed).

The yardstick is tests/scene_shadow_model.py: scene_model.render's first hit, then the header's rule as a brute force over every
occluder, float32 with the kernel's nesting.  Both sides perform the same operations in the same order without contraction and
occlusion is an OR, so there is no tolerance to choose: colour and every G-buffer field are compared on bits (NaNs in the same place
count as equal), expected and allowed number of differing pixels: 0.

CPU part: the model's own properties (an empty path to the light gives scene_model's frame, a point light gives vis 0 or 1, a
half-blocked light gives the blocked share within the binomial band, the light's own emitter casts no shadow, dl == 0 gives no NaN),
every `alt` of the model acts on some scene, and the (pixel, sample) pairs on which the gate changes the answer are counted.
GPU part: the device against the model.

The binomial band.  With S samples per pixel and per-pixel blocked share b_p (analytic: the occluder is a half-plane sheet just
under a horizontal light over a horizontal floor, so a sample is blocked iff u lies below a threshold that depends on the pixel's
x), the mean visibility over N pixels has expectation mean(1 - b_p) and variance sum(b_p (1 - b_p)) / (S N^2); the band is 4 sigma.
"""
import ctypes
import functools

import numpy as np
import pytest

import scene_model as sm
import scene_pose_model as pm
import scene_shadow_model as ssm
import test_animated_scene as tas
import test_resident_scene as trs
import test_scene_model as tsm
from test_scene_model import FRAME, SEED, counts

F = np.float32
BUILDS = trs.BUILDS
SIZES = [(1, 1), (7, 5), (65, 4), (257, 3)]         # one lane; one partial wave; a wave seam; a block seam and a one-lane tail
EDGE = ("A", "B", "F_cube", "F_sphere", "E_plus")


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def _basis(n):
    n = np.asarray(n, np.float64) / np.linalg.norm(n)
    a = np.cross(n, (0.0, 0.0, 1.0) if abs(n[2]) < 0.9 else (1.0, 0.0, 0.0))
    a /= np.linalg.norm(a)
    return n, a, np.cross(n, a)


def _add(pkg, s, geoms=(), tris=(), ids=(90, 91, 92, 93, 94, 95)):
    """A copy of scene dict s with primitives (tsm._geoms records) and triangles (tsm._tri) added under fresh object ids."""
    s = dict(s)
    ids = list(ids)
    if len(geoms):
        g = tsm._geoms(pkg, *geoms)
        old = s["geoms"] if s["geoms"] is not None else np.zeros(0, g.dtype)
        if s["geom_ids"] is not None:
            s["geom_ids"] = np.concatenate([s["geom_ids"], np.array([ids.pop() for _ in geoms], np.int32)])
        s["geoms"] = np.concatenate([old, g])
    if len(tris):
        t = np.stack(tris)
        n_old = 0 if s["tris"] is None else len(s["tris"])
        s["tris"] = t if not n_old else np.concatenate([np.asarray(s["tris"], F), t])
        s["tri_ids"] = np.concatenate([s["tri_ids"] if n_old else np.zeros(0, np.int32), np.array([ids.pop() for _ in tris], np.int32)])
        s["tri_albedo"] = np.concatenate([s["tri_albedo"] if n_old else np.zeros((0, 3), F), tsm._colours(len(tris), 16)])
        if s["tri_tex"] is not None:
            s["tri_tex"] = np.concatenate([s["tri_tex"], np.full(len(tris), -1, np.int32)])
    return s


def _sheet(centre, n, size):
    """Two triangles on the same three points with opposite windings, perpendicular to n: one of them faces any ray that crosses."""
    _, a, b = _basis(n)
    c = np.asarray(centre, np.float64)
    p0, p1, p2 = c + size * a, c + size * b, c - size * (a + b)
    return [tsm._tri(p0, p1, p2, k=1), tsm._tri(p0, p2, p1, k=2)]


@functools.lru_cache(maxsize=None)
def _edge(name):
    """(scene, light kwargs): an edge scene of test_resident_scene.py with an occluder - a two-sided triangle sheet and a sphere, or
    for E_plus (no triangles: n_tris == 0 stays) a cube and a sphere - between what the camera looks at and the light."""
    import __graft_entry__ as ge
    pkg = ge.load_package()
    s = tsm._scene(name)
    target = {"A": (0, 0, 0), "B": (0, 0, 1), "F_cube": (0, -3, -2), "F_sphere": (0, -2, -2), "E_plus": (2, 2, 2)}[name]
    L, T = np.asarray(s["light"], np.float64), np.asarray(target, np.float64)
    mid, n = 0.5 * (L + T), L - T
    size = 0.22 * np.linalg.norm(n)
    _, a, b = _basis(n)
    ball = (1, tuple(mid + 1.2 * size * a), (0, 0, 0), (size, size, size), (0.5, 0.6, 0.7), 0.0)
    if name == "E_plus":
        s = _add(pkg, s, geoms=[(0, tuple(mid - 0.8 * size * a), (10, 20, 30), (size, size, 0.3 * size), (0.6, 0.5, 0.4), 0.0), ball])
    elif name == "A":       # triangles only: n_geoms == 0 stays
        s = _add(pkg, s, tris=_sheet(mid, n, size) + _sheet(mid + 1.5 * size * a + 0.1 * n, n, 0.5 * size)[:1])
    else:
        s = _add(pkg, s, geoms=[ball], tris=_sheet(mid - 0.5 * size * a, n, size))
    return s, dict(centre=tuple(s["light"]), edge_u=tuple(0.35 * size * a), edge_v=tuple(0.35 * size * b))


@functools.lru_cache(maxsize=None)
def _stage():
    """Primitives and triangles made for the rules: a floor (cube), an occluding cube over it, an EMITTING sphere between the two that
    is half under the cube, the light's own emitting cube around the light's centre, and a ceiling triangle that faces down and
    passes exactly through the light's centre (the light's parallelogram lies in its plane: t of that triangle is dl but for
    rounding)."""
    import __graft_entry__ as ge
    pkg = ge.load_package()
    geoms = tsm._geoms(pkg, (0, (0, -0.5, 0), (0, 0, 0), (12, 1, 12), (0.8, 0.8, 0.8), 0.0), (0, (0, 6, 0), (0, 0, 0), (1.5, 0.5, 1.5), (1, 1, 1), 5.0),
                       (0, (-1.5, 3, 0), (0, 15, 0), (2, 0.25, 2), (0.7, 0.4, 0.3), 0.0), (1, (-0.4, 1.2, 0.3), (0, 0, 0), (1.2, 1.2, 1.2), (1, 0.9, 0.8), 2.0))
    up = tsm._tri((-4, 6, -4), (4, 6, -4), (0, 6, 5))
    down = tsm._tri((-4, 6, -4), (0, 6, 5), (4, 6, -4))
    s = dict(cam=tsm._cam(pkg, (0, 4.5, 9), (0, 0.5, 0), 30.0), geoms=geoms, geom_ids=np.array([3, 4, 5, 6], np.int32), tris=np.stack([up, down]),
             tri_ids=np.array([7, 8], np.int32), tri_albedo=tsm._colours(2, 7), tri_tex=None, textures=None, light=tuple(pkg.scene.light_position(geoms)))
    return s, dict(centre=s["light"], edge_u=(0.7, 0, 0), edge_v=(0, 0, 0.7))


@functools.lru_cache(maxsize=None)
def _half():
    """A triangle floor at y = 0 under a horizontal light at y = 5, and a two-sided sheet at y = 4.95 that covers x < 0."""
    import __graft_entry__ as ge
    pkg = ge.load_package()
    floor = [tsm._tri((-6, 0, -6), (-6, 0, 6), (6, 0, 6)), tsm._tri((-6, 0, -6), (6, 0, 6), (6, 0, -6))]
    sheet = [tsm._tri((0, 4.95, -40), (0, 4.95, 40), (-80, 4.95, 0)), tsm._tri((0, 4.95, -40), (-80, 4.95, 0), (0, 4.95, 40))]
    s = dict(cam=tsm._cam(pkg, (0, 6, 8), (0, 0, 0), 25.0), geoms=tsm._geoms(pkg), geom_ids=None, tris=np.stack(floor + sheet),
             tri_ids=np.array([1, 1, 2, 2], np.int32), tri_albedo=tsm._colours(4, 8), tri_tex=None, textures=None, light=(0.0, 5.0, 0.0))
    return s, dict(centre=s["light"], edge_u=(1.0, 0, 0), edge_v=(0, 0, 0.5))


@functools.lru_cache(maxsize=None)
def _graze():
    """The scene on which the GATE decides samples.  A wall, an occluder (both windings) and the light lie in ONE plane, turned out
    of the axes; the light's centre stands 1e-6 behind it.  A shadow ray then runs within rounding of the occluder's plane: the
    determinant of the triangle test is a difference of products that cancel to a few 1e-7, its reciprocal is wrong by a factor of
    order one, and with it t - the float32 test accepts hits that lie nowhere near the triangle, before the ray has reached its
    padded box (t < tn).  The contract drops them; an ungated brute force would not."""
    import __graft_entry__ as ge
    from temporal_harness import rotation
    pkg = ge.load_package()
    R = rotation("x", 25.0) @ rotation("y", -35.0)
    P = lambda x, y, z=0.0: tuple(float(c) for c in R @ np.array([x, y, z], np.float64))      # noqa: E731
    tris = [tsm._tri(P(-4, -3), P(2, -3), P(-4, 3)), tsm._tri(P(2, -3), P(2, 3), P(-4, 3), k=1),
            tsm._tri(P(3, -1.5), P(4.5, 0), P(3, 1.5), k=2), tsm._tri(P(3, -1.5), P(3, 1.5), P(4.5, 0), k=3)]
    s = dict(cam=tsm._cam(pkg, P(0, 0, 9), P(0, 0, 0), 25.0), geoms=tsm._geoms(pkg), geom_ids=None, tris=np.stack(tris),
             tri_ids=np.array([1, 1, 2, 3], np.int32), tri_albedo=tsm._colours(4, 9), tri_tex=None, textures=None, light=P(8, 0, -1e-6))
    return s, dict(centre=s["light"], edge_u=P(0, 0.5, 0), edge_v=(0.0, 0.0, 0.0))


def _args(s):
    return s["cam"], s["geoms"], s["geom_ids"], s["tris"], s["tri_ids"], s["tri_albedo"], s["tri_tex"], s["textures"]


@functools.lru_cache(maxsize=None)
def _first(kind, name, W, H, frame, seed, noise=0.6):
    """scene_model.render's frame and the emitter mask of an input: computed once, shared, never written to."""
    s = _input(kind, name)[0]
    first = sm.render(W, H, frame, *_args(s), s["light"], seed=seed, noise=noise, fireflies=0.02 if noise else 0.0)
    em = ssm.emitter_mask(W, H, s["cam"], s["geoms"], s["geom_ids"], s["tris"], s["tri_ids"])
    for a in first + (em,):
        a.setflags(write=False)
    return first, em


def _input(kind, name):
    if kind == "edge":
        return _edge(name)
    if kind == "made":
        return {"stage": _stage, "half": _half, "graze": _graze}[name]()
    if kind == "plain":                                     # an edge scene as it is, with a small area light
        s = tsm._scene(name)
        return s, dict(centre=tuple(s["light"]), edge_u=(0.2, 0, 0), edge_v=(0, 0.2, 0))
    s, W, H = trs._recorded(name, 0)
    return s, dict(centre=tuple(float(c) for c in s["light"]), edge_u=(0.5, 0, 0), edge_v=(0, 0, 0.5))


@functools.lru_cache(maxsize=None)
def _model(kind, name, W, H, samples, point=False, alt=None, frame=FRAME, seed=SEED, noise=0.6, centre=None):
    s, lk = _input(kind, name)
    lt = ssm.light(centre or lk["centre"], samples=samples) if point else ssm.light(centre or lk["centre"], lk["edge_u"], lk["edge_v"], samples)
    if centre is None:
        first, em = _first(kind, name, W, H, frame, seed, noise)
    else:
        first = sm.render(W, H, frame, *_args(s), centre, seed=seed, noise=noise, fireflies=0.02 if noise else 0.0)
        em = _first(kind, name, W, H, frame, seed, noise)[1]
    col, gb, info = ssm.render(W, H, frame, *_args(s), lt, seed=seed, noise=noise, fireflies=0.02 if noise else 0.0, alt=alt, first=first, emitters=em)
    col.setflags(write=False)
    return (col, gb), info, lt


def _no_difference(got, ref, what):
    c = counts(got, ref)
    print(f"{what}: differing pixels {c} (expected and allowed: 0)")
    assert not any(c.values()), f"{what}: {c}"


# ---- CPU 1: the model's own properties -------------------------------------------------------------------------------------------------
def test_an_empty_path_to_the_light_gives_scene_models_frame():
    """Scene C (textured quads in one plane, the light in front of it) and scene D (NaN normals): no sample is occluded - t_lo keeps
    the surface from shadowing itself - and colour and G-buffer are scene_model.render's on every bit."""
    for name in ("C", "D"):
        W, H = 67, 41
        (col, gb), info, _ = _model("plain", name, W, H, 3)
        first = _first("plain", name, W, H, FRAME, SEED)[0]
        print(f"scene {name}: {int(info['cast'].sum())} pixels cast rays, {int(info['occluded'].sum())} samples occluded")
        if name == "C":
            assert info["cast"].sum() > 1000 and not info["occluded"].any()
            _no_difference((col, gb), first, f"scene {name}, shadowed model vs scene_model")
        for f in tsm.FIELDS:
            assert not tsm.differing(gb[f], first[1][f]).any(), f
        assert not tsm.differing(col, first[0])[info["vis"] == 1].any()


def test_a_point_light_gives_hard_shadows():
    for name in EDGE:
        _, info, _ = _model("edge", name, 67, 41, 3, point=True)
        vis = info["vis"][info["cast"]]
        dark = int((vis == 0).sum())
        print(f"scene {name}: point light, {len(vis)} pixels cast, {dark} dark")
        assert np.isin(vis, (0.0, 1.0)).all() and 0 < dark < len(vis)


def test_area_light_gives_penumbrae_on_every_edge_scene():
    for name in EDGE:
        _, info, _ = _model("edge", name, 67, 41, 64)
        vis = info["vis"][info["cast"]]
        part = int(((vis > 0) & (vis < 1)).sum())
        print(f"scene {name}: 64 samples, {len(vis)} pixels cast, {int((vis == 0).sum())} dark, {part} in a penumbra")
        assert part > 10 and (vis == 1).sum() > 10


def test_half_blocked_light_is_inside_the_binomial_band():
    W, H, S = 67, 41, 64
    (_, gb), info, lt = _model("made", "half", W, H, S)
    floor = (gb["geomId"] == 1) & (np.abs(gb["position"][..., 0]) < 4)
    px, py = gb["position"][..., 0][floor].astype(np.float64), gb["position"][..., 1][floor].astype(np.float64)
    tau = 0.05 / (5.0 - py)                                 # the sheet lies 0.05 under the light: the crossing is L (1 - tau) + p tau
    blocked = np.clip(0.5 + (-px * tau / (1.0 - tau)) / (2.0 * lt["edge_u"][0]), 0.0, 1.0)
    want, sigma = float((1.0 - blocked).mean()), float(np.sqrt((blocked * (1.0 - blocked)).sum() / S) / len(px))
    got = float(info["vis"][floor].astype(np.float64).mean())
    print(f"half-blocked light: {len(px)} floor pixels x {S} samples, blocked share {blocked.min():.4f}..{blocked.max():.4f}, mean visibility {got:.5f}, "
          f"expected {want:.5f} +- {sigma:.5f} (1 sigma)")
    assert len(px) > 500 and abs(got - want) <= 4.0 * sigma


def test_the_lights_own_emitter_casts_no_shadow_and_emitters_cast_no_ray():
    W, H = 67, 41
    (col, gb), info, _ = _model("made", "stage", W, H, 3, point=True)
    first, em = _first("made", "stage", W, H, FRAME, SEED)
    assert em.sum() > 10 and not info["cast"][em].any() and not tsm.differing(col, first[0])[em].any()
    floor = (gb["geomId"] == 3) & (gb["position"][..., 0] > 1.5)      # beside the occluding cube and the emitting sphere: only the light's cube is above
    print(f"stage: {int(em.sum())} emitter pixels, {int(floor.sum())} floor pixels under the light's own cube alone")
    assert floor.sum() > 100 and (info["vis"][floor] == 1).all()
    with_emitters = _model("made", "stage", W, H, 3, point=True, alt="emitter_occludes")[1]["vis"]
    assert (with_emitters[floor] == 0).all()


def test_a_light_on_the_surface_gives_no_nan():
    W, H = 67, 41
    first = _first("edge", "B", W, H, FRAME, SEED)[0]
    y, x = 20, 40
    assert first[1]["geomId"][y, x] >= 0
    centre = tuple(float(c) for c in first[1]["position"][y, x])
    (col, gb), info, _ = _model("edge", "B", W, H, 3, point=True, centre=centre)
    j = int(np.flatnonzero(info["pixels"] == y * W + x)[0])
    assert (info["dl"][:, j] == 0).all() and not info["occluded"][:, j].any()
    assert np.isfinite(col).all() and info["vis"][y, x] == 1


# ---- CPU 2: each alt acts, and the gate --------------------------------------------------------------------------------------------------
ALT_SCENES = [("edge", n) for n in EDGE] + [("made", "stage"), ("made", "half"), ("made", "graze")]


def test_each_alt_acts():
    """Pixels on which the frame of the model and of a wrong variant of it differ, per scene (67x41, 3 samples): every alt changes
    some scene."""
    W, H = 67, 41
    total = {a: 0 for a in ssm.ALTS}
    for kind, name in ALT_SCENES:
        ref = _model(kind, name, W, H, 3)[0]
        row = {}
        for alt in ssm.ALTS:
            row[alt] = tsm.any_differs(_model(kind, name, W, H, 3, alt=alt)[0], ref)
            total[alt] += row[alt]
        print(f"scene {name}: {row}")
    print(f"all scenes: {total}")
    for alt, n in total.items():
        assert n > 0, f"`{alt}` changes no pixel of any scene"


GATE_ZERO = [("edge", "A"), ("edge", "B"), ("edge", "F_cube"), ("edge", "F_sphere"), ("edge", "E_plus"), ("made", "stage"), ("made", "half"),
             ("rec", "cornell"), ("rec", "room")]


@pytest.mark.parametrize("kind,name", GATE_ZERO)
def test_the_gate_changes_no_sample(kind, name):
    """(pixel, sample) pairs whose occlusion differs between the contract and an ungated brute force."""
    W, H, S = {"cornell": (96, 96, 3), "room": (128, 72, 1)}.get(name, (67, 41, 3))
    info = _model(kind, name, W, H, S, frame=0 if kind == "rec" else FRAME, seed=1 if kind == "rec" else SEED)[1]
    print(f"{name} {W}x{H}, {S} samples: {info['occluded'].size} (pixel, sample) pairs, {int(info['occluded'].sum())} occluded, "
          f"ungated differs on {info['ungated_differs']}")
    assert info["occluded"].any() and info["ungated_differs"] == 0


def test_the_gate_decides_samples_of_the_grazing_scene():
    """The one scene here on which it is NOT zero (DESIGN 5.4h names it): made for it, see _graze."""
    W, H, S = 67, 41, 3
    info = _model("made", "graze", W, H, S)[1]
    print(f"graze {W}x{H}, {S} samples: {info['occluded'].size} (pixel, sample) pairs, {int(info['occluded'].sum())} occluded, "
          f"ungated differs on {info['ungated_differs']}")
    assert info["ungated_differs"] > 0


# ---- CPU 3: what examples/shadowed_scene.cpp measures, on the oracle ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _example_scene():
    """The room of examples/shadowed_scene.cpp with its block at rest, under the example's light and the synthetic scene's camera."""
    import __graft_entry__ as ge
    pkg = ge.load_package()
    z = (0, 0, 0)
    geoms = tsm._geoms(pkg, (0, (0, 0, 0), z, (12, 0.2, 12), (0.8, 0.8, 0.8), 0.0), (0, (0, 5, -6), z, (12, 10, 0.2), (0.8, 0.8, 0.7), 0.0),
                       (0, (-6, 5, 0), z, (0.2, 10, 12), (0.8, 0.3, 0.3), 0.0), (0, (6, 5, 0), z, (0.2, 10, 12), (0.3, 0.8, 0.3), 0.0),
                       (0, (0, 9.9, 0), z, (3, 0.1, 3), (1, 1, 1), 5.0), (0, (-2.5, 1.1, 0), z, (2, 2, 2), (0.3, 0.4, 0.9), 0.0))
    return geoms, pkg.synth.camera_for_frame(0, False), dict(centre=(0.0, 9.5, 0.0), edge_u=(1.5, 0.0, 0.0), edge_v=(0.0, 0.0, 1.5))


def test_denoised_shadow_beats_the_noisy_one_after_eight_static_frames(pkg, orc):
    """64x36, noise 0 (the visibility estimate is the only noise), eight frames of the scene at rest: one shadow ray per pixel through
    the oracle's full SVGF against the 64-ray frame, by tests/quality_model.py.  The gate is the issue's: the denoised frame beats the
    noisy one in PSNR and in SSIM.  Recorded on the last frame: noisy 43.95 dB / SSIM 0.9972, denoised 46.42 dB / SSIM 0.9983 (few of the
    2 304 pixels lie in the penumbra: the camera sees the floor at a flat angle)."""
    import quality_model as qm
    from temporal_harness import scales
    W, H, N = 64, 36, 8
    geoms, cam, lk = _example_scene()
    p = pkg.reference_defaults().set(temporal_enable=1, spatial_enable=1)
    p.reproj_scale[0], p.reproj_scale[1] = scales(pkg, W, H)
    first = sm.render(W, H, 0, cam, geoms, None, None, None, None, None, None, lk["centre"], seed=7, noise=0.0, fireflies=0.0)
    em = ssm.emitter_mask(W, H, cam, geoms, None, None, None)
    o = orc.Oracle(pkg, W, H, threads=4)
    try:
        for f in range(N):
            frame = lambda samples: ssm.render(W, H, f, cam, geoms, None, None, None, None, None, None, ssm.light(samples=samples, **lk), seed=7,   # noqa: E731
                                               noise=0.0, fireflies=0.0, first=first, emitters=em)
            noisy, gb, info = frame(1)
            out = o.denoise(noisy, gb, cam, p).reshape(H, W, 3)
    finally:
        o.free()
    ref = frame(64)[0]
    qn, qd = qm.meter(noisy, ref), qm.meter(out, ref)
    print(f"frame {N - 1}: noisy {qn['psnr_db']:.2f} dB / SSIM {qn['mean_ssim']:.4f}, denoised {qd['psnr_db']:.2f} dB / SSIM {qd['mean_ssim']:.4f}; "
          f"{int((frame(64)[2]['vis'] < 1).sum())} pixels of the reference are shadowed")
    assert qd["psnr_db"] > qn["psnr_db"] and qd["mean_ssim"] > qn["mean_ssim"]


# ---- CPU 4: argument errors answered before any device work ------------------------------------------------------------------------------
def test_argument_errors_without_a_device(pkg):
    lib, B = pkg.load_library(), pkg.binding
    cam, sp, planes = B.SvgfCamera(), B.SvgfSynthParams(), B.SvgfPlanarGBuffer()
    ok = B.SvgfSceneLight.make((0, 1, 0), (1, 0, 0), (0, 0, 1), 4)
    call = lambda lt, gb=1, pl=None, scene=None: lib.svgf_scene_draw_shadowed(scene, 1, gb, pl, 8, 8, ctypes.byref(cam), ctypes.byref(sp), lt, None)  # noqa: E731
    assert call(None) == -1 and call(ctypes.byref(ok)) == -1                     # a NULL light; a NULL scene
    for n in (0, -1, 65):
        assert call(ctypes.byref(B.SvgfSceneLight.make((0, 1, 0), samples=n))) == -1, n
    for field in ("centre", "edge_u", "edge_v"):
        for bad in (np.nan, np.inf, -np.inf):
            lt = B.SvgfSceneLight.make((0, 1, 0), samples=1)
            getattr(lt, field)[1] = bad
            assert call(ctypes.byref(lt)) == -1, (field, bad)
    assert call(ctypes.byref(ok), gb=1, pl=ctypes.byref(planes)) == -1 and call(ctypes.byref(ok), gb=None, pl=None) == -1
    assert ctypes.sizeof(B.SvgfSceneLight) == 40 and B.SCENE_MAX_SHADOW_SAMPLES == 64


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------
def _draw(pkg, scene, W, H, s, lt, frame=FRAME, seed=SEED, noise=0.6, stream=None, bufs=None, sync=True):
    import torch
    rgb, gbt = bufs or trs._buffers(W, H)
    light = pkg.binding.SvgfSceneLight.make(lt["centre"], lt["edge_u"], lt["edge_v"], lt["samples"])
    scene.draw_shadowed(rgb, gbt, W, H, s["cam"], light, frame, seed=seed, noise=noise, fireflies=0.02 if noise else 0.0, stream=stream)
    if not sync:
        return None
    torch.cuda.synchronize()
    return trs._host(pkg, rgb, gbt, W, H)


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", SIZES)
def test_sizes_and_seams(pkg, W, H):
    s = _edge("B")[0]
    scene = trs._create(pkg, s)
    ref, info, lt = _model("edge", "B", W, H, 3)
    got = _draw(pkg, scene, W, H, s, lt)
    scene.free()
    _no_difference(got, ref, f"scene B {W}x{H}, 3 samples")


@pytest.mark.gpu
@pytest.mark.parametrize("name", EDGE)
def test_edge_scene_with_an_occluder_equals_the_model(pkg, name):
    W, H = 67, 41
    s = _edge(name)[0]
    scene = trs._create(pkg, s)
    for samples, point in ((3, False), (1, False), (64, False), (3, True)):
        ref, info, lt = _model("edge", name, W, H, samples, point)
        assert info["occluded"].any() and not info["occluded"].all()
        _no_difference(_draw(pkg, scene, W, H, s, lt), ref, f"scene {name}, {samples} samples, {'point' if point else 'area'} light")
    scene.free()


@pytest.mark.gpu
@pytest.mark.parametrize("name,W,H,samples", [("cornell", 96, 96, 3), ("room", 128, 72, 1)])
def test_recorded_scene_equals_the_model(pkg, name, W, H, samples):
    s = trs._recorded(name, 0)[0]
    scene = trs._create(pkg, s)
    ref, info, lt = _model("rec", name, W, H, samples, frame=0, seed=1)
    got = _draw(pkg, scene, W, H, s, lt, frame=0, seed=1)
    scene.free()
    print(f"{name}: {int(info['occluded'].sum())} of {info['occluded'].size} samples occluded")
    _no_difference(got, ref, f"{name} {W}x{H}, {samples} samples")


@pytest.mark.gpu
def test_made_scenes_equal_the_model(pkg):
    """The stage (emitters, the light's own cube, the ceiling triangle through the light), the half-blocked light and the grazing
    scene, where the gate decides samples."""
    W, H = 67, 41
    for name, samples in (("stage", 3), ("half", 64), ("graze", 3)):
        s = _input("made", name)[0]
        scene = trs._create(pkg, s)
        ref, _, lt = _model("made", name, W, H, samples)
        _no_difference(_draw(pkg, scene, W, H, s, lt), ref, f"{name}, {samples} samples")
        scene.free()


@pytest.mark.gpu
def test_a_light_inside_an_occluder_leaves_the_ambient_term(pkg):
    """Scene B, a point light at the centre of its sphere, noise 0: every pixel that casts a ray is occluded or faces away, so the
    colour is albedo * 0.15 exactly."""
    W, H = 67, 41
    s = _edge("B")[0]
    centre = (2.5, 1.2, 0.0)
    ref, info, lt = _model("edge", "B", W, H, 3, point=True, noise=0.0, centre=centre)
    cast = info["cast"]
    want = (ref[1]["albedo"] * F(0.15)).astype(F)
    assert cast.sum() > 500 and not tsm.differing(ref[0], want)[cast].any(), "the model is not all dark"
    scene = trs._create(pkg, s)
    got = _draw(pkg, scene, W, H, s, lt, noise=0.0)
    scene.free()
    _no_difference(got, ref, "light inside the sphere")


@pytest.mark.gpu
def test_a_light_on_the_surface(pkg):
    W, H = 67, 41
    s = _edge("B")[0]
    first = _first("edge", "B", W, H, FRAME, SEED)[0]
    centre = tuple(float(c) for c in first[1]["position"][20, 40])
    ref, info, lt = _model("edge", "B", W, H, 3, point=True, centre=centre)
    scene = trs._create(pkg, s)
    got = _draw(pkg, scene, W, H, s, lt)
    scene.free()
    assert np.isfinite(got[0]).all()
    _no_difference(got, ref, "light on a surface point")


@pytest.mark.gpu
def test_planar_target_equals_the_model(pkg):
    import torch
    from temporal_harness import _hip
    W, H = 67, 41
    s = _edge("F_cube")[0]
    ref, _, lt = _model("edge", "F_cube", W, H, 3)
    scene = trs._create(pkg, s)
    den = pkg.Denoiser(W, H, 0)
    planes = den.planar_gbuffer()
    rgb = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    scene.draw_shadowed(rgb, planes, W, H, s["cam"], pkg.binding.SvgfSceneLight.make(lt["centre"], lt["edge_u"], lt["edge_v"], 3), FRAME, seed=SEED)
    torch.cuda.synchronize()
    hip = _hip()
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    gb = np.zeros((H, W), dtype=pkg.synth.GBUFFER_DTYPE)
    for field, ptr in (("normal", planes.normal), ("position", planes.position), ("albedo", planes.albedo), ("geomId", planes.geom_id)):
        host = np.zeros((H, W, 3) if field != "geomId" else (H, W), F if field != "geomId" else np.int32)
        assert hip.hipMemcpy(host.ctypes.data, ptr, host.nbytes, 2) == 0
        gb[field] = host
    gb["ialbedo"] = F(1.0)
    got = (rgb.cpu().numpy(), gb)
    den.free(); scene.free()
    _no_difference(got, ref, "scene F_cube, planar target")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "cornell"])
def test_every_tree_draws_the_same_shadowed_frame(pkg, name):
    (kind, W, H, S, fr, sd) = ("edge", 67, 41, 3, FRAME, SEED) if name == "A" else ("rec", 96, 96, 3, 0, 1)
    s = _input(kind, name)[0]
    ref, _, lt = _model(kind, name, W, H, S, frame=fr, seed=sd)
    frames = []
    for ml, sp in BUILDS:
        scene = trs._create(pkg, s, ml, sp)
        frames.append(_draw(pkg, scene, W, H, s, lt, frame=fr, seed=sd))
        scene.free()
    for (ml, sp), fr_ in zip(BUILDS, frames):
        _no_difference(fr_, ref, f"{name}, leaf {ml} split {sp}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["C", "G"])
def test_unobstructed_scene_is_svgf_scene_draw_on_bits(pkg, name):
    """Scene C: nothing stands between the quads and the light.  Scene G: the light's side of the cube and the sphere is free; the
    model says which pixels are unoccluded and on those the two draws agree on every bit, the G-buffer everywhere."""
    W, H = 67, 41
    s = tsm._scene(name)
    ref, info, lt = _model("plain", name, W, H, 3)
    scene = trs._create(pkg, s)
    got = _draw(pkg, scene, W, H, s, lt)
    plain = trs._draw(pkg, scene, W, H, s, FRAME, SEED)
    scene.free()
    _no_difference(got, ref, f"scene {name} vs the model")
    free = info["vis"] == 1
    assert free.sum() > 1000 and (name != "C" or free.all())
    for f in tsm.FIELDS:
        assert not tsm.differing(got[1][f], plain[1][f]).any(), f
    assert not tsm.differing(got[0], plain[0])[free].any()


@functools.lru_cache(maxsize=None)
def _block_light():
    s, tables = tas._block_inputs()
    L = np.asarray(s["light"], np.float64)
    return dict(centre=tuple(float(c) for c in L), edge_u=(0.8, 0.0, 0.0), edge_v=(0.0, 0.0, 0.8))


@functools.lru_cache(maxsize=None)
def _block_frame(f, W, H, samples, noise=0.6):
    """Frame f of f15's turning block (box_room, the block 9 degrees and 1.0 in x further per frame) under the area light: the model on
    the posed arrays."""
    s, tables = tas._block_inputs()
    ps = pm.posed_scene(s, tables[f])
    lk = _block_light()
    lt = ssm.light(lk["centre"], lk["edge_u"], lk["edge_v"], samples)
    col, gb, info = ssm.render(W, H, f, ps["cam"], ps["geoms"], None, None, None, None, None, None, lt, seed=3, noise=noise, fireflies=0.02 if noise else 0.0)
    return (col, gb), info, lt


@pytest.mark.gpu
def test_the_shadow_follows_the_pose(pkg):
    W, H = 96, 96
    s, tables = tas._block_inputs()
    scene = trs._create(pkg, s)
    scene.enable_pose(len(s["geoms"]))
    vis = []
    for f in (0, 2):
        ref, info, lt = _block_frame(f, W, H, 4)
        scene.pose(tas._dev(tables[f]))
        _no_difference(_draw(pkg, scene, W, H, s, lt, frame=f, seed=3), ref, f"turning block, pose {f}")
        vis.append(info["vis"])
    scene.free()
    moved = int((vis[0] != vis[1]).sum())
    print(f"visibility differs between pose 0 and pose 2 on {moved} pixels")
    assert moved > 50


@pytest.mark.gpu
def test_eight_shadowed_draws_queued_without_host_waits(pkg):
    import torch
    W, H = 67, 41
    s = _edge("A")[0]
    scene = trs._create(pkg, s)
    st = torch.cuda.Stream()
    bufs = [trs._buffers(W, H) for _ in range(8)]
    lt = _model("edge", "A", W, H, 3)[2]
    for f, b in enumerate(bufs):
        _draw(pkg, scene, W, H, s, lt, frame=f, stream=st, bufs=b, sync=False)
    st.synchronize()
    for f, (rgb, gbt) in enumerate(bufs):
        _no_difference(trs._host(pkg, rgb, gbt, W, H), _model("edge", "A", W, H, 3, frame=f)[0], f"queued draw, frame {f}")
    scene.free()


@pytest.mark.gpu
def test_a_captured_shadowed_draw_is_one_kernel_node_and_replays_the_same_bits(pkg):
    import torch
    hip = tas._graph_api()
    W, H = 67, 41
    s = _edge("B")[0]
    ref, _, lt = _model("edge", "B", W, H, 3)
    scene = trs._create(pkg, s)
    st = torch.cuda.Stream()
    bufs = trs._buffers(W, H)
    _draw(pkg, scene, W, H, s, lt, stream=st, bufs=bufs, sync=False)       # eager first: a first launch may set kernel attributes
    st.synchronize()
    graph, gexec = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipStreamBeginCapture(st.cuda_stream, 2) == 0
    _draw(pkg, scene, W, H, s, lt, stream=st, bufs=bufs, sync=False)       # recorded, not executed
    assert hip.hipStreamEndCapture(st.cuda_stream, ctypes.byref(graph)) == 0 and graph.value
    types = tas._node_types(hip, graph)
    assert hip.hipGraphInstantiate(ctypes.byref(gexec), graph, None, None, 0) == 0
    with torch.cuda.stream(st):
        bufs[0].zero_(); bufs[1].zero_()
    assert hip.hipGraphLaunch(gexec, st.cuda_stream) == 0
    st.synchronize()
    got = trs._host(pkg, *bufs, W, H)
    hip.hipGraphExecDestroy(gexec); hip.hipGraphDestroy(graph)
    scene.free()
    print(f"captured shadowed draw = node types {types}")
    assert types == [0], types
    _no_difference(got, ref, "replayed shadowed draw")


@pytest.mark.gpu
def test_every_error_code(pkg):
    B = pkg.binding
    s = _edge("B")[0]
    scene = trs._create(pkg, s)
    lib = scene.lib
    cam, sp, planes = B.SvgfCamera(), B.SvgfSynthParams(), B.SvgfPlanarGBuffer()
    ok = ctypes.byref(B.SvgfSceneLight.make((0, 1, 0), (1, 0, 0), (0, 0, 1), 4))
    c, p = ctypes.byref(cam), ctypes.byref(sp)
    f = lib.svgf_scene_draw_shadowed
    assert f(scene.h, 1, 1, None, 0, 8, c, p, ok, None) == -1 and f(scene.h, 1, 1, None, 8, -1, c, p, ok, None) == -1
    assert f(scene.h, None, 1, None, 8, 8, c, p, ok, None) == -1 and f(scene.h, 1, None, None, 8, 8, c, p, ok, None) == -1
    assert f(scene.h, 1, 1, None, 8, 8, None, p, ok, None) == -1 and f(scene.h, 1, 1, None, 8, 8, c, None, ok, None) == -1
    assert f(scene.h, 1, 1, None, 8, 8, c, p, None, None) == -1 and f(None, 1, 1, None, 8, 8, c, p, ok, None) == -1
    assert f(scene.h, 1, 1, ctypes.byref(planes), 8, 8, c, p, ok, None) == -1          # both targets
    assert f(scene.h, 1, None, ctypes.byref(planes), 8, 8, c, p, ok, None) == -1       # planes without normal, position, geom_id
    assert f(scene.h, 1, 1, None, 1 << 14, 1 << 13, c, p, ok, None) == -5              # width * height == 2^31 / 16
    for n in (0, 65):
        assert f(scene.h, 1, 1, None, 8, 8, c, p, ctypes.byref(B.SvgfSceneLight.make((0, 1, 0), samples=n)), None) == -1
    bad = B.SvgfSceneLight.make((0, 1, 0), samples=1)
    bad.edge_v[2] = float("nan")
    assert f(scene.h, 1, 1, None, 8, 8, c, p, ctypes.byref(bad), None) == -1
    # and the scene still draws
    W, H = 7, 5
    ref, _, lt = _model("edge", "B", W, H, 3)
    _no_difference(_draw(pkg, scene, W, H, s, lt), ref, "after the refused calls")
    scene.free()


@pytest.mark.gpu
def test_pose_shadowed_draw_denoise_sequence(pkg, orc):
    """128x72, six frames of the turning block on one stream: pose -> shadowed draw (1 sample) -> svgf_denoise (temporal pass), with
    the object motion table and the history clamp on and off, against tests/temporal_model.py fed the model's frames."""
    import torch
    import temporal_model as tm
    from temporal_harness import assert_frames_equal, read_states, scales, synth_params
    W, H = 128, 72
    s, tables = tas._block_inputs()
    n = len(s["geoms"])
    held, frames, motion = pkg.binding.pose_identity(n), [], []
    for f, t in enumerate(tables):
        (col, gb), _, lt = _block_frame(f, W, H, 1)
        frames.append((np.asarray(col, F).reshape(H, W, 3), gb.reshape(H, W)))
        motion.append(pm.motion_rows(held, t))
        held = t
    M = orc.view_matrix(pkg, s["cam"])
    p = synth_params(pkg, W, H)
    for with_table, (radius, k) in ((True, (1, 1.5)), (True, (0, 0.0)), (False, (1, 1.5)), (False, (0, 0.0))):
        want = tm.run_sequence(frames, tables=motion if with_table else None, views=[M] * len(frames), scale=scales(pkg, W, H), radius=radius, k=k)
        scene = trs._create(pkg, s)
        scene.enable_pose(n)
        den = pkg.Denoiser(W, H)
        den.set_capture(True)
        t_x = tas._motion_buffer(n)
        if with_table:
            den.set_object_motion(t_x)
        den.set_history_clamp(radius, k)
        rgb, gbt = trs._buffers(W, H)
        out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        got = []
        try:
            for f, t in enumerate(tables):
                scene.pose(tas._dev(t), t_x)
                _draw(pkg, scene, W, H, s, lt, frame=f, seed=3, bufs=(rgb, gbt), sync=False)
                den.denoise(out, rgb, gbt, s["cam"], p)
                torch.cuda.synchronize()
                got.append(read_states(den))
        finally:
            den.free(); scene.free()
        assert_frames_equal(got, want, f"table {with_table}, clamp radius {radius}")
