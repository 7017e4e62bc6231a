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

import scene_harness as sh
import scene_model as sm
import scene_pose_model as pm
import scene_shadow_model as ssm
import test_scene_model as tsm
from test_scene_model import FRAME, SEED

F = np.float32


# ---- CPU 1: the model's own properties -------------------------------------------------------------------------------------------------
def test_an_empty_path_to_the_light_gives_scene_models_frame():
    """Scene C (textured quads in one plane, the light in front of it) and scene D (NaN normals): no sample is occluded - t_lo keeps
    the surface from shadowing itself - and colour and G-buffer are scene_model.render's on every bit."""
    for name in ("C", "D"):
        W, H = 67, 41
        (col, gb), info, _ = sh.shadow_model("plain", name, W, H, 3)
        first = sh.first_hit("plain", name, W, H, FRAME, SEED)[0]
        print(f"scene {name}: {int(info['cast'].sum())} pixels cast rays, {int(info['occluded'].sum())} samples occluded")
        if name == "C":
            assert info["cast"].sum() > 1000 and not info["occluded"].any()
            sh.same((col, gb), first, f"scene {name}, shadowed model vs scene_model")
        for f in tsm.FIELDS:
            assert not tsm.differing(gb[f], first[1][f]).any(), f
        assert not tsm.differing(col, first[0])[info["vis"] == 1].any()


def test_a_point_light_gives_hard_shadows():
    for name in sh.EDGE:
        _, info, _ = sh.shadow_model("edge", name, 67, 41, 3, point=True)
        vis = info["vis"][info["cast"]]
        dark = int((vis == 0).sum())
        print(f"scene {name}: point light, {len(vis)} pixels cast, {dark} dark")
        assert np.isin(vis, (0.0, 1.0)).all() and 0 < dark < len(vis)


def test_area_light_gives_penumbrae_on_every_edge_scene():
    for name in sh.EDGE:
        _, info, _ = sh.shadow_model("edge", name, 67, 41, 64)
        vis = info["vis"][info["cast"]]
        part = int(((vis > 0) & (vis < 1)).sum())
        print(f"scene {name}: 64 samples, {len(vis)} pixels cast, {int((vis == 0).sum())} dark, {part} in a penumbra")
        assert part > 10 and (vis == 1).sum() > 10


def test_half_blocked_light_is_inside_the_binomial_band():
    W, H, S = 67, 41, 64
    (_, gb), info, lt = sh.shadow_model("made", "half", W, H, S)
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
    (col, gb), info, _ = sh.shadow_model("made", "stage", W, H, 3, point=True)
    first, em = sh.first_hit("made", "stage", W, H, FRAME, SEED)
    assert em.sum() > 10 and not info["cast"][em].any() and not tsm.differing(col, first[0])[em].any()
    floor = (gb["geomId"] == 3) & (gb["position"][..., 0] > 1.5)      # beside the occluding cube and the emitting sphere: only the light's cube is above
    print(f"stage: {int(em.sum())} emitter pixels, {int(floor.sum())} floor pixels under the light's own cube alone")
    assert floor.sum() > 100 and (info["vis"][floor] == 1).all()
    with_emitters = sh.shadow_model("made", "stage", W, H, 3, point=True, alt="emitter_occludes")[1]["vis"]
    assert (with_emitters[floor] == 0).all()


def test_a_light_on_the_surface_gives_no_nan():
    W, H = 67, 41
    first = sh.first_hit("edge", "B", W, H, FRAME, SEED)[0]
    y, x = 20, 40
    assert first[1]["geomId"][y, x] >= 0
    centre = tuple(float(c) for c in first[1]["position"][y, x])
    (col, gb), info, _ = sh.shadow_model("edge", "B", W, H, 3, point=True, centre=centre)
    j = int(np.flatnonzero(info["pixels"] == y * W + x)[0])
    assert (info["dl"][:, j] == 0).all() and not info["occluded"][:, j].any()
    assert np.isfinite(col).all() and info["vis"][y, x] == 1


# ---- CPU 2: each alt acts, and the gate --------------------------------------------------------------------------------------------------
ALT_SCENES = [("edge", n) for n in sh.EDGE] + [("made", "stage"), ("made", "half"), ("made", "graze")]


def test_each_alt_acts():
    """Pixels on which the frame of the model and of a wrong variant of it differ, per scene (67x41, 3 samples): every alt changes
    some scene."""
    W, H = 67, 41
    total = {a: 0 for a in ssm.ALTS}
    for kind, name in ALT_SCENES:
        ref = sh.shadow_model(kind, name, W, H, 3)[0]
        row = {}
        for alt in ssm.ALTS:
            row[alt] = tsm.any_differs(sh.shadow_model(kind, name, W, H, 3, alt=alt)[0], ref)
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
    info = sh.shadow_model(kind, name, W, H, S, frame=0 if kind == "rec" else FRAME, seed=1 if kind == "rec" else SEED)[1]
    print(f"{name} {W}x{H}, {S} samples: {info['occluded'].size} (pixel, sample) pairs, {int(info['occluded'].sum())} occluded, "
          f"ungated differs on {info['ungated_differs']}")
    assert info["occluded"].any() and info["ungated_differs"] == 0


def test_the_gate_decides_samples_of_the_grazing_scene():
    """The one scene here on which it is NOT zero (DESIGN 5.4h names it): made for it, see scene_harness._graze."""
    W, H, S = 67, 41, 3
    info = sh.shadow_model("made", "graze", W, H, S)[1]
    print(f"graze {W}x{H}, {S} samples: {info['occluded'].size} (pixel, sample) pairs, {int(info['occluded'].sum())} occluded, "
          f"ungated differs on {info['ungated_differs']}")
    assert info["ungated_differs"] > 0


# ---- CPU 3: what examples/shadowed_scene.cpp measures, on the oracle ------------------------------------------------------------------------
def test_denoised_shadow_beats_the_noisy_one_after_eight_static_frames(pkg, orc):
    """64x36, noise 0 (the visibility estimate is the only noise), eight frames of the scene at rest: one shadow ray per pixel through
    the oracle's full SVGF against the 64-ray frame, by tests/quality_model.py.  The gate is the issue's: the denoised frame beats the
    noisy one in PSNR and in SSIM.  Recorded on the last frame: noisy 43.95 dB / SSIM 0.9972, denoised 46.42 dB / SSIM 0.9983 (few of the
    2 304 pixels lie in the penumbra: the camera sees the floor at a flat angle)."""
    import quality_model as qm
    from temporal_harness import scales
    W, H, N = 64, 36, 8
    geoms, cam, lk = sh.example_scene()
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
@pytest.mark.gpu
@pytest.mark.parametrize("W,H", sh.SIZES)
def test_sizes_and_seams(pkg, W, H):
    s = sh.edge("B")[0]
    scene = sh.create(pkg, s)
    ref, info, lt = sh.shadow_model("edge", "B", W, H, 3)
    got = sh.draw(pkg, sh.SHADOWED, scene, W, H, s, lt)
    scene.free()
    sh.same(got, ref, f"scene B {W}x{H}, 3 samples")


@pytest.mark.gpu
@pytest.mark.parametrize("name", sh.EDGE)
def test_edge_scene_with_an_occluder_equals_the_model(pkg, name):
    W, H = 67, 41
    s = sh.edge(name)[0]
    scene = sh.create(pkg, s)
    for samples, point in ((3, False), (1, False), (64, False), (3, True)):
        ref, info, lt = sh.shadow_model("edge", name, W, H, samples, point)
        assert info["occluded"].any() and not info["occluded"].all()
        sh.same(sh.draw(pkg, sh.SHADOWED, scene, W, H, s, lt), ref, f"scene {name}, {samples} samples, {'point' if point else 'area'} light")
    scene.free()


@pytest.mark.gpu
@pytest.mark.parametrize("name,W,H,samples", [("cornell", 96, 96, 3), ("room", 128, 72, 1)])
def test_recorded_scene_equals_the_model(pkg, name, W, H, samples):
    s = sh.recorded(name, 0)[0]
    scene = sh.create(pkg, s)
    ref, info, lt = sh.shadow_model("rec", name, W, H, samples, frame=0, seed=1)
    got = sh.draw(pkg, sh.SHADOWED, scene, W, H, s, lt, frame=0, seed=1)
    scene.free()
    print(f"{name}: {int(info['occluded'].sum())} of {info['occluded'].size} samples occluded")
    sh.same(got, ref, f"{name} {W}x{H}, {samples} samples")


@pytest.mark.gpu
def test_made_scenes_equal_the_model(pkg):
    """The stage (emitters, the light's own cube, the ceiling triangle through the light), the half-blocked light and the grazing
    scene, where the gate decides samples."""
    W, H = 67, 41
    for name, samples in (("stage", 3), ("half", 64), ("graze", 3)):
        s = sh.scene_input("made", name)[0]
        scene = sh.create(pkg, s)
        ref, _, lt = sh.shadow_model("made", name, W, H, samples)
        sh.same(sh.draw(pkg, sh.SHADOWED, scene, W, H, s, lt), ref, f"{name}, {samples} samples")
        scene.free()


@pytest.mark.gpu
def test_a_light_inside_an_occluder_leaves_the_ambient_term(pkg):
    """Scene B, a point light at the centre of its sphere, noise 0: every pixel that casts a ray is occluded or faces away, so the
    colour is albedo * 0.15 exactly."""
    W, H = 67, 41
    s = sh.edge("B")[0]
    centre = (2.5, 1.2, 0.0)
    ref, info, lt = sh.shadow_model("edge", "B", W, H, 3, point=True, noise=0.0, centre=centre)
    cast = info["cast"]
    want = (ref[1]["albedo"] * F(0.15)).astype(F)
    assert cast.sum() > 500 and not tsm.differing(ref[0], want)[cast].any(), "the model is not all dark"
    scene = sh.create(pkg, s)
    got = sh.draw(pkg, sh.SHADOWED, scene, W, H, s, lt, dict(noise=0.0))
    scene.free()
    sh.same(got, ref, "light inside the sphere")


@pytest.mark.gpu
def test_a_light_on_the_surface(pkg):
    W, H = 67, 41
    s = sh.edge("B")[0]
    first = sh.first_hit("edge", "B", W, H, FRAME, SEED)[0]
    centre = tuple(float(c) for c in first[1]["position"][20, 40])
    ref, info, lt = sh.shadow_model("edge", "B", W, H, 3, point=True, centre=centre)
    scene = sh.create(pkg, s)
    got = sh.draw(pkg, sh.SHADOWED, scene, W, H, s, lt)
    scene.free()
    assert np.isfinite(got["color"]).all()
    sh.same(got, ref, "light on a surface point")


@pytest.mark.gpu
def test_planar_target_equals_the_model(pkg):
    W, H = 67, 41
    s = sh.edge("F_cube")[0]
    ref, _, lt = sh.shadow_model("edge", "F_cube", W, H, 3)
    sh.check_planar_target(pkg, sh.SHADOWED, sh.case(s, W, H, lt), ref, "scene F_cube, planar target")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "cornell"])
def test_every_tree_draws_the_same_shadowed_frame(pkg, name):
    (kind, W, H, S, fr, sd) = ("edge", 67, 41, 3, FRAME, SEED) if name == "A" else ("rec", 96, 96, 3, 0, 1)
    s = sh.scene_input(kind, name)[0]
    ref, _, lt = sh.shadow_model(kind, name, W, H, S, frame=fr, seed=sd)
    sh.check_every_tree(pkg, sh.SHADOWED, sh.case(s, W, H, lt, frame=fr, seed=sd), ref, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["C", "G"])
def test_unobstructed_scene_is_svgf_scene_draw_on_bits(pkg, name):
    """Scene C: nothing stands between the quads and the light.  Scene G: the light's side of the cube and the sphere is free; the
    model says which pixels are unoccluded and on those the two draws agree on every bit, the G-buffer everywhere."""
    W, H = 67, 41
    s = tsm._scene(name)
    ref, info, lt = sh.shadow_model("plain", name, W, H, 3)
    scene = sh.create(pkg, s)
    got = sh.draw(pkg, sh.SHADOWED, scene, W, H, s, lt)
    plain = sh.draw_frame(pkg, scene, W, H, s, FRAME, SEED)
    scene.free()
    sh.same(got, ref, f"scene {name} vs the model")
    free = info["vis"] == 1
    assert free.sum() > 1000 and (name != "C" or free.all())
    for f in tsm.FIELDS:
        assert not tsm.differing(got["gb"][f], plain[1][f]).any(), f
    assert not tsm.differing(got["color"], plain[0])[free].any()


@functools.lru_cache(maxsize=None)
def _block_frame(f, W, H, samples, noise=0.6):
    """Frame f of f15's turning block (box_room, the block 9 degrees and 1.0 in x further per frame) under the area light: the model on
    the posed arrays."""
    s, tables = sh.block_inputs()
    ps = pm.posed_scene(s, tables[f])
    lk = sh.block_light()
    lt = ssm.light(lk["centre"], lk["edge_u"], lk["edge_v"], samples)
    col, gb, info = ssm.render(W, H, f, ps["cam"], ps["geoms"], None, None, None, None, None, None, lt, seed=3, noise=noise, fireflies=0.02 if noise else 0.0)
    return (col, gb), info, lt


@pytest.mark.gpu
def test_the_shadow_follows_the_pose(pkg):
    W, H = 96, 96
    s, tables = sh.block_inputs()
    scene = sh.create(pkg, s)
    scene.enable_pose(len(s["geoms"]))
    vis = []
    for f in (0, 2):
        ref, info, lt = _block_frame(f, W, H, 4)
        scene.pose(sh.dev(tables[f]))
        sh.same(sh.draw(pkg, sh.SHADOWED, scene, W, H, s, lt, frame=f, seed=3), ref, f"turning block, pose {f}")
        vis.append(info["vis"])
    scene.free()
    moved = int((vis[0] != vis[1]).sum())
    print(f"visibility differs between pose 0 and pose 2 on {moved} pixels")
    assert moved > 50


@pytest.mark.gpu
def test_eight_shadowed_draws_queued_without_host_waits(pkg):
    W, H = 67, 41
    lt = sh.shadow_model("edge", "A", W, H, 3)[2]
    sh.check_queued(pkg, sh.SHADOWED, sh.case(sh.edge("A")[0], W, H, lt), lambda f: sh.shadow_model("edge", "A", W, H, 3, frame=f)[0], "queued draw",
                    own_stream=False)


@pytest.mark.gpu
def test_a_captured_shadowed_draw_is_one_kernel_node_and_replays_the_same_bits(pkg):
    W, H = 67, 41
    ref, _, lt = sh.shadow_model("edge", "B", W, H, 3)
    sh.check_captured(pkg, sh.SHADOWED, sh.case(sh.edge("B")[0], W, H, lt), ref, "shadowed draw", own_stream=False)


@pytest.mark.gpu
def test_every_error_code(pkg):
    B = pkg.binding
    s = sh.edge("B")[0]
    scene = sh.create(pkg, s)
    lib = scene.lib
    c, p = ctypes.byref(B.SvgfCamera()), ctypes.byref(B.SvgfSynthParams())
    ok = ctypes.byref(B.SvgfSceneLight.make((0, 1, 0), (1, 0, 0), (0, 0, 1), 4))
    f = lambda h=scene.h, rgb=1, gb=1, pl=None, w=8, hh=8, cm=c, spp=p, lt=ok: lib.svgf_scene_draw_shadowed(h, rgb, gb, pl, w, hh, cm, spp, lt, None)  # noqa: E731
    assert f(rgb=None) == -1
    sh.check_common_refusals(B, f)
    # and the scene still draws
    W, H = 7, 5
    ref, _, lt = sh.shadow_model("edge", "B", W, H, 3)
    sh.same(sh.draw(pkg, sh.SHADOWED, scene, W, H, s, lt), ref, "after the refused calls")
    scene.free()


@pytest.mark.gpu
def test_pose_shadowed_draw_denoise_sequence(pkg, orc):
    """128x72, six frames of the turning block on one stream: pose -> shadowed draw (1 sample) -> svgf_denoise (temporal pass), with
    the object motion table and the history clamp on and off, against tests/temporal_model.py fed the model's frames."""
    import torch
    import temporal_model as tm
    from temporal_harness import assert_frames_equal, read_states, scales, synth_params
    W, H = 128, 72
    s, tables = sh.block_inputs()
    n = len(s["geoms"])
    frames, motion = [], sh.block_motion(pkg, tables)
    for f in range(len(tables)):
        (col, gb), _, lt = _block_frame(f, W, H, 1)
        frames.append((np.asarray(col, F).reshape(H, W, 3), gb.reshape(H, W)))
    M = orc.view_matrix(pkg, s["cam"])
    p = synth_params(pkg, W, H)
    for with_table, (radius, k) in ((True, (1, 1.5)), (True, (0, 0.0)), (False, (1, 1.5)), (False, (0, 0.0))):
        want = tm.run_sequence(frames, tables=motion if with_table else None, views=[M] * len(frames), scale=scales(pkg, W, H), radius=radius, k=k)
        scene = sh.create(pkg, s)
        scene.enable_pose(n)
        den = pkg.Denoiser(W, H)
        den.set_capture(True)
        t_x = sh.motion_buffer(n)
        if with_table:
            den.set_object_motion(t_x)
        den.set_history_clamp(radius, k)
        rgb, gbt = sh.buffers(W, H)
        out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        got = []
        try:
            for f, t in enumerate(tables):
                scene.pose(sh.dev(t), t_x)
                sh.draw(pkg, sh.SHADOWED, scene, W, H, s, lt, frame=f, seed=3, bufs=dict(color=rgb, gb=gbt), sync=False)
                den.denoise(out, rgb, gbt, s["cam"], p)
                torch.cuda.synchronize()
                got.append(read_states(den))
        finally:
            den.free(); scene.free()
        assert_frames_equal(got, want, f"table {with_table}, clamp radius {radius}")
