"""The deep traced scene (include/svgf_path.h row f19, libsvgf_path.so): svgf_path_draw and svgf_path_draw_split trace paths of up to
eight diffuse bounces with next-event estimation at every vertex and Russian roulette.

The yardstick is tests/scene_path_model.py on top of tests/scene_trace_model.py and tests/scene_split_model.py.  Both sides perform the
same operations in the same order without contraction, and the nearest hit does not depend on the tree, so there is no tolerance to
choose: colour, D, I and every G-buffer field are compared on bits (NaNs in the same place count as equal), expected and allowed number
of differing pixels: 0.

CPU part: exports and refusals; the model's identities (depth 1 is f17's and f18's model), the furnace by depth, the roulette's
unbiasedness, colour picked up twice, every `alt` acts, the coverage condition of the GPU cases, and denoised against noisy on the
oracle.  GPU part: the device against the model.

The coverage condition (test_gpu_cases_reach_depth_two_and_the_roulette): every (scene, size, parameters) the GPU tests draw at 67x41 or
larger with max_depth >= 2 has at least 100 paths with a hit at bounce 2 and, where rr_depth > 0, at least 100 roulette kills and 100
survivals in the model - a comparison on bits says nothing about code that no path reaches.  The open edge scenes of rows f14-f17
(A, B, F_sphere, E_plus) fall short at 67x41 (most second bounces miss), so the parameter product runs on F_cube and on closed
scenes; scene A (triangles only, the six builds) is drawn at 134x82 with eight paths, where it passes.
"""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import scene_harness as sh
import scene_model as sm
import scene_path_model as spm
import scene_pose_model as pm
import scene_shadow_model as ssm
import scene_split_model as splm
import scene_trace_model as stm
import test_scene_model as tsm
from conftest import ROOT
from test_scene_model import FRAME, SEED, differing

F = np.float32


# ---- CPU 1: exports, declarations, refusals --------------------------------------------------------------------------------------------
def test_the_three_symbols_are_declared_listed_and_exported(pkg):
    B = pkg.binding
    assert B.PATH_EXPORTS == ["svgf_path_draw", "svgf_path_draw_split", "svgf_path_version"]
    assert ctypes.sizeof(B.SvgfPathParams) == 20 and B.PATH_MAX_PATHS == 8 and B.PATH_MAX_DEPTH == 8
    text = open(os.path.join(ROOT, "include", "svgf_path.h")).read()
    assert re.search(r"#define SVGF_PATH_MAX_PATHS 8\b", text) and re.search(r"#define SVGF_PATH_MAX_DEPTH 8\b", text)
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(svgf_[a-z_]+)\s*\(", src))
    assert declared == set(B.PATH_EXPORTS)
    nm = lambda path, how: subprocess.run(["nm", "-D", how, path], stdout=subprocess.PIPE, text=True, check=True).stdout      # noqa: E731
    assert os.path.exists(B.LIB_PATH_PATH), "libsvgf_path.so is built by __graft_entry__.build()"
    exported = {ln.split()[-1] for ln in nm(B.LIB_PATH_PATH, "--defined-only").splitlines() if ln.strip()}
    assert set(B.PATH_EXPORTS) <= exported and not any(n.startswith("svgf_") and n not in B.PATH_EXPORTS for n in exported)
    undefined = nm(B.LIB_PATH_PATH, "--undefined-only")
    assert "svgf_scene_view" in undefined and "getenv" not in undefined and "svgf_trace_" not in undefined
    needed = subprocess.run(["readelf", "-d", B.LIB_PATH_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "libsvgf_hip.so" in needed and "libsvgf_trace.so" not in needed and "libsvgf_split.so" not in needed
    assert callable(pkg.Scene.draw_path) and callable(pkg.Scene.draw_path_split)
    print(f"libsvgf_hip.so {os.path.getsize(B.LIB_PATH)} bytes, libsvgf_path.so {os.path.getsize(B.LIB_PATH_PATH)} bytes")


def test_path_argument_errors_without_a_device(pkg):
    """Every refusal of both calls is answered before any device work: none of these calls needs a device (there is no scene without
    one, so the scene is NULL throughout, which is itself refused; the GPU test repeats the list with a scene)."""
    B = pkg.binding
    lib = pkg.load_path_library()
    assert lib.svgf_path_version() == pkg.load_library().svgf_version()
    cam, sp, planes = B.SvgfCamera(), B.SvgfSynthParams(), B.SvgfPlanarGBuffer()
    ok, pp = B.SvgfSceneLight.make((0, 1, 0), (1, 0, 0), (0, 0, 1), 4), B.SvgfPathParams(1, 4, 2, 0.15, 1)
    L, P = ctypes.byref(ok), ctypes.byref(pp)
    plain = lambda lt, pp, rgb=3, gb=4, pl=None, w=8, h=8: lib.svgf_path_draw(None, rgb, gb, pl, w, h, ctypes.byref(cam), ctypes.byref(sp), lt, pp, None)  # noqa: E731
    split = lambda lt, pp, d=1, i=2, rgb=3, gb=4, pl=None, w=8, h=8: lib.svgf_path_draw_split(    # noqa: E731
        None, d, i, rgb, gb, pl, w, h, ctypes.byref(cam), ctypes.byref(sp), lt, pp, None)
    for call in (plain, split):
        assert call(None, P) == -1 and call(L, None) == -1 and call(L, P) == -1
        for n in (0, -1, 65):
            assert call(ctypes.byref(B.SvgfSceneLight.make((0, 1, 0), samples=n)), P) == -1, n
        assert call(L, P, pl=ctypes.byref(planes)) == -1 and call(L, P, gb=None) == -1
        assert call(L, P, w=0) == -1 and call(L, P, h=-3) == -1
        for bad in sh.BAD_PARAMS:
            assert call(L, ctypes.byref(B.SvgfPathParams(*bad))) == -1, bad
    assert plain(L, P, rgb=None) == -1
    assert split(L, P, d=None) == -1 and split(L, P, i=None) == -1 and split(L, P, d=5, i=5) == -1 and split(L, P, rgb=None) == -1


# ---- CPU 2: the model's own properties -------------------------------------------------------------------------------------------------
def test_a_moved_seed_moves_every_stream():
    """scene_path_model.stream_seed: the device adds 128 (k - 1) + 16 j to the stream, the model to the seed - the same hash."""
    for seed, frame, delta in ((5, 3, 0), (5, 3, 16), (SEED, FRAME, 128), (1, 0, 128 * 7 + 16 * 7), (0xFFFFFFF0, 9, 1000)):
        for k in (0, 7, 266):
            assert np.array_equal(stm.synth.hash_uniform(spm.stream_seed(seed, delta), frame, 257, k), stm.synth.hash_uniform(seed, frame, 257, k + delta))


@pytest.mark.parametrize("kind,name,kw", [("edge", "B", {}), ("edge", "F_cube", {}), ("made", "stage", {}), ("traced", "furnace", dict(noise=0.0, ambient=1.0))])
def test_depth_one_is_the_traced_and_the_split_model(kind, name, kw):
    W, H, J = 67, 41, 3
    ref = sh.split_model(kind, name, W, H, J, **kw)
    for R in (0, 1):
        m = sh.path_model(kind, name, W, H, J, 1, R, **kw)
        c = sh.split_counts(m, ref)
        print(f"{name}, max_depth 1, rr_depth {R}: differing pixels {c} (expected and allowed: 0)")
        assert not any(c.values()), c
    assert (ref["I"] > 0).any()


def test_the_furnace_by_depth():
    """f17's furnace with ambient = 0: a vertex on a white object adds 1 * 0 and keeps thr = 1, the enclosure adds 0.5 * 2 = 1 and ends
    the path, nothing misses.  So every path returns exactly 0 or exactly 1, the longer path is the shorter one continued, and fewer
    paths are still empty-handed the deeper they may go."""
    W, H, J = 48, 27, 4
    prev, share = None, {}
    for K in (1, 2, 4, 8):
        m = sh.path_model("traced", "furnace", W, H, J, K, 0, noise=0.0, ambient=0.0)
        info = m["info"]
        cast, acc = info["cast"], np.stack(info["acc"])            # [3, J, n]
        assert cast.sum() > 200 and ((acc == 0) | (acc == 1)).all() and (acc[0] == acc[1]).all() and (acc[0] == acc[2]).all()
        ind = info["ind"][cast]
        whole = ind * F(J)
        assert (whole == np.round(whole)).all() and (whole >= 0).all() and (whole <= J).all()
        assert not differing(m["I"], info["ind"])[cast].any()
        share[K] = float((acc[0] == 0).mean())
        print(f"furnace, max_depth {K}: {acc[0].size} paths, share returning 0: {share[K]:.5f}; per depth {spm.COUNTS}: {sh.counts_row(info)}")
        assert all(d["misses"] == 0 for d in info["depth"])
        if prev is not None:
            assert (ind >= prev).all()
        prev = ind
    assert share[1] >= share[2] >= share[4] >= share[8] and share[8] < share[1] and share[1] > 0


def test_roulette_is_unbiased_in_the_model():
    """cornell (closed) at 48x48, noise 0, one path of up to 8 bounces, 8 frames, rr_depth 1 against 0.  The statistic is the mean of
    ind (over channels, casting pixels and frames); its standard error is estimated per side as sqrt(mean over pixels of the sample
    variance over the frames / number of values).  The two means must agree within 4 standard errors of their difference (the two
    errors added in quadrature; the sides share every stream but the roulette's, so this is generous), and the same roulette WITHOUT the
    division by q must not."""
    W, H, N = 48, 48, 8
    s, lk = sh.scene_input("rec", "cornell")
    lt = ssm.light(lk["centre"], lk["edge_u"], lk["edge_v"], 1)
    first, em = sh.first_hit("rec", "cornell", W, H, 0, 1, 0.0)
    stat = {}
    for tag, R, alt in (("rr_depth 0", 0, None), ("rr_depth 1", 1, None), ("no compensation", 1, "no_roulette_compensation")):
        vals, kills, surv = [], 0, 0
        for f in range(N):
            info = spm.render(W, H, f, *sh.args_of(s), lt, spm.params(1, 8, R), seed=1, noise=0.0, fireflies=0.0, alt=alt, first=first, emitters=em,
                              emittance=sh.emittance("rec", "cornell", W, H))[4]
            vals.append(info["ind"][info["cast"]].astype(np.float64).mean(axis=-1))
            kills += sum(d["rr_kills"] for d in info["depth"]); surv += sum(d["rr_survivals"] for d in info["depth"])
        v = np.stack(vals)
        stat[tag] = (v.mean(), np.sqrt(v.var(axis=0, ddof=1).mean() / v.size))
        print(f"{tag}: mean ind {stat[tag][0]:.5f} +- {stat[tag][1]:.5f} over {v.size} values; roulette kills {kills}, survivals {surv}")
    (m0, e0), (m1, e1), (mx, ex) = stat["rr_depth 0"], stat["rr_depth 1"], stat["no compensation"]
    band = 4.0 * np.hypot(e0, e1)
    print(f"|difference| {abs(m1 - m0):.5f} (allowed {band:.5f}); without the compensation {abs(mx - m0):.5f}")
    assert abs(m1 - m0) <= band and abs(mx - m0) > band and abs(mx - m0) > 4.0 * np.hypot(e0, ex)


def test_colour_is_picked_up_twice():
    """`bleed` under a ceiling: on the floor next to the red wall the indirect term is redder at depth 4 than at depth 1 - light that
    met the wall, then the ceiling or the wall again, is there only at depth >= 2."""
    W, H, J = 48, 27, 8
    ratio = {}
    for K in (1, 4):
        m = sh.path_model("path", "bleed_ceiling", W, H, J, K, 0, noise=0.0)
        x, I = m["gb"]["position"][..., 0], m["I"].astype(np.float64)      # noqa: E741
        near = (m["gb"]["geomId"] == 0) & (x < -2.0)
        assert near.sum() > 20
        ratio[K] = I[near][:, 0].sum() / I[near][:, 1].sum()
        print(f"bleed under a ceiling, max_depth {K}: {int(near.sum())} floor pixels within one unit of the wall, red / green of I {ratio[K]:.4f}")
    assert ratio[1] > 1.0 and ratio[4] > ratio[1]


ALT_SCENES = [("edge", "F_cube", 67, 41), ("path", "bleed_ceiling", 67, 41), ("rec", "cornell", 67, 41), ("made", "stage", 67, 41),
              ("path", "furnace07", 67, 41), ("path", "far_sheet", 67, 41)]


def test_each_alt_acts():
    """Pixels on which the frame of the model and of a wrong variant of it differ, per scene, at 3 paths of up to 4 bounces with the
    roulette from bounce 1 on: every alt changes some scene.  `t_lo_from_first_pos` needs the scene made for it (scene_harness._far_sheet)."""
    J, K, R = 3, 4, 1
    total = {a: 0 for a in spm.ALTS}
    for kind, name, W, H in ALT_SCENES:
        ref = sh.path_model(kind, name, W, H, J, K, R)
        row = {}
        for alt in spm.ALTS:
            m = sh.path_model(kind, name, W, H, J, K, R, alt=alt)
            row[alt] = tsm.any_differs((m["color"], m["gb"]), (ref["color"], ref["gb"]))
            total[alt] += row[alt]
        print(f"scene {name} {W}x{H}: {row}")
    print(f"all scenes: {total}")
    for alt, n in total.items():
        assert n > 0, f"`{alt}` changes no pixel of any scene"


# ---- the GPU cases, and the condition they have to meet ---------------------------------------------------------------------------------
# (kind, name, W, H, paths, max_depth, rr_depth, shadow_secondary, point light): a pruned product at 67x41 - depths 1 / 2 / 4 / 8, paths
# 1 / 3 / 8, rr_depth 0 / 1 / 2, shadow_secondary 0 / 1, point / area light, every value at least twice - over the scenes that meet the
# coverage condition (rr_depth 2 with max_depth 2 never draws a roulette number, so that pair is absent)
PRODUCT = [("edge", "F_cube", 67, 41, 1, 1, 0, 1, False), ("edge", "F_cube", 67, 41, 3, 2, 1, 0, True), ("edge", "F_cube", 67, 41, 8, 4, 2, 1, False),
           ("edge", "F_cube", 67, 41, 1, 8, 1, 1, True), ("edge", "F_cube", 67, 41, 3, 4, 0, 0, False), ("edge", "F_cube", 67, 41, 8, 2, 0, 1, True),
           ("path", "bleed_ceiling", 67, 41, 3, 2, 1, 1, False), ("path", "bleed_ceiling", 67, 41, 1, 4, 2, 0, True),
           ("path", "bleed_ceiling", 67, 41, 3, 8, 1, 1, False), ("path", "bleed_ceiling", 67, 41, 8, 1, 2, 0, True),
           ("rec", "cornell", 67, 41, 3, 4, 1, 1, True), ("rec", "cornell", 67, 41, 1, 8, 2, 0, False), ("rec", "cornell", 67, 41, 8, 2, 0, 1, True),
           ("made", "stage", 67, 41, 8, 4, 1, 1, False), ("made", "stage", 67, 41, 8, 8, 2, 0, True)]
RECORDED = [("rec", "cornell", 96, 96, 1, 4, 2, 1, False), ("rec", "room", 128, 72, 1, 2, 1, 1, False)]
SPECIAL = [("path", "bleed_nan", 67, 41, 3, 3, 2, 1, False), ("traced", "textured", 67, 41, 3, 2, 0, 1, False)]
SPLIT = [("edge", "F_cube", 67, 41, 3, 4, 2, 1, False), ("path", "bleed_ceiling", 67, 41, 1, 4, 2, 0, True), ("rec", "cornell", 67, 41, 8, 2, 0, 1, True)]
TREES = [("edge", "A", 134, 82, 8, 4, 1, 1, False), ("rec", "cornell", 96, 96, 1, 4, 2, 1, False)]
QUEUED = ("edge", "F_cube", 67, 41, 2, 3, 2, 1, False)
BLOCK = [(96, 96, 2, 3, 2), (128, 72, 1, 3, 2)]                 # the posed block: W, H, paths, max_depth, rr_depth
COVERED = PRODUCT + RECORDED + SPECIAL + SPLIT + TREES + [QUEUED]


def _case_model(case, **kw):
    kind, name, W, H, J, K, R, sec, point = case
    return sh.path_model(kind, name, W, H, J, K, R, sec, 1, point, **kw)


def _covered(what, K, R, info):
    second = info["depth"][1]["hits"]
    kills, surv = (sum(d[k] for d in info["depth"]) for k in ("rr_kills", "rr_survivals"))
    print(f"{what}: paths with a hit at bounce 2: {second}; roulette kills {kills}, survivals {surv}; per depth {spm.COUNTS}: {sh.counts_row(info)}")
    assert second >= 100, what
    if R > 0:
        assert kills >= 100 and surv >= 100, what


def test_gpu_cases_reach_depth_two_and_the_roulette():
    values = {k: set() for k in ("paths", "depth", "rr", "sec", "point")}
    for case in PRODUCT:
        for k, v in zip(("paths", "depth", "rr", "sec", "point"), case[4:]):
            values[k].add(v)
    assert values == dict(paths={1, 3, 8}, depth={1, 2, 4, 8}, rr={0, 1, 2}, sec={0, 1}, point={False, True})
    for pos, want in ((4, (1, 3, 8)), (5, (1, 2, 4, 8)), (6, (0, 1, 2)), (7, (0, 1)), (8, (False, True))):
        for v in want:
            assert sum(1 for case in PRODUCT if case[pos] == v) >= 2, (pos, v)
    for case in sorted(set(COVERED)):
        kind, name, W, H, J, K, R, sec, point = case
        if K >= 2 and W * H >= 67 * 41:
            _covered(f"{name} {W}x{H}, {J} paths, max_depth {K}, rr_depth {R}, secondary shadow {sec}, {'point' if point else 'area'} light", K, R,
                     _case_model(case)["info"])
    W, H, J, K, R = BLOCK[0]
    _covered(f"turning block {W}x{H} at rest, {J} paths, max_depth {K}, rr_depth {R}", K, R, _block_model(0, W, H, J, K, R, posed=False)["info"])
    for (W, H, J, K, R), poses in zip(BLOCK, ((0, 2), (0, 1, 2, 3))):
        for f in poses:
            _covered(f"turning block {W}x{H}, pose {f}, {J} paths, max_depth {K}, rr_depth {R}", K, R, _block_model(f, W, H, J, K, R)["info"])


# ---- CPU 3: what examples/path_scene.cpp measures, on the oracle -----------------------------------------------------------------------
def test_denoised_deep_paths_beat_the_noisy_frame_after_eight_static_frames(pkg, orc):
    """64x36, noise 0, eight frames of the example's room with the block at rest, one path of up to 4 bounces (roulette from bounce 2)
    and one shadow ray per pixel through the oracle's full SVGF, against the model's converged frame of the same depth: 8 paths x 64
    shadow rays without roulette, averaged over 16 frame seeds.  The gate is the issue's: the denoised frame beats the noisy one in
    PSNR.  Recorded on the last frame: noisy 10.53 dB / SSIM 0.4641, denoised 18.52 dB / SSIM 0.6347."""
    import quality_model as qm
    from temporal_harness import scales
    W, H, N = 64, 36, 8
    geoms, cam, lk = sh.example_scene()
    p = pkg.reference_defaults().set(temporal_enable=1, spatial_enable=1)
    p.reproj_scale[0], p.reproj_scale[1] = scales(pkg, W, H)
    first = sm.render(W, H, 0, cam, geoms, None, None, None, None, None, None, lk["centre"], seed=7, noise=0.0, fireflies=0.0)
    em = ssm.emitter_mask(W, H, cam, geoms, None, None, None)
    emit = splm.emittance_plane(W, H, cam, geoms, None, None, None)
    frame = lambda f, J, R, samples: spm.render(W, H, f, cam, geoms, None, None, None, None, None, None, ssm.light(samples=samples, **lk),   # noqa: E731
                                                spm.params(J, 4, R), seed=7, noise=0.0, fireflies=0.0, first=first, emitters=em, emittance=emit)
    o = orc.Oracle(pkg, W, H, threads=4)
    try:
        for f in range(N):
            noisy, gb = frame(f, 1, 2, 1)[:2]
            out = o.denoise(noisy, gb, cam, p).reshape(H, W, 3)
    finally:
        o.free()
    ref = np.mean([frame(100 + k, 8, 0, 64)[0].astype(np.float64) for k in range(16)], axis=0).astype(F)
    qn, qd = qm.meter(noisy, ref), qm.meter(out, ref)
    print(f"frame {N - 1}: noisy {qn['psnr_db']:.2f} dB / SSIM {qn['mean_ssim']:.4f}, denoised {qd['psnr_db']:.2f} dB / SSIM {qd['mean_ssim']:.4f}")
    assert qd["psnr_db"] > qn["psnr_db"]


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------
def _what(case):
    kind, name, W, H, J, K, R, sec, point = case
    return f"{name} {W}x{H}, {J} paths, max_depth {K}, rr_depth {R}, secondary shadow {sec}, {'point' if point else 'area'} light"


def _bound(case, m, **more):
    kind, name, W, H, J, K, R, sec, point = case
    return sh.case(sh.scene_input(kind, name)[0], W, H, m["lt"], sh.path_args(J, K, R, sec, **more), m["frame"], m["seed"])


def _draw_case(pkg, case, split=False, rgb=True, **kw):
    m = _case_model(case, **kw)
    return sh.draw_case(pkg, sh.PATH, _bound(case, m, **kw), split=split, rgb=rgb), m


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", sh.SIZES)
def test_path_sizes_and_seams(pkg, W, H):
    got, m = _draw_case(pkg, ("edge", "B", W, H, 2, 3, 2, 1, False))
    sh.same(got, m, f"scene B {W}x{H}, 2 paths, max_depth 3, rr_depth 2")


@pytest.mark.gpu
@pytest.mark.parametrize("case", PRODUCT, ids=lambda c: f"{c[1]}-J{c[4]}-K{c[5]}-R{c[6]}-s{c[7]}-{'point' if c[8] else 'area'}")
def test_parameter_product_equals_the_model(pkg, case):
    got, m = _draw_case(pkg, case)
    sh.same(got, m, _what(case))


@pytest.mark.gpu
@pytest.mark.parametrize("case", RECORDED, ids=lambda c: c[1])
def test_recorded_scene_equals_the_model(pkg, case):
    got, m = _draw_case(pkg, case)
    print(f"{case[1]}: per depth {spm.COUNTS}: {sh.counts_row(m['info'])}")
    sh.same(got, m, _what(case))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 4, 8])
def test_the_furnace_on_the_device(pkg, K):
    W, H, J = 48, 27, 4
    got, m = _draw_case(pkg, ("traced", "furnace", W, H, J, K, 0, 1, False), noise=0.0, ambient=0.0)
    sh.same(got, m, f"furnace, max_depth {K}")
    cast = m["info"]["cast"]
    want = (got["gb"]["albedo"] * m["info"]["ind"]).astype(F)            # ((alb * (0 + ind)) * 1) * 1
    assert not differing(got["color"], want)[cast].any()


@pytest.mark.gpu
def test_nan_normals_behind_the_first_hit(pkg):
    """scene_harness._bleed_nan: pixels whose first hit is the sheet without normals cast paths that end at once, and paths that land on it later
    end there; the model counts both."""
    case = SPECIAL[0]
    got, m = _draw_case(pkg, case)
    first = int(((m["gb"]["geomId"] == 7) & m["info"]["cast"]).sum())
    on_sheet = sum(int((g == 7).sum()) for g in m["info"]["hit_gid"][:-1])
    print(f"{first} pixels see the sheet without normals; {on_sheet} paths land on it before their last bounce")
    assert first > 50 and on_sheet > 100
    sh.same(got, m, _what(case))


@pytest.mark.gpu
def test_a_textured_mesh_behind_the_second_hit(pkg):
    case = SPECIAL[1]
    got, m = _draw_case(pkg, case)
    s = sh.scene_input("traced", "textured")[0]
    tex_ids = list(set(np.asarray(s["tri_ids"])[np.asarray(s["tri_tex"]) >= 0].tolist()))
    on_texture = int(np.isin(m["info"]["hit_gid"][1], tex_ids).sum())
    print(f"{on_texture} of {m['info']['depth'][1]['alive']} second bounces end on a textured triangle")
    assert on_texture > 0
    sh.same(got, m, _what(case))


@pytest.mark.gpu
def test_planar_target_equals_the_model(pkg):
    case = PRODUCT[2]
    m = _case_model(case)
    sh.check_planar_target(pkg, sh.PATH, _bound(case, m), m, "scene F_cube, planar target")


@pytest.mark.gpu
@pytest.mark.parametrize("case", SPLIT, ids=lambda c: c[1])
def test_split_form_equals_the_model_and_recomposes(pkg, case):
    W, H = case[2:4]
    for rgb in (True, False):
        got, m = _draw_case(pkg, case, split=True, rgb=rgb)
        sh.same(got, m, f"{_what(case)}, out_rgb {'given' if rgb else 'NULL'}", split=True, rgb=rgb)
    assert (m["I"] > 0).any()
    want = splm.compose((m["gb"]["albedo"] * m["gb"]["ialbedo"]).astype(F), m["D"], m["I"])
    assert not differing(sh.compose_on_device(pkg, got, W, H), want).any(), "albedo * (D + I) through svgf_trace_compose"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["B", "F_cube"])
def test_depth_one_is_the_other_libraries_on_bits(pkg, name):
    W, H, J = 67, 41, 3
    s = sh.edge(name)[0]
    lt = sh.traced_model("edge", name, W, H, J)[2]
    scene = sh.create(pkg, s)
    traced = sh.draw(pkg, sh.TRACED, scene, W, H, s, lt, sh.trace_args(J))
    split = sh.draw(pkg, sh.TRACED, scene, W, H, s, lt, sh.trace_args(J), split=True)
    for R in (0, 2):
        sh.same(sh.draw(pkg, sh.PATH, scene, W, H, s, lt, sh.path_args(J, 1, R)), traced, f"scene {name}: max_depth 1, rr_depth {R} vs svgf_trace_draw")
        sh.same(sh.draw(pkg, sh.PATH, scene, W, H, s, lt, sh.path_args(J, 1, R), split=True), split, f"scene {name}: max_depth 1, rr_depth {R} vs svgf_trace_draw_split",
                split=True)
    lt3 = sh.shadow_model("edge", name, W, H, 3)[2]
    shadowed = sh.draw(pkg, sh.SHADOWED, scene, W, H, s, lt3)
    sh.same(sh.draw(pkg, sh.PATH, scene, W, H, s, lt3, sh.path_args(0, 4, 2)), shadowed, f"scene {name}: paths 0, ambient 0.15 vs svgf_scene_draw_shadowed")
    scene.free()


@pytest.mark.gpu
@pytest.mark.parametrize("case", TREES, ids=lambda c: c[1])
def test_every_tree_draws_the_same_deep_frame(pkg, case):
    m = _case_model(case)
    sh.check_every_tree(pkg, sh.PATH, _bound(case, m), m, case[1])


@functools.lru_cache(maxsize=None)
def _block_model(f, W, H, J, K, R, posed=True, noise=0.6):
    """Frame f of f15's turning block under f16's area light: the model on the posed arrays (posed=False: the scene as uploaded)."""
    s, tables = sh.block_inputs()
    ps = pm.posed_scene(s, tables[f]) if posed else s
    lk = sh.block_light()
    lt = ssm.light(lk["centre"], lk["edge_u"], lk["edge_v"], 1)
    col, gb, D, I, info = spm.render(W, H, f, ps["cam"], ps["geoms"], None, None, None, None, None, None, lt, spm.params(J, K, R), seed=3,      # noqa: E741
                                     noise=noise, fireflies=0.02 if noise else 0.0)
    return dict(color=col, gb=gb, D=D, I=I, info=info, lt=lt)


@pytest.mark.gpu
def test_the_paths_follow_the_pose(pkg):
    W, H, J, K, R = BLOCK[0]
    s, tables = sh.block_inputs()
    scene = sh.create(pkg, s)
    m = _block_model(0, W, H, J, K, R, posed=False)
    sh.same(sh.draw(pkg, sh.PATH, scene, W, H, s, m["lt"], sh.path_args(J, K, R), frame=0, seed=3), m, "turning block, before any pose")
    scene.enable_pose(len(s["geoms"]))
    ind = []
    for f in (0, 2):
        m = _block_model(f, W, H, J, K, R)
        scene.pose(sh.dev(tables[f]))
        sh.same(sh.draw(pkg, sh.PATH, scene, W, H, s, m["lt"], sh.path_args(J, K, R), frame=f, seed=3), m, f"turning block, pose {f}")
        sh.same(sh.draw(pkg, sh.PATH, scene, W, H, s, m["lt"], sh.path_args(J, K, R), split=True, frame=f, seed=3), m, f"turning block, pose {f}, split form",
                split=True)
        ind.append(m["info"]["ind"])
    scene.free()
    assert int((ind[0] != ind[1]).any(axis=-1).sum()) > 50


@pytest.mark.gpu
def test_eight_path_draws_queued_without_host_waits(pkg):
    sh.check_queued(pkg, sh.PATH, _bound(QUEUED, _case_model(QUEUED)), lambda f: _case_model(QUEUED, frame=f), "queued path draw")


@pytest.mark.gpu
@pytest.mark.parametrize("split", [False, True])
def test_a_captured_path_draw_is_one_kernel_node_and_replays_the_same_bits(pkg, split):
    m = _case_model(QUEUED)
    sh.check_captured(pkg, sh.PATH, _bound(QUEUED, m), m, "path draw", split=split)


@pytest.mark.gpu
def test_every_error_code_of_both_calls(pkg):
    import torch
    B = pkg.binding
    s = sh.edge("B")[0]
    scene = sh.create(pkg, s)
    lib = pkg.load_path_library()
    c, p = ctypes.byref(B.SvgfCamera()), ctypes.byref(B.SvgfSynthParams())
    ok = ctypes.byref(B.SvgfSceneLight.make((0, 1, 0), (1, 0, 0), (0, 0, 1), 4))
    pp = ctypes.byref(B.SvgfPathParams(1, 4, 2, 0.15, 1))
    guard = torch.full((64,), 7.0, dtype=torch.float32, device="cuda")       # every pointer below is this buffer: a refused call writes nothing
    a = guard.data_ptr()
    plain = lambda h=scene.h, rgb=a, gb=a, pl=None, w=1, hh=1, cm=c, spp=p, lt=ok, t=pp: lib.svgf_path_draw(h, rgb, gb, pl, w, hh, cm, spp, lt, t, None)  # noqa: E731
    split = lambda h=scene.h, d=a, i=a + 16, rgb=a, gb=a, pl=None, w=1, hh=1, cm=c, spp=p, lt=ok, t=pp: lib.svgf_path_draw_split(   # noqa: E731
        h, d, i, rgb, gb, pl, w, hh, cm, spp, lt, t, None)
    assert plain(rgb=None) == -1
    assert split(d=None) == -1 and split(i=None) == -1 and split(d=a, i=a) == -1
    for f in (plain, split):
        sh.check_common_refusals(B, f, (B.SvgfPathParams, sh.BAD_PARAMS))
    torch.cuda.synchronize()
    assert (guard.cpu().numpy() == F(7.0)).all()
    case = ("edge", "B", 7, 5, 2, 3, 2, 1, False)
    m = _case_model(case)
    sh.same(sh.draw(pkg, sh.PATH, scene, 7, 5, s, m["lt"], sh.path_args(2, 3, 2)), m, "after the refused calls")
    sh.same(sh.draw(pkg, sh.PATH, scene, 7, 5, s, m["lt"], sh.path_args(2, 3, 2), split=True), m, "after the refused calls, split form", split=True)
    scene.free()


# ---- GPU: end to end -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_pose_split_path_draw_two_denoises_compose_sequence(pkg, orc):
    """128x72, four frames of the turning block on one stream: pose -> svgf_path_draw_split (1 path of up to 3 bounces, roulette from
    bounce 2, 1 shadow ray) -> svgf_denoise of each term in a context of its own (temporal pass, sepcolor 1 / addcolor 0, the object
    motion table on; the f8 firefly filter on the indirect context only) -> svgf_trace_compose.  Each context against
    tests/temporal_model.py behind tests/firefly_model.py, the composed image against compose() of the two outputs, all on bits."""
    (W, H, J, K, R), N = BLOCK[1], 4
    sh.run_split_denoise_compose(pkg, orc, sh.PATH, [_block_model(f, W, H, J, K, R) for f in range(N)], W, H, sh.path_args(J, K, R),
                                 ("direct context", "indirect context"), form="filtered")
