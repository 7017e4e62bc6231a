"""The resident scene (include/svgf.h row f14: svgf_scene_create / svgf_scene_draw* / svgf_bvh_build_host).

The contract is a gated brute force that every BVH reproduces (the header states it; tests/resident_scene_model.py restates the
padded box, the slab test and the gate in numpy).  CPU part: the builder's invariants on recorded and adversarial triangle sets, the
gate precondition of every input the GPU part draws (the ungated winner of each pixel passes its own gate, so the frame is
tests/scene_model.py's and svgf_scene_render_mesh's), and the argument errors that need no device.  GPU part: the drawn frame
against the model AND against svgf_scene_render_mesh on bits, all fields and the colour (NaNs in the same place equal); the expected
number of differing pixels is 0 and the allowance is test_scene_model.py's cap(W, H).

The builder's leaf rule, as implemented and tested: every leaf holds 1 .. max_leaf_tris triangles, with no exception at the depth
bound - a node with n triangles and r levels left is only created with n <= max_leaf_tris * 2^r, so the bound is met by splitting
evenly early enough, never by a larger leaf.
"""
import ctypes
import functools

import numpy as np
import pytest

import resident_scene_model as rm
import scene_harness as sh
import scene_model as sm
import test_scene_model as tsm
from test_scene_model import FRAME, SEED, cap, counts

F = np.float32
EDGE_WITH_TRIS = ("A", "B", "C", "D", "F_cube", "F_sphere")


# ---- CPU 1: the builder ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sh.TRI_SETS)
def test_builder_invariants(pkg, name):
    tris = sh.tri_set(name)
    n = len(tris)
    lo, hi = rm.padded_boxes(tris)
    for ml, sp in sh.BUILDS:
        nodes, order, depth = pkg.bvh_build_host(tris, ml, sp)
        again = pkg.bvh_build_host(tris, ml, sp)
        assert nodes.tobytes() == again[0].tobytes() and np.array_equal(order, again[1]) and depth == again[2], "two builds differ"
        if n == 0:
            assert len(nodes) == 0 and depth == 0
            continue
        assert sorted(order.tolist()) == list(range(n)), "order is not a permutation"
        leaf = nodes["count"] > 0
        assert len(nodes) == 2 * int(leaf.sum()) - 1, "n_nodes is not 2 * n_leaves - 1"
        assert nodes["count"].min() >= 0 and nodes["count"][leaf].max() <= ml, "a leaf holds more than max_leaf_tris"
        # a walk from the root: every node reached once, levels, every position of `order` in exactly one leaf
        seen, covered, deepest = np.zeros(len(nodes), int), np.zeros(n, int), 0
        todo = [(0, 0)]
        while todo:
            k, level = todo.pop()
            seen[k] += 1
            deepest = max(deepest, level)
            nd = nodes[k]
            if nd["count"] > 0:
                covered[int(nd["first"]):int(nd["first"]) + int(nd["count"])] += 1
            else:
                assert 1 <= nd["first"] and nd["first"] + 1 < len(nodes)
                todo += [(int(nd["first"]), level + 1), (int(nd["first"]) + 1, level + 1)]
        assert (seen == 1).all() and (covered == 1).all(), "a node or a triangle is reached more or less than once"
        assert deepest == depth <= pkg.binding.SCENE_MAX_DEPTH
        # boxes: the union of the model's padded boxes below the node, on bits (checked on every node of small trees, a sample of large ones)
        pick = range(len(nodes)) if len(nodes) <= 700 else np.random.default_rng(ml + sp).choice(len(nodes), 300, replace=False).tolist() + [0]
        for k in pick:
            ids = order[rm.leaves_below(nodes, k)]
            assert nodes[k]["lo"].tobytes() == lo[ids].min(axis=0).tobytes() and nodes[k]["hi"].tobytes() == hi[ids].max(axis=0).tobytes(), f"node {k}"
        print(f"{name} leaf {ml} split {sp}: {len(nodes)} nodes, {int(leaf.sum())} leaves, depth {depth}")


def test_builder_reorders_scene_A_duplicates(pkg):
    """Scene A stores one triangle twice (indices 5 and 6).  At least one of the six builds places index 6 before 5, so the draw's
    'lowest index wins a tie' (GPU test below) is decided by the draw and not by the builder's order."""
    flipped = []
    for ml, sp in sh.BUILDS:
        order = pkg.bvh_build_host(sh.tri_set("A"), ml, sp)[1].tolist()
        flipped.append(order.index(6) < order.index(5))
    print("index 6 before 5 per build:", dict(zip(sh.BUILDS, flipped)))
    assert any(flipped)


# ---- CPU 2: the gate precondition of every input the GPU part draws ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gate(kind, name, f, W, H):
    s = tsm._scene(name) if kind == "edge" else sh.recorded(name, f)[0]
    return rm.gate_report(W, H, s["cam"], s["tris"])


GATE_CASES = [("edge", n, 0, W, H) for n in EDGE_WITH_TRIS for W, H in tsm.SIZES] + \
             [("rec", "cornell", f, 96, 96) for f in range(4)] + [("rec", "room", 0, 128, 72), ("rec", "bunny", 0, 128, 72)]


@pytest.mark.parametrize("kind,name,f,W,H", GATE_CASES)
def test_gate_precondition(kind, name, f, W, H):
    """The ungated winner of every pixel passes its own gate (padded box, t >= tn): 0 pixels, no allowance.  (The gate does not depend
    on SvgfSynthParams, so one camera covers every frame number drawn with it.)"""
    r = _gate(kind, name, f, W, H)
    print(f"{name} frame {f} {W}x{H}: {int((r['best'] >= 0).sum())} pixels with a triangle winner, {r['winner_fails']} winners fail the gate; "
          f"{r['pairs']} accepted (ray, triangle) pairs, {r['pair_fails']} fail it")
    assert r["winner_fails"] == 0
    if W * H > 1:
        assert (r["best"] >= 0).sum() > cap(W, H), "the input shows no triangles"


def test_axis_parallel_rays_take_the_flat_branch():
    """Scene A at 67x41: the centre column / row have a direction component of exactly 0, and every triangle is flat in z or nearly."""
    r = _gate("edge", "A", 0, 67, 41)
    print(f"scene A 67x41: {r['flat_rays']} rays with |d_c| < 2^-100 on some axis")
    assert r["flat_rays"] >= 67


# ---- CPU 3: argument errors answered before any device work ----------------------------------------------------------------------------
def test_argument_errors(pkg):
    lib = pkg.load_library()
    B = pkg.binding
    tris = np.ascontiguousarray(sh.tri_set("A"), F).reshape(-1, 24)
    n = len(tris)
    ids, alb = np.zeros(n, np.int32), np.zeros((n, 3), F)
    h = ctypes.c_void_p()

    def create(tr=tris, n_tris=n, bp=None, out=h, device=0, tri_ids=ids):
        return lib.svgf_scene_create(device, None, 0, None, tr.ctypes.data if tr is not None else None, tri_ids.ctypes.data if tri_ids is not None else None,
                                     alb.ctypes.data, n_tris, None, None, None, 0, ctypes.byref(bp) if bp is not None else None,
                                     ctypes.byref(out) if out is not None else None)
    assert create(out=None) == -1
    assert create(tr=None) == -1 and create(tri_ids=None) == -1 and create(n_tris=-1) == -1 and create(n_tris=(1 << 20) + 1) == -1
    for bp in ((9, 0), (-1, 0), (4, 2), (4, -1)):
        assert create(bp=B.SvgfSceneBuildParams(*bp)) == -1, bp
    for v, c, bad in ((0, 0, np.nan), (2, 1, np.inf), (1, 2, -np.inf)):
        t = tris.copy()
        t[n // 2, 8 * v + c] = bad
        assert create(tr=t) == -1, (v, c, bad)
    assert create(device=64) == -5 and create(device=-1) == -5          # SVGF_ERR_UNSUPPORTED, as svgf_scene_render_mesh answers
    assert h.value is None
    cam, sp, light = B.SvgfCamera(), B.SvgfSynthParams(), (ctypes.c_float * 3)()
    planes = B.SvgfPlanarGBuffer()
    assert lib.svgf_scene_draw(None, 1, 1, 8, 8, ctypes.byref(cam), ctypes.byref(sp), light, None) == -1
    assert lib.svgf_scene_draw_planar(None, 1, ctypes.byref(planes), 8, 8, ctypes.byref(cam), ctypes.byref(sp), light, None) == -1
    assert lib.svgf_scene_info(None, ctypes.byref(B.SvgfSceneInfo())) == -1
    assert lib.svgf_scene_destroy(None) == 0
    nodes, order = np.zeros(2 * n, B.BVH_NODE_DTYPE), np.zeros(n, np.int32)
    nn, dp = ctypes.c_int(), ctypes.c_int()
    build = lambda tr, n_tris, nd, od, bp=None: lib.svgf_bvh_build_host(tr, n_tris, bp, nd, ctypes.byref(nn), od, ctypes.byref(dp))   # noqa: E731
    assert build(tris.ctypes.data, n, nodes.ctypes.data, order.ctypes.data) == 0 and nn.value > 0
    assert build(None, n, nodes.ctypes.data, order.ctypes.data) == -1 and build(tris.ctypes.data, n, None, order.ctypes.data) == -1
    assert build(tris.ctypes.data, n, nodes.ctypes.data, None) == -1 and build(tris.ctypes.data, -1, nodes.ctypes.data, order.ctypes.data) == -1
    assert build(tris.ctypes.data, n, nodes.ctypes.data, order.ctypes.data, ctypes.byref(B.SvgfSceneBuildParams(0, 3))) == -1
    assert lib.svgf_bvh_build_host(tris.ctypes.data, n, None, nodes.ctypes.data, None, order.ctypes.data, ctypes.byref(dp)) == -1


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", EDGE_WITH_TRIS + ("E_plus", "G"))
def test_draw_equals_model_and_mesh_path_on_edge_scene(pkg, name):
    s = tsm._scene(name)
    scene = sh.create(pkg, s)
    for W, H in tsm.SIZES:
        got = sh.draw_frame(pkg, scene, W, H, s, FRAME, SEED)
        sh.same_capped(got, tsm._model(name, W, H), W, H, f"scene {name} vs model")
        sh.same_capped(got, tsm._device(pkg, W, H, s, FRAME, SEED), W, H, f"scene {name} vs svgf_scene_render_mesh")
    assert scene.info()["n_nodes"] == (0 if s["tris"] is None else 2 * scene.info()["n_leaves"] - 1)
    scene.free()


@pytest.mark.gpu
def test_draw_planar_equals_model_on_textures(pkg):
    """Scene C through svgf_scene_draw_planar into a context's planes."""
    W, H = tsm.SIZES[0]
    s = tsm._scene("C")
    scene = sh.create(pkg, s)
    den = pkg.Denoiser(W, H, 0)
    got = sh.pair(sh.draw(pkg, sh.RESIDENT, scene, W, H, s, None, planes=den.planar_gbuffer()))
    sh.same_capped(got, tsm._model("C", W, H), W, H, "scene C planar vs model")
    sh.same_capped(got, tsm._device(pkg, W, H, s, FRAME, SEED, planar=True), W, H, "scene C planar vs svgf_scene_render_mesh_planar")
    den.free(); scene.free()


@pytest.mark.gpu
@pytest.mark.parametrize("scene_name,frames", [("room", (0,)), ("cornell", (0, 3)), ("bunny", (0,))])
def test_draw_equals_model_and_mesh_path_on_recorded_scene(pkg, scene_name, frames):
    """bunny: against svgf_scene_render_mesh only (the numpy frame over 4 968 triangles is what would make this slow; its gate
    precondition is test_gate_precondition's)."""
    scene = sh.create(pkg, sh.recorded(scene_name, 0)[0])
    for f in frames:
        s, W, H = sh.recorded(scene_name, f)
        got = sh.draw_frame(pkg, scene, W, H, s, f, 1)
        if scene_name != "bunny":
            sh.same_capped(got, tsm._recorded_model(sh.RECORDED[scene_name], scene_name, f), W, H, f"{scene_name} frame {f} vs model")
        ref = tsm._device(pkg, W, H, s, f, 1)
        assert np.isin(ref[1]["geomId"], np.unique(s["tri_ids"])).mean() > 0.01, "the scene's meshes should be in the picture"
        sh.same_capped(got, ref, W, H, f"{scene_name} frame {f} vs svgf_scene_render_mesh")
    scene.free()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["room", "A"])
def test_every_tree_draws_the_same_frame(pkg, name):
    (s, W, H) = sh.recorded("room", 0) if name == "room" else (tsm._scene("A"), 67, 41)
    frames, infos = [], []
    for ml, sp in sh.BUILDS:
        scene = sh.create(pkg, s, ml, sp)
        frames.append(sh.draw_frame(pkg, scene, W, H, s, FRAME, SEED))
        infos.append(scene.info())
        scene.free()
    assert len({(i["n_nodes"], i["depth"]) for i in infos}) >= 4, "the builds should differ in shape"
    for (ml, sp), fr in zip(sh.BUILDS[1:], frames[1:]):
        c = counts(fr, frames[0])
        assert not any(c.values()), f"leaf {ml} split {sp} differs from leaf 1 split 0: {c}"


@pytest.mark.gpu
def test_ties_lowest_index_and_primitive_win(pkg):
    """Scene A: triangle 5 (geomId 14) is stored again as 6 (geomId 15): 14 wins on every pixel, in every build, also where the
    builder placed 6 before 5.  Scene B: a triangle (geomId 9) lies in the plane of the cube's front face: the cube keeps the tie."""
    W, H = 67, 41
    A, B = tsm._scene("A"), tsm._scene("B")
    want = tsm._model("A", W, H)[1]["geomId"]
    assert (want == 14).sum() > cap(W, H) and not (want == 15).any()
    for ml, sp in sh.BUILDS:
        scene = sh.create(pkg, A, ml, sp)
        gid = sh.draw_frame(pkg, scene, W, H, A, FRAME, SEED)[1]["geomId"]
        scene.free()
        assert np.array_equal(gid, want), f"leaf {ml} split {sp}: {int((gid != want).sum())} pixels, {int((gid == 15).sum())} show the copy"
    ref, le = tsm._model("B", W, H)[1]["geomId"], tsm._model("B", W, H, "tri_le")[1]["geomId"]
    assert ((le == 9) & (ref == 7)).sum() > cap(W, H), "scene B should hold a tie between triangle 2 and the cube"
    scene = sh.create(pkg, B)
    gid = sh.draw_frame(pkg, scene, W, H, B, FRAME, SEED)[1]["geomId"]
    scene.free()
    assert np.array_equal(gid, ref)


@pytest.mark.gpu
def test_eight_draws_queued_without_host_waits(pkg):
    import torch
    W, H = 67, 41
    s = tsm._scene("A")
    scene = sh.create(pkg, s)
    st = torch.cuda.Stream()
    bufs = [sh.buffers(W, H) for _ in range(8)]
    for f, (rgb, gbt) in enumerate(bufs):
        scene.draw(rgb, gbt, W, H, s["cam"], s["light"], f, seed=SEED, stream=st)
    st.synchronize()
    for f, (rgb, gbt) in enumerate(bufs):
        ref = sm.render(W, H, f, s["cam"], s["geoms"], s["geom_ids"], s["tris"], s["tri_ids"], s["tri_albedo"], None, None, s["light"], seed=SEED)
        sh.same_capped(sh.host(pkg, rgb, gbt, W, H), ref, W, H, f"queued draw, frame {f}")
    scene.free()


@pytest.mark.gpu
def test_a_captured_draw_replays_the_same_bits(pkg):
    import torch
    W, H = 67, 41
    s = tsm._scene("B")
    scene = sh.create(pkg, s)
    st = torch.cuda.Stream()
    rgb, gbt = sh.buffers(W, H)
    record = lambda: scene.draw(rgb, gbt, W, H, s["cam"], s["light"], FRAME, seed=SEED, stream=st)      # noqa: E731
    record()                                # eager first: a first launch may set kernel attributes
    st.synchronize()
    want = sh.host(pkg, rgb, gbt, W, H)
    graph = sh.Captured(st, record)         # recorded, not executed
    with torch.cuda.stream(st):
        rgb.zero_(); gbt.zero_()
    graph.launch()
    st.synchronize()
    got = sh.host(pkg, rgb, gbt, W, H)
    graph.destroy()
    scene.free()
    assert (got[1]["geomId"] >= 0).any() and not any(counts(got, want).values())
    sh.same_capped(got, tsm._model("B", W, H), W, H, "replayed draw vs model")


@pytest.mark.gpu
def test_draws_feed_a_denoise_sequence_on_one_stream(pkg):
    """cornell 96x96, frames 0..2 of the recorded cameras: draw -> svgf_denoise -> draw -> ... on one stream without host waits equals
    the same sequence fed by svgf_scene_render_mesh, on bits."""
    import torch
    N = 3
    st = torch.cuda.Stream()
    p = pkg.reference_defaults().set(temporal_enable=1, spatial_enable=1)
    outs = {}
    scene = sh.create(pkg, sh.recorded("cornell", 0)[0])
    for path in ("draw", "mesh"):
        s0, W, H = sh.recorded("cornell", 0)
        den = pkg.Denoiser(W, H, 0)
        rgb, gbt = sh.buffers(W, H)
        out = [torch.empty((H, W, 3), dtype=torch.float32, device="cuda") for _ in range(N)]
        for f in range(N):
            s = sh.recorded("cornell", f)[0]
            if path == "draw":
                scene.draw(rgb, gbt, W, H, s["cam"], s["light"], f, stream=st)
            else:
                pkg.binding.scene_render_mesh(rgb, gbt, W, H, s["cam"], s["geoms"], s["geom_ids"], s["tris"], s["tri_ids"], s["tri_albedo"], frame=f,
                                              tri_tex=s["tri_tex"], textures=s["textures"], light=s["light"], stream=st)
            den.denoise(out[f], rgb, gbt, s["cam"], p, stream=st)
        st.synchronize()
        outs[path] = [o.cpu().numpy() for o in out]
        den.free()
    scene.free()
    for f in range(N):
        assert np.isfinite(outs["mesh"][f]).all() and outs["mesh"][f].max() > 0
        assert np.array_equal(outs["draw"][f], outs["mesh"][f]), f"frame {f}"


@pytest.mark.gpu
def test_scene_info_and_draw_argument_errors(pkg):
    B = pkg.binding
    s = sh.recorded("cornell", 0)[0]
    for ml, sp in ((0, 0), (1, 1), (8, 0)):
        scene = sh.create(pkg, s, ml, sp)
        nodes, order, depth = pkg.bvh_build_host(s["tris"], ml, sp)
        i = scene.info()
        print(f"cornell leaf {ml} split {sp}: {i}")
        assert (i["n_geoms"], i["n_tris"], i["n_tex"]) == (len(s["geoms"]), len(s["tris"]), 1)
        assert (i["n_nodes"], i["n_leaves"], i["depth"], i["max_leaf_tris"]) == (len(nodes), int((nodes["count"] > 0).sum()), depth, ml or 4)
        assert i["device_bytes"] >= s["tris"].nbytes + nodes.nbytes + order.nbytes + s["textures"][0].nbytes
        scene.free()
    scene = sh.create(pkg, s)
    lib = scene.lib
    cam, sp_, light = B.SvgfCamera(), B.SvgfSynthParams(), (ctypes.c_float * 3)()
    args = (ctypes.byref(cam), ctypes.byref(sp_), light, None)
    assert lib.svgf_scene_draw(scene.h, 1, 1, 0, 8, *args) == -1 and lib.svgf_scene_draw(scene.h, 1, 1, 8, -1, *args) == -1
    assert lib.svgf_scene_draw(scene.h, None, 1, 8, 8, *args) == -1 and lib.svgf_scene_draw(scene.h, 1, None, 8, 8, *args) == -1
    assert lib.svgf_scene_draw(scene.h, 1, 1, 1 << 14, 1 << 13, *args) == -5         # width * height == 2^31 / 16
    assert lib.svgf_scene_draw_planar(scene.h, 1, None, 8, 8, *args) == -1
    assert lib.svgf_scene_draw_planar(scene.h, 1, ctypes.byref(B.SvgfPlanarGBuffer()), 8, 8, *args) == -1
    scene.free()
