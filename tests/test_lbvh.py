"""Row f24: the device BVH builder (include/svgf_lbvh.h, libsvgf_lbvh.so) and svgf_scene_adopt_tree (include/svgf.h).

CPU: tests/lbvh_model.py implements the header's normative text independently (numpy keys, numpy's sort, a sequential top-down Karras
tree); the model's trees and svgf_lbvh_build_host's are held to the invariants and to each other - keys, order, first / count on bits,
boxes by value - on every case; the host builder runs under AddressSanitizer / UBSan as a stand-alone program; every refusal that
needs no device; the new library's exports and NEEDED entries, and the seven companions' export lists as they were.

GPU: svgf_lbvh_build against the model on the scene's boxes as drawn (svgf_scene_read kind 1) across every seam of the kernel plan;
the frame with the tree attached against the frame of the scene's own tree on every bit; detach; pose -> build -> draw against
pose (refit) -> draw; capture.  In every GPU test the tree is read back and held to the model BEFORE a draw walks it: a wrong tree
fails a comparison and never reaches the walk.
"""
import ctypes
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import lbvh_model as lm
import resident_scene_model as rm
import scene_harness as sh
import test_scene_model as tsm
from conftest import ROOT
from test_scene_model import FRAME, SEED

F = np.float32
W0, H0 = 67, 41
ERR = -1                # SVGF_ERR_INVALID_ARG


# ---- CPU inputs --------------------------------------------------------------------------------------------------------------------------
def _random_boxes(n, seed, spread=3.0):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-spread, spread, (n, 3)).astype(F)
    h = rng.uniform(0.001, 0.2, (n, 3)).astype(F)
    return lm.boxes_of((c - h).astype(F), (c + h).astype(F))


def _tri_boxes(name):
    return lm.boxes_of(*rm.padded_boxes(sh.tri_set(name)))


@functools.lru_cache(maxsize=None)
def _case(name):
    """(NODE[n] padded boxes, leaf_tris)"""
    if name[0] == "n" and name[1].isdigit():         # n<count>_L<leaf>
        n, L = (int(x[1:]) for x in name.split("_"))
        return _random_boxes(n, 24 + n), L
    if name == "coincident4096":
        return np.repeat(_tri_boxes("one"), 4096), 1
    if name == "zero_area":
        return _tri_boxes("zero_area257"), 4
    if name == "one_axis":
        return _tri_boxes("line4096"), 4
    if name == "two_clusters":
        b = _random_boxes(600, 5, 1.0)
        b["lo"][300:, 0] += F(1e6); b["hi"][300:, 0] += F(1e6)
        return b, 4
    if name == "nan_inf":
        b = _random_boxes(301, 6)
        b["lo"][7, 0], b["hi"][7, 2] = np.nan, np.nan
        b["lo"][8], b["hi"][8] = np.nan, np.nan
        b["lo"][11, 1], b["hi"][12, 1] = -np.inf, np.inf
        b["lo"][13], b["hi"][13] = -np.inf, np.inf
        b["lo"][14], b["hi"][14] = np.inf, np.inf
        return b, 4
    if name in ("room", "bunny"):
        return _tri_boxes(name), 4
    raise KeyError(name)


CASES = ["n1_L4", "n2_L4", "n3_L4", "n4_L4", "n5_L4", "n1_L1", "n2_L1", "n8_L8", "n9_L8", "n1027_L1", "n1027_L8", "coincident4096", "zero_area",
         "one_axis", "two_clusters", "nan_inf", "room", "bunny"]


@functools.lru_cache(maxsize=None)
def _model(name):
    boxes, L = _case(name)
    return lm.build(boxes, L)


# ---- CPU 1: the model and the invariants ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_model_trees_hold_the_invariants(name):
    boxes, L = _case(name)
    m = _model(name)
    depth = lm.check_invariants(m["nodes"], m["order"], m["keys"], boxes, L, m["info"]["depth_bound"])
    print(f"{name}: n {len(boxes)} leaves {m['info']['n_leaves']} key_bits {m['info']['key_bits']} depth {depth} <= {m['info']['depth_bound']}")
    if name == "coincident4096":
        assert depth == m["info"]["idx_bits"] == 12, "coincident triangles differ in their index bits alone: a complete tree over them"


def test_bit_budget():
    assert lm.bits(1) == (1, 10, 31) and lm.bits(2) == (1, 10, 31) and lm.bits(3) == (2, 10, 32) and lm.bits(5) == (3, 10, 33)
    assert lm.bits(1 << 18) == (18, 10, 48) and lm.bits((1 << 18) + 1) == (19, 9, 46) and lm.bits(1 << 20) == (20, 9, 47)
    assert all(lm.bits(n)[2] <= 48 for n in (1, 2, 1000, 1 << 16, (1 << 16) + 1, 1 << 19, (1 << 19) + 1, 1 << 20))


# ---- CPU 2: the host builder --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_host_builder_equals_the_model(pkg, name):
    boxes, L = _case(name)
    nodes, order, keys, info = pkg.lbvh_build_host(boxes, L)
    m = _model(name)
    assert {k: info[k] for k in m["info"]} == m["info"]
    lm.check_invariants(nodes, order, keys, boxes, L, info["depth_bound"])
    lm.same_tree(nodes, order, keys, m, name)


def test_host_builder_default_leaf_and_null_keys(pkg):
    boxes = _random_boxes(37, 3)
    lib = pkg.load_lbvh_library()
    nodes, order, info = np.zeros(2 * 10, lm.NODE), np.zeros(37, np.int32), pkg.SvgfLbvhInfo()
    assert lib.svgf_lbvh_build_host(boxes.ctypes.data, 37, None, nodes.ctypes.data, order.ctypes.data, None, ctypes.byref(info)) == 0
    assert info.leaf_tris == 4 and info.n_leaves == 10
    lm.same_tree(nodes[:info.n_nodes], order, None, lm.build(boxes, 4), "NULL params, NULL keys")


def test_host_builder_native_program_under_sanitizers(tmp_path):
    import shutil
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "lbvh_host_main")
    src = [os.path.join(ROOT, "tests", "native", "lbvh_host_main.cpp"), os.path.join(ROOT, "cuda-path-tracer-denoising_amd", "csrc", "svgf_lbvh_host.cpp")]
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-I",
                        os.path.join(ROOT, "include")] + src + ["-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "all trees hold" in r.stdout, r.stdout


# ---- CPU 3: refusals that need no device ------------------------------------------------------------------------------------------------
def test_refusals_without_a_device(pkg):
    lib, lb = pkg.load_library(), pkg.load_lbvh_library()
    buf = np.zeros(64, np.uint8)
    assert lib.svgf_scene_adopt_tree(None, buf.ctypes.data, buf.ctypes.data, 1, 1, 0) == ERR
    assert lib.svgf_scene_adopt_tree(None, None, None, 0, 0, 0) == ERR
    h = ctypes.c_void_p(77)
    assert lb.svgf_lbvh_create(None, None, ctypes.byref(h)) == ERR and not h.value, "a refused create clears *out"
    assert lb.svgf_lbvh_create(None, ctypes.byref(pkg.SvgfLbvhParams(9)), ctypes.byref(h)) == ERR
    assert lb.svgf_lbvh_create(None, None, None) == ERR
    assert lb.svgf_lbvh_build(None, None) == ERR
    assert lb.svgf_lbvh_attach(None, None) == ERR
    assert lb.svgf_lbvh_info(None, ctypes.byref(pkg.SvgfLbvhInfo())) == ERR
    assert lb.svgf_lbvh_read(None, 0, buf.ctypes.data, 32) == ERR
    lb.svgf_lbvh_destroy(None)
    assert lb.svgf_lbvh_version() == lib.svgf_version()
    boxes = _random_boxes(5, 1)
    nodes, order, keys, info = np.zeros(4, lm.NODE), np.zeros(5, np.int32), np.zeros(5, np.uint64), pkg.SvgfLbvhInfo()
    P = lambda L: ctypes.byref(pkg.SvgfLbvhParams(L))      # noqa: E731
    a = [boxes.ctypes.data, 5, P(4), nodes.ctypes.data, order.ctypes.data, keys.ctypes.data, ctypes.byref(info)]
    for k, v in ((0, None), (1, 0), (1, -1), (1, (1 << 20) + 1), (2, P(9)), (2, P(-1)), (3, None), (4, None), (6, None)):
        bad = list(a)
        bad[k] = v
        assert lb.svgf_lbvh_build_host(*bad) == ERR, (k, v)
    assert lb.svgf_lbvh_build_host(*a) == 0


# ---- CPU 4: the library's surface, and the companions' as it was ---------------------------------------------------------------------------
def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return sorted(ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("svgf_"))


def test_exports_and_links(pkg):
    B, bld = pkg.binding, pkg.build
    path = bld.build_lbvh()
    assert path == B.LIB_LBVH_PATH and os.path.basename(path) == "libsvgf_lbvh.so"
    assert _exports(path) == sorted(B.LBVH_EXPORTS)
    out = subprocess.run(["readelf", "-d", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    needed = sorted(ln.split("[")[1].split("]")[0] for ln in out.splitlines() if "(NEEDED)" in ln and "[libsvgf_" in ln)
    assert needed == ["libsvgf_hip.so"], needed
    assert "svgf_scene_adopt_tree" in _exports(bld.LIB) and "svgf_scene_adopt_tree" in B.EXPORTS
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "companion_abi.json")))
    for c in B.COMPANIONS:
        assert _exports(B.companion_path(c.name)) == sorted(golden["exports"][f"{c.name.upper()}_EXPORTS"]) == sorted(c.exports), c.name
    paths = bld.build_all()
    assert len(paths) == 8 and path not in paths
    assert [c.name for c in bld.COMPANIONS] == [c.name for c in B.COMPANIONS] and "lbvh" not in [c.name for c in bld.COMPANIONS]
    assert [b.name for b in bld.BUILDERS] == ["lbvh"] and "-ffp-contract=off" in bld.BUILDERS[0].flags
    assert not [m for m in vars(pkg.Scene) if m.startswith("draw") and "tree" in m]


# ---- GPU helpers ----------------------------------------------------------------------------------------------------------------------------
def _tri_scene(tris, n_obj=3):
    n = len(tris)
    return dict(cam=tsm._scene("A")["cam"], geoms=None, geom_ids=None, tris=tris, tri_ids=(np.arange(n) % n_obj).astype(np.int32),
                tri_albedo=tsm._colours(n, 15), tri_tex=None, textures=None, light=(1.0, 3.0, 4.0))


@functools.lru_cache(maxsize=None)
def _small_tris(n, seed=24):
    rng = np.random.default_rng(seed + n)
    c = rng.uniform(-2, 2, (n, 1, 3)).astype(F)
    t = np.zeros((n, 3, 8), F)
    t[:, :, 0:3] = c + rng.uniform(-0.05, 0.05, (n, 3, 3)).astype(F)
    return t


def _checked_build(pkg, scene, tree, what, stream=None, twice=False):
    """build, read back, hold to the model on the scene's boxes as drawn; returns the model.  Nothing walks the tree in here."""
    import torch
    tree.build(stream)
    torch.cuda.synchronize()
    boxes = scene.read(1)
    info = tree.info()
    m = lm.build(boxes, info["leaf_tris"])
    assert {k: info[k] for k in m["info"]} == m["info"], what
    got = [tree.read(k) for k in (0, 1, 2)]
    lm.same_tree(got[0], got[1], got[2], m, what)
    if twice:
        tree.build(stream)
        torch.cuda.synchronize()
        again = [tree.read(k) for k in (0, 1, 2)]
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again)), f"{what}: a second build gives other bytes"
    return m


# ---- GPU 1: the device build equals the model -----------------------------------------------------------------------------------------------
# n_tris = 4 * leaves - 1: leaf counts 1, 2, 3, 256, 257 (a workgroup seam of the hierarchy), 512, 513 (the tile seam), 1025, 4097 (a top
# over 9 tiles); 65 537 triangles: 33 sort blocks, a scan over 8 448 histogram entries, 17 bits of index
DEVICE_SIZES = [(3, 4), (7, 4), (11, 4), (1023, 4), (1027, 4), (2047, 4), (2051, 4), (4099, 4), (16387, 4), (65537, 4), (1027, 1), (1027, 8), (1, 4), (2, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,L", DEVICE_SIZES)
def test_device_build_equals_the_model(pkg, n, L):
    scene = sh.create(pkg, _tri_scene(_small_tris(n)))
    tree = pkg.SceneTree.create(scene, L)
    try:
        m = _checked_build(pkg, scene, tree, f"n {n} L {L}", twice=True)
        depth = lm.check_invariants(m["nodes"], m["order"], m["keys"], scene.read(1), L, m["info"]["depth_bound"])
        print(f"n {n} L {L}: leaves {m['info']['n_leaves']} launches {m['info']['launches']} depth {depth} <= {m['info']['depth_bound']}")
    finally:
        tree.free(); scene.free()


@pytest.mark.gpu
@pytest.mark.parametrize("name,L", [("copies300", 1), ("copies300", 4), ("line4096", 4), ("zero_area257", 4)])
def test_device_build_on_degenerate_inputs(pkg, name, L):
    scene = sh.create(pkg, _tri_scene(sh.tri_set(name)))
    tree = pkg.SceneTree.create(scene, L)
    try:
        _checked_build(pkg, scene, tree, f"{name} L {L}", twice=True)
    finally:
        tree.free(); scene.free()


@pytest.mark.gpu
def test_device_build_on_boxes_that_are_not_finite(pkg):
    """svgf_scene_create refuses a vertex that is not finite; a pose table does not: object 0 NaN, object 1 inf, object 2 moved."""
    s = _tri_scene(_small_tris(301))
    table = pkg.binding.pose_identity(3)
    table[2] = pkg.binding.pose_rigid((0, 1, 0), 0.0, (0, 0, 0), (0.25, -0.125, 0.5))
    table["xf"][0], table["inv"][0] = np.nan, np.nan
    table["xf"][1], table["inv"][1] = np.inf, np.inf
    scene = sh.create(pkg, s)
    scene.enable_pose(3)
    tree = pkg.SceneTree.create(scene, 4)
    try:
        tree.attach()
        scene.pose(sh.dev(table))
        m = _checked_build(pkg, scene, tree, "NaN / inf boxes", twice=True)
        boxes = scene.read(1)
        assert np.isnan(boxes["lo"]).any(), "the input should hold NaN"
        lm.check_invariants(m["nodes"], m["order"], m["keys"], boxes, 4, m["info"]["depth_bound"])
        tree.detach()
    finally:
        tree.free(); scene.free()


# ---- GPU 2: the same frame, attached and detached -------------------------------------------------------------------------------------------
def _frame_input(name):
    if name in ("cornell", "room"):
        s, _, _ = sh.recorded(name, 0)
        return s, dict(centre=tuple(float(c) for c in s["light"]), edge_u=(0.4, 0.0, 0.0), edge_v=(0.0, 0.0, 0.4))
    return sh.edge(name)


def _four_draws(pkg, scene, s, lt, den):
    lt3 = dict(lt, samples=3)
    return dict(draw=sh.draw(pkg, sh.RESIDENT, scene, W0, H0, s, None),
                planar=sh.draw(pkg, sh.RESIDENT, scene, W0, H0, s, None, planes=den.planar_gbuffer()),
                shadowed=sh.draw(pkg, sh.SHADOWED, scene, W0, H0, s, lt3),
                traced=sh.draw(pkg, sh.TRACED, scene, W0, H0, s, lt3, sh.trace_args(1)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "B", "cornell", "room"])
def test_attached_tree_draws_the_same_frame_and_detach_restores(pkg, name):
    s, lt = _frame_input(name)
    scene = sh.create(pkg, s)
    den = pkg.Denoiser(W0, H0, 0)
    tree = pkg.SceneTree.create(scene, 4)
    try:
        own_info, own_view, own_nodes, own_order = scene.info(), scene.view(), scene.read(2), scene.read(4)
        own = _four_draws(pkg, scene, s, lt, den)
        m = _checked_build(pkg, scene, tree, name)
        tree.attach()
        info, view = scene.info(), scene.view()
        assert (info["n_nodes"], info["n_leaves"], info["depth"]) == (m["info"]["n_nodes"], m["info"]["n_leaves"], m["info"]["depth_bound"])
        assert view["nodes"] != own_view["nodes"] and view["order"] != own_view["order"] and view["n_nodes"] == m["info"]["n_nodes"]
        assert view["tri_boxes"] == own_view["tri_boxes"] and view["tris"] == own_view["tris"]
        lm.same_tree(scene.read(2), scene.read(4), None, m, f"{name}: svgf_scene_read kinds 2 / 4 on the adopted tree")
        got = _four_draws(pkg, scene, s, lt, den)
        for k in own:
            sh.same(got[k], own[k], f"{name} {k}: adopted tree vs the scene's own")
        tree.detach()
        assert scene.info() == own_info and scene.view() == own_view
        assert scene.read(2).tobytes() == own_nodes.tobytes() and scene.read(4).tobytes() == own_order.tobytes()
        sh.same(sh.draw(pkg, sh.RESIDENT, scene, W0, H0, s, None), own["draw"], f"{name}: after the detach")
    finally:
        tree.free(); den.free(); scene.free()


# ---- GPU 3: the posed block -----------------------------------------------------------------------------------------------------------------
def _posed_input():
    s = tsm._scene("A")                  # ids 10..17: 16 and 17 lie beyond a table of 16
    return s, 16


def _tables(pkg, s, n_obj):
    B = pkg.binding
    pivot = tuple(float(v) for v in np.asarray(s["tris"], F).reshape(-1, 8)[:, 0:3].mean(axis=0).astype(F))
    out = []
    for p in (B.pose_rigid((0, 1, 0), 0.0, (0, 0, 0), (0.25, -0.125, 0.5)), B.pose_rigid((0, 1, 0), np.deg2rad(9.0), pivot, (0.25, 0, 0)),
              B.pose_rigid((0.3, -0.5, 0.8), np.deg2rad(170.0), pivot, (0.125, 0.0625, -0.25))):
        t = B.pose_identity(n_obj)
        for k in range(n_obj):
            if k % 3 != 2:
                t[k] = p
        out.append(t)
    return out


@pytest.mark.gpu
def test_pose_build_draw_equals_pose_refit_draw(pkg):
    import torch
    s, n_obj = _posed_input()
    refit, built = sh.create(pkg, s), sh.create(pkg, s)
    refit.enable_pose(n_obj); built.enable_pose(n_obj)
    tree = pkg.SceneTree.create(built, 4)
    st = sh.open_stream(True)
    try:
        tree.attach()
        for k, t in enumerate(_tables(pkg, s, n_obj)):
            table = sh.dev(t)
            refit.pose(table)
            want = sh.draw(pkg, sh.RESIDENT, refit, W0, H0, s, None)
            built.pose(table)
            _checked_build(pkg, built, tree, f"pose {k}")
            assert built.read(1).tobytes() == refit.read(1).tobytes(), "the two scenes should hold the same posed boxes"
            sh.same(sh.draw(pkg, sh.RESIDENT, built, W0, H0, s, None), want, f"pose {k}: pose, build, draw vs pose (refit), draw")
        # a pose on an adopted tree is the pose kernel alone; on the scene's own tree it refits too
        table = sh.dev(_tables(pkg, s, n_obj)[0])
        torch.cuda.synchronize()
        adopted = sh.Captured(st, lambda: built.pose(table, stream=st))
        own = sh.Captured(st, lambda: refit.pose(table, stream=st))
        types = (adopted.types, own.types)
        adopted.destroy(); own.destroy()
        print(f"captured pose: adopted tree {types[0]}, own tree {types[1]}")
        assert types[0] == [0] and len(types[1]) > 1 and all(t == 0 for t in types[1])
        # after a detach the next pose refits the scene's own nodes from the posed boxes as before
        tree.detach()
        t = _tables(pkg, s, n_obj)[2]
        built.pose(sh.dev(t)); refit.pose(sh.dev(t))
        torch.cuda.synchronize()
        assert built.read(2).tobytes() == refit.read(2).tobytes(), "own nodes after detach + pose"
        sh.same(sh.draw(pkg, sh.RESIDENT, built, W0, H0, s, None), sh.draw(pkg, sh.RESIDENT, refit, W0, H0, s, None), "after detach + pose")
    finally:
        st.close()
        tree.free(); refit.free(); built.free()


# ---- GPU 4: capture ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n,L", [(2051, 4), (1, 4)])
def test_a_captured_build_is_launches_kernel_nodes(pkg, n, L):
    scene = sh.create(pkg, _tri_scene(_small_tris(n)))
    tree = pkg.SceneTree.create(scene, L)
    st = sh.open_stream(True)
    try:
        m = _checked_build(pkg, scene, tree, f"eager n {n}", stream=st.cuda_stream)
        want = [tree.read(k) for k in (0, 1, 2)]
        graph = sh.Captured(st, lambda: tree.build(st.cuda_stream))
        types = graph.types
        graph.launch(); graph.launch()
        st.synchronize()
        got = [tree.read(k) for k in (0, 1, 2)]
        graph.destroy()
        print(f"n {n}: captured build = {len(types)} nodes, info.launches {m['info']['launches']}")
        assert len(types) == tree.info()["launches"] == m["info"]["launches"] and all(t == 0 for t in types), types
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)), "a replayed build gives other bytes"
    finally:
        st.close()
        tree.free(); scene.free()


@pytest.mark.gpu
def test_a_captured_pose_build_draw_replays_with_the_table_of_the_moment(pkg):
    import torch
    s, n_obj = _posed_input()
    scene = sh.create(pkg, s)
    scene.enable_pose(n_obj)
    tree = pkg.SceneTree.create(scene, 4)
    st = sh.open_stream(True)
    try:
        tree.attach()
        t1, t2 = _tables(pkg, s, n_obj)[1:3]
        table = sh.dev(t1)
        rgb, gbt = sh.buffers(W0, H0)
        want = []
        for t in (t1, t2):                                               # the ordered calls, the tree checked before each draw
            with torch.cuda.stream(st.torch):
                table.copy_(sh.dev(t))
            scene.pose(table, stream=st.cuda_stream)
            _checked_build(pkg, scene, tree, "ordered calls", stream=st.cuda_stream)
            scene.draw(rgb, gbt, W0, H0, s["cam"], s["light"], FRAME, seed=SEED, stream=st.cuda_stream)
            st.synchronize()
            want.append(sh.host(pkg, rgb, gbt, W0, H0))
        torch.cuda.synchronize()

        def record():
            scene.pose(table, stream=st.cuda_stream)
            tree.build(st.cuda_stream)
            scene.draw(rgb, gbt, W0, H0, s["cam"], s["light"], FRAME, seed=SEED, stream=st.cuda_stream)
        graph = sh.Captured(st, record)
        assert len(graph.types) == 2 + tree.info()["launches"] and all(t == 0 for t in graph.types), graph.types
        for k, t in enumerate((t1, t2)):
            with torch.cuda.stream(st.torch):
                table.copy_(sh.dev(t)); rgb.zero_(); gbt.zero_()
            graph.launch()
            st.synchronize()
            sh.same(sh.host(pkg, rgb, gbt, W0, H0), want[k], f"replay {k} vs the ordered calls")
        graph.destroy()
        tree.detach()
    finally:
        st.close()
        tree.free(); scene.free()


# ---- GPU 5: errors with a device present --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_errors_with_a_device(pkg):
    import torch
    lib, lb = pkg.load_library(), pkg.load_lbvh_library()
    s = _tri_scene(_small_tris(11))
    scene, other = sh.create(pkg, s), sh.create(pkg, s)
    empty = pkg.Scene.create(tsm._scene("E_plus")["geoms"], None, None, None, None)
    tree = pkg.SceneTree.create(scene, 4)
    try:
        m = _checked_build(pkg, scene, tree, "11 triangles")
        own = sh.draw(pkg, sh.RESIDENT, scene, W0, H0, s, None)
        h = ctypes.c_void_p(77)
        assert lb.svgf_lbvh_create(empty.h, None, ctypes.byref(h)) == ERR and not h.value, "a scene without triangles"
        for L in (-1, 9):
            assert lb.svgf_lbvh_create(scene.h, ctypes.byref(pkg.SvgfLbvhParams(L)), ctypes.byref(h)) == ERR
        assert lb.svgf_lbvh_create(scene.h, None, None) == ERR
        assert lb.svgf_lbvh_attach(tree.h, other.h) == ERR and lb.svgf_lbvh_attach(tree.h, None) == ERR
        buf = np.zeros(32 * m["info"]["n_nodes"] + 8, np.uint8)
        assert lb.svgf_lbvh_read(tree.h, 3, buf.ctypes.data, 32 * m["info"]["n_nodes"]) == ERR and lb.svgf_lbvh_read(tree.h, -1, buf.ctypes.data, 4) == ERR
        assert lb.svgf_lbvh_read(tree.h, 0, buf.ctypes.data, 32 * m["info"]["n_nodes"] + 8) == ERR and lb.svgf_lbvh_read(tree.h, 0, None, 32 * m["info"]["n_nodes"]) == ERR
        assert lb.svgf_lbvh_info(tree.h, None) == ERR
        nodes, order = torch.zeros(32 * 5 + 16, dtype=torch.uint8, device="cuda"), torch.zeros(64, dtype=torch.uint8, device="cuda")
        N, O = nodes.data_ptr(), order.data_ptr()
        assert N % 16 == 0 and O % 16 == 0
        before = (scene.info(), scene.view())
        for bad in ((N, O, 5, 4, 3), (N, O, 5, 3, 49), (N, O, 5, 3, -1), (N, O, 1, 0, 0), (N, O, 23, 12, 3), (N + 4, O, 5, 3, 3), (N, O + 4, 5, 3, 3),
                    (N, None, 5, 3, 3)):
            assert lib.svgf_scene_adopt_tree(scene.h, *bad) == ERR, bad
        assert lib.svgf_scene_adopt_tree(empty.h, N, O, 1, 1, 0) == ERR and lib.svgf_scene_adopt_tree(empty.h, None, None, 0, 0, 0) == ERR
        assert (scene.info(), scene.view()) == before, "a refused adoption touches the scene"
        sh.same(sh.draw(pkg, sh.RESIDENT, scene, W0, H0, s, None), own, "after the refusals")
    finally:
        tree.free(); scene.free(); other.free(); empty.free()
