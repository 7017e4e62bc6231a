"""Row f25: the device SAH build (include/svgf_sah.h, libsvgf_sah.so) - svgf_bvh_build_host's tree over the triangles as drawn.

CPU: tests/sah_model.py restates the header's normative text sequentially in numpy; the model and the relaid host tree
(sah_model.relayout of svgf_bvh_build_host's nodes) are held to each other - order, first, count on bits, boxes by value - and to the
invariants of the sparse layout on every case, the chain set (on which the depth rule acts) among them; the library's exports and
NEEDED entries; every refusal that needs no device.

GPU: svgf_sah_build against the model (the relaid host tree at the two largest sizes) on every byte, padding included, across the
seams of the kernel plan (SVGF_SAH_SMALL triangles: the small-subtree limit); posed scenes; a pose table that is not finite; the frame with the
tree attached against the scene's own on every bit; capture; errors.  In every GPU test the tree is read back and compared BEFORE a
draw walks it: a wrong tree fails a comparison and never reaches the walk.
"""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import resident_scene_model as rm
import sah_model as sm
import scene_harness as sh
import test_scene_model as tsm
from conftest import ROOT
from test_scene_model import FRAME, SEED

F = np.float32
W0, H0 = 67, 41
ERR = -1                # SVGF_ERR_INVALID_ARG
SMALL = sm.SMALL


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _random_tris(n, seed=25):
    rng = np.random.default_rng(seed + n)
    c = rng.uniform(-2, 2, (n, 1, 3)).astype(F)
    t = np.zeros((n, 3, 8), F)
    t[:, :, 0:3] = c + rng.uniform(-0.05, 0.05, (n, 3, 3)).astype(F)
    return t


@functools.lru_cache(maxsize=None)
def _tris(name):
    if name[0] == "n" and name[1:].isdigit():
        return _random_tris(int(name[1:]))
    if name == "coincident4096":
        return np.repeat(sh.tri_set("one"), 4096, axis=0)
    if name == "two_clusters":
        t = _random_tris(600, 5).copy()
        t[300:, :, 0] += F(1e6)
        return t
    if name == "chain":
        return sm.chain_set()
    return sh.tri_set(name)


CPU_CASES = [(f"n{n}", L) for L in (1, 4, 8) for n in sorted({1, 2, 3, L, L + 1})] + \
    [("copies300", 1), ("copies300", 4), ("line4096", 4), ("zero_area257", 4), ("two_clusters", 4), ("room", 4), ("bunny", 4), ("cornell", 4),
     ("chain", 1), ("chain", 4)]


@functools.lru_cache(maxsize=None)
def _model(name, L):
    t = _tris(name)
    return sm.build(t, rm.padded_boxes(t), L)


def _host(pkg, tris, L):
    nodes, order, depth = pkg.bvh_build_host(tris, L, 0)
    return sm.relayout(nodes, len(order)), order, depth, len(nodes)


# ---- CPU 1: the model is the relaid host tree --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,L", CPU_CASES)
def test_model_equals_the_relaid_host_tree(pkg, name, L):
    t, m = _tris(name), _model(name, L)
    rec, order, depth, n_nodes = _host(pkg, t, L)
    sm.same_tree(rec, order, m["records"], m["order"], f"{name} L {L}: host builder vs model")
    got = sm.check_invariants(m["records"], m["order"], rm.padded_boxes(t), L, m["info"]["depth_bound"])
    c = m["counts"]
    print(f"{name} L {L}: n {len(t)} nodes {c['n_nodes']} leaves {c['n_leaves']} depth {c['depth']} forced {c['forced_splits']}")
    assert got == {k: c[k] for k in got} and (c["n_nodes"], c["depth"]) == (n_nodes, depth)
    assert c["n_nodes"] == 2 * c["n_leaves"] - 1
    if name == "chain":
        assert c["depth"] == 48 and c["forced_splits"] >= 1, "the chain set no longer reaches the depth rule"


def test_layout_rule(pkg):
    """Collision-free (relayout asserts it per split), L = 1 leaves no padding, the capacity is what svgf_scene_adopt_tree checks."""
    for name, L in (("n257", 1), ("n257", 4), ("zero_area257", 1)):
        t = _tris(name)
        rec, order, _, n_nodes = _host(pkg, t, L)
        owned = (rec["count"] > 0) | (rec["first"] > 0)
        owned[0] = True
        assert int(owned.sum()) == n_nodes and len(rec) == 2 * len(t) - 1
        assert (L != 1) or owned.all()
        inner = rec["first"][owned & (rec["count"] == 0)]
        assert len(set(inner.tolist())) == len(inner) and np.all(inner % 2 == 1)
    assert SMALL == pkg.sah.SAH_SMALL == 256
    assert sm.info_of(256, 0)["launches"] == 2 and sm.info_of(257, 4)["launches"] == 2 + 5 * 5 and sm.info_of(1 << 20, 4)["launches"] == 2 + 5 * 16
    assert sm.info_of(1, 4)["depth_bound"] == 0 and sm.info_of(40, 4)["depth_bound"] == 39 and sm.info_of(4097, 4)["depth_bound"] == 48


# ---- CPU 2: the library's surface ----------------------------------------------------------------------------------------------------------
def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return sorted(ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("svgf_"))


def test_exports_and_links(pkg):
    bld = pkg.build
    path = bld.build_sah()
    assert os.path.basename(path) == "libsvgf_sah.so" and path == pkg.binding.companion_path("sah")
    header = open(os.path.join(ROOT, "include", "svgf_sah.h")).read()
    declared = sorted(set(re.findall(r"^\s*(?:int|void)\s+(svgf_sah_\w+)\(", header, re.M)))
    assert declared == sorted(pkg.sah.SAH_EXPORTS) == _exports(path)
    out = subprocess.run(["readelf", "-d", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    needed = sorted(ln.split("[")[1].split("]")[0] for ln in out.splitlines() if "(NEEDED)" in ln and "[libsvgf_" in ln)
    assert needed == ["libsvgf_hip.so"], needed
    undefined = subprocess.run(["nm", "-D", "--undefined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "getenv" not in undefined
    wanted = {ln.split()[-1] for ln in undefined.splitlines() if ln.split() and ln.split()[-1].startswith("svgf_")}
    assert wanted == {"svgf_scene_view", "svgf_scene_adopt_tree"}, wanted
    assert [b.name for b in bld.TREE_BUILDERS] == ["sah"] and "-ffp-contract=off" in bld.TREE_BUILDERS[0].flags
    assert path not in bld.build_all()
    assert pkg.SahTree is pkg.sah.SahTree and ctypes.sizeof(pkg.sah.SvgfSahInfo) == 32 and ctypes.sizeof(pkg.sah.SvgfSahCounts) == 16


# ---- CPU 3: refusals that need no device ---------------------------------------------------------------------------------------------------
def test_refusals_without_a_device(pkg):
    lib, ls = pkg.load_library(), pkg.load_sah_library()
    buf = np.zeros(64, np.uint8)
    h = ctypes.c_void_p(77)
    assert ls.svgf_sah_create(None, None, ctypes.byref(h)) == ERR and not h.value, "a refused create clears *out"
    for L in (-1, 9):
        assert ls.svgf_sah_create(None, ctypes.byref(pkg.SvgfSahParams(L)), ctypes.byref(h)) == ERR
    assert ls.svgf_sah_create(None, None, None) == ERR
    assert ls.svgf_sah_build(None, None) == ERR
    assert ls.svgf_sah_attach(None, None) == ERR
    assert ls.svgf_sah_info(None, ctypes.byref(pkg.SvgfSahInfo())) == ERR
    assert ls.svgf_sah_read(None, 0, buf.ctypes.data, 32) == ERR
    ls.svgf_sah_destroy(None)
    assert ls.svgf_sah_version() == lib.svgf_version()


# ---- GPU helpers ----------------------------------------------------------------------------------------------------------------------------
def _tri_scene(tris, n_obj=3):
    n = len(tris)
    return dict(cam=tsm._scene("A")["cam"], geoms=None, geom_ids=None, tris=tris, tri_ids=(np.arange(n) % n_obj).astype(np.int32),
                tri_albedo=tsm._colours(n, 15), tri_tex=None, textures=None, light=(1.0, 3.0, 4.0))


def _read(tree):
    return [tree.read(k) for k in (0, 1, 2)]


def _checked_build(pkg, scene, tree, what, stream=None, twice=False, host=False, model=None):
    """build, read back, hold to the model (or the relaid host tree) of the scene's triangles as drawn on every byte; returns the
    expected tree.  Nothing walks the tree in here."""
    import torch
    tree.build(stream)
    torch.cuda.synchronize()
    tris, boxes, info = scene.read(0), scene.read(1), tree.info()
    L = info["max_leaf_tris"]
    assert info == dict(sm.info_of(len(tris), L), device_bytes=info["device_bytes"]), what
    got = _read(tree)
    if host:
        rec, order, depth, n_nodes = _host(pkg, tris, L)
        m = dict(records=rec, order=order, counts=dict(n_nodes=n_nodes, n_leaves=(n_nodes + 1) // 2, depth=depth, forced_splits=int(got[2][3])))
        assert np.array_equal(np.stack([boxes["lo"], boxes["hi"]]), np.stack(rm.padded_boxes(tris))), "the boxes as drawn are the host builder's"
    else:
        m = model or sm.build(tris, boxes, L)
    sm.same_tree(got[0], got[1], m["records"], m["order"], what, bytes_too=True)
    assert dict(zip(("n_nodes", "n_leaves", "depth", "forced_splits"), got[2].tolist())) == m["counts"] == tree.counts(), what
    if twice:
        tree.build(stream)
        torch.cuda.synchronize()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, _read(tree))), f"{what}: a second build gives other bytes"
    return m


def _fill_state(scene, tree, byte):
    """Every byte a build touches set to `byte`: the records stand at the start of the tree's one allocation (svgf_sah.h), and an
    attached scene hands their address out."""
    import torch
    from temporal_harness import _hip
    tree.attach()
    base = scene.view()["nodes"]
    tree.detach()
    hip = _hip()
    hip.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
    torch.cuda.synchronize()
    assert hip.hipMemset(base, byte, tree.info()["device_bytes"]) == 0
    torch.cuda.synchronize()


# ---- GPU 1: the device build equals the model on every byte ----------------------------------------------------------------------------------
# SMALL - 1 / SMALL / SMALL + 1: the small-subtree limit (one wave in LDS; SMALL + 1 is the smallest tree with a large-node round);
# 2 SMALL + 1: two blocks of positions and a third's first; 4097 and 65537: many slots per round, against the relaid host tree
DEVICE_SIZES = [(n, L) for L in (1, 4, 8) for n in sorted({1, 2, 3, L, L + 1, SMALL - 1, SMALL, SMALL + 1, 2 * SMALL + 1})] + \
    [(n, L) for n in (4097, 65537) for L in (1, 4, 8)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,L", DEVICE_SIZES)
def test_device_build_equals_the_model(pkg, n, L):
    scene = sh.create(pkg, _tri_scene(_random_tris(n)))
    tree = pkg.SahTree(scene, L)
    try:
        m = _checked_build(pkg, scene, tree, f"n {n} L {L}", twice=True, host=n > 2 * SMALL + 1)
        print(f"n {n} L {L}: launches {tree.info()['launches']} counts {m['counts']}")
        if n in (SMALL + 1, 4097):
            want = _read(tree)
            _fill_state(scene, tree, 0xFF)
            tree.build()
            assert all(a.tobytes() == b.tobytes() for a, b in zip(want, _read(tree))), "a build over a state of 0xFF bytes gives other bytes"
    finally:
        tree.free(); scene.free()


@pytest.mark.gpu
@pytest.mark.parametrize("name,L", [("coincident4096", 1), ("coincident4096", 4), ("line4096", 4), ("zero_area257", 4), ("two_clusters", 4), ("chain", 1),
                                    ("chain", 4), ("room", 4), ("bunny", 4)])
def test_device_build_on_named_inputs(pkg, name, L):
    scene = sh.create(pkg, _tri_scene(_tris(name)))
    tree = pkg.SahTree(scene, L)
    try:
        big = name in ("coincident4096", "line4096", "bunny")
        m = _checked_build(pkg, scene, tree, f"{name} L {L}", twice=True, host=big, model=None if big or name != "chain" else _model(name, L))
        print(f"{name} L {L}: counts {tree.counts()}")
        if name == "chain":
            assert m["counts"]["depth"] == 48 and m["counts"]["forced_splits"] >= 1
    finally:
        tree.free(); scene.free()


# ---- GPU 2: posed scenes -------------------------------------------------------------------------------------------------------------------
def _posed_input():
    return tsm._scene("A"), 16              # ids 10..17: 16 and 17 lie beyond a table of 16


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
    s, n_obj = _posed_input()
    refit, built = sh.create(pkg, s), sh.create(pkg, s)
    refit.enable_pose(n_obj); built.enable_pose(n_obj)
    tree = pkg.SahTree(built, 4)
    try:
        tree.attach()
        for k, t in enumerate(_tables(pkg, s, n_obj)):
            table = sh.dev(t)
            refit.pose(table)
            want = sh.draw(pkg, sh.RESIDENT, refit, W0, H0, s, None)
            built.pose(table)
            _checked_build(pkg, built, tree, f"pose {k}")                   # the model of the triangles as drawn (svgf_scene_read kind 0)
            assert built.read(0).tobytes() == refit.read(0).tobytes(), "the two scenes should hold the same posed triangles"
            sh.same(sh.draw(pkg, sh.RESIDENT, built, W0, H0, s, None), want, f"pose {k}: pose, build, draw vs pose (refit), draw")
        tree.detach()
    finally:
        tree.free(); refit.free(); built.free()


@pytest.mark.gpu
def test_device_build_on_vertices_that_are_not_finite(pkg):
    """svgf_scene_create refuses a vertex that is not finite; a pose table does not: object 0 NaN, object 1 inf, object 2 moved.  The
    tree is held to the invariants alone, and never attached or drawn."""
    import torch
    s = _tri_scene(_random_tris(601))
    table = pkg.binding.pose_identity(3)
    table[2] = pkg.binding.pose_rigid((0, 1, 0), 0.0, (0, 0, 0), (0.25, -0.125, 0.5))
    table["xf"][0], table["inv"][0] = np.nan, np.nan
    table["xf"][1], table["inv"][1] = np.inf, np.inf
    scene = sh.create(pkg, s)
    scene.enable_pose(3)
    tree = pkg.SahTree(scene, 4)
    try:
        scene.pose(sh.dev(table))
        tree.build()
        torch.cuda.synchronize()
        boxes = scene.read(1)
        assert not np.isfinite(scene.read(0)[:, :, 0:3]).all(), "the input should hold vertices that are not finite"
        got = _read(tree)
        found = sm.check_invariants(got[0], got[1], boxes, 4, tree.info()["depth_bound"])
        c = tree.counts()
        print(f"NaN / inf vertices: counts {c}")
        assert found == {k: c[k] for k in found} and c["depth"] <= 48
        tree.build()
        torch.cuda.synchronize()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, _read(tree))), "a second build gives other bytes"
    finally:
        tree.free(); scene.free()


# ---- GPU 3: the same frame, attached and detached -------------------------------------------------------------------------------------------
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
    tree = pkg.SahTree(scene, 4)
    try:
        own_info, own_view, own_nodes, own_order = scene.info(), scene.view(), scene.read(2), scene.read(4)
        own = _four_draws(pkg, scene, s, lt, den)
        m = _checked_build(pkg, scene, tree, name)
        sm.same_tree(m["records"], m["order"], sm.relayout(own_nodes, len(own_order)), own_order, f"{name}: the scene's own tree, relaid")
        tree.attach()
        info, view, n = scene.info(), scene.view(), len(own_order)
        assert (info["n_nodes"], info["n_leaves"], info["depth"]) == (2 * n - 1, n, min(48, n - 1)), "the scene is handed the capacity"
        assert view["nodes"] != own_view["nodes"] and view["order"] != own_view["order"] and view["n_nodes"] == 2 * n - 1
        assert view["tri_boxes"] == own_view["tri_boxes"] and view["tris"] == own_view["tris"]
        sm.same_tree(scene.read(2), scene.read(4), m["records"], m["order"], f"{name}: svgf_scene_read kinds 2 / 4 on the adopted tree", bytes_too=True)
        got = _four_draws(pkg, scene, s, lt, den)
        for k in own:
            sh.same(got[k], own[k], f"{name} {k}: adopted tree vs the scene's own")
        tree.detach()
        assert scene.info() == own_info and scene.view() == own_view
        assert scene.read(2).tobytes() == own_nodes.tobytes() and scene.read(4).tobytes() == own_order.tobytes()
        sh.same(sh.draw(pkg, sh.RESIDENT, scene, W0, H0, s, None), own["draw"], f"{name}: after the detach")
    finally:
        tree.free(); den.free(); scene.free()


# ---- GPU 4: capture ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n,L", [(2051, 4), (1, 4)])
def test_a_captured_build_is_launches_kernel_nodes(pkg, n, L):
    scene = sh.create(pkg, _tri_scene(_random_tris(n)))
    tree = pkg.SahTree(scene, L)
    st = sh.open_stream(True)
    try:
        _checked_build(pkg, scene, tree, f"eager n {n}", stream=st.cuda_stream, host=True)
        want = _read(tree)
        graph = sh.Captured(st, lambda: tree.build(st.cuda_stream))
        types = graph.types
        graph.launch(); graph.launch()
        st.synchronize()
        got = _read(tree)
        graph.destroy()
        print(f"n {n}: captured build = {len(types)} nodes, info.launches {tree.info()['launches']}")
        assert len(types) == tree.info()["launches"] == sm.info_of(n, L)["launches"] and all(t == 0 for t in types), types
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
    tree = pkg.SahTree(scene, 4)
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
    ls = pkg.load_sah_library()
    s = _tri_scene(_random_tris(11))
    scene, other = sh.create(pkg, s), sh.create(pkg, s)
    empty = pkg.Scene.create(tsm._scene("E_plus")["geoms"], None, None, None, None)
    tree = pkg.SahTree(scene, 4)
    try:
        _checked_build(pkg, scene, tree, "11 triangles")
        h = ctypes.c_void_p(77)
        assert ls.svgf_sah_create(empty.h, None, ctypes.byref(h)) == ERR and not h.value, "a scene without triangles"
        for L in (-1, 9):
            assert ls.svgf_sah_create(scene.h, ctypes.byref(pkg.SvgfSahParams(L)), ctypes.byref(h)) == ERR
        assert ls.svgf_sah_create(scene.h, None, None) == ERR
        assert ls.svgf_sah_attach(tree.h, other.h) == ERR and ls.svgf_sah_attach(tree.h, None) == ERR
        buf = np.zeros(32 * 21 + 8, np.uint8)
        assert ls.svgf_sah_read(tree.h, 3, buf.ctypes.data, 32 * 21) == ERR and ls.svgf_sah_read(tree.h, -1, buf.ctypes.data, 4) == ERR
        assert ls.svgf_sah_read(tree.h, 0, buf.ctypes.data, 32 * 21 + 8) == ERR and ls.svgf_sah_read(tree.h, 0, None, 32 * 21) == ERR
        assert ls.svgf_sah_read(tree.h, 1, buf.ctypes.data, 40) == ERR and ls.svgf_sah_read(tree.h, 2, buf.ctypes.data, 32) == ERR
        assert ls.svgf_sah_read(tree.h, 0, buf.ctypes.data, 32 * 21) == 0 and ls.svgf_sah_read(tree.h, 2, buf.ctypes.data, 16) == 0
        assert ls.svgf_sah_info(tree.h, None) == ERR
        with pkg.SahTree(scene) as default:
            assert default.info()["max_leaf_tris"] == 4
    finally:
        tree.free(); scene.free(); other.free(); empty.free()
