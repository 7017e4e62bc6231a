"""The scene producer (csrc/svgf_scene.hip, k_scene_frame) against tests/scene_model.py, an operation-for-operation float32 model of
all of its branches: triangles, the two corner-weight orders, textures with both clamps and the descriptor offsets, `geom_ids`,
NaN normals, rays parallel to a slab from a camera in a face plane, cameras inside a primitive, rotated / non-uniformly scaled
primitives, and the reference's own scenes.

CPU part: the model equals scene.render_scene where there are no triangles, is consistent with the G-buffers the reference's path
tracer recorded, and every edge scene ACTS: the model and a named wrong variant of it differ on more pixels than a GPU test may
leave out (`cap`), so no edge can hide in that allowance.
GPU part: svgf_scene_render_mesh equals the model on the bits of geomId, normal, position, albedo, ialbedo and colour (NaNs in the
same place count as equal).  The kernel has no transcendental call, division and sqrtf are correctly rounded and contraction is
off, so the expected number of differing pixels is 0; the allowance is test_scene.py's, cap = max(2, W*H // 20000) per field.
"""
import functools
import os

import numpy as np
import pytest

import scene_model as sm
from conftest import ROOT

F = np.float32
SCENE = os.path.join(ROOT, "tests", "golden", "scenes", "box_room.txt")
REF_DIR = os.path.join(ROOT, "tests", "golden", "ref_scenes")
FIELDS = ("geomId", "normal", "position", "albedo", "ialbedo")
SIZES = [(67, 41), (1, 1)]          # 67x41: eleven 256-thread blocks, the last one partial


def cap(W, H):
    return max(2, W * H // 20000)


def differing(a, b):
    """[H, W] mask of the pixels on which two planes differ in bits; NaNs in the same place are equal."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    if a.dtype.kind != "f":
        bad = a != b
    else:
        na, nb = np.isnan(a), np.isnan(b)
        bad = (na != nb) | (~na & ~nb & (a.view(np.uint32) != b.view(np.uint32)))
    return bad.reshape(bad.shape[0], bad.shape[1], -1).any(axis=-1)


def counts(got, ref):
    """Per field and for the colour: how many pixels differ.  got / ref = (color, gbuffer)."""
    out = {f: int(np.count_nonzero(differing(got[1][f], ref[1][f]))) for f in FIELDS}
    out["color"] = int(np.count_nonzero(differing(got[0], ref[0])))
    return out


def any_differs(got, ref):
    bad = differing(got[0], ref[0])
    for f in FIELDS:
        bad |= differing(got[1][f], ref[1][f])
    return int(np.count_nonzero(bad))


# ---- the edge scenes, built from arrays -------------------------------------------------------------------------------------------------
def _cam(pkg, eye, look, fovy=45.0):
    sc = pkg.scene.Scene(materials={}, objects=[], camera=dict(eye=eye, lookat=look, fovy=fovy), skipped=[])
    return pkg.scene.camera_for_frame(sc, 0, False)


def _geoms(pkg, *recs):
    """recs: (type, trans, rotat, scale, albedo, emittance)"""
    out = np.zeros(len(recs), dtype=pkg.scene.SCENE_GEOM_DTYPE)
    for g, (kind, trans, rotat, scale, albedo, emit) in zip(out, recs):
        xf, inv, invT = pkg.scene._transform(trans, rotat, scale)
        g["type"], g["material"], g["albedo"], g["emittance"] = kind, 0, np.array(albedo, F), F(emit)
        g["xf"], g["inv"], g["invT"] = xf.reshape(-1), inv.reshape(-1), invT.reshape(-1)
    return out


_NRM = np.array([[0.3, 0.1, 1.0], [-0.2, 0.4, 0.9], [0.1, -0.3, 0.8]], F)       # one normal per corner, none of unit length
_UV = np.array([[0.1, 0.2], [0.9, 0.3], [0.4, 0.8]], F)


def _tri(p0, p1, p2, nrm=_NRM, uv=_UV, k=0):
    """float32[3, 8]: pos, normal, uv per corner; k varies the normals from triangle to triangle."""
    t = np.zeros((3, 8), F)
    t[:, 0:3] = np.array([p0, p1, p2], F)
    t[:, 3:6] = np.asarray(nrm, F) * F(1.0 + 0.25 * k) if np.any(nrm) else 0
    t[:, 6:8] = np.asarray(uv, F)
    return t


def _unit(pkg):
    """Distance between neighbouring pixel centres of the 67x41 frame in the plane 5 in front of the camera: vertices at whole
    multiples of it fall on pixel centres, so shared edges and corners are hit with bx == 0, by == 0 and bx + by == 1."""
    return F(5) * pkg.synth._pixel_length(67, 41, 45.0)[0]


def _colours(n, seed):
    return np.random.default_rng(seed).uniform(0.2, 0.95, size=(n, 3)).astype(F)


def _scene_A(pkg):
    """Triangles only.  A fan of four around the frame's centre (shared edges along the centre row and column, a hypotenuse through
    pixel centres), a back-facing triangle in front of it (culled), a triangle stored twice with two ids and a third one that
    overlaps both in their plane (the first of equals wins)."""
    u = _unit(pkg)
    P = lambda x, y, z=0.0: (F(x) * u, F(y) * u, F(z))      # noqa: E731
    C, R0, R1, R2, R3 = P(0, 0), P(16, 0), P(0, 12), P(-16, 0), P(0, -12)
    dup = (P(18, -18, -1), P(32, -18, -1), P(18, 18, -1))
    tris = [_tri(C, R0, R1, k=0), _tri(C, R1, R2, k=1), _tri(C, R2, R3, k=2), _tri(C, R3, R0, k=3),
            _tri(P(-8, -6, 1), P(0, 8, 1), P(8, -6, 1), k=4),                                # clockwise: culled
            _tri(*dup, k=5), _tri(*dup, k=6), _tri(P(14, -10, -1), P(30, 0, -1), P(14, 10, -1), k=7),
            _tri(P(-30, -15, 0.5), P(-18, -15, -0.5), P(-24, 15, 0.0), k=8)]
    return dict(cam=_cam(pkg, (0, 0, 5), (0, 0, 0)), geoms=_geoms(pkg), geom_ids=None, tris=np.stack(tris),
                tri_ids=np.array([10, 11, 10, 12, 13, 14, 15, 16, 17], np.int32), tri_albedo=_colours(9, 1), tri_tex=None, textures=None,
                light=(1.0, 3.0, 4.0), alts=("tri_le", "no_cull", "normal_uv_weights", "tri_albedo_shift"))


def _scene_B(pkg):
    """Triangles and primitives: a triangle in front of a cube, one behind it that shows around it, one in the plane of the cube's
    front face (the primitive keeps a tie), geom_ids that are not the identity and share the value 7 with a triangle."""
    geoms = _geoms(pkg, (0, (0, 0, 0), (0, 0, 0), (2, 2, 2), (0.8, 0.3, 0.2), 0.0), (1, (2.5, 1.2, 0), (0, 0, 0), (1.5, 1.5, 1.5), (0.2, 0.7, 0.9), 0.0))
    tris = [_tri((-0.75, -0.5, 2), (0.25, -0.5, 2), (-0.75, 0.5, 2), k=0), _tri((-3, -2, -3), (3, -2, -3), (0, 3, -3), k=1),
            _tri((0.25, -0.5, 1), (1.5, -0.5, 1), (0.25, 0.875, 1), k=2)]
    return dict(cam=_cam(pkg, (0, 0, 5), (0, 0, 0), 22.5), geoms=geoms, geom_ids=np.array([7, 3], np.int32), tris=np.stack(tris),
                tri_ids=np.array([5, 7, 9], np.int32), tri_albedo=_colours(3, 2), tri_tex=None, textures=None, light=(-2.0, 4.0, 5.0),
                alts=("tri_le", "geom_ids_identity", "tri_from_inf"))


def _scene_C(pkg):
    """Textures: 5x3, then 8x4 at byte offset 45.  The left quad runs uv over [-0.5, 1.5]^2 (every clamp of X and Y), the right
    quad has corners at exactly 0 and 1 and one pair beyond, a strip above carries tri_tex == -1."""
    u = _unit(pkg)
    P = lambda x, y: (F(x) * u, F(y) * u, F(0))              # noqa: E731
    rng = np.random.default_rng(3)
    textures = [rng.permutation(256)[:45].astype(np.uint8).reshape(3, 5, 3), rng.permutation(256)[:96].astype(np.uint8).reshape(4, 8, 3)]
    a, b, c, d = P(-30, -16), P(-2, -16), P(-2, 16), P(-30, 16)
    ua, ub, uc, ud = (-0.5, -0.5), (1.5, -0.5), (1.5, 1.5), (-0.5, 1.5)
    e, f, g, h = P(2, -16), P(30, -16), P(30, 16), P(2, 16)
    tris = [_tri(a, b, c, uv=(ua, ub, uc), k=0), _tri(a, c, d, uv=(ua, uc, ud), k=1),
            _tri(e, f, g, uv=((0, 0), (1, 0), (1, 1)), k=2), _tri(e, g, h, uv=((0, 0), (1.25, 1), (-0.25, 1)), k=3),
            _tri(P(-20, 17), P(20, 17), P(0, 20), k=4)]
    return dict(cam=_cam(pkg, (0, 0, 5), (0, 0, 0)), geoms=_geoms(pkg), geom_ids=None, tris=np.stack(tris),
                tri_ids=np.array([1, 1, 2, 2, 3], np.int32), tri_albedo=_colours(5, 4), tri_tex=np.array([0, 0, 1, 1, -1], np.int32),
                textures=textures, light=(0.0, 2.0, 6.0),
                alts=("uv_normal_weights", "tex_x_shift", "tex_y_shift", "no_clamp_low", "no_clamp_high", "tex_ignore", "tex_swap"))


def _scene_D(pkg):
    """A mesh without normals (mesh.scene_triangles writes zeros): the normal is 0/0 = NaN, the Lambert term's fmaxf turns its NaN into
    0 and the colour is the ambient term.  One triangle with normals and a cube stand beside it."""
    zero = np.zeros((3, 3), F)
    tris = [_tri((-2, -1.5, 0), (0.5, -1.5, 0), (-2, 1.5, 0), nrm=zero), _tri((0.5, -1.5, 0), (0.5, 1.5, 0.5), (-2, 1.5, 0), nrm=zero),
            _tri((0.75, -1, 0), (2.25, -1, 0), (0.75, 1, 0), k=1)]
    geoms = _geoms(pkg, (0, (0, 0, -2), (0, 0, 0), (6, 1, 1), (0.5, 0.5, 0.5), 0.0))
    return dict(cam=_cam(pkg, (0, 0, 5), (0, 0, 0), 22.5), geoms=geoms, geom_ids=None, tris=np.stack(tris), tri_ids=np.array([4, 4, 5], np.int32),
                tri_albedo=_colours(3, 5), tri_tex=None, textures=None, light=(1.0, 2.0, 5.0), alts=("lam_nan",))


def _scene_E(pkg, side):
    """The grazing camera: a cube of edge 4 and a camera ON the planes of two of its faces, looking along -z.  The centre row's rays
    have qd.y == 0 and the centre column's qd.x == 0.  side = +1: qo == +0.5, so t2 = 0/0 = NaN and t1 = +-inf — glm::min / max
    return t2 and the slab is skipped (the ray runs in the face plane and hits the front face's edge), fminf / fmaxf return t1 and the
    ray misses.  side = -1: qo == -0.5, t1 = NaN and t2 = +-inf — glm and fminf / fmaxf both return t2 and the ray misses, numpy's
    minimum / maximum return the NaN and it hits."""
    s = F(2.0 * side)
    geoms = _geoms(pkg, (0, (0, 0, 0), (0, 0, 0), (4, 4, 4), (0.7, 0.6, 0.3), 0.0), (1, (0.5 * side, 0.5 * side, 4), (0, 0, 0), (1, 1, 1), (0.3, 0.4, 0.8), 0.0))
    return dict(cam=_cam(pkg, (s, s, 9), (s, s, 0), 22.5), geoms=geoms, geom_ids=None, tris=None, tri_ids=None, tri_albedo=None, tri_tex=None,
                textures=None, light=(0.0, 6.0, 8.0), alts=("fminmax_slab", "std_slab") if side > 0 else ("nan_slab", "std_slab"))


def _scene_F(pkg, kind):
    """The camera inside a cube / inside a sphere (the `inside` branch with the leaving face, the sphere's far root), with a small
    primitive of the other kind and a triangle in the same room."""
    if kind == 0:
        geoms = _geoms(pkg, (0, (0, 0, 0), (0, 20, 0), (8, 6, 10), (0.8, 0.8, 0.7), 0.0), (1, (-0.5, 0, -1.5), (0, 0, 0), (1, 1, 1), (0.9, 0.3, 0.3), 0.0))
        cam, alts = _cam(pkg, (1, 0.5, 2), (0, 0, -3), 40.0), ("no_inside",)
    else:
        geoms = _geoms(pkg, (1, (0, 0, 0), (0, 0, 30), (9, 7, 8), (0.6, 0.8, 0.7), 0.0), (0, (-0.5, -0.5, -2), (10, 20, 0), (1, 1, 1), (0.9, 0.6, 0.2), 0.0))
        cam, alts = _cam(pkg, (0.5, 0.25, 1), (0, 0, -2), 40.0), ("sphere_near_root",)
    tris = [_tri((0.5, -1, -2), (1.5, -1, -2.5), (1, 0.5, -2))]
    return dict(cam=cam, geoms=geoms, geom_ids=np.array([2, 0], np.int32), tris=np.stack(tris), tri_ids=np.array([1], np.int32),
                tri_albedo=_colours(1, 6), tri_tex=None, textures=None, light=(0.0, 1.5, 0.0), alts=alts)


def _scene_G(pkg):
    """A cube rotated about all three axes and a visible sphere scaled by (3, 1, 2) and rotated: its normals go through invT."""
    geoms = _geoms(pkg, (0, (-1.8, 0, 0), (20, 30, 40), (1.5, 1, 2), (0.8, 0.5, 0.3), 0.0), (1, (1.5, 0.3, 0), (10, 25, -30), (3, 1, 2), (0.3, 0.6, 0.9), 0.0))
    return dict(cam=_cam(pkg, (0, 1, 7), (0, 0, 0), 22.5), geoms=geoms, geom_ids=None, tris=None, tri_ids=None, tri_albedo=None, tri_tex=None,
                textures=None, light=(2.0, 5.0, 6.0), alts=("sphere_normal_xf", "cube_normal_unrotated"))


SCENES = {"A": _scene_A, "B": _scene_B, "C": _scene_C, "D": _scene_D, "E_plus": lambda p: _scene_E(p, 1), "E_minus": lambda p: _scene_E(p, -1),
          "F_cube": lambda p: _scene_F(p, 0), "F_sphere": lambda p: _scene_F(p, 1), "G": _scene_G}
FRAME, SEED = 3, 11


@functools.lru_cache(maxsize=None)
def _scene(name):
    import __graft_entry__ as ge
    return SCENES[name](ge.load_package())


@functools.lru_cache(maxsize=None)
def _model(name, W, H, alt=None):
    """The model's frame of an edge scene: computed once, shared by the CPU and the GPU tests, never written to."""
    s = _scene(name)
    col, gb = sm.render(W, H, FRAME, s["cam"], s["geoms"], s["geom_ids"], s["tris"], s["tri_ids"], s["tri_albedo"], s["tri_tex"], s["textures"],
                        s["light"], seed=SEED, alt=alt)
    col.setflags(write=False); gb.setflags(write=False)
    return col, gb


def _sizes(name):
    return SIZES + ([(33, 9)] if name.startswith("E") else [])


# ---- CPU: the model against what is already pinned ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,frame,moving", [(67, 41, 0, False), (67, 41, 5, True), (130, 9, 0, False), (130, 9, 5, True)])
def test_model_without_triangles_equals_render_scene(pkg, W, H, frame, moving):
    """box_room.txt: every field and the colour, bit for bit — the new model is tied to the oracle test_scene.py holds the device to."""
    sc = pkg.scene.parse_scene(open(SCENE).read())
    g = pkg.scene.geom_array(sc)
    cam = pkg.scene.camera_for_frame(sc, frame, moving)
    ref = pkg.scene.render_scene(W, H, frame, g, cam, seed=5)
    got = sm.render(W, H, frame, cam, g, None, None, None, None, None, None, pkg.scene.light_position(g), seed=5)
    c = counts(got, ref)
    print(f"model vs scene.render_scene {W}x{H} frame {frame}: differing pixels {c}")
    assert len(np.unique(ref[1]["geomId"])) >= 4 and not any(c.values())        # the frame shows several objects, and all is equal


@pytest.fixture(scope="module")
def ref_scenes_dir(tmp_path_factory):
    """The reference's scenes/ directory as test_ref_scenes.py unpacks it."""
    import tarfile
    d = tmp_path_factory.mktemp("ref_scenes_model")
    with tarfile.open(os.path.join(REF_DIR, "scene_files.tar.gz")) as tar:
        if hasattr(tarfile, "data_filter"):
            tar.extractall(d, filter="data")
        else:
            tar.extractall(d)
    return str(d)


def _recorded_cam(z, f, fovy):
    c = z["cams"][f]
    return dict(right=c[0:3].astype(F), up=c[3:6].astype(F), view=c[6:9].astype(F), position=c[9:12].astype(F), fovy_deg=float(fovy))


@functools.lru_cache(maxsize=None)
def _recorded_model(name, scene, f):
    """The model's frame f of a recorded reference scene, through <scene>_producer_inputs.npz exactly as the device test feeds it."""
    import __graft_entry__ as ge
    pkg = ge.load_package()
    z = np.load(os.path.join(REF_DIR, name + ".npz"))
    pi = np.load(os.path.join(REF_DIR, scene + "_producer_inputs.npz"))
    textures = [pi[k] for k in sorted(pi.files) if k.startswith("texture") and k != "textured_objects"] if "tri_tex" in pi.files else None
    col, gb = sm.render(int(z["W"]), int(z["H"]), f, _recorded_cam(z, f, pi["fovy"]), pi["geoms"], pi["geom_ids"], pi["tris"], pi["tri_ids"],
                        pi["tri_albedo"], pi["tri_tex"] if textures else None, textures, pkg.scene.light_position(pi["geoms"]))
    col.setflags(write=False); gb.setflags(write=False)
    return col, gb


RECORDED = [("cornell96_static", "cornell"), ("room128x72_static_sepcolor", "room")]


@pytest.mark.parametrize("name,scene", RECORDED)
def test_model_is_consistent_with_the_reference_gbuffer(pkg, name, scene, ref_scenes_dir):
    """Frame 0 of the recorded scenes: the bars of test_first_hit_with_meshes_matches_reference_gbuffer, and the same geomId as
    mesh.first_hit_gbuffer wherever that agrees with the recording (cornell with its texture; room's inputs carry none)."""
    from importlib import import_module
    mesh = import_module(pkg.__name__ + ".mesh")
    z = np.load(os.path.join(REF_DIR, name + ".npz"))
    pi = np.load(os.path.join(REF_DIR, scene + "_producer_inputs.npz"))
    W, H = int(z["W"]), int(z["H"])
    _, gb = _recorded_model(name, scene, 0)
    ref = z["gbuffer"][0]
    same = gb["geomId"] == ref["geomId"]
    assert same.mean() >= 0.995, f"{name}: geomId agrees on {same.mean():.4f}"
    hit = same & (ref["geomId"] >= 0)
    assert np.abs(gb["position"][hit] - ref["position"][hit]).max() <= 1e-3
    assert np.abs(gb["normal"][hit] - ref["normal"][hit]).max() <= 1e-3
    textured = np.isin(ref["geomId"], pi["textured_objects"])
    if "tri_tex" in pi.files:
        assert (hit & textured).any() and np.abs(gb["albedo"][hit] - ref["albedo"][hit]).max() <= 2.01 / 255.0
    else:
        assert np.abs(gb["albedo"][hit & ~textured] - ref["albedo"][hit & ~textured]).max() <= 2.01 / 255.0
    miss = same & (ref["geomId"] < 0)
    if miss.any():
        assert np.abs(gb["position"][miss] - ref["position"][miss]).max() <= 1e-5
    sc = pkg.scene.parse_scene(open(os.path.join(ref_scenes_dir, scene + ".txt")).read())
    tris = mesh.scene_triangles(sc, os.path.join(ref_scenes_dir, "Models"))
    with np.errstate(all="ignore"):
        fh = mesh.first_hit_gbuffer(W, H, sc, _recorded_cam(z, 0, sc.camera["fovy"]), tris, mesh.load_textures(sc, os.path.join(ref_scenes_dir, "Textures")))
    agree = fh["geomId"] == ref["geomId"]
    n_bad = int(np.count_nonzero((gb["geomId"] != fh["geomId"]) & agree))
    print(f"{name}: model vs recording: geomId differs on {int((~same).sum())} pixels; first_hit_gbuffer vs recording: {int((~agree).sum())}; "
          f"model vs first_hit_gbuffer where that agrees with the recording: {n_bad}")
    assert n_bad == 0


@pytest.mark.parametrize("name", list(SCENES))
def test_each_edge_acts(name):
    """The model against each wrong variant the scene is there to catch: more than `cap` pixels differ, at every size above 1x1."""
    s = _scene(name)
    for W, H in _sizes(name)[:1] + _sizes(name)[2:]:
        ref = _model(name, W, H)
        hit = int(np.count_nonzero(ref[1]["geomId"] >= 0))
        print(f"scene {name} {W}x{H}: {hit} of {W * H} pixels hit, ids {sorted(set(ref[1]['geomId'].ravel().tolist()))}, cap {cap(W, H)}")
        for alt in s["alts"]:
            n = any_differs(_model(name, W, H, alt), ref)
            print(f"  {alt}: {n} pixels differ")
            assert n > cap(W, H), f"scene {name} {W}x{H}: `{alt}` changes only {n} pixels, a test that allows {cap(W, H)} could not see it"
    if name == "D":
        nan = np.isnan(_model(name, 67, 41)[1]["normal"]).any(axis=-1)
        print(f"  NaN normals on {int(nan.sum())} pixels")
        assert nan.sum() > cap(67, 41) and np.isfinite(_model(name, 67, 41)[0]).all()


# ---- GPU: the device against the model ---------------------------------------------------------------------------------------------------
def _device(pkg, W, H, s, frame, seed, planar=False):
    import torch
    rgb = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    geoms = s["geoms"]
    args = (W, H, s["cam"], geoms, s["geom_ids"] if s["geom_ids"] is not None else np.zeros(0, np.int32),
            s["tris"] if s["tris"] is not None else np.zeros((0, 3, 8), F), s["tri_ids"] if s["tri_ids"] is not None else np.zeros(0, np.int32),
            s["tri_albedo"] if s["tri_albedo"] is not None else np.zeros((0, 3), F))
    kw = dict(frame=frame, tri_tex=s["tri_tex"], textures=s["textures"], seed=seed, light=s["light"])
    gb = np.zeros((H, W), dtype=pkg.synth.GBUFFER_DTYPE)
    if not planar:
        gbt = torch.empty((H * W * 52,), dtype=torch.uint8, device="cuda")
        pkg.binding.scene_render_mesh(rgb, gbt, *args, **kw)
        torch.cuda.synchronize()
        return rgb.cpu().numpy(), gbt.cpu().numpy().view(pkg.synth.GBUFFER_DTYPE).reshape(H, W)
    import ctypes
    from temporal_harness import _hip
    den = pkg.Denoiser(W, H, 0)
    planes = den.planar_gbuffer()
    pkg.binding.scene_render_mesh(rgb, planes, *args, **kw)
    torch.cuda.synchronize()
    hip = _hip()
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    for field, ptr in (("normal", planes.normal), ("position", planes.position), ("albedo", planes.albedo), ("geomId", planes.geom_id)):
        host = np.zeros((H, W, 3) if field != "geomId" else (H, W), F if field != "geomId" else np.int32)
        assert hip.hipMemcpy(host.ctypes.data, ptr, host.nbytes, 2) == 0
        gb[field] = host
    gb["ialbedo"] = F(1.0)          # the planes carry albedo * ialbedo with ialbedo == 1
    den.free()
    return rgb.cpu().numpy(), gb


def _check(got, ref, W, H, what):
    c = counts(got, ref)
    print(f"{what} {W}x{H}: differing pixels {c} (expected 0, cap {cap(W, H)})")
    for f, n in c.items():
        assert n <= cap(W, H), f"{what} {W}x{H}: {f} differs on {n} pixels"
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_device_equals_model_on_edge_scene(pkg, name):
    for W, H in _sizes(name):
        _check(_device(pkg, W, H, _scene(name), FRAME, SEED), _model(name, W, H), W, H, f"scene {name}")


@pytest.mark.gpu
def test_device_planar_entry_equals_model_on_textures(pkg):
    """Scene C through svgf_scene_render_mesh_planar into a context's planes: the same model."""
    W, H = SIZES[0]
    _check(_device(pkg, W, H, _scene("C"), FRAME, SEED, planar=True), _model("C", W, H), W, H, "scene C, planar")


@pytest.mark.gpu
@pytest.mark.parametrize("name,scene", RECORDED)
def test_device_equals_model_on_recorded_scene(pkg, name, scene):
    """The reference's cameras with <scene>_producer_inputs.npz, cornell with its real texture: the device equals the model on bits.
    (The loose comparison with the reference's own G-buffer stays in test_ref_scenes.py.)"""
    z = np.load(os.path.join(REF_DIR, name + ".npz"))
    pi = np.load(os.path.join(REF_DIR, scene + "_producer_inputs.npz"))
    W, H = int(z["W"]), int(z["H"])
    textures = [pi[k] for k in sorted(pi.files) if k.startswith("texture") and k != "textured_objects"] if "tri_tex" in pi.files else None
    for f in ((0, z["cams"].shape[0] - 1) if scene == "cornell" else (0,)):       # (room: 2 810 triangles in the numpy loop, one frame)
        s = dict(cam=_recorded_cam(z, f, pi["fovy"]), geoms=pi["geoms"], geom_ids=pi["geom_ids"], tris=pi["tris"], tri_ids=pi["tri_ids"],
                 tri_albedo=pi["tri_albedo"], tri_tex=pi["tri_tex"] if textures else None, textures=textures, light=pkg.scene.light_position(pi["geoms"]))
        got = _device(pkg, W, H, s, f, 1)
        ref = _recorded_model(name, scene, f)
        assert np.isin(ref[1]["geomId"], np.unique(pi["tri_ids"])).mean() > 0.01, "the scene's meshes should be in the picture"
        _check(got, ref, W, H, f"{name} frame {f}")
