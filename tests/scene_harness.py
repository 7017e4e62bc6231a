"""What the scene-draw suites share (tests/test_resident_scene.py, test_animated_scene.py, test_shadowed_scene.py, test_traced_scene.py,
test_split_scene.py, test_path_scene.py, test_gloss_scene.py, test_virtual_scene.py, test_rough_scene.py, test_highlight_scene.py): the
device plumbing (buffers, streams, graph capture, the planar reader), the inputs and the numpy models more than one suite draws, each
behind the lru_cache it always had, one record per draw family with one draw() and one same() on top of it, and the GPU test bodies
every family repeats (planar target, every tree, queued draws, a captured draw, the common refusals, the closing pose -> split draw ->
two denoises -> compose sequence).  The suites import this module and no other suite.  Test infrastructure only; not part of the package."""
import ctypes
import dataclasses
import functools
import os
import tarfile

import numpy as np

import scene_gloss_model as gm
import scene_model as sm
import scene_path_model as spm
import scene_pose_model as pm
import scene_rough_model as rm
import scene_shadow_model as ssm
import scene_split_model as splm
import scene_trace_model as stm
import scene_virtual_model as vm
import temporal_model as tm
import test_scene_model as tsm
from test_scene_model import FRAME, REF_DIR, SEED, cap, counts, differing

F = np.float32
BUILDS = [(ml, sp) for ml in (1, 4, 8) for sp in (0, 1)]
SIZES = [(1, 1), (7, 5), (65, 4), (257, 3)]         # one lane; one partial wave; a wave seam; a block seam and a one-lane tail
EDGE = ("A", "B", "F_cube", "F_sphere", "E_plus")
RECORDED = {"cornell": "cornell96_static", "room": "room128x72_static_sepcolor", "bunny": "bunny128x72_static"}
W0, H0 = 67, 41


# ---- device plumbing ---------------------------------------------------------------------------------------------------------------------
def create(pkg, s, ml=0, sp=0):
    return pkg.Scene.create(s["geoms"], s["geom_ids"], s["tris"], s["tri_ids"], s["tri_albedo"], s["tri_tex"], s["textures"], ml, sp)


def buffers(W, H):
    import torch
    return torch.empty((H, W, 3), dtype=torch.float32, device="cuda"), torch.empty((H * W * 52,), dtype=torch.uint8, device="cuda")


def host(pkg, rgb, gbt, W, H):
    return rgb.cpu().numpy(), gbt.cpu().numpy().view(pkg.synth.GBUFFER_DTYPE).reshape(H, W)


def split_buffers(W, H, rgb=True):
    import torch
    img = lambda: torch.full((H, W, 3), float("nan"), dtype=torch.float32, device="cuda")      # noqa: E731
    return dict(D=img(), I=img(), color=img() if rgb else None, gb=torch.empty((H * W * 52,), dtype=torch.uint8, device="cuda"))


def chain_buffer(W, H):
    import torch
    return torch.full((H, W), -77, dtype=torch.int32, device="cuda")


def light(pkg, lt):
    return pkg.binding.SvgfSceneLight.make(lt["centre"], lt["edge_u"], lt["edge_v"], lt["samples"])


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def motion_buffer(n):
    import torch
    return torch.full((n, 12), float("nan"), dtype=torch.float32, device="cuda")


def free(*tables):
    for t in tables:
        if t is not None:
            t.free()


def read_planes(pkg, planes, W, H):
    """The four planes of a context's planar G-buffer as one GBUFFER_DTYPE[H, W] on the host (ialbedo 1: the planes hold the product)."""
    from temporal_harness import _hip
    hip = _hip()
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    gb = np.zeros((H, W), dtype=pkg.synth.GBUFFER_DTYPE)
    for field, ptr in (("normal", planes.normal), ("position", planes.position), ("albedo", planes.albedo), ("geomId", planes.geom_id)):
        plane = np.zeros((H, W, 3) if field != "geomId" else (H, W), F if field != "geomId" else np.int32)
        rc = hip.hipMemcpy(plane.ctypes.data, ptr, plane.nbytes, 2)
        assert rc == 0, f"hipMemcpy of the {field} plane: {rc}"
        gb[field] = plane
    gb["ialbedo"] = F(1.0)
    return gb


class OwnStream:
    """A non-blocking HIP stream of the test's own, destroyed by close(): the tests that use it take nothing from torch's pool of
    streams and leave the process with the streams it had (tests/test_stream_gpu.py's timing test depends on which hardware queue the
    NEXT two pool streams land on, and with it on every stream a test file in front of it leaves behind)."""

    def __init__(self):
        import torch
        from temporal_harness import _hip
        self.hip = _hip()
        self.hip.hipStreamCreateWithFlags.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
        self.hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
        h = ctypes.c_void_p()
        rc = self.hip.hipStreamCreateWithFlags(ctypes.byref(h), 1)
        assert rc == 0 and h.value, f"hipStreamCreateWithFlags: {rc}"
        self.cuda_stream = h.value
        self.torch = torch.cuda.ExternalStream(h.value)

    def synchronize(self):
        self.torch.synchronize()

    def close(self):
        self.synchronize()
        rc = self.hip.hipStreamDestroy(self.cuda_stream)
        assert rc == 0, f"hipStreamDestroy: {rc}"


class _PoolStream:
    """torch.cuda.Stream() behind OwnStream's interface: what the three oldest suites (resident, animated, shadowed; traced with
    them) have always queued on."""

    def __init__(self):
        import torch
        self.torch = torch.cuda.Stream()
        self.cuda_stream = self.torch.cuda_stream

    def synchronize(self):
        self.torch.synchronize()

    close = synchronize


def open_stream(own):
    return OwnStream() if own else _PoolStream()


def graph_api():
    from temporal_harness import _hip
    hip = _hip()
    vp = ctypes.c_void_p
    hip.hipStreamEndCapture.argtypes = [vp, ctypes.POINTER(vp)]
    hip.hipGraphInstantiate.argtypes = [ctypes.POINTER(vp), vp, vp, vp, ctypes.c_size_t]
    hip.hipGraphLaunch.argtypes = [vp, vp]
    hip.hipGraphExecDestroy.argtypes = [vp]
    hip.hipGraphDestroy.argtypes = [vp]
    hip.hipGraphGetNodes.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t)]
    hip.hipGraphNodeGetType.argtypes = [vp, ctypes.POINTER(ctypes.c_int)]
    return hip


def node_types(hip, graph):
    n = ctypes.c_size_t(0)
    rc = hip.hipGraphGetNodes(graph, None, ctypes.byref(n))
    assert rc == 0, f"hipGraphGetNodes: {rc}"
    arr = (ctypes.c_void_p * max(n.value, 1))()
    rc = hip.hipGraphGetNodes(graph, arr, ctypes.byref(n))
    assert rc == 0, f"hipGraphGetNodes: {rc}"
    types = []
    for k in range(n.value):
        t = ctypes.c_int(-1)
        rc = hip.hipGraphNodeGetType(arr[k], ctypes.byref(t))
        assert rc == 0, f"hipGraphNodeGetType: {rc}"
        types.append(t.value)
    return types        # hipGraphNodeTypeKernel 0, Memcpy 1, Memset 2


class Captured:
    """What record() enqueues on `st` (a stream with .cuda_stream), captured in relaxed mode and not executed: `types` are the
    graph's node types; launch() replays it on the same stream (instantiated on first use), destroy() releases graph and executable."""

    def __init__(self, st, record):
        self.hip, self.st, self.graph, self.gexec = graph_api(), st, ctypes.c_void_p(), ctypes.c_void_p()
        begin = self.hip.hipStreamBeginCapture
        begin.argtypes = [ctypes.c_void_p, ctypes.c_int]
        rc = begin(st.cuda_stream, 2)            # hipStreamCaptureModeRelaxed
        assert rc == 0, f"begin capture: {rc}"
        record()
        rc = self.hip.hipStreamEndCapture(st.cuda_stream, ctypes.byref(self.graph))
        assert rc == 0 and self.graph.value, f"hipStreamEndCapture: {rc}"
        self.types = node_types(self.hip, self.graph)

    def launch(self):
        if not self.gexec.value:
            rc = self.hip.hipGraphInstantiate(ctypes.byref(self.gexec), self.graph, None, None, 0)
            assert rc == 0, f"hipGraphInstantiate: {rc}"
        rc = self.hip.hipGraphLaunch(self.gexec, self.st.cuda_stream)
        assert rc == 0, f"hipGraphLaunch: {rc}"

    def destroy(self):
        if self.gexec.value:
            self.hip.hipGraphExecDestroy(self.gexec)
        self.hip.hipGraphDestroy(self.graph)


# ---- inputs: recorded scenes, triangle sets, edge scenes with an occluder, made scenes --------------------------------------------------
@functools.lru_cache(maxsize=None)
def recorded(scene, f):
    """A recorded reference scene at frame f of its recorded cameras, as the dict the edge scenes use, and its frame size."""
    import __graft_entry__ as ge
    pkg = ge.load_package()
    z = np.load(os.path.join(REF_DIR, RECORDED[scene] + ".npz"))
    pi = np.load(os.path.join(REF_DIR, scene + "_producer_inputs.npz"))
    textures = [pi[k] for k in sorted(pi.files) if k.startswith("texture") and k != "textured_objects"] if "tri_tex" in pi.files else None
    s = dict(cam=tsm._recorded_cam(z, f, pi["fovy"]), geoms=pi["geoms"], geom_ids=pi["geom_ids"], tris=pi["tris"], tri_ids=pi["tri_ids"],
             tri_albedo=pi["tri_albedo"], tri_tex=pi["tri_tex"] if textures else None, textures=textures, light=pkg.scene.light_position(pi["geoms"]))
    return s, int(z["W"]), int(z["H"])


@functools.lru_cache(maxsize=None)
def scene_text(name):
    with tarfile.open(os.path.join(REF_DIR, "scene_files.tar.gz")) as tar:
        return tar.extractfile(name + ".txt").read().decode()


def _tri_rows(p0, p1, p2):
    t = np.zeros((3, 8), F)
    t[:, 0:3] = np.array([p0, p1, p2], F)
    return t


@functools.lru_cache(maxsize=None)
def tri_set(name):
    """float32[n, 3, 8]: the recorded meshes, scene A and the adversarial sets of the builder test."""
    if name in RECORDED:
        return recorded(name, 0)[0]["tris"]
    if name == "A":
        return tsm._scene("A")["tris"]
    one = _tri_rows((0, 0, 0), (1, 0, 0), (0, 1, 0.5))
    rng = np.random.default_rng(14)
    if name == "one":
        return one[None]
    if name == "none":
        return np.zeros((0, 3, 8), F)
    if name == "copies300":
        return np.repeat(one[None], 300, axis=0)
    if name == "zero_area257":      # every triangle a point; all on one point but the last few, which are points elsewhere
        pts = np.concatenate([np.zeros((250, 3), F), rng.uniform(-1, 1, (7, 3)).astype(F)])
        t = np.zeros((257, 3, 8), F)
        t[:, :, 0:3] = pts[:, None, :]
        return t
    if name == "huge_over_500":
        c = rng.uniform(-1, 1, (500, 1, 3)).astype(F)
        small = np.zeros((500, 3, 8), F)
        small[:, :, 0:3] = c + rng.uniform(-0.01, 0.01, (500, 3, 3)).astype(F)
        return np.concatenate([_tri_rows((-1000, -1000, 0), (1000, -1000, 0), (0, 1000, 0))[None], small])
    if name == "line4096":
        t = np.zeros((4096, 3, 8), F)
        x = np.arange(4096, dtype=F)[:, None]
        t[:, :, 0] = x + np.array([0, 0.5, 0.25], F)
        t[:, :, 1] = np.array([0, 0, 0.5], F)
        return t
    raise KeyError(name)


TRI_SETS = ("room", "bunny", "cornell", "A", "one", "none", "copies300", "zero_area257", "huge_over_500", "line4096")


def _basis(n):
    n = np.asarray(n, np.float64) / np.linalg.norm(n)
    a = np.cross(n, (0.0, 0.0, 1.0) if abs(n[2]) < 0.9 else (1.0, 0.0, 0.0))
    a /= np.linalg.norm(a)
    return n, a, np.cross(n, a)


def add_objects(pkg, s, geoms=(), tris=(), ids=(90, 91, 92, 93, 94, 95)):
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
def edge(name):
    """(scene, light kwargs): an edge scene of test_scene_model.py with an occluder - a two-sided triangle sheet and a sphere, or
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
        s = add_objects(pkg, s, geoms=[(0, tuple(mid - 0.8 * size * a), (10, 20, 30), (size, size, 0.3 * size), (0.6, 0.5, 0.4), 0.0), ball])
    elif name == "A":       # triangles only: n_geoms == 0 stays
        s = add_objects(pkg, s, tris=_sheet(mid, n, size) + _sheet(mid + 1.5 * size * a + 0.1 * n, n, 0.5 * size)[:1])
    else:
        s = add_objects(pkg, s, geoms=[ball], tris=_sheet(mid - 0.5 * size * a, n, size))
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


def _turned(x, y, z=0.0):
    from temporal_harness import rotation
    return tuple(float(c) for c in (rotation("x", 25.0) @ rotation("y", -35.0)) @ np.array([x, y, z], np.float64))


@functools.lru_cache(maxsize=None)
def _graze():
    """The scene on which the GATE decides shadow samples.  A wall, an occluder (both windings) and the light lie in ONE plane, turned
    out of the axes; the light's centre stands 1e-6 behind it.  A shadow ray then runs within rounding of the occluder's plane: the
    determinant of the triangle test is a difference of products that cancel to a few 1e-7, its reciprocal is wrong by a factor of
    order one, and with it t - the float32 test accepts hits that lie nowhere near the triangle, before the ray has reached its
    padded box (t < tn).  The contract drops them; an ungated brute force would not."""
    import __graft_entry__ as ge
    pkg = ge.load_package()
    P = _turned
    tris = [tsm._tri(P(-4, -3), P(2, -3), P(-4, 3)), tsm._tri(P(2, -3), P(2, 3), P(-4, 3), k=1),
            tsm._tri(P(3, -1.5), P(4.5, 0), P(3, 1.5), k=2), tsm._tri(P(3, -1.5), P(3, 1.5), P(4.5, 0), k=3)]
    s = dict(cam=tsm._cam(pkg, P(0, 0, 9), P(0, 0, 0), 25.0), geoms=tsm._geoms(pkg), geom_ids=None, tris=np.stack(tris),
             tri_ids=np.array([1, 1, 2, 3], np.int32), tri_albedo=tsm._colours(4, 9), tri_tex=None, textures=None, light=P(8, 0, -1e-6))
    return s, dict(centre=s["light"], edge_u=P(0, 0.5, 0), edge_v=(0.0, 0.0, 0.0))


@functools.lru_cache(maxsize=None)
def furnace():
    """A sphere and a cube of albedo 1 that do not emit, inside an emitting cube of albedo 0.5 and emittance 2, the camera inside; the
    light's centre so far away that 4 + dist2 overflows and the light's term is exactly 0 everywhere.  With ambient = 1 every bounce
    brings back exactly 1: the enclosure 0.5 * 2, the two objects 1 * (1 + 0)."""
    import __graft_entry__ as ge
    pkg = ge.load_package()
    z = (0, 0, 0)
    geoms = tsm._geoms(pkg, (0, (0, 0, 0), z, (10, 10, 10), (0.5, 0.5, 0.5), 2.0), (1, (-1.2, -0.3, 0), z, (2, 2, 2), (1, 1, 1), 0.0),
                       (0, (1.4, 0.2, -0.5), (0, 30, 15), (1.5, 1.5, 1.5), (1, 1, 1), 0.0))
    s = dict(cam=tsm._cam(pkg, (0, 0.4, 2.6), (0, 0, 0), 40.0), geoms=geoms, geom_ids=None, tris=None, tri_ids=None, tri_albedo=None,
             tri_tex=None, textures=None, light=(0.0, 1e20, 0.0))
    return s, dict(centre=s["light"], edge_u=(0.0, 0.0, 0.0), edge_v=(0.0, 0.0, 0.0))


@functools.lru_cache(maxsize=None)
def _bleed():
    """A white floor, a red wall standing on it at x = -3 and a white back wall; the light above the middle of the floor."""
    import __graft_entry__ as ge
    pkg = ge.load_package()
    z = (0, 0, 0)
    geoms = tsm._geoms(pkg, (0, (0, -0.1, 0), z, (12, 0.2, 12), (0.9, 0.9, 0.9), 0.0), (0, (-3.1, 3, 0), z, (0.2, 6, 12), (0.9, 0.1, 0.1), 0.0),
                       (0, (0, 3, -6.1), z, (12, 6, 0.2), (0.9, 0.9, 0.9), 0.0))
    s = dict(cam=tsm._cam(pkg, (1.5, 5, 9), (0, 0, 0), 40.0), geoms=geoms, geom_ids=None, tris=None, tri_ids=None, tri_albedo=None,
             tri_tex=None, textures=None, light=(0.0, 6.0, 0.0))
    return s, dict(centre=s["light"], edge_u=(0.5, 0.0, 0.0), edge_v=(0.0, 0.0, 0.5))


@functools.lru_cache(maxsize=None)
def _graze_bounce():
    """The scene on which the GATE decides bounce hits, after _graze.  A wall and an occluder (both windings) lie in ONE plane,
    turned out of the axes, and the wall's vertex normals lie IN that plane, towards the occluder.  Almost every bounce leaves the
    plane; the fallback direction of the rejection sampler (a = b = 0, two pixels in a thousand) is the normal itself and runs within
    rounding of the plane of all four triangles, where the float32 test accepts hits that lie nowhere near the triangle."""
    import __graft_entry__ as ge
    pkg = ge.load_package()
    P = _turned
    nrm = np.array([P(1, 0, 0)] * 3, F)
    tris = [tsm._tri(P(-4, -3), P(2, -3), P(-4, 3), nrm=nrm), tsm._tri(P(2, -3), P(2, 3), P(-4, 3), nrm=nrm, k=1),
            tsm._tri(P(3, -1.5), P(4.5, 0), P(3, 1.5), k=2), tsm._tri(P(3, -1.5), P(3, 1.5), P(4.5, 0), k=3)]
    s = dict(cam=tsm._cam(pkg, P(-1, 0, 5), P(-1, 0, 0), 25.0), geoms=tsm._geoms(pkg), geom_ids=None, tris=np.stack(tris),
             tri_ids=np.array([1, 1, 2, 3], np.int32), tri_albedo=tsm._colours(4, 9), tri_tex=None, textures=None, light=P(0, 0, 6))
    return s, dict(centre=s["light"], edge_u=P(0.3, 0, 0), edge_v=P(0, 0.3, 0))


@functools.lru_cache(maxsize=None)
def textured_floor():
    """Scene C's textured quads (in the plane z = 0, facing the camera) and a floor primitive under them that reaches towards the
    camera: half of its bounce goes back and up, onto the textured triangles."""
    import __graft_entry__ as ge
    pkg = ge.load_package()
    s = tsm._scene("C")
    P = np.asarray(s["tris"], F).reshape(-1, 3, 8)[:, :, :3].reshape(-1, 3)
    lo, hi = P.min(axis=0).astype(np.float64), P.max(axis=0).astype(np.float64)
    e = float((hi - lo).max())
    slab = (0, (0.0, lo[1] - 0.02 * e, 0.25 * e), (0, 0, 0), (e, 0.02 * e, 0.5 * e), (0.8, 0.8, 0.8), 0.0)
    s = add_objects(pkg, s, geoms=[slab])
    return s, dict(centre=tuple(s["light"]), edge_u=(0.2, 0, 0), edge_v=(0, 0.2, 0))


@functools.lru_cache(maxsize=None)
def _bleed_ceiling():
    """`bleed` (a white floor, a red wall, a white back wall) under a white ceiling: light that left the red wall comes back to
    the floor by way of the ceiling too."""
    import __graft_entry__ as ge
    pkg = ge.load_package()
    s, lk = _bleed()
    s = dict(s)
    s["geoms"] = np.concatenate([s["geoms"], tsm._geoms(pkg, (0, (0, 6.35, 0), (0, 0, 0), (12, 0.5, 12), (0.9, 0.9, 0.9), 0.0))])
    return s, lk


@functools.lru_cache(maxsize=None)
def _bleed_nan():
    """_bleed_ceiling with a two-sided sheet WITHOUT normals floating over the floor: a path that lands on it has a NaN normal at that
    vertex, its next direction is NaN, and it ends there - behind the first hit, where f17 never looked."""
    s, lk = _bleed_ceiling()
    s = dict(s)
    zero = np.zeros((3, 3), F)
    p0, p1, p2 = (-4.5, 1.5, -3.0), (4.5, 1.5, -3.0), (0.0, 5.0, 3.0)
    s["tris"] = np.stack([tsm._tri(p0, p1, p2, nrm=zero), tsm._tri(p0, p2, p1, nrm=zero)])
    s["tri_ids"], s["tri_albedo"] = np.array([7, 7], np.int32), tsm._colours(2, 3)
    return s, lk


@functools.lru_cache(maxsize=None)
def _furnace07():
    """The furnace with the two objects at albedo 0.7: closed, and the throughput falls, so the roulette kills."""
    s, lk = furnace()
    s = dict(s)
    g = np.array(s["geoms"], copy=True)
    g["albedo"][1:] = F(0.7)
    s["geoms"] = g
    return s, lk


@functools.lru_cache(maxsize=None)
def _far_sheet():
    """The scene on which t_lo must be formed from the CURRENT vertex.  A floor around the origin (first hits with |x| of a few units:
    t_lo about 2^-10 ... 2^-8), a wall whose face stands at z = -30 (a vertex there: t_lo = 30 * 2^-10 = 0.029), and 0.01 in front of
    that face a one-sided sheet that faces the WALL: the camera's rays and the bounce from the floor cross it from behind, a bounce that
    leaves the wall meets its front at t = 0.01 / cos - below the wall vertex's t_lo for most directions, above the floor vertex's."""
    import __graft_entry__ as ge
    pkg = ge.load_package()
    z = (0, 0, 0)
    geoms = tsm._geoms(pkg, (0, (0, -0.5, 0), z, (16, 1, 16), (0.8, 0.8, 0.8), 0.0), (0, (0, 20, -31), z, (120, 60, 2), (0.7, 0.7, 0.9), 0.0))
    a, b, c, d = (-60, -5, -29.99), (60, -5, -29.99), (60, 50, -29.99), (-60, 50, -29.99)
    tris = [tsm._tri(a, c, b), tsm._tri(a, d, c, k=1)]                 # e1 x e2 points to -z, towards the wall
    s = dict(cam=tsm._cam(pkg, (0, 5, 9), (0, 0, 0), 30.0), geoms=geoms, geom_ids=None, tris=np.stack(tris), tri_ids=np.array([5, 5], np.int32),
             tri_albedo=tsm._colours(2, 4), tri_tex=None, textures=None, light=(0.0, 8.0, 0.0))
    return s, dict(centre=s["light"], edge_u=(0.5, 0.0, 0.0), edge_v=(0.0, 0.0, 0.5))


_MADE = {"made": {"stage": _stage, "half": _half, "graze": _graze},
         "traced": {"furnace": furnace, "bleed": _bleed, "graze": _graze_bounce, "textured": textured_floor},
         "path": {"bleed_ceiling": _bleed_ceiling, "bleed_nan": _bleed_nan, "furnace07": _furnace07, "far_sheet": _far_sheet}}


def scene_input(kind, name):
    """(scene, light kwargs) of an input by kind: "edge" (an edge scene with its occluder), "plain" (an edge scene as it is, with a
    small area light), "rec" (a recorded scene at frame 0), "made" / "traced" / "path" (the scenes made for rows f16 / f17 / f19)."""
    if kind == "edge":
        return edge(name)
    if kind in _MADE:
        return _MADE[kind][name]()
    if kind == "plain":
        s = tsm._scene(name)
        return s, dict(centre=tuple(s["light"]), edge_u=(0.2, 0, 0), edge_v=(0, 0.2, 0))
    s, W, H = recorded(name, 0)
    return s, dict(centre=tuple(float(c) for c in s["light"]), edge_u=(0.5, 0, 0), edge_v=(0, 0, 0.5))


@functools.lru_cache(maxsize=None)
def example_scene():
    """The room of examples/shadowed_scene.cpp with its block at rest, under the example's light and the synthetic scene's camera."""
    import __graft_entry__ as ge
    pkg = ge.load_package()
    z = (0, 0, 0)
    geoms = tsm._geoms(pkg, (0, (0, 0, 0), z, (12, 0.2, 12), (0.8, 0.8, 0.8), 0.0), (0, (0, 5, -6), z, (12, 10, 0.2), (0.8, 0.8, 0.7), 0.0),
                       (0, (-6, 5, 0), z, (0.2, 10, 12), (0.8, 0.3, 0.3), 0.0), (0, (6, 5, 0), z, (0.2, 10, 12), (0.3, 0.8, 0.3), 0.0),
                       (0, (0, 9.9, 0), z, (3, 0.1, 3), (1, 1, 1), 5.0), (0, (-2.5, 1.1, 0), z, (2, 2, 2), (0.3, 0.4, 0.9), 0.0))
    return geoms, pkg.synth.camera_for_frame(0, False), dict(centre=(0.0, 9.5, 0.0), edge_u=(1.5, 0.0, 0.0), edge_v=(0.0, 0.0, 1.5))


def args_of(s):
    return s["cam"], s["geoms"], s["geom_ids"], s["tris"], s["tri_ids"], s["tri_albedo"], s["tri_tex"], s["textures"]


# ---- the turning block of box_room ------------------------------------------------------------------------------------------------------
BLOCK = (96, 96, 2, 3, 2)                 # the posed block of the gloss, virtual, rough and highlight suites: W, H, paths, max_depth, rr_depth
BLOCK_ALPHA, BLOCK_GA = 0.2, 0.3


@functools.lru_cache(maxsize=None)
def block_inputs():
    """box_room as a resident scene of primitives; six frames, the block 9 degrees further about y through its centre and 1.0
    further in x per frame (test_object_motion.py's motion), as pose tables over the rest state."""
    import __graft_entry__ as ge
    from temporal_harness import BLOCK as B, SCENE
    pkg = ge.load_package()
    sc = pkg.scene.parse_scene(open(SCENE).read())
    cam = pkg.scene.camera_for_frame(sc, 0, False)
    geoms = pkg.scene.geom_array(sc)
    centre = tuple(float(v) for v in sc.objects[B]["trans"])
    tables = []
    for f in range(6):
        t = pkg.binding.pose_identity(len(geoms))
        t[B] = pkg.binding.pose_rigid((0, 1, 0), np.deg2rad(9.0 * f), centre, (1.0 * f, 0, 0))
        tables.append(t)
    s = dict(cam=cam, geoms=geoms, geom_ids=None, tris=None, tri_ids=None, tri_albedo=None, tri_tex=None, textures=None,
             light=pkg.scene.light_position(geoms))
    return s, tables


@functools.lru_cache(maxsize=None)
def block_light():
    s, tables = block_inputs()
    L = np.asarray(s["light"], np.float64)
    return dict(centre=tuple(float(c) for c in L), edge_u=(0.8, 0.0, 0.0), edge_v=(0.0, 0.0, 0.8))


def block_table():
    from temporal_harness import BLOCK as B
    s, _ = block_inputs()
    return gm.table(len(s["geoms"]), **{f"g{B}": (1.0, 0.0, 1.0, (0.9, 0.9, 0.9))})


def block_rough():
    from temporal_harness import BLOCK as B
    a = np.zeros(len(block_inputs()[0]["geoms"]), F)
    a[B] = BLOCK_ALPHA
    return a


def block_motion(pkg, tables):
    """Per frame the rows svgf_scene_pose writes for `tables`, the held table starting as the identity."""
    held, rows = pkg.binding.pose_identity(len(tables[0])), []
    for t in tables:
        rows.append(pm.motion_rows(held, t))
        held = t
    return rows


@functools.lru_cache(maxsize=None)
def traced_block_frame(f, W, H, J, samples=1, noise=0.6):
    """Frame f of the turning block under its area light: the traced model on the posed arrays."""
    s, tables = block_inputs()
    ps = pm.posed_scene(s, tables[f])
    lk = block_light()
    lt = ssm.light(lk["centre"], lk["edge_u"], lk["edge_v"], samples)
    col, gb, info = stm.render(W, H, f, ps["cam"], ps["geoms"], None, None, None, None, None, None, lt, stm.params(J), seed=3, noise=noise,
                               fireflies=0.02 if noise else 0.0)
    return (col, gb), info, lt


@functools.lru_cache(maxsize=None)
def gloss_block_model(f, W, H, J, K, R, posed=True):
    """Frame f of the turning block, the block a mirror, under its area light: the gloss model on the posed arrays."""
    s, tables = block_inputs()
    ps = pm.posed_scene(s, tables[f]) if posed else s
    lk = block_light()
    lt = ssm.light(lk["centre"], lk["edge_u"], lk["edge_v"], 1)
    col, gb, D, I, info = gm.render(W, H, f, ps["cam"], ps["geoms"], None, None, None, None, None, None, lt, spm.params(J, K, R), block_table(), seed=3)      # noqa: E741
    return dict(color=col, gb=gb, D=D, I=I, info=info, lt=lt)


# ---- the models of rows f16 to f19, computed once per case and shared --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def first_hit(kind, name, W, H, frame, seed, noise=0.6):
    """scene_model.render's frame and the emitter mask of an input: computed once, shared, never written to."""
    s = scene_input(kind, name)[0]
    first = sm.render(W, H, frame, *args_of(s), s["light"], seed=seed, noise=noise, fireflies=0.02 if noise else 0.0)
    em = ssm.emitter_mask(W, H, s["cam"], s["geoms"], s["geom_ids"], s["tris"], s["tri_ids"])
    for a in first + (em,):
        a.setflags(write=False)
    return first, em


@functools.lru_cache(maxsize=None)
def shadow_model(kind, name, W, H, samples, point=False, alt=None, frame=FRAME, seed=SEED, noise=0.6, centre=None):
    s, lk = scene_input(kind, name)
    lt = ssm.light(centre or lk["centre"], samples=samples) if point else ssm.light(centre or lk["centre"], lk["edge_u"], lk["edge_v"], samples)
    if centre is None:
        first, em = first_hit(kind, name, W, H, frame, seed, noise)
    else:
        first = sm.render(W, H, frame, *args_of(s), centre, seed=seed, noise=noise, fireflies=0.02 if noise else 0.0)
        em = first_hit(kind, name, W, H, frame, seed, noise)[1]
    col, gb, info = ssm.render(W, H, frame, *args_of(s), lt, seed=seed, noise=noise, fireflies=0.02 if noise else 0.0, alt=alt, first=first, emitters=em)
    col.setflags(write=False)
    return (col, gb), info, lt


@functools.lru_cache(maxsize=None)
def traced_model(kind, name, W, H, J, sec=1, samples=1, point=False, alt=None, frame=FRAME, seed=SEED, noise=0.6, ambient=0.15):
    s, lk = scene_input(kind, name)
    lt = ssm.light(lk["centre"], samples=samples) if point else ssm.light(lk["centre"], lk["edge_u"], lk["edge_v"], samples)
    first, em = first_hit(kind, name, W, H, frame, seed, noise)
    col, gb, info = stm.render(W, H, frame, *args_of(s), lt, stm.params(J, ambient, sec), seed=seed, noise=noise, fireflies=0.02 if noise else 0.0,
                               alt=alt, first=first, emitters=em)
    col.setflags(write=False)
    return (col, gb), info, lt


@functools.lru_cache(maxsize=None)
def emittance(kind, name, W, H):
    s = scene_input(kind, name)[0]
    e = splm.emittance_plane(W, H, s["cam"], s["geoms"], s["geom_ids"], s["tris"], s["tri_ids"])
    e.setflags(write=False)
    return e


@functools.lru_cache(maxsize=None)
def split_model(kind, name, W, H, J, sec=1, samples=1, point=False, frame=FRAME, seed=SEED, noise=0.6, ambient=0.15):
    """dict(D, I, color, gb, info, lt): the split model on top of the cached traced model."""
    (col, gb), info, lt = traced_model(kind, name, W, H, J, sec, samples, point, None, frame, seed, noise, ambient)
    s = scene_input(kind, name)[0]
    D, I, col, gb, info = splm.render(W, H, frame, *args_of(s), lt, stm.params(J, ambient, sec), seed=seed, noise=noise,     # noqa: E741
                                      fireflies=0.02 if noise else 0.0, traced=(col, gb, info), emittance=emittance(kind, name, W, H))
    D.setflags(write=False); I.setflags(write=False)
    return dict(D=D, I=I, color=col, gb=gb, info=info, lt=lt)


@functools.lru_cache(maxsize=None)
def path_model(kind, name, W, H, J, K, R, sec=1, samples=1, point=False, alt=None, frame=None, seed=None, noise=0.6, ambient=0.15):
    """dict(color, gb, D, I, info, lt) of scene_path_model.render; a recorded scene at frame 0, seed 1 unless told otherwise."""
    frame = (0 if kind == "rec" else FRAME) if frame is None else frame
    seed = (1 if kind == "rec" else SEED) if seed is None else seed
    s, lk = scene_input(kind, name)
    lt = ssm.light(lk["centre"], samples=samples) if point else ssm.light(lk["centre"], lk["edge_u"], lk["edge_v"], samples)
    first, em = first_hit(kind, name, W, H, frame, seed, noise)
    col, gb, D, I, info = spm.render(W, H, frame, *args_of(s), lt, spm.params(J, K, R, ambient, sec), seed=seed, noise=noise,       # noqa: E741
                                     fireflies=0.02 if noise else 0.0, alt=alt, first=first, emitters=em, emittance=emittance(kind, name, W, H))
    for a in (col, D, I):
        a.setflags(write=False)
    return dict(color=col, gb=gb, D=D, I=I, info=info, lt=lt, frame=frame, seed=seed)


def counts_row(info):
    return [tuple(d[k] for k in spm.COUNTS) for d in info["depth"]]


BAD_TRACE = [(-1, 0.15, 1), (9, 0.15, 1), (1, float("nan"), 1), (1, float("inf"), 1), (1, -0.5, 1), (1, 0.15, 2), (1, 0.15, -1)]
BAD_PARAMS = [(-1, 4, 2, 0.15, 1), (9, 4, 2, 0.15, 1), (1, 0, 0, 0.15, 1), (1, 9, 0, 0.15, 1), (1, -1, 0, 0.15, 1), (1, 4, -1, 0.15, 1), (1, 4, 9, 0.15, 1),
              (1, 4, 2, float("nan"), 1), (1, 4, 2, float("inf"), 1), (1, 4, 2, -0.5, 1), (1, 4, 2, 0.15, 2), (1, 4, 2, 0.15, -1)]
BAD_VIRTUAL = [(0, 0), (-1, 0), (9, 0), (4, -1), (4, (1 << 24) + 1)]
BAD_GUIDE_ALPHA = [-0.5, float("nan"), float("inf"), -float("inf")]


# ---- the inputs and models of rows f20 to f22 --------------------------------------------------------------------------------------------
def room(pkg, *extra, block=True):
    geoms, cam, lk = example_scene()
    geoms = geoms if block else geoms[:5]
    if extra:
        geoms = np.concatenate([geoms, tsm._geoms(pkg, *extra)])
    s = dict(cam=cam, geoms=geoms, geom_ids=None, tris=None, tri_ids=None, tri_albedo=None, tri_tex=None, textures=None, light=lk["centre"])
    return s, lk


@functools.lru_cache(maxsize=None)
def glass_pair():
    """The f16 room (its block taken out) with a glass sphere (id 5) and a glass cube turned 30 degrees about y (id 6), both of scale
    3 and ior 1.5, with a spec that is not 1, so that the weight of a Fresnel reflection differs from a transmission's."""
    import __graft_entry__ as ge
    pkg = ge.load_package()
    s, lk = room(pkg, (1, (-2.2, 1.7, 0.0), (0, 0, 0), (3, 3, 3), (0.95, 0.95, 0.95), 0.0), (0, (2.2, 1.7, 0.0), (0, 30, 0), (3, 3, 3), (0.9, 0.95, 1.0), 0.0),
                 block=False)
    return s, lk, gm.table(7, g5=(0.0, 1.0, 1.5, (0.9, 0.8, 0.7)), g6=(0.0, 1.0, 1.5, (0.7, 0.8, 0.9)))


@functools.lru_cache(maxsize=None)
def _mirror_partial():
    """The f16 room with its block: the floor (id 0) reflects with probability 0.5 and a red spec, the back wall (id 1) always."""
    import __graft_entry__ as ge
    s, lk = room(ge.load_package())
    return s, lk, gm.table(6, g0=(0.5, 0.0, 1.0, (0.9, 0.3, 0.3)), g1=(1.0, 0.0, 1.0, (0.9, 0.9, 0.9)))


@functools.lru_cache(maxsize=None)
def mirror_mesh():
    """f19's textured mesh over a floor primitive: every mesh id gets a mirror lobe of probability 0.6 and, as a scene file would give
    it, a refract > 0 that the draw has to ignore on triangles; the floor is a full mirror, so that paths reach the mesh again."""
    s, lk = textured_floor()
    ids = sorted(set(np.asarray(s["tri_ids"]).tolist()))
    floor = int(s["geom_ids"][-1]) if s["geom_ids"] is not None else len(s["geoms"]) - 1
    n = max(ids + [floor]) + 1
    entries = {f"g{i}": (0.6, 1.0, 1.5, (0.8, 0.9, 1.0)) for i in ids}
    entries[f"g{floor}"] = (0.7, 0.0, 1.0, (0.9, 0.9, 0.9))
    return s, lk, gm.table(n, **entries)


@functools.lru_cache(maxsize=None)
def _cornell():
    """The recorded cornell with the table scene.surface_table makes of its own file."""
    import __graft_entry__ as ge
    pkg = ge.load_package()
    s, lk = scene_input("rec", "cornell")
    return s, lk, pkg.scene.surface_table(pkg.scene.parse_scene(scene_text("cornell")))


@functools.lru_cache(maxsize=None)
def _mirror_hall():
    """Two full mirrors facing each other - the f16 room's back wall (id 1) and a wall behind the camera (id 5) - with a glass sphere
    (id 6) and an emitting panel that faces the back wall (id 7) between them, the room's block taken out: the chains reach the cap
    (mirror to mirror), miss (the room is open at the top and between the floor and the wall behind the camera) and end on the emitter
    (the panel's reflection in the back wall)."""
    import __graft_entry__ as ge
    z = (0, 0, 0)
    s, lk = room(ge.load_package(), (0, (0, 5, 12.0), z, (12, 10, 0.2), (0.8, 0.8, 0.7), 0.0), (1, (1.5, 2.0, -1.0), z, (2.5, 2.5, 2.5), (0.95, 0.95, 0.95), 0.0),
                 (0, (0.0, 9.0, 6.5), z, (12, 4, 0.2), (1, 1, 1), 4.0), block=False)
    return s, lk, gm.table(8, g1=(1.0, 0.0, 1.0, (0.9, 0.9, 0.9)), g5=(1.0, 0.0, 1.0, (0.9, 0.9, 0.9)), g6=(0.0, 1.0, 1.5, (0.9, 0.8, 0.7)))


@functools.lru_cache(maxsize=None)
def _rough_floor():
    """The f16 room with its diffuse block; the floor (id 0) is a full mirror (the case's roughness makes it rough)."""
    import __graft_entry__ as ge
    s, lk = room(ge.load_package())
    return s, lk, gm.table(6, g0=(1.0, 0.0, 1.0, (0.9, 0.9, 0.9)))


@functools.lru_cache(maxsize=None)
def rough_sphere():
    """glass_pair's glass pair (ids 5 and 6) with a full-mirror sphere (id 7) between and in front of them."""
    import __graft_entry__ as ge
    pkg = ge.load_package()
    s, lk = room(pkg, (1, (-2.2, 1.7, 0.0), (0, 0, 0), (3, 3, 3), (0.95, 0.95, 0.95), 0.0), (0, (2.2, 1.7, 0.0), (0, 30, 0), (3, 3, 3), (0.9, 0.95, 1.0), 0.0),
                 (1, (0.0, 1.2, 2.5), (0, 0, 0), (2, 2, 2), (0.95, 0.95, 0.95), 0.0), block=False)
    return s, lk, gm.table(8, g5=(0.0, 1.0, 1.5, (0.9, 0.8, 0.7)), g6=(0.0, 1.0, 1.5, (0.7, 0.8, 0.9)), g7=(1.0, 0.0, 1.0, (0.9, 0.9, 0.9)))


@functools.lru_cache(maxsize=None)
def _floor_from_above():
    """The rough floor seen straight down from (0, 6, 0): the ray of the central pixel of an odd-sized frame is the view direction
    (0, -1, 0) itself, so that there v is the floor's normal, Vh has no tangential part and T1 is the degenerate tangent's (1, 0, 0)."""
    s, lk, tab = _rough_floor()
    cam = dict(s["cam"], right=np.array([1, 0, 0], F), up=np.array([0, 0, -1], F), view=np.array([0, -1, 0], F), position=np.array([0, 6, 0], F))
    return dict(s, cam=cam), lk, tab


@functools.lru_cache(maxsize=None)
def cornell_rough():
    """The recorded cornell's roughness per object, scene.roughness_table's of its own file."""
    import __graft_entry__ as ge
    pkg = ge.load_package()
    return tuple(float(a) for a in pkg.scene.roughness_table(pkg.scene.parse_scene(scene_text("cornell"))))


def mesh_rough():
    tab = mirror_mesh()[2]
    return tuple(0.25 if r > 0 else 0.0 for r in tab["reflect"])


def _f19(kind, name):
    s, lk = scene_input(kind, name)
    return s, lk, None


# (scene, light kwargs, surface table or None) by name: every input of the gloss, virtual, rough and highlight suites
INPUTS = {"glass_pair": glass_pair, "mirror_partial": _mirror_partial, "mirror_mesh": mirror_mesh, "cornell": _cornell,
          "F_cube": lambda: _f19("edge", "F_cube"), "stage": lambda: _f19("made", "stage"), "bleed_ceiling": lambda: _f19("path", "bleed_ceiling"),
          "cornell_plain": lambda: _f19("rec", "cornell"), "mirror_hall": _mirror_hall, "rough_floor": _rough_floor, "rough_sphere": rough_sphere,
          "floor_from_above": _floor_from_above}
GLOSS_RECORDED = ("cornell", "cornell_plain")


@functools.lru_cache(maxsize=None)
def gloss_first(name, W, H, frame, seed, noise=0.6):
    s = INPUTS[name]()[0]
    first = sm.render(W, H, frame, *args_of(s), s["light"], seed=seed, noise=noise, fireflies=0.02 if noise else 0.0)
    em = ssm.emitter_mask(W, H, s["cam"], s["geoms"], s["geom_ids"], s["tris"], s["tri_ids"])
    emit = splm.emittance_plane(W, H, s["cam"], s["geoms"], s["geom_ids"], s["tris"], s["tri_ids"])
    for a in first + (em, emit):
        a.setflags(write=False)
    return first, em, emit


def table_of(name, table):
    """table: "own" (the input's), "empty" (no records), "diffuse" (as many records as the input's, all diffuse), None."""
    own = INPUTS[name]()[2]
    if table == "own":
        return own
    if table == "diffuse":
        return gm.table(16 if own is None else len(own))
    return np.zeros(0, gm.SURFACE_DTYPE) if table == "empty" else None


@functools.lru_cache(maxsize=None)
def gloss_model(name, W, H, J, K, R, sec=1, point=False, alt=None, frame=None, seed=None, table="own", keep_rays=False):
    """dict(color, gb, D, I, info, lt, frame, seed, tab) of scene_gloss_model.render; a recorded scene at frame 0, seed 1 unless told."""
    frame = (0 if name in GLOSS_RECORDED else FRAME) if frame is None else frame
    seed = (1 if name in GLOSS_RECORDED else SEED) if seed is None else seed
    s, lk, _ = INPUTS[name]()
    tab = table_of(name, table)
    lt = ssm.light(lk["centre"], samples=1) if point else ssm.light(lk["centre"], lk["edge_u"], lk["edge_v"], 1)
    first, em, emit = gloss_first(name, W, H, frame, seed)
    col, gb, D, I, info = gm.render(W, H, frame, *args_of(s), lt, spm.params(J, K, R, 0.15, sec), tab, seed=seed, alt=alt, first=first,      # noqa: E741
                                    emitters=em, emittance=emit, keep_rays=keep_rays)
    for a in (col, D, I):
        a.setflags(write=False)
    return dict(color=col, gb=gb, D=D, I=I, info=info, lt=lt, frame=frame, seed=seed, tab=tab)


# (name, W, H, paths, max_depth, rr_depth, shadow_secondary, point light): the gloss suite's cases, which the virtual cases build on
GLOSS_CASES = [("glass_pair", W0, H0, 4, 4, 2, 1, False), ("mirror_partial", W0, H0, 3, 3, 0, 1, True), ("mirror_mesh", W0, H0, 2, 3, 2, 1, False),
               ("cornell", 96, 96, 1, 4, 2, 1, False), ("glass_pair", W0, H0, 4, 8, 1, 1, False)]
GLOSS_QUEUED = ("glass_pair", W0, H0, 2, 3, 2, 1, False)
HALL = ("mirror_hall", W0, H0, 2, 3, 2, 1, False)
# (the gloss case, max_chain, id_offset): the virtual suite's cases, which the rough and the highlight suites hold their identities on
VCASES = [(GLOSS_CASES[0], 8, 0), (GLOSS_CASES[0], 2, 100), (GLOSS_CASES[1], 1, 100), (GLOSS_CASES[1], 8, 0), (GLOSS_CASES[2], 2, 0), (GLOSS_CASES[3], 8, 100),
          (GLOSS_CASES[3], 1, 0), (HALL, 1, 0), (HALL, 2, 100), (HALL, 8, 0)]


def gloss_what(case):
    name, W, H, J, K, R, sec, point = case
    return f"{name} {W}x{H}, {J} paths, max_depth {K}, rr_depth {R}, secondary shadow {sec}, {'point' if point else 'area'} light"


def vid(vc):
    c, mc, off = vc
    return f"{c[0]}-J{c[3]}-K{c[4]}-chain{mc}-off{off}"


def virtual_what(vc):
    return f"{gloss_what(vc[0])}, max_chain {vc[1]}, id_offset {vc[2]}"


@functools.lru_cache(maxsize=None)
def vmodel(case, max_chain, id_offset, alt=None, table="own", frame=None):
    """dict(color, gb, D, I, chain, info, first_gb, lt, frame, seed, tab): scene_virtual_model.render on the (shared, unchanged) gloss
    model of the case."""
    kw = {k: v for k, v in (("table", table), ("frame", frame)) if v != ("own" if k == "table" else None)}
    m = gloss_model(*case, **kw)                   # the keywords the gloss suite's own calls use, so that the cache is shared
    name, W, H = case[:3]
    s = INPUTS[name]()[0]
    col, gb, D, I, chain, info = vm.render(W, H, m["frame"], *args_of(s), m["lt"], None, m["tab"], vm.params(max_chain, id_offset), seed=m["seed"],      # noqa: E741
                                           alt=alt, base=(m["color"], m["gb"], m["D"], m["I"], m["info"]))
    return dict(color=col, gb=gb, D=D, I=I, chain=chain, info=info, first_gb=m["gb"], lt=m["lt"], frame=m["frame"], seed=m["seed"], tab=m["tab"])


# (name, W, H, paths, max_depth, rr_depth, shadow_secondary, point light), the roughness per object id, guide_alpha, max_chain, id_offset
def rc(name, J, K, R, rough, ga, mc=4, off=0, W=W0, H=H0, point=False):
    return ((name, W, H, J, K, R, 1, point), tuple(rough) if not callable(rough) else rough, ga, mc, off)


# the rough suite's cases, which the highlight suite holds `enable 0` on
RCASES = [rc("rough_floor", 1, 4, 2, (0.1,), 0.0), rc("rough_floor", 3, 2, 0, (0.5,), 0.3), rc("rough_floor", 3, 4, 2, (0.1,), 0.3, 4, 100),
          rc("rough_floor", 1, 1, 0, (0.5,), 1.0), rc("mirror_partial", 3, 4, 2, (0.3, 0.2), 0.3, point=True), rc("mirror_partial", 1, 2, 0, (0.3, 0.2), 0.0),
          rc("mirror_mesh", 3, 4, 2, mesh_rough, 1.0), rc("rough_sphere", 3, 4, 2, (0, 0, 0, 0, 0, 0.4, 0.4, 0.2), 0.3, 8),
          rc("rough_sphere", 1, 2, 0, (0, 0, 0, 0, 0, 0.4, 0.4, 0.2), 0.0, 8, 100), rc("mirror_hall", 1, 4, 2, (0, 0.2), 0.0, 8),
          rc("mirror_hall", 3, 2, 0, (0, 0.2), 0.3, 8, 100), rc("mirror_hall", 3, 4, 2, (0, 0.2, 0, 0, 0, 0.6), 0.3, 2),
          rc("mirror_hall", 1, 1, 0, (0, 0.2, 0, 0, 0, 0.6), 1.0, 8), rc("cornell", 1, 4, 2, cornell_rough, 0.0, 4, 0, 96, 96),
          rc("cornell", 1, 4, 2, cornell_rough, 1.0, 4, 0, 96, 96)]
# the exception of the rough suite's coverage: the degenerate tangent occurs on one pixel of a case made for it
ABOVE = rc("floor_from_above", 8, 2, 0, (0.5,), 0.0, W=7, H=5)


def rough_of(case):
    r = case[1]() if callable(case[1]) else case[1]
    return None if r is None else np.asarray(r, F)


def rid(c):
    c, r, ga, mc, off = c
    return f"{c[0]}-{c[1]}x{c[2]}-J{c[3]}-K{c[4]}-R{c[5]}-ga{ga}-chain{mc}-off{off}-{'fn' if callable(r) else 'a' + '_'.join(str(a) for a in r)}"


def rough_what(c):
    r = rough_of(c)
    return f"{gloss_what(c[0])}, roughness {None if r is None else [float(a) for a in r]}, guide_alpha {c[2]}, max_chain {c[3]}, id_offset {c[4]}"


@functools.lru_cache(maxsize=None)
def _rough_base(case, rough, alt=None, frame=None, table="own"):
    """What does not depend on the guide: scene_gloss_model.render's results with the roughness table, on the gloss suite's
    (shared, unchanged) first hits."""
    name, W, H, J, K, R, sec, point = case
    frame = (0 if name in ("cornell",) else FRAME) if frame is None else frame
    seed = 1 if name in ("cornell",) else SEED
    s, lk, _ = INPUTS[name]()
    tab = table_of(name, table)
    lt = ssm.light(lk["centre"], samples=1) if point else ssm.light(lk["centre"], lk["edge_u"], lk["edge_v"], 1)
    first, em, emit = gloss_first(name, W, H, frame, seed)
    r = None if rough is None else np.asarray(rough() if callable(rough) else rough, F)
    out = rm.render(W, H, frame, *args_of(s), lt, spm.params(J, K, R, 0.15, sec), tab, None, r, 0.0, seed=seed, alt=alt, first=first, emitters=em,
                    emittance=emit)
    return dict(base=(out[0], out[5]["first_gb"], out[2], out[3], out[5]), lt=lt, frame=frame, seed=seed, tab=tab, rough=r)


@functools.lru_cache(maxsize=None)
def rmodel(case, rough, ga, mc, off, alt=None, frame=None, table="own"):
    """dict(color, gb, D, I, chain, info, lt, frame, seed, tab, rough) of scene_rough_model.render."""
    b = _rough_base(case, rough, None if alt == "guide_alpha_compared_the_wrong_way" else alt, frame, table)
    name, W, H = case[:3]
    s = INPUTS[name]()[0]
    info0 = {k: v for k, v in b["base"][4].items() if k not in ("guide", "first_gb", "guide_events")}
    col, gb, D, I, chain, info = rm.render(W, H, b["frame"], *args_of(s), b["lt"], None, b["tab"], vm.params(mc, off), b["rough"], ga, seed=b["seed"],      # noqa: E741
                                           alt=alt, base=b["base"][:4] + (info0,))
    return dict(b, color=col, gb=gb, D=D, I=I, chain=chain, info=info)


def disc_points(n, rng):
    p = rng.uniform(-1, 1, (4 * n, 2))
    p = p[(p * p).sum(1) < 1][:n]
    assert len(p) == n, "too few points fell inside the disc"
    return p[:, 0].copy(), p[:, 1].copy()


def view_dir(c, n):
    """A direction d with v.n = c about the normal n, off the frame's axes."""
    T, B = rm.frame_of([np.array([x]) for x in n], np.float64)
    s = np.sqrt(1 - c * c)
    v = [s * (0.6 * T[k][0] + 0.8 * B[k][0]) + c * n[k] for k in range(3)]
    return [-x for x in v]


# ---- the draw families: one record each, one draw, one comparison -----------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Family:
    """A draw family: the Scene method of its plain and of its split form, the keyword parameters a case may set, and whether it takes
    a GlossTable, writes a chain plane, takes a RoughTable."""
    name: str
    plain: str
    split: str = None
    params: tuple = ()
    table: bool = False
    chain: bool = False
    rough: bool = False


_SYNTH = ("noise",)                       # fireflies follow it: 0.02 with noise, 0 without
_TRACE = _SYNTH + ("bounce_samples", "ambient", "shadow_secondary")
_PATH = _SYNTH + ("paths", "max_depth", "rr_depth", "ambient", "shadow_secondary")
_GUIDE, _LOBE, _SHINE = ("max_chain", "id_offset"), ("guide_alpha",), ("enable", "clamp")
RESIDENT = Family("resident", "draw")
SHADOWED = Family("shadowed", "draw_shadowed", params=_SYNTH)
TRACED = Family("traced", "draw_traced", "draw_traced_split", _TRACE)
PATH = Family("path", "draw_path", "draw_path_split", _PATH)
GLOSS = Family("gloss", "draw_gloss", "draw_gloss_split", _PATH, table=True)
VIRTUAL = Family("virtual", "draw_virtual", "draw_virtual_split", _PATH + _GUIDE, table=True, chain=True)
ROUGH = Family("rough", "draw_rough", "draw_rough_split", _PATH + _GUIDE + _LOBE, table=True, chain=True, rough=True)
HIGHLIGHT = Family("highlight", "draw_highlight", "draw_highlight_split", _PATH + _GUIDE + _LOBE + _SHINE, table=True, chain=True, rough=True)


def trace_args(J, sec=1, **more):
    return dict(bounce_samples=J, shadow_secondary=sec, **more)


def path_args(J, K, R, sec=1, **more):
    return dict(paths=J, max_depth=K, rr_depth=R, shadow_secondary=sec, **more)


def draw_buffers(fam, W, H, split=False, rgb=True, chain=True):
    """The device outputs of one draw: color and gb, D and I for the split form (color None with rgb False), chain where the family
    has one (None with chain False)."""
    if split:
        b = split_buffers(W, H, rgb)
    else:
        b = dict(zip(("color", "gb"), buffers(W, H)))
    if fam.chain:
        b["chain"] = chain_buffer(W, H) if chain else None
    return b


def to_host(pkg, b, W, H, planes=None):
    """draw_buffers' tensors on the host; the G-buffer from `planes` where the draw went there."""
    out = {k: (None if t is None else t.cpu().numpy()) for k, t in b.items() if k != "gb"}
    out["gb"] = read_planes(pkg, planes, W, H) if planes is not None else b["gb"].cpu().numpy().view(pkg.synth.GBUFFER_DTYPE).reshape(H, W)
    return out


def draw(pkg, fam, scene, W, H, s, lt, args=None, *, split=False, rgb=True, chain=True, frame=FRAME, seed=SEED, stream=None, bufs=None, sync=True,
         planes=None, tables=None):
    """One draw of a family.  `args`: the family's own parameters by the binding's keyword names (Family.params); `tables`: dict(table
    =GlossTable or None, rough=RoughTable or None) where the family takes them; `lt`: the model's light (the resident draw takes the
    scene's point light instead); `bufs`: draw_buffers' dict to draw into (a fresh one otherwise); `planes`: a context's planar
    G-buffer as the target in the texels' place.  Returns to_host's dict, or None with sync False."""
    import torch
    args, tables = dict(args or {}), dict(tables or {})
    unknown = set(args) - set(fam.params)
    assert not unknown, f"{fam.name} draw: no parameter {sorted(unknown)}"
    assert set(tables) <= ({"table"} if fam.table else set()) | ({"rough"} if fam.rough else set()), f"{fam.name} draw: takes no {sorted(tables)}"
    b = bufs or draw_buffers(fam, W, H, split, rgb, chain)
    noise = args.pop("noise", 0.6)
    kw = dict(args, seed=seed, noise=noise, fireflies=0.02 if noise else 0.0, stream=stream, **tables)
    if fam.chain:
        kw["out_chain"] = b["chain"]
    target = planes if planes is not None else b["gb"]
    source = s["light"] if fam is RESIDENT else light(pkg, lt)
    if split:
        assert fam.split, f"the {fam.name} family has no split form"
        getattr(scene, fam.split)(b["D"], b["I"], target, W, H, s["cam"], source, frame, out_rgb=b["color"], **kw)
    else:
        getattr(scene, fam.plain)(b["color"], target, W, H, s["cam"], source, frame, **kw)
    if not sync:
        return None
    torch.cuda.synchronize()
    return to_host(pkg, b, W, H, planes)


def pair(got):
    """(colour, G-buffer) of a draw's result: what test_scene_model.counts and the capped comparison take."""
    return got["color"], got["gb"]


def draw_frame(pkg, scene, W, H, s, frame, seed):
    """The resident draw's frame as a (colour, G-buffer) pair."""
    return pair(draw(pkg, RESIDENT, scene, W, H, s, None, frame=frame, seed=seed))


def split_counts(got, ref, rgb=True):
    c = counts((got["color"] if rgb else ref["color"], got["gb"]), (ref["color"], ref["gb"]))
    if not rgb:
        del c["color"]
    c["direct"] = int(np.count_nonzero(differing(got["D"], ref["D"])))
    c["indirect"] = int(np.count_nonzero(differing(got["I"], ref["I"])))
    return c


def chain_counts(m, ref):
    c = split_counts(m, ref)
    c["chain"] = int((m["chain"] != ref["chain"]).sum())
    return c


def same(got, model, what, split=False, rgb=True, chain=True):
    """A draw's result (or a model's frame) against a model or another draw, dicts or (colour, G-buffer) pairs: colour and every
    G-buffer field, D and I for the split form, and the chain plane where the draw wrote one (chain False: the reference is of a family
    without it).  Expected and allowed number of differences: 0."""
    got, ref = (x if isinstance(x, dict) else dict(color=x[0], gb=x[1]) for x in (got, model))
    c = split_counts(got, ref, rgb) if split else counts(pair(got), pair(ref))
    print(f"{what}: differing pixels {c} (expected and allowed: 0)")
    assert not any(c.values()), f"{what}: {c}"
    if chain and got.get("chain") is not None:
        assert ref.get("chain") is not None, f"{what}: the reference carries no chain plane"
        bad = int((got["chain"] != ref["chain"]).sum())
        print(f"{what}: differing chain counts {bad} (expected and allowed: 0)")
        assert got["chain"].dtype == np.int32 and bad == 0, f"{what}: chain differs on {bad} pixels"


def same_capped(got, ref, W, H, what):
    """The resident and the animated suite's comparison of (colour, G-buffer) pairs: expected 0, allowed test_scene_model.cap(W, H)."""
    c = counts(got, ref)
    print(f"{what} {W}x{H}: differing pixels {c} (expected 0, cap {cap(W, H)})")
    for f, k in c.items():
        assert k <= cap(W, H), f"{what} {W}x{H}: {f} differs on {k} pixels"


# ---- the GPU test bodies every family repeats --------------------------------------------------------------------------------------------
def case(s, W, H, lt, args=None, frame=FRAME, seed=SEED, tab=None, rough=None):
    """What the bodies below draw: the scene dict, the size, the model's light, the family's parameters, and the host-side surface
    table and roughness array of the families that take them."""
    return dict(s=s, W=W, H=H, lt=lt, args=args or {}, frame=frame, seed=seed, tab=tab, rough=rough)


def gloss_case(c, m, **more):
    """case() of a (name, W, H, paths, max_depth, rr_depth, shadow_secondary, point light) tuple and its model, which carries the
    light, frame, seed, surface table and roughness; `more`: the parameters the later families add."""
    name, W, H, J, K, R, sec, point = c
    return case(INPUTS[name]()[0], W, H, m["lt"], path_args(J, K, R, sec, **more), m["frame"], m["seed"], m["tab"], m.get("rough"))


def tables_of(pkg, fam, c):
    t = {}
    if fam.table:
        t["table"] = None if c["tab"] is None else pkg.GlossTable(c["tab"])
    if fam.rough:
        t["rough"] = None if c["rough"] is None else pkg.RoughTable(c["rough"])
    return t


def draw_case(pkg, fam, c, **kw):
    """One draw of a case on a scene and tables of its own."""
    scene, tb = create(pkg, c["s"]), tables_of(pkg, fam, c)
    try:
        return draw(pkg, fam, scene, c["W"], c["H"], c["s"], c["lt"], c["args"], frame=c["frame"], seed=c["seed"], tables=tb, **kw)
    finally:
        free(*tb.values())
        scene.free()


def check_planar_target(pkg, fam, c, model, what, forms=(False,), rgb=True):
    """The case drawn into a context's planar G-buffer, plain form and / or split form (`forms`: split False / True)."""
    W, H = c["W"], c["H"]
    scene, tb = create(pkg, c["s"]), tables_of(pkg, fam, c)
    den = pkg.Denoiser(W, H, 0)
    try:
        for split in forms:
            got = draw(pkg, fam, scene, W, H, c["s"], c["lt"], c["args"], split=split, rgb=rgb, frame=c["frame"], seed=c["seed"], tables=tb,
                       planes=den.planar_gbuffer())
            same(got, model, what + (", split form" if split and len(forms) > 1 else ""), split=split, rgb=rgb)
    finally:
        den.free()
        free(*tb.values())
        scene.free()


def check_every_tree(pkg, fam, c, model, name):
    tb = tables_of(pkg, fam, c)
    try:
        for ml, sp in BUILDS:
            scene = create(pkg, c["s"], ml, sp)
            got = draw(pkg, fam, scene, c["W"], c["H"], c["s"], c["lt"], c["args"], frame=c["frame"], seed=c["seed"], tables=tb)
            scene.free()
            same(got, model, f"{name}, leaf {ml} split {sp}")
    finally:
        free(*tb.values())


def check_queued(pkg, fam, c, model_of_frame, what, n=8, split=False, own_stream=True):
    """n draws of frames 0 .. n - 1 queued on one stream without a host wait between them, each into buffers of its own."""
    import torch
    W, H = c["W"], c["H"]
    scene, tb = create(pkg, c["s"]), tables_of(pkg, fam, c)
    st = open_stream(own_stream)
    bufs = [draw_buffers(fam, W, H, split) for _ in range(n)]
    torch.cuda.synchronize()
    for f, b in enumerate(bufs):
        draw(pkg, fam, scene, W, H, c["s"], c["lt"], c["args"], split=split, frame=f, seed=c["seed"], stream=st, bufs=b, sync=False, tables=tb)
    st.close()
    try:
        for f, b in enumerate(bufs):
            same(to_host(pkg, b, W, H), model_of_frame(f), f"{what}, frame {f}", split=split)
    finally:
        free(*tb.values())
        scene.free()


def check_captured(pkg, fam, c, model, what, split=False, own_stream=True):
    """The draw once eagerly (a first launch may set kernel attributes), then captured: one kernel node, and its replay into zeroed
    buffers gives the model's bits."""
    import torch
    W, H = c["W"], c["H"]
    scene, tb = create(pkg, c["s"]), tables_of(pkg, fam, c)
    st = open_stream(own_stream)
    b = draw_buffers(fam, W, H, split)
    torch.cuda.synchronize()
    record = lambda: draw(pkg, fam, scene, W, H, c["s"], c["lt"], c["args"], split=split, frame=c["frame"], seed=c["seed"], stream=st, bufs=b,      # noqa: E731
                          sync=False, tables=tb)
    record()
    st.synchronize()
    cap_ = Captured(st, record)
    with torch.cuda.stream(st.torch):
        for t in b.values():
            t.zero_()
    cap_.launch()
    st.synchronize()
    got = to_host(pkg, b, W, H)
    cap_.destroy()
    st.close()
    free(*tb.values())
    scene.free()
    print(f"captured {what} (split {split}) = node types {cap_.types}")
    assert cap_.types == [0], f"captured {what}: node types {cap_.types}, expected one kernel node"
    same(got, model, f"replayed {what}", split=split)


def check_common_refusals(B, f, params=None):
    """The refusals every draw entry point shares.  f(**overrides) calls it with valid arguments but for the overrides h (scene), gb
    (texels), pl (planes), w, hh, cm (camera), spp (synth params), lt (light), t (the trace / path parameter block).  params: (the
    block's ctypes class, the family's list of bad blocks), or None where the entry point takes none."""
    planes = ctypes.byref(B.SvgfPlanarGBuffer())
    nan_light = B.SvgfSceneLight.make((0, 1, 0), samples=1)
    nan_light.edge_v[2] = float("nan")
    refused = [dict(h=None), dict(w=0), dict(hh=-1), dict(cm=None), dict(spp=None), dict(lt=None), dict(gb=None), dict(pl=planes), dict(gb=None, pl=planes)]
    refused += [dict(lt=ctypes.byref(B.SvgfSceneLight.make((0, 1, 0), samples=n))) for n in (0, 65)] + [dict(lt=ctypes.byref(nan_light))]
    what = ["h NULL", "width 0", "height -1", "camera NULL", "synth params NULL", "light NULL", "no target", "both targets", "empty planes",
            "0 light samples", "65 light samples", "a NaN in the light"]
    if params is not None:
        block, bad = params
        refused += [dict(t=None)] + [dict(t=ctypes.byref(block(*v))) for v in bad]
        what += ["parameter block NULL"] + [f"parameter block {v}" for v in bad]
    for name, kw in zip(what, refused):
        rc_ = f(**kw)
        assert rc_ == -1, f"{name}: {rc_}, expected -1"
    rc_ = f(w=1 << 14, hh=1 << 13)                     # width * height == 2^31 / 16
    assert rc_ == -5, f"2^14 x 2^13: {rc_}, expected -5 (SVGF_ERR_UNSUPPORTED)"


def compose_on_device(pkg, got, W, H):
    """svgf_trace_compose of a split draw's host result, back on the host."""
    import torch
    d, i = torch.from_numpy(got["D"]).cuda(), torch.from_numpy(got["I"]).cuda()
    tex = torch.from_numpy(np.ascontiguousarray(got["gb"]).view(np.uint8).reshape(-1).copy()).cuda()
    out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    pkg.trace_compose(out, d, i, tex, W, H)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def run_split_denoise_compose(pkg, orc, fam, models, W, H, args, what, tab=None, rough=None, form="checked"):
    """The closing sequence on the turning block, frame f drawn with frame number f and seed 3: pose -> the family's split draw (no
    out_rgb) -> svgf_denoise of D and of I each in a context of its own (sepcolor 1 / addcolor 0, the temporal pass alone, so that
    temporal_model.py is the whole filter) -> svgf_trace_compose.  The composed image is compose() of the two outputs, and every state
    of both contexts after every frame is temporal_model.run_sequence's fed the models' D (or I) and G-buffer, on bits.
    Two forms.  "checked" (virtual, rough, highlight): each frame's draw is waited for and held to its model.  "filtered" (split,
    path): the draw is not waited for, the pose's motion rows are both contexts' object motion table (and the model's), and the f8
    firefly filter of rank 2 is on the indirect context (tests/firefly_model.py filters the model's input).  what: (label of D, label of I)
    for the failure messages.  Returns (states, reference), each per term."""
    import torch
    import firefly_model as fm
    from temporal_harness import assert_frames_equal, read_states, scales, synth_params
    assert form in ("checked", "filtered"), f"no form {form!r}"
    filtered = form == "filtered"
    N = len(models)
    s, tables = block_inputs()
    tables = tables[:N]
    rows = block_motion(pkg, tables) if filtered else None
    lt = models[0]["lt"]
    views = [orc.view_matrix(pkg, s["cam"])] * N
    p = synth_params(pkg, W, H, sepcolor=1, addcolor=0)
    ranks = {"D": 0, "I": 2 if filtered else 0}
    ref = {}
    for key, rank in ranks.items():
        fed = [(fm.firefly_filter(np.asarray(m[key], F).reshape(H, W, 3), rank, 1.0), m["gb"].reshape(H, W)) for m in models]
        ref[key] = tm.run_sequence(fed, tables=rows, views=views, scale=scales(pkg, W, H))
    check_draw = not filtered
    scene = create(pkg, s)
    scene.enable_pose(len(s["geoms"]))
    tb = tables_of(pkg, fam, dict(tab=tab, rough=rough))
    dens = {"D": pkg.Denoiser(W, H), "I": pkg.Denoiser(W, H)}
    t_x = motion_buffer(len(s["geoms"])) if filtered else None
    for key, den in dens.items():
        den.set_capture(True)
        if filtered:
            den.set_object_motion(t_x)
            den.set_firefly_filter(ranks[key], 1.0)
    b = draw_buffers(fam, W, H, split=True, rgb=False)
    outs = {k: torch.empty((H, W, 3), dtype=torch.float32, device="cuda") for k in ("D", "I", "C")}
    states = {"D": [], "I": []}
    try:
        for f in range(N):
            scene.pose(dev(tables[f]), t_x)
            got = draw(pkg, fam, scene, W, H, s, lt, args, split=True, rgb=False, frame=f, seed=3, bufs=b, sync=check_draw, tables=tb)
            if check_draw:
                same(got, models[f], f"frame {f}", split=True, rgb=False)
            for key, den in dens.items():
                den.denoise(outs[key], b[key], b["gb"], s["cam"], p)
            pkg.trace_compose(outs["C"], outs["D"], outs["I"], b["gb"], W, H)
            torch.cuda.synchronize()
            for key, den in dens.items():
                states[key].append(read_states(den))
            alb = (models[f]["gb"]["albedo"] * models[f]["gb"]["ialbedo"]).astype(F)
            want = splm.compose(alb, outs["D"].cpu().numpy(), outs["I"].cpu().numpy())
            assert not differing(outs["C"].cpu().numpy(), want).any(), f"frame {f}: the composed image"
    finally:
        for den in dens.values():
            den.free()
        free(*tb.values())
        scene.free()
    for key, label in zip(("D", "I"), what):
        assert_frames_equal(states[key], ref[key], label)
    return states, ref
