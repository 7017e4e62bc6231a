"""libsvgf_deform.so (include/svgf_deform.h, row f26): skinned triangles in a resident scene - per frame a bone table deforms the
triangles as drawn, and the previous frame's positions become the per-pixel previous position svgf_motion_reproject takes.  Built by
the companions' recipe (build.SCENE_WRITERS), loaded like them (binding._load_linked), no companion draw.  The two product entry
points the library needs (include/svgf_scene_write.h: svgf_scene_drawn_arrays, svgf_scene_refit) are declared here too, on the product
library's handle; binding.py's pinned tables stay as they are.  The wrapper mirrors sah.SahTree."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import binding as _b

DEFORM_READ_CUR, DEFORM_READ_PREV, DEFORM_READ_SLOT = 0, 1, 2
DEFORM_MAX_BONES = 1024


class SvgfDeformInfo(C.Structure):
    _fields_ = [("n_tris", C.c_int), ("n_skinned", C.c_int), ("n_bones", C.c_int), ("launches", C.c_int), ("device_bytes", C.c_ulonglong)]


# every symbol include/svgf_deform.h declares
_DEFORM_PROTOTYPES = {
    "svgf_deform_check_rig_host": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]),
    "svgf_deform_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "svgf_deform_apply": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "svgf_deform_prev_positions": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(_b.SvgfCamera), C.POINTER(C.c_float),
                                             C.c_void_p]),
    "svgf_deform_info": (C.c_int, [C.c_void_p, C.POINTER(SvgfDeformInfo)]),
    "svgf_deform_read": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_ulonglong]),
    "svgf_deform_destroy": (None, [C.c_void_p]),
    "svgf_deform_version": (C.c_int, None),
}
DEFORM_EXPORTS = list(_DEFORM_PROTOTYPES)
# every symbol include/svgf_scene_write.h declares (libsvgf_hip.so)
_SCENE_WRITE_PROTOTYPES = {
    "svgf_scene_drawn_arrays": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "svgf_scene_refit": (C.c_int, [C.c_void_p, C.c_void_p]),
}
SCENE_WRITE_EXPORTS = list(_SCENE_WRITE_PROTOTYPES)


def load_deform_library():
    """libsvgf_deform.so (row f26)."""
    return _b._load_linked("deform", lambda name: _DEFORM_PROTOTYPES)


def _product():
    """The product library with the two row-f26 prototypes declared on it; a library that lacks them is an error."""
    lib = _b.load_library()
    if getattr(lib.svgf_scene_refit, "argtypes", None) is None:
        _b._declare(lib, _SCENE_WRITE_PROTOTYPES)
    return lib


def scene_refit(scene, stream=None):
    """svgf_scene_refit: the two refit launches of svgf_scene_pose on the scene's own nodes, from the boxes as drawn.  Asynchronous."""
    _b._call(_product(), "svgf_scene_refit", scene.h, _b._stream(stream))


def drawn_arrays(scene) -> tuple[int, int]:
    """svgf_scene_drawn_arrays (host only): the writable device pointers (triangles, padded boxes) of a posed scene, as integers."""
    t, b = C.c_void_p(), C.c_void_p()
    _b._call(_product(), "svgf_scene_drawn_arrays", scene.h, C.byref(t), C.byref(b))
    return int(t.value or 0), int(b.value or 0)


def rig_arrays(tri_index, bone, weight):
    """The three rig arrays in the layout the library takes: int32[n], uint16[n, 3, 4], float32[n, 3, 4]."""
    ti = np.ascontiguousarray(tri_index, dtype=np.int32).reshape(-1)
    return ti, np.ascontiguousarray(bone, dtype=np.uint16).reshape(len(ti), 3, 4), np.ascontiguousarray(weight, dtype=np.float32).reshape(len(ti), 3, 4)


def check_rig_host(n_tris: int, tri_index, bone, weight, n_bones: int) -> int:
    """svgf_deform_check_rig_host (no device needed): the return code, 0 for a rig svgf_deform_create accepts."""
    ti, bo, we = rig_arrays(tri_index, bone, weight)
    return int(load_deform_library().svgf_deform_check_rig_host(int(n_tris), ti.ctypes.data, len(ti), bo.ctypes.data, we.ctypes.data, int(n_bones)))


class DeformRig:
    """Skinned triangles of a posed resident scene (libsvgf_deform.so, row f26): create once (one allocation; not under capture) before
    anything deforms the scene, apply(bones, stream) per frame behind the pose - one launch, legal under capture - then a tree
    (scene_refit, SceneTree.build or SahTree.build), the draw, and prev_positions(...) for svgf_motion_reproject.  free() before the
    scene's.  Usable as a context manager."""

    def __init__(self, scene, tri_index, bone, weight, n_bones: int):
        self.lib, self.scene, self.h, self.n_bones = load_deform_library(), scene, None, int(n_bones)
        ti, bo, we = rig_arrays(tri_index, bone, weight)
        h = C.c_void_p()
        _b._call(self.lib, "svgf_deform_create", scene.h, ti.ctypes.data, len(ti), bo.ctypes.data, we.ctypes.data, self.n_bones, C.byref(h))
        self.h = h

    def _call(self, symbol, *args):
        _b._call(self.lib, symbol, self.h, *args)

    def apply(self, bones, stream=None):
        """svgf_deform_apply: `bones` is DEVICE memory of n_bones SCENE_POSE_DTYPE records (a torch tensor of 24 * n_bones float32 or a
        raw pointer), read when the kernel runs.  Asynchronous on `stream`; never waits."""
        self._call("svgf_deform_apply", _b._ptr(bones), self.n_bones, _b._stream(stream))

    def prev_positions(self, out_prev_pos, out_geom_id, width: int, height: int, camera, pixel_length=None, stream=None):
        """svgf_deform_prev_positions: device float32[width * height * 3] and int32[width * height] (or None).  pixel_length defaults
        as Scene.draw's does."""
        cam, sp = _b._view(camera, width, height, 0, 0, 0.0, 0.0, pixel_length, camera_fovy=True)
        self._call("svgf_deform_prev_positions", _b._ptr(out_prev_pos), _b._ptr(out_geom_id), int(width), int(height), C.byref(cam), sp.pixel_length,
                   _b._stream(stream))

    def info(self) -> dict:
        i = SvgfDeformInfo()
        self._call("svgf_deform_info", C.byref(i))
        return {k: int(getattr(i, k)) for k, _ in SvgfDeformInfo._fields_}

    def read(self, which: int) -> np.ndarray:
        """svgf_deform_read (blocking): 0 cur float32[n_skinned, 3, 3], 1 prev the same, 2 slot int32[n_tris]."""
        i = self.info()
        out = np.zeros(i["n_tris"], np.int32) if int(which) == 2 else np.zeros((i["n_skinned"], 3, 3), np.float32)
        self._call("svgf_deform_read", int(which), out.ctypes.data, out.nbytes)
        return out

    def free(self):
        if self.h:
            self.lib.svgf_deform_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


def tube_rig(segments: int = 12, sides: int = 10, length: float = 4.0, radius: float = 0.25, base=(0.0, 0.0, 0.0)):
    """A tube that stands on `base` along +y, and a two-bone rig for it: (tris float32[n, 3, 8], bone uint16[n, 3, 4], weight
    float32[n, 3, 4]) with n = 2 * segments * sides, outward windings and normals, uv = (angle, height) in 0..1.  Bone 0 holds the
    lower third, bone 1 the upper third, and the weights cross over linearly between them; influences 2 and 3 are bone 0 at weight 0."""
    F = np.float32
    ang = np.arange(sides + 1, dtype=np.float64) * (2.0 * np.pi / sides)
    hgt = np.arange(segments + 1, dtype=np.float64) / segments

    def vertex(i, j):
        n = (np.cos(ang[i % sides]), 0.0, np.sin(ang[i % sides]))
        p = (base[0] + radius * n[0], base[1] + length * hgt[j], base[2] + radius * n[2])
        w1 = F(min(max((hgt[j] - 1.0 / 3.0) * 3.0, 0.0), 1.0))
        return np.array(p + n + (i / sides, hgt[j]), F), (F(1.0) - w1, w1, F(0.0), F(0.0))
    tris, weight = [], []
    for j in range(segments):
        for i in range(sides):
            a, b, c, d = vertex(i, j), vertex(i + 1, j), vertex(i + 1, j + 1), vertex(i, j + 1)
            for corners in ((a, d, b), (b, d, c)):
                tris.append(np.stack([v for v, _ in corners]))
                weight.append(np.array([w for _, w in corners], F))
    tris, weight = np.stack(tris), np.stack(weight)
    bone = np.zeros(weight.shape, np.uint16)
    bone[:, :, 1] = 1
    return tris, bone, weight


def bend_bones(angle_rad: float, pivot, axis=(0.0, 0.0, 1.0)) -> np.ndarray:
    """The two-bone table of tube_rig: SCENE_POSE_DTYPE[2], bone 0 the identity, bone 1 a rotation by angle_rad about `axis` through
    `pivot` (svgf_pose_rigid)."""
    t = _b.pose_identity(2)
    t[1] = _b.pose_rigid(axis, float(angle_rad), pivot, (0.0, 0.0, 0.0))
    return t
