"""libsvgf_sah.so (include/svgf_sah.h, row f25): svgf_bvh_build_host's binned-SAH tree over a resident scene's triangles as drawn,
built on the device.  Built by the companions' recipe (build.TREE_BUILDERS), loaded like them (binding._load_linked), no companion
draw.  The wrapper mirrors binding.SceneTree (row f24)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import binding as _b

SAH_READ_RECORDS, SAH_READ_ORDER, SAH_READ_COUNTS = 0, 1, 2
SAH_SMALL = 256


class SvgfSahParams(C.Structure):
    _fields_ = [("max_leaf_tris", C.c_int)]


class SvgfSahInfo(C.Structure):
    _fields_ = [("n_tris", C.c_int), ("max_leaf_tris", C.c_int), ("n_records", C.c_int), ("depth_bound", C.c_int), ("launches", C.c_int),
                ("device_bytes", C.c_ulonglong)]


class SvgfSahCounts(C.Structure):
    _fields_ = [("n_nodes", C.c_int), ("n_leaves", C.c_int), ("depth", C.c_int), ("forced_splits", C.c_int)]


# every symbol include/svgf_sah.h declares
_SAH_PROTOTYPES = {
    "svgf_sah_create": (C.c_int, [C.c_void_p, C.POINTER(SvgfSahParams), C.POINTER(C.c_void_p)]),
    "svgf_sah_build": (C.c_int, [C.c_void_p, C.c_void_p]),
    "svgf_sah_attach": (C.c_int, [C.c_void_p, C.c_void_p]),
    "svgf_sah_info": (C.c_int, [C.c_void_p, C.POINTER(SvgfSahInfo)]),
    "svgf_sah_read": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_ulonglong]),
    "svgf_sah_destroy": (None, [C.c_void_p]),
    "svgf_sah_version": (C.c_int, None),
}
SAH_EXPORTS = list(_SAH_PROTOTYPES)


def load_sah_library():
    """libsvgf_sah.so (row f25)."""
    return _b._load_linked("sah", lambda name: _SAH_PROTOTYPES)


class SahTree:
    """The tree svgf_scene_create would build from a resident scene's triangles as they are drawn now, built on the device by
    libsvgf_sah.so (row f25): create once (one allocation; not under capture), build(stream) per frame behind the pose -
    info()["launches"] kernel launches and nothing else, legal under capture - attach() once, detach() before free().  Usable as a
    context manager."""

    def __init__(self, scene, max_leaf_tris: int = 0):
        self.lib, self.scene, self.h = load_sah_library(), scene, None
        h, p = C.c_void_p(), SvgfSahParams(int(max_leaf_tris))
        _b._call(self.lib, "svgf_sah_create", scene.h, C.byref(p), C.byref(h))
        self.h = h

    def _call(self, symbol, *args):
        _b._call(self.lib, symbol, self.h, *args)

    def build(self, stream=None):
        """svgf_sah_build: asynchronous on `stream`; never waits."""
        self._call("svgf_sah_build", _b._stream(stream))

    def attach(self):
        self._call("svgf_sah_attach", self.scene.h)

    def detach(self):
        self.scene.adopt_tree(None)

    def info(self) -> dict:
        i = SvgfSahInfo()
        self._call("svgf_sah_info", C.byref(i))
        return {k: int(getattr(i, k)) for k, _ in SvgfSahInfo._fields_}

    def read(self, which: int) -> np.ndarray:
        """svgf_sah_read (blocking): 0 records BVH_NODE_DTYPE[2 n_tris - 1], 1 order int32[n_tris], 2 the four counts int32[4]."""
        i = self.info()
        n, dt = {0: (i["n_records"], _b.BVH_NODE_DTYPE), 1: (i["n_tris"], np.int32), 2: (4, np.int32)}[int(which)]
        out = np.zeros(n, dt)
        self._call("svgf_sah_read", int(which), out.ctypes.data, out.nbytes)
        return out

    def counts(self) -> dict:
        """SvgfSahCounts of the last build (blocking): n_nodes, n_leaves, depth, forced_splits."""
        c = self.read(SAH_READ_COUNTS)
        return {k: int(v) for (k, _), v in zip(SvgfSahCounts._fields_, c)}

    def free(self):
        if self.h:
            self.lib.svgf_sah_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
