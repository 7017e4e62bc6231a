"""libsvgf_restir.so (include/svgf_restir.h, row f27): many-light direct lighting of a resident scene's G-buffer by reservoir
resampling - a table of parallelogram lights, a per-size state of two reservoir planes, two launches per frame that write the
demodulated direct term D, and the all-lights truth it is scored against.  Built by the companions' recipe (build.LIGHT_SAMPLERS),
loaded like them (binding._load_linked), no companion draw; binding.py's pinned tables stay as they are.  The wrappers mirror
deform.DeformRig and binding's device tables."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import binding as _b

RESTIR_READ_H, RESTIR_READ_T, RESTIR_READ_PREV_NORMAL, RESTIR_READ_PREV_ID = 0, 1, 2, 3
RESTIR_MAX_LIGHTS, RESTIR_MAX_CANDIDATES, RESTIR_MAX_NEIGHBOURS = 65536, 32, 8
LIGHT_DTYPE = np.dtype([("centre", np.float32, 3), ("edge_u", np.float32, 3), ("edge_v", np.float32, 3), ("power", np.float32, 3)])
RESERVOIR_DTYPE = np.dtype([("j", np.int32), ("u", np.float32), ("v", np.float32), ("M", np.float32), ("W", np.float32), ("phat", np.float32),
                            ("zero", np.int32, 2)])


class SvgfLight(C.Structure):
    _fields_ = [("centre", C.c_float * 3), ("edge_u", C.c_float * 3), ("edge_v", C.c_float * 3), ("power", C.c_float * 3)]


class SvgfRestirParams(C.Structure):
    _fields_ = [("candidates", C.c_int), ("temporal", C.c_int), ("m_cap", C.c_float), ("neighbours", C.c_int), ("radius", C.c_float),
                ("normal_min_dot", C.c_float)]


class SvgfRestirInfo(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("n_ids", C.c_int), ("launches", C.c_int), ("device_bytes", C.c_ulonglong)]


# every symbol include/svgf_restir.h declares
_vp, _planes, _synth = C.c_void_p, C.POINTER(_b.SvgfPlanarGBuffer), C.POINTER(_b.SvgfSynthParams)
_RESTIR_PROTOTYPES = {
    "svgf_lights_create": (C.c_int, [C.c_int, _vp, C.c_int, C.POINTER(_vp)]),
    "svgf_lights_destroy": (None, [_vp]),
    "svgf_lights_size": (C.c_int, [_vp]),
    "svgf_restir_create": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(_vp)]),
    "svgf_restir_reset": (C.c_int, [_vp, _vp]),
    "svgf_restir_destroy": (None, [_vp]),
    "svgf_restir_info": (C.c_int, [_vp, C.POINTER(SvgfRestirInfo)]),
    "svgf_restir_read": (C.c_int, [_vp, C.c_int, _vp, C.c_ulonglong]),
    "svgf_restir_frame": (C.c_int, [_vp, _vp, _vp, _planes, _vp, C.POINTER(SvgfRestirParams), _synth, C.c_float, _vp, _vp]),
    "svgf_lights_draw_all": (C.c_int, [_vp, _vp, _vp, _planes, C.c_int, C.c_int, C.c_int, _synth, C.c_float, _vp, _vp]),
    "svgf_restir_version": (C.c_int, None),
}
RESTIR_EXPORTS = list(_RESTIR_PROTOTYPES)


def load_restir_library():
    """libsvgf_restir.so (row f27)."""
    return _b._load_linked("restir", lambda name: _RESTIR_PROTOTYPES)


def lights(centre, edge_u=None, edge_v=None, power=30.0) -> np.ndarray:
    """LIGHT_DTYPE[n] from arrays of n centres, half-edges (None: point lights) and powers (a scalar, rgb, or n x rgb)."""
    c = np.asarray(centre, np.float32).reshape(-1, 3)
    out = np.zeros(len(c), LIGHT_DTYPE)
    out["centre"] = c
    if edge_u is not None:
        out["edge_u"] = np.asarray(edge_u, np.float32)
    if edge_v is not None:
        out["edge_v"] = np.asarray(edge_v, np.float32)
    pw = np.asarray(power, np.float32)
    out["power"] = np.broadcast_to(pw if pw.ndim != 1 or len(pw) == 3 else pw[:, None], (len(c), 3))
    return out


def params(candidates: int = 8, temporal: int = 1, m_cap: float = 20.0, neighbours: int = 3, radius: float = 30.0,
           normal_min_dot: float = 0.9) -> SvgfRestirParams:
    return SvgfRestirParams(int(candidates), int(temporal), float(m_cap), int(neighbours), float(radius), float(normal_min_dot))


def _target(gbuffer):
    planar = isinstance(gbuffer, _b.SvgfPlanarGBuffer)
    return (None, C.byref(gbuffer)) if planar else (_b._ptr(gbuffer), None)


def _synth_params(frame, seed):
    return _b.SvgfSynthParams(int(frame), int(seed), 0.0, 0.0, (0.0, 0.0))


class LightTable:
    """svgf_lights: n SvgfLight records (LIGHT_DTYPE) on one device.  Allocates and uploads once; usable as a context manager."""

    def __init__(self, records, device: int = 0):
        self.lib = load_restir_library()
        arr = np.ascontiguousarray(records, dtype=LIGHT_DTYPE).reshape(-1)
        self.h, h = C.c_void_p(), C.c_void_p()      # a table whose create failed stays without a handle
        _b._call(self.lib, "svgf_lights_create", int(device), arr.ctypes.data, len(arr), C.byref(h))
        self.h, self.device = h, int(device)

    def __len__(self):
        return int(self.lib.svgf_lights_size(self.h))

    def draw_all(self, scene, gbuffer, width: int, height: int, out_D, frame: int, seed: int = 1, samples: int = 1, ambient: float = 0.15,
                 stream=None):
        """svgf_lights_draw_all: every light with `samples` shadow rays each, the truth of Restir.frame.  `gbuffer` is AoS texels or a
        SvgfPlanarGBuffer.  One launch on `stream`; never waits."""
        sp = _synth_params(frame, seed)
        _b._call(self.lib, "svgf_lights_draw_all", scene.h, self.h, *_target(gbuffer), int(width), int(height), int(samples), C.byref(sp),
                 float(ambient), _b._ptr(out_D), _b._stream(stream))

    def free(self):
        if self.h:
            self.lib.svgf_lights_destroy(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


class ReservoirState:
    """What Restir and restir_gi.RestirGI are apart from frame(): the reservoir state of one frame size over one resident scene (create
    once: one allocation, not under capture), reset(stream) that forgets the history in one launch, info(), read(), free() before the
    scene's, and the context manager.  A subclass names its library's symbol prefix, loader, reservoir dtype and info struct; a later
    resampler subclasses this."""
    PREFIX, LOAD, DTYPE, INFO = None, None, None, None
    _target, _synth_params = staticmethod(_target), staticmethod(_synth_params)

    def __init__(self, scene, width: int, height: int):
        self.lib, self.scene, self.h, self.width, self.height = self.LOAD(), scene, None, int(width), int(height)
        h = C.c_void_p()
        _b._call(self.lib, self.PREFIX + "_create", scene.h, self.width, self.height, C.byref(h))
        self.h = h

    def _call(self, symbol, *args):
        _b._call(self.lib, symbol, self.h, *args)

    def reset(self, stream=None):
        self._call(self.PREFIX + "_reset", _b._stream(stream))

    def info(self) -> dict:
        i = self.INFO()
        self._call(self.PREFIX + "_info", C.byref(i))
        return {k: int(getattr(i, k)) for k, _ in self.INFO._fields_}

    def read(self, which: int) -> np.ndarray:
        """<prefix>_read (blocking): 0 H, 1 T as DTYPE[height, width]; 2 the previous normals float32[height, width, 3]; 3 the previous
        ids int32[height, width]."""
        shape = (self.height, self.width)
        out = np.zeros(shape, self.DTYPE) if int(which) < 2 else np.zeros(shape + (3,), np.float32) if int(which) == 2 else np.zeros(shape, np.int32)
        self._call(self.PREFIX + "_read", int(which), out.ctypes.data, out.nbytes)
        return out

    def free(self):
        if self.h:
            getattr(self.lib, self.PREFIX + "_destroy")(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


class Restir(ReservoirState):
    """svgf_restir: ReservoirState of RESERVOIR_DTYPE records.  frame(...) per frame behind the draw that wrote the G-buffer - two
    launches, legal under capture - writes D for svgf_denoise / svgf_trace_compose.  Usable as a context manager."""
    PREFIX, LOAD, DTYPE, INFO = "svgf_restir", staticmethod(load_restir_library), RESERVOIR_DTYPE, SvgfRestirInfo

    def frame(self, table: LightTable, gbuffer, out_D, frame: int, seed: int = 1, motion=None, rp: SvgfRestirParams | None = None,
              ambient: float = 0.15, stream=None):
        """svgf_restir_frame: `gbuffer` AoS texels or a SvgfPlanarGBuffer of the state's size, `motion` a SVGF_MOTION_PREV_COORD_F32
        plane or None (no temporal reuse this frame), `rp` from params().  Asynchronous on `stream`; never waits."""
        sp, rp = _synth_params(frame, seed), rp if rp is not None else params()
        self._call("svgf_restir_frame", table.h, *_target(gbuffer), _b._ptr(motion), C.byref(rp), C.byref(sp), float(ambient), _b._ptr(out_D),
                   _b._stream(stream))
