"""libsvgf_restir_gi.so (include/svgf_restir_gi.h, row f28): the one-bounce indirect term of a resident scene's G-buffer by reservoir
resampling of row f17's bounce samples - a per-size state of two reservoir planes, two launches per frame that write the demodulated
indirect term I.  Built by the companions' recipe (build.PATH_RESAMPLERS), loaded like them (binding._load_linked), no companion
draw; binding.py's pinned tables stay as they are.  The wrapper is restir.ReservoirState with this library's frame()."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import binding as _b
from .restir import ReservoirState

RESTIR_GI_READ_H, RESTIR_GI_READ_T, RESTIR_GI_READ_PREV_NORMAL, RESTIR_GI_READ_PREV_ID = 0, 1, 2, 3
RESTIR_GI_MAX_CANDIDATES, RESTIR_GI_MAX_NEIGHBOURS = 8, 8
RESERVOIR_GI_DTYPE = np.dtype([("xs", np.float32, 3), ("M", np.float32), ("ns", np.float32, 3), ("W", np.float32), ("L", np.float32, 3),
                               ("phat", np.float32), ("g", np.float32), ("valid", np.int32), ("zero", np.int32, 2)])


class SvgfRestirGIParams(C.Structure):
    _fields_ = [("candidates", C.c_int), ("temporal", C.c_int), ("m_cap", C.c_float), ("neighbours", C.c_int), ("radius", C.c_float),
                ("normal_min_dot", C.c_float), ("jacobian_max", C.c_float), ("ambient", C.c_float), ("shadow_secondary", C.c_int)]


class SvgfRestirGIInfo(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("n_ids", C.c_int), ("launches", C.c_int), ("device_bytes", C.c_ulonglong)]


# every symbol include/svgf_restir_gi.h declares
_vp, _planes, _synth = C.c_void_p, C.POINTER(_b.SvgfPlanarGBuffer), C.POINTER(_b.SvgfSynthParams)
_RESTIR_GI_PROTOTYPES = {
    "svgf_restir_gi_create": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(_vp)]),
    "svgf_restir_gi_reset": (C.c_int, [_vp, _vp]),
    "svgf_restir_gi_destroy": (None, [_vp]),
    "svgf_restir_gi_info": (C.c_int, [_vp, C.POINTER(SvgfRestirGIInfo)]),
    "svgf_restir_gi_read": (C.c_int, [_vp, C.c_int, _vp, C.c_ulonglong]),
    "svgf_restir_gi_frame": (C.c_int, [_vp, C.POINTER(_b.SvgfSceneLight), _vp, _planes, _vp, C.POINTER(SvgfRestirGIParams), _synth, _vp, _vp]),
    "svgf_restir_gi_version": (C.c_int, None),
}
RESTIR_GI_EXPORTS = list(_RESTIR_GI_PROTOTYPES)


def load_restir_gi_library():
    """libsvgf_restir_gi.so (row f28)."""
    return _b._load_linked("restir_gi", lambda name: _RESTIR_GI_PROTOTYPES)


def gi_params(candidates: int = 1, temporal: int = 1, m_cap: float = 20.0, neighbours: int = 3, radius: float = 30.0, normal_min_dot: float = 0.9,
              jacobian_max: float = 10.0, ambient: float = 0.15, shadow_secondary: int = 1) -> SvgfRestirGIParams:
    return SvgfRestirGIParams(int(candidates), int(temporal), float(m_cap), int(neighbours), float(radius), float(normal_min_dot),
                              float(jacobian_max), float(ambient), int(shadow_secondary))


class RestirGI(ReservoirState):
    """svgf_restir_gi: ReservoirState of RESERVOIR_GI_DTYPE records.  frame(...) per frame behind the draw that wrote the G-buffer - two
    launches, legal under capture - writes I for svgf_denoise / svgf_trace_compose.  Usable as a context manager."""
    PREFIX, LOAD, DTYPE, INFO = "svgf_restir_gi", staticmethod(load_restir_gi_library), RESERVOIR_GI_DTYPE, SvgfRestirGIInfo

    def frame(self, light, gbuffer, out_I, frame: int, seed: int = 1, motion=None, gp: SvgfRestirGIParams | None = None, stream=None):
        """svgf_restir_gi_frame: `light` a SvgfSceneLight (centre and edges are read), `gbuffer` AoS texels or a SvgfPlanarGBuffer of
        the state's size, `motion` a SVGF_MOTION_PREV_COORD_F32 plane or None (no temporal reuse this frame), `gp` from gi_params().
        Asynchronous on `stream`; never waits."""
        sp, gp = self._synth_params(frame, seed), gp if gp is not None else gi_params()
        self._call("svgf_restir_gi_frame", C.byref(light), *self._target(gbuffer), _b._ptr(motion), C.byref(gp), C.byref(sp), _b._ptr(out_I),
                   _b._stream(stream))
