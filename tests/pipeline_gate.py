"""What tests/test_pipeline_order_gpu.py is built from: the GATE that makes a producer late, the caller streams that really run side by
side, the frames, and the yardstick (the same frames ordered on one stream of a fresh plain context).  Test infrastructure only, like
tests/temporal_harness.py; not part of the package.

A gate is one spin kernel of fixed duration (torch.cuda._sleep, calibrated once per process) enqueued on a stream in front of the work
that is to be late.  It reads and writes nothing: everything behind it on its stream is late, everything on other streams runs at once
unless an event says otherwise — and that event is what a scenario tests.  A gate is bounded (GATE_MS, never more than MAX_GATE_MS)
and never released by the host."""
import itertools

import numpy as np
import pytest

from temporal_harness import same_bits, scales

GATE_MS, MAX_GATE_MS = 50.0, 200.0
W, H = 257, 131              # crosses the 64-column and the row-tile seams, several workgroups per level
W2, H2 = 130, 9              # a second size where it costs nothing
CANDIDATES = 6
_cache = {}


# ---- the gate ---------------------------------------------------------------------------------------------------------------------------
def sleep_rate():
    """torch.cuda._sleep cycles per millisecond, measured with two events around one _sleep (once per process; printed)."""
    if "rate" not in _cache:
        import torch
        torch.cuda._sleep(1000)            # (loads the kernel)
        torch.cuda.synchronize()
        n, ms = 2_000_000, 0.0             # 20 ms on the slowest clock _sleep may count (100 MHz), 1 ms on a 2 GHz one
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch.cuda._sleep(n)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            if ms >= 4.0:
                break
            n = int(n * 8.0 / max(ms, 0.05))      # aim at 8 ms
        assert 4.0 <= ms <= MAX_GATE_MS, f"calibration: {n} cycles took {ms:.3f} ms"
        _cache["rate"] = n / ms
        print(f"torch.cuda._sleep: {_cache['rate']:.0f} cycles per ms ({n} cycles in {ms:.2f} ms)")
    return _cache["rate"]


def gate(stream, ms=GATE_MS):
    """Everything enqueued on `stream` behind this call starts `ms` milliseconds late."""
    import torch
    assert 0 < ms <= MAX_GATE_MS
    cycles = int(ms * sleep_rate())
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)


def assert_closed(stream, what):
    """Right behind a scenario's last enqueue: the gate must still be closed, or every producer was on time and nothing was tested."""
    assert not stream.query(), (f"{what}: the gated stream was idle when the last call had been enqueued — the gate ({GATE_MS} ms) had "
                                "opened before the scenario was complete, so the scenario tested nothing")


# ---- caller streams -----------------------------------------------------------------------------------------------------------------------
def caller_streams(pkg, n):
    """n streams of which every pair runs side by side (svgf_streams_overlap == 1), out of CANDIDATES candidates; the candidates and the
    probe's answers are kept for the process, so that the streams stay on the hardware queues they were probed on."""
    import torch
    if "cands" not in _cache:
        _cache["cands"], _cache["pairs"] = [torch.cuda.Stream() for _ in range(CANDIDATES)], {}
    cands, pairs = _cache["cands"], _cache["pairs"]

    def overlap(i, j):
        if (i, j) not in pairs:
            torch.cuda.synchronize()
            pairs[(i, j)] = pkg.binding.streams_overlap(cands[i], cands[j])
        return pairs[(i, j)]
    if ("set", n) not in _cache:
        for combo in itertools.combinations(range(CANDIDATES), n):
            if all(overlap(i, j) for i, j in itertools.combinations(combo, 2)):
                _cache[("set", n)] = [cands[i] for i in combo]
                break
        else:
            pytest.fail(f"no {n} of {CANDIDATES} candidate streams run side by side (svgf_streams_overlap): {pairs}")
    return _cache[("set", n)]


# ---- frames and parameters ----------------------------------------------------------------------------------------------------------------
class Frame:
    def __init__(self, col, gb, cam):
        import torch
        self.cam = cam
        self.col = torch.from_numpy(np.ascontiguousarray(col, dtype=np.float32)).cuda()
        self.gb = torch.from_numpy(gb.view(np.uint8).reshape(-1).copy()).cuda()


def frames(pkg, w, h, n, moving=True, seed=41):
    """n frames of the synthetic scene on the device, every frame in buffers of its own (computed once per process, never written)."""
    import torch
    key = ("frames", w, h, n, moving, seed)
    if key not in _cache:
        _cache[key] = [Frame(*pkg.synth.render_frame(w, h, f, seed=seed, moving=moving)) for f in range(n)]
        torch.cuda.synchronize()
    return _cache[key]


def params(pkg, w=W, h=H, **kw):
    """Full SVGF, five levels, the colour history behind level 1 unless said otherwise; the reprojection exact at the size's aspect
    (temporal_harness.scales: under the reference's own mapping a 130 x 9 image loses every pixel's history, and frames that carry
    nothing over from the last one come out right in any order)."""
    p = pkg.reference_defaults().set(**{**dict(temporal_enable=1, spatial_enable=1, atrous_nlevel=5, history_level=1), **kw})
    p.reproj_scale[0], p.reproj_scale[1] = scales(pkg, w, h)
    return p


def with_(pkg, p, **kw):
    return pkg.SvgfParams.from_buffer_copy(p).set(**kw)


def worth(p):
    """plan_pipeline's `worth` (csrc/svgf_frame.hip): the frames that take the pipeline up when asked to."""
    return bool(p.temporal_enable and p.spatial_enable and p.atrous_nlevel >= 2 and p.right_view_option not in (1, 2)
                and p.history_level != p.atrous_nlevel)


def buffers(w, h, n):
    """n output buffers, zeroed: a copy that ran too early holds zeros, not whatever the allocator left."""
    import torch
    return [torch.zeros((h, w, 3), dtype=torch.float32, device="cuda") for _ in range(n)]


def pipelined_context(pkg, w, h, taa=None):
    import torch
    torch.cuda.synchronize()      # (the queue probe of svgf_create_ex times two kernels)
    d = pkg.Denoiser(w, h, 0, pipelined=True)
    assert d.pipeline_status() == 1, d.last_error()
    if taa:
        d.set_output_taa(*taa)
    return d


# ---- the yardstick and the comparison ----------------------------------------------------------------------------------------------------
def finish(d, outs, nxt):
    """Behind a scenario (or the ordered run): wait for the device, read every frame's output and states 0, 1, 2, then run `nxt`
    (frame, params) as one more ordered frame and read what it returns — it reads everything the context carries from frame to frame,
    the output history included."""
    import torch
    torch.cuda.synchronize()
    res = {"out": [o.cpu().numpy() for o in outs], "state": [d.read_state(k) for k in (0, 1, 2)]}
    fr, p = nxt
    o = buffers(d.width, d.height, 1)[0]
    d.denoise(o, fr.col, fr.gb, fr.cam, p)
    d.sync()
    res["next"] = o.cpu().numpy()
    return res


def ordered(pkg, w, h, seq, plist, nxt, taa=None):
    """The yardstick: frames `seq` with `plist` in turn on ONE stream of a fresh plain context, inputs_ready = 0, no gate.  Kept per
    process and per sequence; never written."""
    key = ("ordered", w, h, tuple(id(f) for f in seq), tuple(bytes(p) for p in plist), id(nxt[0]), bytes(nxt[1]), taa)
    if key not in _cache:
        d = pkg.Denoiser(w, h, 0)
        if taa:
            d.set_output_taa(*taa)
        outs = buffers(w, h, len(seq))
        for o, fr, p in zip(outs, seq, plist):
            assert p.inputs_ready == 0
            d.denoise(o, fr.col, fr.gb, fr.cam, p)
        _cache[key] = finish(d, outs, nxt)
        d.free()
    return _cache[key]


def differing(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if same_bits(a, b):
        return 0
    if a.shape != b.shape or a.dtype != b.dtype:
        return max(a.size, b.size)
    ne = a.view(np.uint32) != b.view(np.uint32)      # (every plane compared here holds 4-byte values)
    if a.dtype.kind == "f":
        ne &= ~(np.isnan(a) & np.isnan(b))
    return int(np.count_nonzero(ne))


def assert_same(got, want, what, extra=()):
    """Every frame's output, the three states and the next frame's output, on bits; `extra`: further (name, got, want) triples.  Every
    difference is listed with the number of values that differ."""
    items = [(f"frame {k}", g, r) for k, (g, r) in enumerate(zip(got["out"], want["out"]))]
    items += [(f"state {k}", g, r) for k, (g, r) in enumerate(zip(got["state"], want["state"]))]
    items += [("the next frame", got["next"], want["next"])] + list(extra)
    assert len(got["out"]) == len(want["out"])
    bad = [(name, differing(g, r)) for name, g, r in items]
    bad = [(name, n) for name, n in bad if n]
    total = sum(n for _, n in bad)
    assert not bad, f"{what}: {total} values differ from the ordered frames: " + ", ".join(f"{name}: {n}" for name, n in bad)
