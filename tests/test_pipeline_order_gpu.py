"""The frame pipeline's ORDERING EDGES, each held with its producer made late (tests/pipeline_gate.py).

tests/test_pipeline_gpu.py and the pipelined legs of the other suites assert that pipelined frames are bit-identical to ordered ones on
frames that run at their natural speed: at the test sizes a frame has finished before the host has enqueued the next call, so a missing
wait changes nothing there.  Here a GATE (a spin kernel of 50 ms, bounded, never released by the host) is enqueued in front of the
producer of each dependency, the whole scenario is enqueued while the gate is still closed (asserted: the gated stream is not idle
behind the last enqueue), and a consumer that fails to wait reads or overwrites stale planes every time.  One scenario per wait of
enqueue_frame (csrc/svgf_frame.hip) and pipeline_wait_gbuffer_readers (csrc/svgf_pipeline.hip); the scenario's docstring names the
line that waits.  The yardstick is never the pipeline: the same frames ordered on one stream of a fresh plain context, without a gate,
compared on bits — every frame's output, states 0, 1 and 2 behind the last frame, and what one more frame returns.

Not reachable by a gate, and not here: whether ev_hist is RECORDED too early inside a frame (the middle of a frame cannot be made late
from outside); svgf_reset / svgf_read_state / svgf_transfer_history (they synchronise the device and would wait the gate out); the
ordered-to-piped switch of a context whose promise the probe refused.

MEASURED on an MI355X (GPU_MAX_HW_QUEUES = 4): 69 cases, all green against the product library, 6.1 s for the module of which
about 3.1 s are gates (62 of 50 ms); torch.cuda._sleep counts 2 397 000 cycles per ms (a gate of 50 ms took 50.0 ms, the other
stream's copy was ready after 0.17 ms).
THE SUITE BITES: the module run once against twelve libraries that each lack ONE wait and nothing else (built in a scratch tree, never
committed).  Every run ended in plain test failures; every wait is seen by the scenario written for it.  Per removed wait: the tests
that failed (cases failed / cases of the test) and the values that differed from the ordered frames in a failing case (least .. most;
a 257 x 131 image has 101 001 values).  Names without the test_ prefix, shortened:
  svgf_frame.hip:332     promised_frames_behind_a_replay 3/3                                             201 995 .. 583 809
  svgf_frame.hip:334     a_frame_waits_for_the_last_frame_of_its_plane_set 7/12                           24 022 .. 101 001
  svgf_frame.hip:340     the_next_first_pass_waits_for_the_history_release 12/12                          14 670 .. 714 925
                         a_frame_waits_..._plane_set 12/12, the_writer_of_out 4/12, pre_and_the_output_history 6/12,
                         what_the_caller_enqueues 3/6                                                     14 670 .. 794 455
  svgf_frame.hip:358     pre_and_the_output_history_wait [copy] 5/6                                      186 539 .. 251 116
  svgf_frame.hip:370     the_writer_of_out [last level writes out] 4/6                                    10 530 .. 303 003
  svgf_frame.hip:371     pre_and_the_output_history_wait [cascade] 4/6, what_the_caller_enqueues 4/6,
                         the_writer_of_out [output pass writes out] 4/6                                    4 015 .. 283 090
  svgf_frame.hip:388     the_writer_of_out [output pass writes out] 4/6                                   10 530 .. 303 003
  svgf_frame.hip:393     what_the_caller_enqueues 6/6, the_writer_of_out 12/12                             3 510 .. 707 007
  svgf_pipeline.hip:157  the_producer_refills [frame n-1 promised, albedo not read] 3/3, [frame n planar, albedo not read]
                                                                                                          77 853 ..  78 517
  svgf_pipeline.hip:158  the_producer_refills [frame n planar, albedo not read], [frame n AoS, albedo not read], [frame n-1
                         promised, albedo not read] 3/3                                                  317 382 .. 410 862
  svgf_pipeline.hip:159  the_producer_refills [frame n AoS, albedo not read]                                        410 862
  svgf_pipeline.hip:160  the_producer_refills [albedo read]: frame n planar, frame n AoS, frame n-1 promised 3/3    3 687 ..   6 141
Where fewer cases fail than a test has, the others held trivially in that process: the runtime had put one of the context's internal
streams on the gated caller stream's hardware queue (the cases that still pass without :370 are the ones that fail without :340, and the
other way round), which is why such scenarios run once per caller stream.  With sepcolor = addcolor = 1 the albedo rule (:160) alone
orders the producer behind everything :157 - :159 wait for, so those three are seen only by the cases whose frames do not modulate;
:160 is seen only by the ones that do.
"""
import ctypes

import pytest

import pipeline_gate as pg
from pipeline_gate import H, H2, W, W2, assert_closed, assert_same, buffers, finish, frames, gate, ordered, params, with_
from temporal_harness import _hip

pytestmark = pytest.mark.gpu
TAA = (0.2, 1.0)
PARITY = pytest.mark.parametrize("k", [2, 3], ids=["even k", "odd k"])
# Where a scenario's late or early work runs on the context's INTERNAL streams, no probe can tell whether the runtime has put one of them
# on the gated caller stream's hardware queue (the scenario would then hold trivially).  The three caller streams lie on three queues
# and the two internal ones on two, so at least one caller stream shares its queue with neither: such scenarios run once with each of
# the three as the gated stream.
GATED = pytest.mark.parametrize("turn", [0, 1, 2], ids=["gate on stream 0", "gate on stream 1", "gate on stream 2"])


def _streams(pkg, turn):
    st = pg.caller_streams(pkg, 3)
    return st[turn:] + st[:turn]


def _on(s):
    import torch
    return torch.cuda.stream(s)


# ---- the module's controls ---------------------------------------------------------------------------------------------------------------
def test_a_gate_holds_its_own_stream_and_no_other(pkg):
    """Gate on A, a small copy on B and an event behind it: the event becomes ready (polled for at most half the gate) while A is
    still busy — the caller streams the scenarios use run side by side, and the gate is as long as it was asked to be."""
    import time
    import torch
    a, b = pg.caller_streams(pkg, 2)
    assert len(pg.caller_streams(pkg, 3)) == 3
    src, dst = torch.ones(1024, device="cuda"), torch.zeros(1024, device="cuda")
    pg.sleep_rate()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    gate(a)
    with _on(b):
        dst.copy_(src, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
    while not ev.query() and time.perf_counter() - t0 < pg.GATE_MS / 2e3:
        pass
    ready, busy, waited = ev.query(), not a.query(), time.perf_counter() - t0
    a.synchronize()
    took = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    print(f"gate of {pg.GATE_MS} ms took {took:.1f} ms; the other stream's copy was ready after {waited * 1e3:.2f} ms")
    assert ready and busy, f"copy on B ready: {ready}, A still busy: {busy} after {waited * 1e3:.2f} ms"
    assert took <= pg.MAX_GATE_MS and bool((dst == 1).all())


def test_the_scenario_frames_take_the_pipeline_up(pkg):
    """plan_pipeline's `worth` for the parameter sets the scenarios rely on, and for the frames that must NOT be worth it."""
    for kw in (dict(), dict(history_level=0), dict(history_level=3), dict(sepcolor=1, addcolor=1)):
        assert pg.worth(params(pkg, **kw)), kw
    for kw in (dict(right_view_option=1), dict(spatial_enable=0), dict(history_level=5)):
        assert not pg.worth(params(pkg, **kw)), kw
    d = pg.pipelined_context(pkg, W2, H2)
    assert d.is_pipelined()
    d.free()


# ---- svgf_frame.hip:340 --------------------------------------------------------------------------------------------------------------------
ON_K = {"history level 0": dict(), "history level 1": dict(), "history level 3": dict(),
        "debug view": dict(right_view_option=1), "no cascade": dict(spatial_enable=0)}
LEVEL = {"history level 0": 0, "history level 3": 3}
RELEASES = [(v, k, W, H) for v in ON_K for k in (2, 3)] + [("history level 1", k, W2, H2) for k in (2, 3)]


@pytest.mark.parametrize("variant,k,w,h", RELEASES, ids=[f"{v}, k = {k}, {w}x{h}" for v, k, w, h in RELEASES])
def test_the_next_first_pass_waits_for_the_history_release(pkg, variant, k, w, h):
    """`ev_hist[1 - pq].wait` (svgf_frame.hip:340).  inputs_ready = 2, frames in turn on A and B; a gate in front of frame k on its
    stream, frame k+1 enqueued at once on the other: its temporal pass must not start before frame k has released its history —
    behind the temporal pass (history_level 0), behind level 1 or 3, or at frame k's end (a debug view, a frame without a cascade)."""
    n = 6
    fr = frames(pkg, w, h, n + 1)
    base = params(pkg, w, h, history_level=LEVEL.get(variant, 1))
    plist = [with_(pkg, base, **(ON_K[variant] if f == k else {})) for f in range(n)]
    want = ordered(pkg, w, h, fr[:n], plist, (fr[n], base))
    st = pg.caller_streams(pkg, 2)
    d = pg.pipelined_context(pkg, w, h)
    outs = buffers(w, h, n)
    for f in range(n):
        s = st[f & 1]
        if f == k:
            gate(s)
        d.denoise(outs[f], fr[f].col, fr[f].gb, fr[f].cam, with_(pkg, plist[f], inputs_ready=2), stream=s)
    assert_closed(st[k & 1], f"{variant}, k = {k}")
    got = finish(d, outs, (fr[n], base))
    assert d.is_pipelined()
    d.free()
    assert_same(got, want, f"{variant}, frame {k} late")


# ---- svgf_frame.hip:334 --------------------------------------------------------------------------------------------------------------------
@GATED
@PARITY
@pytest.mark.parametrize("third", ["a third stream", "the other caller's stream"])
def test_a_frame_waits_for_the_last_frame_of_its_plane_set(pkg, third, k, turn):
    """`ev_done[pq].wait` (svgf_frame.hip:334).  Frames k and k+1 are promised and handed over with the caller streams A and B; A's
    gate is in front of call k, so of frame k only the last level is late (it waits for A's position, :370) while its history was
    released on time.  Frame k+2 (inputs_ready = 2, on a third stream or on B) uses frame k's plane set: it must not start before
    frame k's last level has read that set."""
    n = 7
    fr = frames(pkg, W, H, n + 1)
    base = params(pkg)
    want = ordered(pkg, W, H, fr[:n], [base] * n, (fr[n], base))
    a, b, c = _streams(pkg, turn)
    d = pg.pipelined_context(pkg, W, H)
    outs = buffers(W, H, n)
    promised, on_stream = with_(pkg, base, inputs_ready=1), with_(pkg, base, inputs_ready=2)
    for f in range(n):
        s, p = (a, promised) if f <= k else (b, promised)
        if f == k:
            gate(a)
        if f == k + 2:
            s, p = (c if third == "a third stream" else b), on_stream
        d.denoise(outs[f], fr[f].col, fr[f].gb, fr[f].cam, p, stream=s)
    assert_closed(a, f"frame k + 2 on {third}, k = {k}")
    got = finish(d, outs, (fr[n], base))
    d.free()
    assert_same(got, want, f"frame {k}'s last level late, frame {k + 2} on {third}")


# ---- svgf_frame.hip:370, :388 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(W, H), (W2, H2)], ids=[f"{W}x{H}", f"{W2}x{H2}"])
@pytest.mark.parametrize("taa", [None, TAA], ids=["last level writes out", "output pass writes out"])
@GATED
def test_the_writer_of_out_waits_for_the_callers_stream_position(pkg, turn, taa, w, h):
    """`hipStreamWaitEvent(s, ev_in)` in front of the last level (svgf_frame.hip:370), of the output pass where it is on (:388).  ONE
    output buffer for all promised frames.  On the caller's stream: a gate, then a copy of `out` (frame k-1's result) into a keep
    buffer, then call k: the keep buffer must hold frame k-1."""
    n, k = 6, 3
    fr = frames(pkg, w, h, n + 1)
    base = params(pkg, w, h)
    want = ordered(pkg, w, h, fr[:n], [base] * n, (fr[n], base), taa=taa)
    s = _streams(pkg, turn)[0]
    d = pg.pipelined_context(pkg, w, h, taa=taa)
    out, keep = buffers(w, h, 1)[0], buffers(w, h, n)
    p = with_(pkg, base, inputs_ready=1)
    for f in range(n):
        d.denoise(out, fr[f].col, fr[f].gb, fr[f].cam, p, stream=s)
        if f + 1 == k:
            gate(s)
        with _on(s):
            keep[f].copy_(out, non_blocking=True)
    assert_closed(s, f"one output buffer, output pass {taa}")
    got = finish(d, keep, (fr[n], base))
    d.free()
    assert_same(got, want, f"a reader of `out` behind a gate in front of call {k}")


# ---- svgf_frame.hip:332 (ever_captured) -------------------------------------------------------------------------------------------------------
@GATED
def test_promised_frames_behind_a_replay_of_a_captured_context(pkg, turn):
    """`if (pl.wait_in_first) hipStreamWaitEvent(s, ev_in)` (svgf_frame.hip:332) on a context that has been captured.  As
    test_pipeline_gpu.py::test_a_pipelined_context_joins_a_stream_capture: two eager frames, two frames captured, one replay, four
    eager frames (behind which every event of the pipeline is an eager one again and the promise is back) — then a gate, ANOTHER
    replay behind it, and four promised frames enqueued straight behind that.  The replay touches the context's planes and is visible
    only through the caller's stream: the whole of the first promised frame waits there.  (A static camera: the previous view matrix
    is a kernel argument of the recorded launches.)"""
    import torch
    hip = _hip()
    fr = frames(pkg, W, H, 2, moving=False)
    base = params(pkg)
    want = ordered(pkg, W, H, [fr[f & 1] for f in range(14)], [base] * 14, (fr[0], base))
    p = with_(pkg, base, inputs_ready=1)
    s = _streams(pkg, turn)[0]
    sp = ctypes.c_void_p(s.cuda_stream)
    d = pg.pipelined_context(pkg, W, H)
    pair, eager = buffers(W, H, 2), buffers(W, H, 10)

    def run(outs, first):
        for j, o in enumerate(outs):
            f = fr[(first + j) & 1]
            d.denoise(o, f.col, f.gb, f.cam, p, stream=s)
    run(eager[0:2], 0)
    s.synchronize()
    graph, gexec = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipStreamBeginCapture(sp, 0) == 0
    run(pair, 2)
    assert hip.hipStreamEndCapture(sp, ctypes.byref(graph)) == 0
    assert hip.hipGraphInstantiate(ctypes.byref(gexec), graph, None, None, 0) == 0
    assert hip.hipGraphLaunch(gexec, sp) == 0
    with _on(s):
        first = [o.clone() for o in pair]
    run(eager[2:6], 4)
    torch.cuda.synchronize()
    gate(s)
    assert hip.hipGraphLaunch(gexec, sp) == 0
    with _on(s):
        second = [o.clone() for o in pair]
    run(eager[6:10], 10)
    assert_closed(s, "promised frames behind a replay")
    got = finish(d, eager[0:2] + first + eager[2:6] + second + eager[6:10], (fr[0], base))
    hip.hipGraphExecDestroy(gexec)
    hip.hipGraphDestroy(graph)
    d.free()
    assert_same(got, want, "promised frames behind a late replay")


# ---- svgf_frame.hip:358, :371, :393 -----------------------------------------------------------------------------------------------------------
def _alternating_callers_with_the_output_pass(pkg, exit_, k, turn):
    """Output pass on; promised frames handed over with A and B in turn, a copy of every frame's `out` enqueued right behind its call
    on the same stream; the gate in front of call k makes frame k's output pass late (it waits for the caller's position), not its
    levels.  Frame k+1 exits by its cascade or (`copy`) by the copy of a frame with spatial_enable = 0."""
    key = ("alternating", exit_, k, turn)
    if key not in pg._cache:
        n = 7
        fr = frames(pkg, W, H, n + 1)
        base = params(pkg)
        plist = [with_(pkg, base, **(dict(spatial_enable=0) if exit_ == "copy" and f == k + 1 else {})) for f in range(n)]
        want = ordered(pkg, W, H, fr[:n], plist, (fr[n], base), taa=TAA)
        st = _streams(pkg, turn)[:2]
        d = pg.pipelined_context(pkg, W, H, taa=TAA)
        outs, keep = buffers(W, H, n), buffers(W, H, n)
        for f in range(n):
            s = st[f & 1]
            if f == k:
                gate(s)
            d.denoise(outs[f], fr[f].col, fr[f].gb, fr[f].cam, with_(pkg, plist[f], inputs_ready=1), stream=s)
            with _on(s):
                keep[f].copy_(outs[f], non_blocking=True)
        assert_closed(st[k & 1], f"output pass, frame k + 1 exits by its {exit_}, k = {k}")
        got = finish(d, outs, (fr[n], base))
        d.free()
        pg._cache[key] = (got, want, [o.cpu().numpy() for o in keep])
    return pg._cache[key]


@GATED
@PARITY
@pytest.mark.parametrize("exit_", ["cascade", "copy"])
def test_pre_and_the_output_history_wait_for_the_other_paritys_end(pkg, exit_, k, turn):
    """`ev_done[1 - pq].wait` in front of the last level (svgf_frame.hip:371) and of the copy a frame without a cascade exits by
    (:358): frame k+1 must neither overwrite the ONE `pre` plane nor read the output history before frame k's late output pass ran."""
    got, want, _ = _alternating_callers_with_the_output_pass(pkg, exit_, k, turn)
    assert_same(got, want, f"frame {k}'s output pass late, frame {k + 1} exits by its {exit_}")


@GATED
@PARITY
def test_what_the_caller_enqueues_behind_a_call_sees_out(pkg, k, turn):
    """`ev_done[pq].wait(pl.s_user)` (svgf_frame.hip:393).  In the scenario above frame k+1 is late for a reason that is not its own
    caller's stream (B is never gated: it waits for frame k's end): the copy of its `out` enqueued right behind call k+1 on B must
    hold frame k+1, and so must every later one."""
    _, want, keep = _alternating_callers_with_the_output_pass(pkg, "cascade", k, turn)
    bad = [(f, pg.differing(g, r)) for f, (g, r) in enumerate(zip(keep, want["out"]))]
    bad = [(f, n) for f, n in bad if n]
    assert not bad, (f"{sum(n for _, n in bad)} values differ from the ordered frames in the copies enqueued behind the calls: " +
                     ", ".join(f"frame {f}: {n}" for f, n in bad))


# ---- svgf_pipeline.hip:157-160 ------------------------------------------------------------------------------------------------------------------
def _planar_ordered(pkg, n, aos, modulate):
    key = ("planar ordered", n, tuple(sorted(aos)), modulate)
    if key not in pg._cache:
        import torch
        base = params(pkg, sepcolor=modulate, addcolor=modulate)
        cams = [pkg.synth.camera_for_frame(f, True) for f in range(n + 1)]
        d = pkg.Denoiser(W, H, 0)
        rgb, outs = buffers(W, H, n + 1), buffers(W, H, n + 1)
        gbt = torch.empty((H * W * 52,), dtype=torch.uint8, device="cuda")
        for f in range(n + 1):
            if f == n:
                torch.cuda.synchronize()
                res = {"out": [o.cpu().numpy() for o in outs[:n]], "state": [d.read_state(k) for k in (0, 1, 2)]}
            if f in aos:
                pkg.binding.synth_render(rgb[f], gbt, W, H, cams[f], f, seed=19)
                d.denoise(outs[f], rgb[f], gbt, cams[f], base)
            else:
                pkg.binding.synth_render_planar(rgb[f], d.planar_gbuffer(), W, H, cams[f], f, seed=19)
                d.denoise_planar(outs[f], rgb[f], cams[f], base)
        d.sync()
        res["next"] = outs[n].cpu().numpy()
        d.free()
        pg._cache[key] = res
    return pg._cache[key]


TAIL = "frame n-1 promised, its tail late"
REFILLS = [(v, m, 0) for v in ("frame n planar", "frame n AoS") for m in (1, 0)] + [(TAIL, m, t) for m in (1, 0) for t in (0, 1, 2)]


@pytest.mark.parametrize("variant,modulate,turn", REFILLS,
                         ids=[f"{v}, {'albedo read' if m else 'albedo not read'}, gate on stream {t}" for v, m, t in REFILLS])
def test_the_producer_refills_the_planar_planes_behind_their_last_readers(pkg, variant, modulate, turn):
    """pipeline_wait_gbuffer_readers (svgf_pipeline.hip:157-160).  Planar frames on A and B in turn, the producer on a stream P of its
    own: svgf_planar_gbuffer_stream(P), then the fill of the next frame's planes on P at once.
    frame n planar / AoS: inputs_ready = 2, a gate in front of frame n makes its temporal pass (the last reader of the planes as the
    PREVIOUS G-buffer) and its last level late: P waits for ev_tdone (:158), or for frame n's end where frame n was an AoS frame
    (:159); with sepcolor = addcolor = 1 the last level reads the ONE albedo plane and P waits for frame n's end either way (:160).
    frame n-1 promised: the gate in front of its call makes only its last level late (a reader of the planes as the CURRENT
    G-buffer) while frame n's temporal pass is on time: P waits for the end of the frame before last (:157).
    Each variant runs with the albedo read and not read: where it is read, the albedo rule orders P behind frame n's end, which lies
    behind everything :158 and :159 wait for, and behind frame n-1's end one fill earlier than :157 does — only frames that do not
    modulate leave those three waits to themselves."""
    import torch
    N, n = 6, 3
    aos = {n} if variant == "frame n AoS" else set()
    tail = variant.startswith("frame n-1")
    gated = n - 1 if tail else n
    want = _planar_ordered(pkg, N, aos, modulate)
    base = params(pkg, sepcolor=modulate, addcolor=modulate)
    cams = [pkg.synth.camera_for_frame(f, True) for f in range(N + 1)]
    a, b, prod = _streams(pkg, turn)
    d = pg.pipelined_context(pkg, W, H)
    rgb, outs = buffers(W, H, N + 1), buffers(W, H, N + 1)
    gbt = torch.empty((H * W * 52,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for f in range(N):
        s = (a, b)[f & 1]
        promised = tail and f == gated
        if f in aos:
            pkg.binding.synth_render(rgb[f], gbt, W, H, cams[f], f, seed=19, stream=s)
        else:
            pkg.binding.synth_render_planar(rgb[f], d.planar_gbuffer(stream=prod), W, H, cams[f], f, seed=19, stream=prod)
        if promised:
            torch.cuda.synchronize()      # the promise: the planes and the colour are complete at call time
        if f == gated:
            gate(s)
        if f not in aos and not promised:
            s.wait_stream(prod)
        p = with_(pkg, base, inputs_ready=1 if promised else 2)
        if f in aos:
            d.denoise(outs[f], rgb[f], gbt, cams[f], p, stream=s)
        else:
            d.denoise_planar(outs[f], rgb[f], cams[f], p, stream=s)
    assert_closed((a, b)[gated & 1], variant)
    torch.cuda.synchronize()
    got = {"out": [o.cpu().numpy() for o in outs[:N]], "state": [d.read_state(k) for k in (0, 1, 2)]}
    pkg.binding.synth_render_planar(rgb[N], d.planar_gbuffer(), W, H, cams[N], N, seed=19)
    d.denoise_planar(outs[N], rgb[N], cams[N], base)
    d.sync()
    got["next"] = outs[N].cpu().numpy()
    assert d.is_pipelined()
    d.free()
    assert_same(got, want, f"{variant}, sepcolor = addcolor = {modulate}")
