"""The lane-marching kernel (csrc/svgf_atrous_lane_impl.h) and the strip kernel (csrc/svgf_atrous_strip.hip) at steps 8, 16 and 32
against the CPU oracle, on frames those levels act on.

tests/test_coarse_levels_coverage.py holds the inputs, the sizes and, without a GPU, the proof that on them level k moves the frame,
every sigma acts at level k, the 16 outer taps act, and (temporal leg) the variance a level writes is read by the next.  This module
runs them on the device:

  * every size x target level k = 3, 4, 5 x kernel_variant 4 (lane), 2 (strip), 0 (automatic): levels k - 1 and k, level k both as
    the LAST level (atrous_nlevel = k: the instantiation without variance accumulators) and as an INNER level (atrous_nlevel = k + 1,
    history_level = k: it writes the variance level k + 1 reads, and level k + 1's output is compared too; for k = 5 that is the
    lattice kernel at step 64, and the strip variant is skipped there: the library refuses six levels on the strip kernel);
  * the temporal leg: levels 3 .. 6 of the second frame with blur_variance 1 and 0, the history length, the temporal variance;
  * forced segment lengths 1, 2, 3 (experiments build) at levels 4 and 5 of the two wide sizes: a seam every one to three lattice
    rows, so that every output row has a tap across one;
  * non-finite texels on the level-5 frame of 1921 x 193.

Each level is read as the colour history with history_level = that level (read_state(2)); the oracle side is ONE cascade per size and
parameter set (test_coarse_levels_coverage.frame_cascade), shared by every test here and never written to.

Every comparison prints the worst error within two lattice columns or rows of a seam (strip, chunk, segment) beside the worst
elsewhere, and a failing level says where its worst pixel lies in the kernel's own coordinates (where_worst).

Bar: TOL = 1e-5 per level, the suite's bar for these kernels (test_kernel_geometry_gpu.TOL, test_parity_gpu.TOL_STRIP).  A wrong tap
shows as an error of the size of the level's own change: at least 1e-3 on 90 % of these pixels, a hundred times the bar.  Should a
level exceed the bar, look at structure first (seam rows or columns, one phase, one chunk, one segment length): structure is a bug.
Only unstructured rounding may move the bar, and then against the reference: to max(1e-5, 4 x the float32 oracle's worst error
against the float64 model on the same level inputs) and never above the project's contract of 1e-4.

MEASURED on an MI355X (256 CUs), worst relerr of a level over its arrangements, `within two lattice columns / rows of a seam` /
`elsewhere`; the bar did not move.  The figures of 257, 481 and 961 x 193 were within the bar in that run but were not kept; every run
prints them.  The forced segment lengths and the non-finite leg as it stands (NaN texel in x-phase 0) have NOT run on a device yet:
their first run will show whether 1e-5 and TOL_ACROSS_L hold there.
  non-temporal, 1921 x 193   lane: level 4 1.7e-6 / 1.9e-6, level 5 1.7e-6 / 2.1e-6   strip: level 4 1.8e-6 / 1.8e-6, level 5 1.8e-6 / 2.1e-6
                             level 6 (lattice kernel, reading level 5's variance) 2.5e-6; the three smaller sizes: every level within
                             the bar (their figures are printed by every run)
  non-finite texels (x-phase 5) lane: level 4 1.7e-6 / 2.1e-6, level 5 1.7e-6 / 2.5e-6   strip: level 4 1.8e-6 / 1.8e-6, level 5 1.8e-6 / 2.1e-6
  temporal, 257 x 193        lane: level 3 3.5e-6 / 3.2e-6, level 4 4.8e-6 / 3.5e-6, level 5 3.9e-6 / 3.9e-6, level 6 4.0e-6
                             strip: level 3 2.8e-6 / 3.3e-6, level 4 3.0e-6 / 3.9e-6, level 5 4.6e-6 / 3.7e-6
                             history length equal, variance after the temporal pass bit-equal to the oracle's
The float32 oracle against the float64 model on the same level inputs (the reference's own rounding on these frames,
test_coarse_levels_coverage.py): 5.8e-7 .. 7.6e-7 in colour on the non-temporal frames, 5.4e-7 .. 7.1e-7 on the temporal ones
(variance: up to 1.4e-6).  The kernels' 1.7e-6 .. 4.8e-6 is 2 - 7 times that and unstructured: seams and interior agree within a factor of
1.5 everywhere."""
import numpy as np
import pytest

from conftest import relerr
from test_coarse_levels_coverage import (GEOMETRY, H, LANE_CHUNK, LANE_GROUP, LANE_STRIP, SIZES, STRIP_TX, TARGETS, TEMPORAL_SIZE,
                                         TEMPORAL_TARGETS, cascade, frame, frame_cascade, oracle_level, size_id, target_params, temporal_cascade,
                                         temporal_frames, temporal_params, temporal_state, with_)

pytestmark = pytest.mark.gpu

TOL = 1e-5               # lane / strip kernel vs oracle, every level
TOL_LATTICE = 4e-5       # level 6 (step 64) of the inner arrangement at k = 5: the lattice kernel's bar (test_lattice_gpu.TOL)
TOL_VARIANCE = 2e-4      # variance after the temporal pass (test_parity_gpu.test_sequences_match_oracle_including_state)
TOL_ACROSS_L = 1e-6      # two segment lengths, per level (test_kernel_geometry_gpu.TOL_ACROSS_L)
VARIANTS = [(4, "lane"), (2, "strip"), (0, "auto")]
FORCED_L = (1, 2, 3)
FORCED_SIZES = [(961, H), (1921, H)]
FORCED_KERNELS = [(4, "lane", "lane_segrows"), (2, "strip", "strip_segrows")]


def device_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- a pixel in the kernels' coordinates --------------------------------------------------------------------------------------------

def column_coordinates(kind, W, step):
    """Per image column: (strip or chunk index, distance in lattice columns to the nearest strip / chunk seam that exists in a
    frame W wide: a large number where the column's strip has no neighbour on either side, number of strips or chunks)."""
    x = np.arange(W)
    if kind == "lane" and step >= 16:
        # a workgroup holds 60 lattice columns (a chunk) of 8 adjacent x-phases (a group), one wave per phase: lane = lattice
        # column inside the chunk; lanes 58 / 59 and 0 / 1 are halo lanes of the neighbouring chunks' waves
        lc = x // step
        index, inside, width = lc // LANE_CHUNK, lc % LANE_CHUNK, LANE_CHUNK
    elif kind == "lane":
        # 480 contiguous pixel columns per strip = 480 / step lattice columns of every x-phase, 60 output lanes per wave
        index, inside, width = x // LANE_STRIP, (x % LANE_STRIP) // step, LANE_STRIP // step
    else:
        # 256 contiguous pixel columns per strip, every x-phase
        index, inside, width = x // STRIP_TX, (x % STRIP_TX) // step, STRIP_TX // step
    n_units = int(index.max()) + 1
    far = 1 << 20
    to_left = np.where(index > 0, inside, far)
    to_right = np.where(index < n_units - 1, width - 1 - inside, far)
    return index, np.minimum(to_left, to_right), n_units


def row_coordinates(Hh, step, seg_rows):
    """Per image row: (segment index, distance in lattice rows to the nearest segment seam, number of segments)."""
    r = np.arange(Hh) // step
    n_segs = ((Hh + step - 1) // step + seg_rows - 1) // seg_rows
    seg, inside = r // seg_rows, r % seg_rows
    far = 1 << 20
    # the last segment of a y-phase may be shorter: its lower neighbour does not exist, whatever `inside` says
    return seg, np.minimum(np.where(seg > 0, inside, far), np.where(seg < n_segs - 1, seg_rows - 1 - inside, far)), n_segs


def near_seams(kind, size, step, seg_rows):
    """Mask of the pixels within two lattice columns of a strip / chunk seam or within two lattice rows of a segment seam."""
    W, Hh = size
    _, dcol, _ = column_coordinates(kind, W, step)
    _, drow, _ = row_coordinates(Hh, step, seg_rows)
    return (drow[:, None] < 2) | (dcol[None, :] < 2)


def where_worst(e, kind, size, step, seg_rows):
    """The worst pixel of a per-pixel error map in the coordinates of the kernel `kind` at `step`."""
    W, Hh = size
    y, x = (int(v) for v in np.unravel_index(np.argmax(e), e.shape))
    index, dcol, n_units = column_coordinates(kind, W, step)
    seg, drow, n_segs = row_coordinates(Hh, step, seg_rows)
    xp, yp = x % step, y % step
    if kind == "lane" and step >= 16:
        col = (f"chunk {index[x]} of {n_units}, lattice column {x // step} = lane {(x // step) % LANE_CHUNK}, x-phase {xp} = phase {xp % LANE_GROUP} "
               f"of group {xp // LANE_GROUP}")
    elif kind == "lane":
        lc = (x % LANE_STRIP) // step
        col = f"strip {index[x]} of {n_units}, lattice column {lc} of the strip = lane {lc % 60} of wave {lc // 60} of x-phase {xp}"
    else:
        col = f"strip {index[x]} of {n_units}, column {x % STRIP_TX} of the strip, x-phase {xp}"
    seam = lambda d: "no seam" if d >= 1 << 20 else f"{d} from the nearest seam"      # noqa: E731
    return (f"{e[y, x]:.3e} at row {y} column {x} [{kind} kernel, step {step}]: {col} ({seam(int(dcol[x]))}, lattice columns); "
            f"y-phase {yp}, lattice row {y // step} = row {(y // step) % seg_rows} of segment {seg[y]} of {n_segs} ({seam(int(drow[y]))}, lattice rows)")


class Report:
    """Collects the comparisons of one test: prints every one, keeps the failures and the worst figures."""

    def __init__(self):
        self.failures, self.worst = [], {}

    def level(self, got, ref, kinds, size, step, seg_rows, what, tol=TOL):
        """`kinds`: the kernels that may have run the level (one, or both for the automatic choice without a record); seg_rows per
        kind.  A level at a step above 32 (lattice kernel) has no seams here."""
        nan = np.isnan(ref)
        assert np.array_equal(np.isnan(got), nan), f"{what}: NaN pattern differs from the oracle's"
        e = relerr(np.where(nan, 0, got), np.where(nan, 0, ref)).max(axis=2)
        worst = float(e.max())
        if step > 32:
            print(f"{what} (step {step}): worst {worst:.2e}")
            where = [f"{worst:.3e} at {np.unravel_index(np.argmax(e), e.shape)}"]
        else:
            where = []
            for kind in kinds:
                near = near_seams(kind, size, step, seg_rows[kind])
                at_seams = f"{e[near].max():.2e}" if near.any() else "-"
                elsewhere = f"{e[~near].max():.2e}" if (~near).any() else "-"
                print(f"{what} (step {step}, {kind} kernel, segments of {seg_rows[kind]}): worst {worst:.2e}; within two lattice columns / rows of a "
                      f"seam {at_seams}, elsewhere {elsewhere}")
                where.append(where_worst(e, kind, size, step, seg_rows[kind]))
        self.worst[what] = worst
        if not worst <= tol:
            self.failures.append(f"{what} (bar {tol:.0e}): " + " | ".join(where))
        return worst

    def check(self):
        assert not self.failures, "; ".join(self.failures)


def segment_rows(pkg, size, step, forced=None):
    """Segment length per kernel at this step: forced, or what the library's search picks on this device (host arithmetic)."""
    if forced:
        return {"lane": forced, "strip": forced}
    n_cu = device_cus()
    return {kind: pkg.binding.atrous_geometry(kind, size[0], size[1], step, 1, 1, n_cu)[0][2] for kind in ("lane", "strip")}


def kinds_of(name):
    return ("lane", "strip") if name == "auto" else (name,)


def run(d, frames, p):
    """(colour history, returned image) after the frames."""
    d.reset()
    for c, g, cam in frames:
        img = d.denoise_host(c, g, cam, p)
    return d.read_state(2), img


def check_target(pkg, d, frames, params, levels_for, size, k, variant, name, rep, what, forced=None):
    """Levels k - 1 and k of the last frame (level k as the last and as an inner level) and level k + 1 against the oracle.
    params(k, **kw): the parameter set; levels_for(h): the oracle cascade of a sequence run with history_level = h (the same for
    every h on a non-temporal frame)."""
    seg = {n: segment_rows(pkg, size, 1 << n, forced) for n in (k - 1, k, k + 1) if (1 << n) <= 32}
    seg[6] = None
    kinds = kinds_of(name)
    # level k is the last level; the colour history is level k - 1
    hist, img = run(d, frames, params(k, history_level=k - 1, kernel_variant=variant))
    ref = levels_for(k - 1)
    rep.level(hist, ref[k - 1][0], kinds, size, 1 << (k - 1), seg[k - 1], f"{what} level {k - 1}")
    rep.level(img, ref[k][0], kinds, size, 1 << k, seg[k], f"{what} level {k} as the last level")
    hist, img2 = run(d, frames, params(k, history_level=k, kernel_variant=variant))
    ref = levels_for(k)
    rep.level(hist, ref[k][0], kinds, size, 1 << k, seg[k], f"{what} level {k} as the last level, colour history")
    if not np.array_equal(hist, img2, equal_nan=True):
        rep.failures.append(f"{what} the colour history of the last level is not the returned image")
    if name == "strip" and k == 5:
        return      # six levels on the strip kernel: refused by the library
    # level k is an inner level and writes the variance level k + 1 reads
    hist, img = run(d, frames, params(k, atrous_nlevel=k + 1, history_level=k, kernel_variant=variant))
    rep.level(hist, ref[k][0], kinds, size, 1 << k, seg[k], f"{what} level {k} as an inner level")
    rep.level(img, ref[k + 1][0], kinds, size, 1 << (k + 1), seg[k + 1], f"{what} level {k + 1}, reading level {k}'s variance",
              tol=TOL_LATTICE if k + 1 == 6 else TOL)


@pytest.mark.experiments
@pytest.mark.parametrize("variant,name", VARIANTS, ids=[n for _, n in VARIANTS])
@pytest.mark.parametrize("k", TARGETS)
@pytest.mark.parametrize("size", SIZES, ids=size_id)
def test_coarse_levels_match_oracle(pkg, orc, size, k, variant, name):
    W, Hh = size
    frames = [frame(pkg, W)]
    ref = frame_cascade(pkg, orc, W, k)
    rep = Report()
    d = pkg.Denoiser(W, Hh, 0)
    check_target(pkg, d, frames, lambda k_, **kw: target_params(pkg, k_, **kw), lambda h: ref, size, k, variant, name, rep,
                 f"{W}x{Hh} {name} target {k}:")
    d.free()
    rep.check()


@pytest.mark.experiments
@pytest.mark.parametrize("variant,name", VARIANTS, ids=[n for _, n in VARIANTS])
@pytest.mark.parametrize("bv", [1, 0], ids=["blur", "noblur"])
@pytest.mark.parametrize("k", TEMPORAL_TARGETS)
def test_coarse_levels_match_oracle_after_a_temporal_pass(pkg, orc, k, bv, variant, name):
    """The second frame of test_coarse_levels_coverage.temporal_frames: the variance the levels read differs from pixel to pixel,
    the 3x3 pre-blur acts (blur_variance 1 against 0), and level k + 1 reads the variance level k wrote."""
    size = W, Hh = TEMPORAL_SIZE
    frames = temporal_frames(pkg)
    rep = Report()
    d = pkg.Denoiser(W, Hh, 0)
    d.set_capture(True)      # read_state(3): the variance right after the temporal pass
    check_target(pkg, d, frames, lambda k_, **kw: temporal_params(pkg, k_, blur_variance=bv, **kw),
                 lambda h: temporal_cascade(pkg, orc, h, blur_variance=bv), size, k, variant, name, rep,
                 f"{W}x{Hh} temporal {name} blur_variance {bv} target {k}:")
    # the state of the last run (history_level = k): history length and the temporal pass's variance
    _, var, hlen = temporal_state(pkg, orc, k, blur_variance=bv)
    assert np.array_equal(d.read_state(0), hlen), "history length differs from the oracle's"
    e = float(relerr(d.read_state(3)[..., None], var[..., None]).max())
    print(f"{W}x{Hh} temporal {name}: variance after the temporal pass vs oracle {e:.2e}")
    assert e <= TOL_VARIANCE, f"variance after the temporal pass: {e:.3e}"
    d.free()
    rep.check()


def expected_kernels(kind, nlevel):
    """level_kernels() of a run with the lane / strip kernel forced (kernel_variant 4 / 2): that kernel at every level.  (Only the
    automatic choice lets the prepare pass of a non-temporal frame ride in a lane first level, recorded as `fused`.)"""
    return [(kind, 1 << n) for n in range(1, nlevel + 1)]


@pytest.mark.experiments
@pytest.mark.parametrize("k", (4, 5))
@pytest.mark.parametrize("size", FORCED_SIZES, ids=size_id)
def test_forced_segment_lengths_at_the_coarse_levels(pkg, orc, size, k, experiments_lib):
    """Segments of 1, 2 and 3 lattice rows: a seam every one to three lattice rows at every level, steps 16 and 32 included."""
    W, Hh = size
    frames = [frame(pkg, W)]
    ref = frame_cascade(pkg, orc, W, k)
    p = target_params(pkg, k, history_level=k - 1)
    rep = Report()
    for variant, kind, knob in FORCED_KERNELS:
        # no knob set: the experiments build computes what the product library computes, bit for bit
        experiments_lib.exp_clear()
        de = pkg.Denoiser(W, Hh, 0)
        exp = run(de, frames, with_(p, kernel_variant=variant))
        rec = de.level_kernels()
        de.free()
        assert [(r[0], r[1]) for r in rec] == expected_kernels(kind, k), f"{W}x{Hh} {kind}: {rec}"
        experiments_lib.use_experiments_library(False)
        dp = pkg.Denoiser(W, Hh, 0)
        prod = run(dp, frames, with_(p, kernel_variant=variant))
        dp.free()
        experiments_lib.use_experiments_library(True)
        assert np.array_equal(prod[0], exp[0]) and np.array_equal(prod[1], exp[1]), f"{W}x{Hh} {kind}: product library != experiments build"
        first = None
        for L in FORCED_L:
            experiments_lib.exp_set(knob, L)
            d = pkg.Denoiser(W, Hh, 0)
            outs = run(d, frames, with_(p, kernel_variant=variant))
            rec = d.level_kernels()
            d.free()
            what = f"{W}x{Hh} {kind} L={L} target {k}:"
            assert [(r[0], r[1]) for r in rec] == expected_kernels(kind, k), f"{what} {rec}"
            for n, out in zip((k - 1, k), outs):
                rep.level(out, ref[n][0], (kind,), size, 1 << n, {kind: L}, f"{what} level {n}")
            if first is None:
                first = outs
                continue
            for n, a, b in zip((k - 1, k), outs, first):
                e = relerr(a, b).max(axis=2)
                print(f"{what} level {n} vs L={FORCED_L[0]}: {e.max():.2e}")
                assert e.max() <= TOL_ACROSS_L, f"{what} level {n} vs segment length {FORCED_L[0]}: {where_worst(e, kind, size, 1 << n, L)}"
        experiments_lib.exp_clear()
    rep.check()


NONFINITE_SIZE = (1921, H)
NONFINITE_X = 59 * 32      # x-phase 0, lattice column 59
_nonfinite = {}


def nonfinite_frame(pkg, orc):
    """The level-5 frame of 1921 x 193 with
      * a NaN position texel at x = 59 * 32, lattice column 59 of x-phase 0 at step 32: output lane 59 of the wave of chunk 0 that
        holds x-phase 0, and a halo lane of the wave of chunk 1 that holds the same phase.  Phase 0 is the only one with a lattice
        column 60 at this width (x = 1920), so that wave has one output lane, and it takes the texel through its halo (i = -1);
        lattice row 6 of y-phase 0, the last row of its segment on both kernels;
      * an inf normal component at x = 1920, lattice column 60, the first (and only) lattice column of chunk 1.
    Neither makes a NaN in the reference: min(1, exp(NaN)) is 1 (a NaN operand loses, as on the GPU), so a tap whose position is
    NaN counts with position weight 1 however far away it is, and a tap whose normal distance is inf counts with weight 0.  The
    oracle's output is finite everywhere; what the comparison holds is that the device gives those taps the same weights.  That the
    chunk-1 output lane sees the NaN texel at all is asserted from the oracle: level 5 alone, run from the clean frame's level 4
    with only that texel changed, moves the pixel of column 1920 in the texel's row by more than 1e-3, a hundred times the bar.
    Returns (frame, oracle cascade), computed once."""
    if not _nonfinite:
        W, Hh = NONFINITE_SIZE
        c, g, cam = frame(pkg, W)
        assert GEOMETRY[NONFINITE_SIZE]["lane"][32][1:] == (7, 1) and GEOMETRY[NONFINITE_SIZE]["strip"][32][2] == 1
        y = 6 * 32
        p = target_params(pkg, 5)
        clean = frame_cascade(pkg, orc, W, 5)
        g_nan = g.copy()
        g_nan["position"][y, NONFINITE_X] = np.nan
        own, _ = oracle_level(pkg, orc, *clean[4], g_nan, 5, p)
        moved = float(relerr(own[y, 60 * 32], clean[5][0][y, 60 * 32]).max())
        print(f"{W}x{Hh}: the NaN texel alone moves level 5 at row {y} column {60 * 32} by {moved:.2e}")
        assert moved > 1e-3, "the output lane of chunk 1 does not see the NaN texel: the leg is vacuous"
        g = g_nan
        g["normal"][y - 32, 60 * 32, 1] = np.inf
        g.setflags(write=False)
        ref = cascade(pkg, orc, c, np.full((Hh, W), 10.0, np.float32), g, p, 5)
        assert all(np.isfinite(lv[0]).all() for lv in ref)
        _nonfinite["frame"] = (c, g, cam)
        _nonfinite["ref"] = ref
    return _nonfinite["frame"], _nonfinite["ref"]


@pytest.mark.experiments
@pytest.mark.parametrize("variant,name", VARIANTS[:2], ids=[n for _, n in VARIANTS[:2]])
def test_non_finite_texels_at_a_chunk_seam(pkg, orc, variant, name):
    """Not compared between two device runs: the careful loop is not bit-reproducible (tests/test_parity_gpu.py)."""
    size = W, Hh = NONFINITE_SIZE
    fr, ref = nonfinite_frame(pkg, orc)
    rep = Report()
    d = pkg.Denoiser(W, Hh, 0)
    hist, img = run(d, [fr], target_params(pkg, 5, history_level=4, kernel_variant=variant))
    d.free()
    seg = {n: segment_rows(pkg, size, 1 << n) for n in (4, 5)}
    rep.level(hist, ref[4][0], (name,), size, 16, seg[4], f"{W}x{Hh} {name} non-finite texels, level 4")
    rep.level(img, ref[5][0], (name,), size, 32, seg[5], f"{W}x{Hh} {name} non-finite texels, level 5")
    rep.check()
