"""The temporal pass's kernels across the product of their features: motion input x object motion table x history clamp radius x
firefly filter x position test (csrc/svgf_kernels.hip: launch_temporal).

Each feature's own suite (test_motion_vectors.py, test_history_clamp.py, test_object_motion.py, test_firefly_filter.py) crosses it
with the features that existed when it arrived.  This file launches what they leave out:
- k_temporal_clamped<MOTION, XF = true, R>, all twelve (the table's suite has <NONE, true, 2> alone; the clamp's sets no table);
- k_temporal_filtered<R> at R = 1 and 3 (the filter's suite runs R = 0 and 2), and at every R with a table set, with the position
  test on, and both: every (MOTION, XF, R) triple that this kernel serves at run time in place of a specialised one;
- the sentence above k_temporal_filtered, that its run-time choices compute what the specialised kernels compute bit for bit,
  between the two kernels themselves.

The yardstick is tests/temporal_model.py fed tests/firefly_model.py's colours (temporal_harness.mixed_model), on the inputs of
test_object_motion.py: mixed_sequence (ray misses, ids beyond the table, non-finite positions, positions behind the camera) and
mixed_table (row 0 the exact identity, row 6 NaN and inf), spatial filter off, states 0 to 4 of all four frames.

Bounds: every comparison is on the bits of every pixel (NaNs in the same place count as equal).  Both sides perform the same
correctly rounded float32 operations in the same order without contraction: there is no arithmetic that may differ, so there is
no tolerance to choose.

Sizes: 67x41 has neither side a multiple of the 64 x 4 tile and 11 tile rows; 130x9 has two column seams and a last tile row one
image row high, so that the R = 3 filtered margin of 4 reaches across a whole neighbouring tile and off the bottom edge."""
import numpy as np
import pytest

import firefly_model as ff
import temporal_model as tm
from temporal_harness import (BAD_ROW, STATES, assert_frames_equal, device_table, mixed_model, mixed_sequence, mixed_table, run_gpu, same_bits,
                              scales, synth_params)

F = np.float32
SIZES = [(67, 41), (130, 9)]
MOTIONS = {"camera": None, "coord_f32": tm.COORD, "delta_f32": tm.D32, "delta_f16": tm.D16}      # the model's fmt; None: no plane
CLAMP_K = {0: 0.0, 1: 1.0, 2: 1.0, 3: 2.5}      # svgf_set_history_clamp(radius, k)
TOLS = (0.0, 0.3)                               # SvgfParams::reproj_position_tol
FILTER_SCALES = (1.0, 1.5, 0.0)
PASS_THROUGH_SCALE = 3.0e38                     # finite, and no colour of mixed_sequence exceeds the bound at this scale


def filter_of(radius, table, tol):
    """The fixed rule that assigns (rank, scale) to a filtered cell.  With c = 2 * table + (tol > 0) = 0..3 the cell's index among
    its radius's four: rank = 1 + (c + radius) % 3 and scale = FILTER_SCALES[(2 c + radius) % 3].  c and 2 c each run through all
    three residues over c = 0..3, so every radius meets every rank and every scale (test_the_rule_gives_every_radius_every_rank_
    and_scale)."""
    c = 2 * int(table) + int(tol > 0)
    return 1 + (c + radius) % 3, FILTER_SCALES[(2 * c + radius) % 3]


CLAMPED_CELLS = [(radius, tol) for radius in (1, 2, 3) for tol in TOLS]                                    # table on, filter off
FILTERED_CELLS = [(radius, table, tol) for radius in (0, 1, 2, 3) for table in (False, True) for tol in TOLS]
DIAGONAL = [(1, 1, 1.0), (3, 3, 1.5)]           # (radius, rank, scale) of the planar and promised legs: table on, tol 0.3, camera path


# ---- 1. CPU: the inputs act ----------------------------------------------------------------------------------------------------------------
def test_the_rule_gives_every_radius_every_rank_and_scale():
    for radius in (0, 1, 2, 3):
        got = [filter_of(radius, table, tol) for r, table, tol in FILTERED_CELLS if r == radius]
        assert len(got) == 4
        assert {rank for rank, _ in got} == {1, 2, 3}, radius
        assert {scale for _, scale in got} == set(FILTER_SCALES), radius


def _changed(a, b):
    """How many pixels are finite in both colour histories and differ."""
    fin = np.isfinite(a).all(axis=-1) & np.isfinite(b).all(axis=-1)
    return int(np.count_nonzero(fin & (a != b).any(axis=-1)))


@pytest.mark.parametrize("motion", list(MOTIONS))
@pytest.mark.parametrize("W,H", SIZES)
def test_model_every_input_acts_on_the_last_frame(pkg, orc, W, H, motion):
    """Conditions, not measurements: a cell of the GPU matrix whose table, position test, clamp or filter changed nothing would
    compare two runs of a smaller kernel.  Filter scale 1.0 throughout; history lengths do not depend on the colour."""
    fmt = MOTIONS[motion]
    last = mixed_sequence(pkg, orc, W, H)[-1][1]["geomId"]

    def hlen(table, tol):
        return mixed_model(pkg, orc, W, H, fmt, tol, 0, 0.0, rank=1, scale=1.0, table=table)[-1]["hlen"]

    n_table = int(np.count_nonzero(hlen(True, 0.0) != hlen(False, 0.0)))
    n_tol = [int(np.count_nonzero(hlen(table, 0.3) != hlen(table, 0.0))) for table in (True, False)]
    print(f"{W}x{H} {motion}: history lengths changed by the table {n_table}, by tol 0.3 with / without the table {n_tol}")
    assert n_table > 0, "the table changes some history length"
    assert n_tol[0] > 0 and n_tol[1] > 0, "tol 0.3 changes some history length, with the table and without"
    bad = last == BAD_ROW
    assert np.count_nonzero(bad) > 0
    for tol in TOLS:
        assert (hlen(True, tol)[bad] == 1).all(), "pixels of the table's NaN / inf row never find history"

    def run(radius, rank):
        return mixed_model(pkg, orc, W, H, fmt, 0.3, radius, CLAMP_K[radius], rank=rank, scale=1.0, table=True)[-1]

    for radius in (1, 2, 3):
        for rank in (1, 2, 3):
            r = run(radius, rank)
            n_clamp, n_filter = _changed(r["color"], run(0, rank)["color"]), _changed(r["color"], run(radius, 0)["color"])
            kept = int(np.count_nonzero(r["hlen"] >= 2))
            print(f"{W}x{H} {motion} radius {radius} rank {rank}: clamp changes {n_clamp} pixels, filter {n_filter}, hlen >= 2 on {kept}")
            assert n_clamp > 0, "the clamp changes a finite pixel"
            assert n_filter > 0, "the filter changes a finite pixel"
            assert kept > 0 and r["hlen"].max() == 4


def test_model_the_pass_through_scale_returns_the_colours(pkg, orc):
    """At rank 1 and scale 3.0e38 the bound is 3.0e38 times the largest neighbour luminance: +inf above a luminance of about 1.13
    and otherwise beyond every colour of the sequence.  (A bound of 0, under black neighbours alone, would still act on a lit
    pixel: the sequence has black pixels, and no lit one among black neighbours only.)"""
    for W, H in SIZES:
        for col, _, _, _ in mixed_sequence(pkg, orc, W, H):
            assert np.isfinite(col).all()
            assert same_bits(ff.firefly_filter(col, 1, PASS_THROUGH_SCALE), col)


# ---- 2. GPU: the matrix ------------------------------------------------------------------------------------------------------------------------
def _inputs(pkg, orc, W, H):
    seq = mixed_sequence(pkg, orc, W, H)
    return [(c, g) for c, g, _, _ in seq], [c for _, _, c, _ in seq]


def _run_cell(pkg, den, t_x, frames, cams, fmt, tol, radius, k, rank, scale, table, leg="aos", promised=False):
    """One cell on `den`: svgf_reset, every setting given anew, the four frames.  The plane, where one is used, is written on the
    device by svgf_motion_reproject with the same table (none: without)."""
    H, W = frames[0][1].shape
    params = synth_params(pkg, W, H, reproj_position_tol=tol)
    if promised:
        params.inputs_ready = 1
    den.reset()
    den.set_object_motion(t_x if table else None)
    den.set_history_clamp(radius, k)
    den.set_firefly_filter(rank, scale)
    return run_gpu(pkg, den, frames, params, cams, leg=leg, plane_fmt=fmt, plane_tables=[mixed_table()] * len(frames) if table else None)


@pytest.mark.gpu
@pytest.mark.parametrize("motion", list(MOTIONS))
@pytest.mark.parametrize("W,H", SIZES)
def test_clamped_kernels_with_the_table_equal_the_model(pkg, orc, W, H, motion):
    """k_temporal_clamped<MOTION, true, R>, R = 1, 2, 3, with and without the position test: one context, six cells."""
    frames, cams = _inputs(pkg, orc, W, H)
    fmt = MOTIONS[motion]
    den, t_x = pkg.Denoiser(W, H), device_table(mixed_table())
    try:
        for radius, tol in CLAMPED_CELLS:
            k = CLAMP_K[radius]
            got = _run_cell(pkg, den, t_x, frames, cams, fmt, tol, radius, k, 0, 1.0, True)
            assert den.history_clamp() == (radius, k) and den.firefly_filter()[0] == 0 and den.object_motion() == (t_x.data_ptr(), 9)
            assert_frames_equal(got, mixed_model(pkg, orc, W, H, fmt, tol, radius, k), f"{W}x{H} {motion} radius {radius} k {k} tol {tol}")
    finally:
        den.free()


@pytest.mark.gpu
@pytest.mark.parametrize("motion", list(MOTIONS))
@pytest.mark.parametrize("W,H", SIZES)
def test_filtered_kernels_equal_the_model(pkg, orc, W, H, motion):
    """k_temporal_filtered<R>, R = 0..3, table off and on, with and without the position test, (rank, scale) by filter_of: one
    context, sixteen cells.  Over the four motion inputs, every (MOTION, XF, R) the kernel decides at run time."""
    frames, cams = _inputs(pkg, orc, W, H)
    fmt = MOTIONS[motion]
    den, t_x = pkg.Denoiser(W, H), device_table(mixed_table())
    try:
        for radius, table, tol in FILTERED_CELLS:
            k, (rank, scale) = CLAMP_K[radius], filter_of(radius, table, tol)
            got = _run_cell(pkg, den, t_x, frames, cams, fmt, tol, radius, k, rank, scale, table)
            assert den.history_clamp() == (radius, k) and den.firefly_filter() == (rank, scale)
            assert den.object_motion() == ((t_x.data_ptr(), 9) if table else (None, 0))
            ref = mixed_model(pkg, orc, W, H, fmt, tol, radius, k, rank=rank, scale=scale, table=table)
            assert_frames_equal(got, ref, f"{W}x{H} {motion} radius {radius} k {k} rank {rank} scale {scale} table {table} tol {tol}")
    finally:
        den.free()


@pytest.mark.gpu
@pytest.mark.parametrize("leg", ["planar", "promised"])
@pytest.mark.parametrize("W,H", SIZES)
def test_filtered_kernels_on_the_planar_and_promised_legs_equal_the_model(pkg, orc, W, H, leg):
    """The diagonal of the matrix — radius 1 with rank 1, radius 3 with rank 3, table on, tol 0.3, camera path — through
    svgf_denoise_planar and on a pipelined context with inputs_ready = 1."""
    frames, cams = _inputs(pkg, orc, W, H)
    den, t_x = pkg.Denoiser(W, H, 0, pipelined=leg == "promised"), device_table(mixed_table())
    try:
        if leg == "promised" and den.pipeline_status() == 2:
            pytest.skip("the context's two streams share a hardware queue: the promise is refused")
        for radius, rank, scale in DIAGONAL:
            k = CLAMP_K[radius]
            got = _run_cell(pkg, den, t_x, frames, cams, None, 0.3, radius, k, rank, scale, True,
                            leg="planar" if leg == "planar" else "aos", promised=leg == "promised")
            ref = mixed_model(pkg, orc, W, H, None, 0.3, radius, k, rank=rank, scale=scale, table=True)
            assert_frames_equal(got, ref, f"{W}x{H} {leg} radius {radius} k {k} rank {rank} scale {scale}")
        if leg == "promised":
            assert den.is_pipelined()
    finally:
        den.free()


@pytest.mark.gpu
def test_non_finite_colours_behind_the_table_are_defined_inputs(pkg, orc):
    """The NaN / +-inf / +-1e38 sprinkling of test_firefly_filter.py::test_non_finite_colours_are_defined_inputs on frame 1 of
    mixed_sequence at 67x41: table on, tol 0.3, camera path, (rank, radius, k) = (1, 1, 1.0) and (3, 3, 2.5), scale 1.0."""
    W, H = 67, 41
    seq, X = mixed_sequence(pkg, orc, W, H), mixed_table()
    bad_values = [F(np.nan), F(np.inf), F(-np.inf), F(1e38), F(-1e38)]
    col1 = seq[1][0].copy()
    flat = col1.reshape(-1, 3)
    pick = np.linspace(0, W * H - 2, 9 * len(bad_values)).astype(int)
    for j, i in enumerate(pick):
        v, where = bad_values[j % len(bad_values)], (j // len(bad_values)) % 3      # one channel, two, all three
        flat[i, :where + 1] = v
        if j % 2:                                                                    # and its right-hand neighbour: another value
            flat[i + 1, :] = bad_values[(j + 1) % len(bad_values)]
    frames, cams = _inputs(pkg, orc, W, H)
    frames[1] = (col1, frames[1][1])
    views = [seq[max(f - 1, 0)][3] for f in range(len(seq))]
    den, t_x = pkg.Denoiser(W, H), device_table(X)
    try:
        for rank, radius, k in ((1, 1, 1.0), (3, 3, 2.5)):
            ref = tm.run_sequence([(ff.firefly_filter(c, rank, 1.0), g) for c, g in frames], tables=[X] * len(frames), views=views,
                                  scale=scales(pkg, W, H), pos_tol=0.3, radius=radius, k=k)
            assert np.isnan(ref[1]["color"]).any() and np.isnan(ref[3]["color"]).any(), "non-finite values reach the history"
            assert np.isfinite(ref[3]["color"]).sum() > ref[3]["color"].size // 2
            got = _run_cell(pkg, den, t_x, frames, cams, None, 0.3, radius, k, rank, 1.0, True)
            assert_frames_equal(got, ref, f"non-finite colours, rank {rank} radius {radius} k {k}")
    finally:
        den.free()


# ---- 3. GPU: the filtered kernel's run-time choices against the specialised kernels ----------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("motion", list(MOTIONS))
def test_filtered_kernel_that_filters_nothing_is_the_clamped_kernel(pkg, orc, motion):
    """67x41, the table set, radius 1 to 3, both tols.  Context A: filter rank 1, scale 3.0e38 — k_temporal_filtered<R>, whose bound
    no colour of the sequence exceeds (test_model_the_pass_through_scale_returns_the_colours; svgf_set_firefly_filter accepts every
    finite scale, so 3.0e38 stands as asked).  Context B: filter off — k_temporal_clamped<MOTION, true, R>.  Every state of every
    frame agrees on its bits: the run-time motion input and the table behind `gid < n_geoms` compute what the template
    parameters compute.  The positions of mixed_sequence are non-finite in places, its colours are not: the filter's NaN rules
    stay inert."""
    W, H = 67, 41
    frames, cams = _inputs(pkg, orc, W, H)
    fmt = MOTIONS[motion]
    a, b, t_x = pkg.Denoiser(W, H), pkg.Denoiser(W, H), device_table(mixed_table())
    try:
        for radius in (1, 2, 3):
            for tol in TOLS:
                k = CLAMP_K[radius]
                on = _run_cell(pkg, a, t_x, frames, cams, fmt, tol, radius, k, 1, PASS_THROUGH_SCALE, True)
                off = _run_cell(pkg, b, t_x, frames, cams, fmt, tol, radius, k, 0, 1.0, True)
                assert a.firefly_filter() == (1, float(F(PASS_THROUGH_SCALE))) and b.firefly_filter()[0] == 0
                for f in range(len(frames)):
                    for name in STATES:
                        assert same_bits(on[f][name], off[f][name]), f"{motion} radius {radius} k {k} tol {tol}: {name}, frame {f}"
    finally:
        a.free(); b.free()
