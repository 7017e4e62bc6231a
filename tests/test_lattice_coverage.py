"""What the lattice kernel's tests cover, pinned without a GPU.

k_atrous_lattice (csrc/svgf_atrous_lattice.hip) runs the a-trous levels of steps 64 and 128.  lattice_geometry()
(csrc/svgf_atrous_geometry.hip) gives a workgroup K = 1, 2, 4 or 8 adjacent x-phases of one y-phase, and cuts a sub-image that is
taller than the LDS budget allows into n_bands row bands of band_rows lattice rows, each staging two lattice rows of its neighbours.
Which of those paths a test runs depends on the frame size alone, so a change of the geometry can empty a test without failing it
(that happened: 3840 x 640 was once banded and is one band today).  This module holds

  * GEOMETRY: the sizes tests/test_lattice_gpu.py runs, with (log2k, n_bands, band_rows) at both steps, compared with the library
    (binding.atrous_geometry; host arithmetic, no device), and the coverage conditions over that table: every K, one / two / three
    bands, a short last band, bands at both steps, and for each K > 1 a width whose last lattice column ends inside a group of K
    phases (the kernel's `if (x >= W) continue`).  K = 1 with several bands is left out on purpose: K = 1 is chosen only
    where eight lattice rows of two phases overflow the LDS budget, a band of one phase then still holds 20 and more rows, and the
    smallest such frame has about 11 M pixels (7500 x 1409), more than a test here can afford an oracle for.
  * the inputs: with the reference's default sigmas a tap 64 - 256 pixels away has next to no weight, and levels 6 - 7 change
    nothing that a test could see.  The lattice tests use FRAME_SEED / WIDE_SIGMAS, and the oracle alone shows here that with them
    both levels move at least 90 % of all pixels by more than 1e-3 (25 times the kernel's bar) and at least 80 % of the pixels of
    every image row by more than 1e-4.  These are conditions on the inputs, not tolerances on a kernel: where a frame misses them,
    the frame is changed."""
import numpy as np
import pytest

from conftest import relerr

# (W, H) -> {step: (log2k, n_bands, band_rows)}
GEOMETRY = {
    (64, 1300): {64: (3, 2, 11), 128: (3, 1, 11)},
    (130, 2500): {64: (3, 3, 14), 128: (3, 2, 10)},
    (97, 2400): {64: (3, 3, 13), 128: (3, 2, 10)},
    (2102, 1217): {64: (2, 2, 10), 128: (2, 1, 10)},
    (4201, 1400): {64: (1, 2, 11), 128: (2, 1, 11)},
    (7500, 520): {64: (0, 1, 9), 128: (2, 1, 5)},
    (1920, 1080): {64: (2, 1, 17), 128: (2, 1, 9)},
    (3840, 2160): {64: (1, 2, 17), 128: (2, 1, 17)},
}
STEPS = (64, 128)
SMALL_SIZES = [(64, 1300), (130, 2500), (97, 2400)]       # the oracle takes 0.1 - 0.4 s per run on 16 threads
LDS_BUDGET = 150 * 1024
STAGED_PIXEL_BYTES = 48

FRAME_SEED = 7
WIDE_SIGMAS = dict(sigma_x=8.0, sigma_l=16.0, sigma_n=4.0)
MIN_CHANGED, MIN_CHANGED_PER_ROW = 0.90, 0.80             # of all pixels by > 1e-3, of every row's pixels by > 1e-4


def size_id(size):
    return f"{size[0]}x{size[1]}"


def lattice_rows(H, step):
    return (H + step - 1) // step


def last_band_rows(H, step, n_bands, band_rows):
    return lattice_rows(H, step) - (n_bands - 1) * band_rows


def lattice_params(pkg, **kw):
    """Sigmas wide enough for taps 64 - 256 pixels away to count; no temporal pass, 7 levels (steps 2 .. 128) unless `kw` says
    otherwise."""
    return pkg.reference_defaults().set(temporal_enable=0, spatial_enable=1, atrous_nlevel=7, history_level=7, **WIDE_SIGMAS).set(**kw)


def frame_and_params(pkg, W, H, **kw):
    """The lattice tests' frame and parameters: unstructured colours over patches of constant geometry, lattice_params()."""
    c, g = pkg.synth.random_frame(W, H, seed=FRAME_SEED)
    cam = pkg.synth.camera_for_frame(0, False)
    p = lattice_params(pkg, **kw)
    if p.paper_steps:
        # Eight levels (steps 1 .. 128) flatten the uniform colours so far that the last one moves only 81 - 92 % of the pixels by
        # more than 1e-3 (oracle, the small sizes).  Cubed, the colours spread about twice as wide around their mean (0 .. 8, mean
        # 2, deviation 2.3) and the last level moves at least 97 %.
        c = c ** 3
    return c, g, cam, p


TEMPORAL_SIZE = (130, 2500)


def temporal_frames(pkg):
    """Two frames of the ray-cast scene under a static camera: the second one's history is an accumulated one (random_frame's
    positions do not reproject), and with the wide sigmas levels 6 and 7 change it as they change the random frames."""
    return [pkg.synth.render_frame(*TEMPORAL_SIZE, f, seed=FRAME_SEED, moving=False) for f in range(2)]


def changed_fractions(cur, prev):
    """(share of all pixels that differ by more than 1e-3, smallest share over the image rows of pixels that differ by more than
    1e-4); relerr, maximum over the channels."""
    e = relerr(cur, prev).max(axis=2)
    return float((e > 1e-3).mean()), float((e > 1e-4).mean(axis=1).min())


def assert_level_changes_the_frame(cur, prev, what):
    frac, row_frac = changed_fractions(cur, prev)
    print(f"{what}: changes {100 * frac:.1f} % of the pixels by > 1e-3, at least {100 * row_frac:.1f} % of every row by > 1e-4")
    assert frac >= MIN_CHANGED and row_frac >= MIN_CHANGED_PER_ROW, \
        f"{what}: the level barely changes this frame ({frac:.3f} of the pixels, {row_frac:.3f} of the weakest row): change the input"


@pytest.mark.experiments
@pytest.mark.parametrize("size", list(GEOMETRY), ids=size_id)
def test_table_is_the_geometry_the_library_launches(pkg, size):
    W, H = size
    for step in STEPS:
        out, est = pkg.binding.atrous_geometry("lattice", W, H, step)
        supported, log2k, pstride, band_rows, n_bands, grid, threads, lds = out
        assert supported, f"{W}x{H} step {step}: the lattice kernel does not run this level (the planner would fall back to gather)"
        assert (log2k, n_bands, band_rows) == GEOMETRY[size][step], f"{W}x{H} step {step}: library {(log2k, n_bands, band_rows)}"
        K, tw, mh = 1 << log2k, (W + step - 1) // step + 4, lattice_rows(H, step)
        # the bands cover the sub-image, none is empty, and the tile of a band fits the budget
        assert (n_bands - 1) * band_rows < mh <= n_bands * band_rows
        assert lds == K * pstride * (band_rows + 4) * STAGED_PIXEL_BYTES <= LDS_BUDGET
        assert grid == step * step // K * n_bands and threads == 1024
        # padding of a phase row: the 16 lanes of a b128 LDS access fall on distinct bank groups (lattice_geometry())
        assert pstride >= tw
        if K > 1:
            assert (12 * pstride) % 64 == {2: 32, 4: 48, 8: 24}[K] and pstride - tw < 16, (K, tw, pstride)
        else:
            assert pstride == tw


def test_table_covers_every_path_of_the_kernel():
    launches = [(size, step) + GEOMETRY[size][step] for size in GEOMETRY for step in STEPS]
    assert {1 << log2k for _, _, log2k, _, _ in launches} == {1, 2, 4, 8}
    assert {n_bands for _, _, _, n_bands, _ in launches} == {1, 2, 3}
    banded = [(size, step, n, rows) for size, step, _, n, rows in launches if n > 1]
    assert {step for _, step, _, _ in banded} == set(STEPS), "row bands at step 64 and at step 128"
    assert any(0 < last_band_rows(H, step, n, rows) < rows for (_, H), step, n, rows in banded), "a last band shorter than the others"
    for K in (2, 4, 8):
        # W mod step is where the last lattice column ends; inside a group of K phases the group's later phases are narrower
        assert any((W % step) % K for (W, _), step, log2k, _, _ in launches if 1 << log2k == K), f"K = {K}: no group with narrower phases"
    # the GPU tests generate the small sizes' seam cases from these
    assert all(GEOMETRY[size][64][1] > 1 for size in SMALL_SIZES)


@pytest.mark.parametrize("size", SMALL_SIZES, ids=size_id)
def test_levels_6_and_7_change_the_frames_the_gpu_tests_use(pkg, orc, size):
    W, H = size
    o = orc.Oracle(pkg, W, H, threads=16)
    levels = {}
    for paper_steps, ks in ((0, (5, 6, 7)), (1, (6, 7, 8))):      # steps 32, 64, 128 either way
        for k in ks:
            c, g, cam, p = frame_and_params(pkg, W, H, atrous_nlevel=k, history_level=k, paper_steps=paper_steps)
            o.reset()
            out = o.denoise(c, g, cam, p)
            levels[k] = o.read_state(2)
            assert np.array_equal(out, levels[k]), "without re-modulation the returned image is the last level"
            assert np.isfinite(out).all()
        for k in ks[1:]:
            assert_level_changes_the_frame(levels[k], levels[k - 1], f"{W}x{H} {'paper steps, ' if paper_steps else ''}level {k}")
    o.free()


def test_levels_6_and_7_change_the_temporal_frames_the_gpu_test_uses(pkg, orc):
    """test_lattice_gpu.test_lattice_levels_after_a_temporal_pass: the ray-cast scene, two frames, static camera."""
    W, H = TEMPORAL_SIZE
    o = orc.Oracle(pkg, W, H, threads=16)
    levels = {}
    for k in (5, 6, 7):
        o.reset()
        for c, g, cam in temporal_frames(pkg):
            o.denoise(c, g, cam, lattice_params(pkg, temporal_enable=1, atrous_nlevel=k, history_level=k))
        levels[k] = o.read_state(2)
    accumulated = float((o.read_state(0) > 1).mean())
    o.free()
    for k in (6, 7):
        assert_level_changes_the_frame(levels[k], levels[k - 1], f"{W}x{H} temporal, frame 2, level {k}")
    assert accumulated >= 0.5, f"only {accumulated:.3f} of the second frame's pixels have an accumulated history"
