"""The spatial variance estimate for short histories, SvgfParams::spatial_variance_frames = K (include/svgf.h; DESIGN.md 8 row
f4): k_spatial_variance (csrc/svgf_kernels.hip), launched by enqueue_frame behind the temporal pass, and the oracle's
svgf_oracle_spatial_variance — both against tests/temporal_model.py::spatial_variance, the float32 numpy model of the pass.

tests/test_f4_options.py compares the kernel with the oracle, two texts written together.  This file gives both a yardstick
that shares no loop with them, and then runs the kernel wherever the frame sequence can launch it.

1. CPU, what pins the model:
   - the oracle, on the bits of every pixel of every frame (noisy_sequence, seven sizes, K = 1, 2, 3, 4, 6);
   - a per-pixel float64 restatement written from the header's sentence, within the rounding of the float32 sums (the one
     derived bound of this file, see _restated);
   - named cases on hand-built 9x9 frames, each asserted by value, each through the model and through the oracle.
2. CPU, conditions on the inputs (not measurements): every cell of the GPU matrix acts, leaves pixels alone, meets the boost
   clamp, estimates of 0 and of +inf, and normal pairs on either side of the predicate's threshold.
3. GPU: the kernel against the model on the bits of all five states of every frame — K by motion input, the diagonal with
   table, position test, clamp and filter on the AoS, planar and promised legs, K changing from call to call and across
   svgf_reset, K that acts on nothing, the debug view, and the estimate's way into the a-trous levels under every kernel
   variant and on promised frames of a pipelined context, AoS and planar (there against the oracle at the project's bar for
   whole frames, relerr <= 1e-4, as test_f4_options.py has it).

Bounds: every comparison against the model is on bits (NaNs in the same place count as equal): both sides perform the same
correctly rounded float32 operations in the same order without contraction, so there is no tolerance to choose.

Sizes: 67x41 and 130x9 for tests/test_temporal_matrix.py's reasons (neither side of 67x41 a multiple of the kernel's 64 x 4
block; 130x9 has two column seams and a last block row one image row high); 1x1, 3x2 and 7x7 have windows larger than the
image, 64x4 is exactly one block and 65x5 one block plus one column and one row."""
import numpy as np
import pytest

from conftest import relerr
import temporal_model as tm
from temporal_harness import (NOISY_FRAMES, STATES, THRESHOLD_STEP, assert_frames_equal, device_table, mixed_model, mixed_table, noisy_sequence,
                              run_gpu, same_bits, synth_params)

F = np.float32
SIZES = [(67, 41), (130, 9)]
SMALL_SIZES = [(1, 1), (3, 2), (7, 7), (64, 4), (65, 5)]
KS_CPU = (1, 2, 3, 4, 6)
KS_GPU = (2, 3, 4, 6)
MOTIONS = {"camera": None, "coord_f32": tm.COORD, "delta_f32": tm.D32, "delta_f16": tm.D16}
CLAMP_K = {0: 0.0, 1: 1.0, 3: 2.5}
DIAGONAL = [(1, 1, 1.0), (3, 3, 1.5)]            # (radius, rank, scale) with K = 3 and 6: table on, tol 0.3, camera path
CALL_KS = (0, 4, 2, 6, 1, 3)
LEVELS, LEVELS_K = 3, 4
UNSUPPORTED = -5                                  # SVGF_ERR_UNSUPPORTED
U = 2.0 ** -24                                    # float32: the relative error of one correctly rounded operation


def plain_model(pkg, orc, W, H, K, **noisy):
    """The model on noisy_sequence: camera path, no table, no position test, clamp and filter off."""
    return mixed_model(pkg, orc, W, H, None, 0.0, table=False, svf=K, noisy=noisy)


def oracle_run(pkg, orc, W, H, K, levels=0, **noisy):
    """The oracle on noisy_sequence: per frame dict(hlen, mom, color, variance, out).  Computed once per session."""
    cache = oracle_run.__dict__.setdefault("cache", {})
    key = (W, H, K, levels, tuple(sorted(noisy.items())))
    if key not in cache:
        p = synth_params(pkg, W, H, spatial_variance_frames=K, spatial_enable=int(levels > 0), atrous_nlevel=max(levels, 1))
        o, res = orc.Oracle(pkg, W, H, threads=4), []
        for col, gb, cam, _ in noisy_sequence(pkg, orc, W, H, **noisy):
            out = o.denoise(col, gb, cam, p).reshape(H, W, 3)
            res.append(dict(hlen=o.read_state(0), mom=o.read_state(1), color=o.read_state(2), variance=o.read_state(3), out=out))
        o.free()
        cache[key] = res
    return cache[key]


# ---- 1. CPU: what pins the model -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", SIZES + SMALL_SIZES)
def test_model_is_the_oracle_on_bits(pkg, orc, W, H):
    for K in KS_CPU:
        ref, got = oracle_run(pkg, orc, W, H, K), plain_model(pkg, orc, W, H, K)
        assert len(ref) == len(got) == NOISY_FRAMES
        for f, (r, g) in enumerate(zip(ref, got)):
            assert np.array_equal(r["hlen"], g["hlen"]), f"{W}x{H} K {K}: history length, frame {f}"
            for name in ("mom", "variance"):
                assert same_bits(r[name], g[name]), f"{W}x{H} K {K}: {name}, frame {f}"


@pytest.mark.parametrize("W,H", SIZES + SMALL_SIZES)
def test_the_part_changes_the_variance_alone(pkg, orc, W, H):
    off, acted = plain_model(pkg, orc, W, H, 0), 0
    for K in KS_CPU + (CALL_KS,):
        on = plain_model(pkg, orc, W, H, K)
        for f, (a, b) in enumerate(zip(on, off)):
            for name in ("hlen", "mom", "color"):
                assert same_bits(a[name], b[name]), f"{W}x{H} K {K}: {name}, frame {f}"
            Kf = K[f] if isinstance(K, tuple) else K
            untouched = a["hlen"] >= Kf
            assert same_bits(a["variance"][untouched], b["variance"][untouched]), f"{W}x{H} K {K}: variance where hlen >= K, frame {f}"
            acted += int(np.count_nonzero(~untouched & ~same_each(a["variance"], b["variance"])))
    assert acted > 0 or W * H < 4, "the part changes some variance"


def same_each(a, b):
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def _restated(mom, hlen, normal, gid, K):
    """The header's sentence, per pixel, in float64: "a pixel whose updated history is shorter than K frames takes its variance
    from the luminance moments of its 7x7 neighbourhood: taps that pass the consistency predicate (same geomId, |n_q - n_p| <=
    0.1) count with weight 1, the pixel itself always; variance = max(0, mean(m2) - mean(m1)^2) * max(1, 4 / history length)".
    The predicate is defined on float32 values, so the distance alone is taken in float32; everything behind it is float64.
    Returns (estimate, bound, finite, acted): finite where every accepted tap's moments are finite.

    The bound on |float32 result - float64 result|, for n accepted taps, u = 2^-24, A = sum|m.x| / n, B = sum|m.y| / n:
    - a sum of n float32 terms added one by one errs by at most u times the sum of its partial sums' magnitudes, which is at most
      (n - 1) u S, S the sum of the magnitudes; the division by n adds u: mean(m2) errs by at most n u B.
    - mean(m1) errs in the same way, and the square doubles the relative error and rounds once itself: (2 n + 1) u A^2 in the
      worst case.  The bound takes less for this term, on an assumption about the inputs: the moments are luminances, none
      negative, and the accepted taps of one window (one surface under the predicate) are of like size, so that the partial
      sums of s1 come to about half of (n - 1) S.  Then ((n - 1) u / 2 + u) doubled, plus u, is (n + 2) u A^2.  A window whose
      first tap outweighs all the others together is outside the assumption and may exceed the bound by up to that factor of two
      on this term.
    - the subtraction rounds once, by at most u (B + A^2), and so does the product with the boost (4 / hlen is exact at history
      lengths 1, 2 and 4 and rounds once at 3): (n + 2) u B + (n + 4) u A^2 in all, no more than (n + 4) u (B + A^2), times the
      boost.
    Where the float64 value lies below the bound the float32 value may be 0 (the cancellation on a flat colour); it is never
    negative, which the caller asserts apart."""
    H, W = hlen.shape
    mom64 = mom.astype(np.float64)
    est, bound = np.zeros((H, W)), np.zeros((H, W))
    finite, acted = np.zeros((H, W), bool), hlen < K
    for y, x in zip(*np.nonzero(acted)):
        taps = []
        for qy in range(max(0, y - 3), min(H, y + 4)):
            for qx in range(max(0, x - 3), min(W, x + 4)):
                if (qy, qx) == (y, x):
                    taps.append((qy, qx))
                elif gid[qy, qx] == gid[y, x]:
                    d = normal[qy, qx] - normal[y, x]
                    with np.errstate(all="ignore"):
                        dist = np.sqrt(F(F(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
                    if dist <= F(0.1):
                        taps.append((qy, qx))
        m = np.array([mom64[t] for t in taps])
        finite[y, x] = np.isfinite(m).all()
        if not finite[y, x]:
            continue
        n = len(taps)
        boost = max(1.0, 4.0 / int(hlen[y, x]))
        est[y, x] = max(0.0, m[:, 1].mean() - m[:, 0].mean() ** 2) * boost
        bound[y, x] = (n + 4) * U * (np.abs(m[:, 1]).sum() / n + (np.abs(m[:, 0]).sum() / n) ** 2) * boost
    return est, bound, finite, acted


@pytest.mark.parametrize("W,H", SIZES + SMALL_SIZES)
def test_model_is_the_float64_restatement_within_rounding(pkg, orc, W, H):
    """K = 6 on every frame.  The restatement reads the oracle's K = 0 states (the part leaves them as they are) and the frame's
    own texels; the model's and the oracle's variances are held to it."""
    K, seq = 6, noisy_sequence(pkg, orc, W, H)
    states, model, oracle = oracle_run(pkg, orc, W, H, 0), plain_model(pkg, orc, W, H, K), oracle_run(pkg, orc, W, H, K)
    compared, worst = 0, 0.0
    for f in range(NOISY_FRAMES):
        gb = seq[f][1]
        est, bound, finite, acted = _restated(states[f]["mom"], states[f]["hlen"], gb["normal"], gb["geomId"], K)
        assert np.array_equal(acted, model[f]["hlen"] < K)
        for name, got in (("model", model[f]["variance"]), ("oracle", oracle[f]["variance"])):
            v = got[finite].astype(np.float64)
            assert np.isfinite(v).all() and (v >= 0).all(), f"{W}x{H} frame {f}: {name}"
            err = np.abs(v - est[finite])
            assert (err <= bound[finite]).all(), f"{W}x{H} frame {f}, {name}: {int((err > bound[finite]).sum())} pixels beyond the bound"
            worst = max(worst, float((err / np.maximum(bound[finite], 1e-300)).max(initial=0.0)))
        compared += int(finite.sum())
    print(f"{W}x{H}: {compared} pixels compared, largest error / bound {worst:.3f}")
    assert compared >= (W * H) // 2, "most pixels have finite windows on some frame"


# ---- named cases on a hand-built 9x9 frame ---------------------------------------------------------------------------------------------------
N9, C9, MARK = 9, (4, 4), F(7.0)      # side, the pixel most cases look at, the variance the temporal pass is taken to have left
BOOST = {1: F(4), 2: F(2), 3: F(4) / F(3), 4: F(1), 5: F(1)}
WINDOW = [(y, x) for y in range(1, 8) for x in range(1, 8)]      # the 49 taps of C9


def _frame(pkg):
    """gid 0, normal (0, 0, 1), history length 1 everywhere; moments small integers that differ from tap to tap (their sums are
    exact in float32 in any order), with one loud tap to the right of C9 so that counting it or not shows."""
    ys, xs = np.mgrid[0:N9, 0:N9]
    m1 = ((3 * ys + 5 * xs) % 7).astype(F)
    m2 = (m1 * m1 + ((ys * xs) % 3).astype(F)).astype(F)
    mom = np.stack([m1, m2], axis=-1)
    mom[4, 5] = (50.0, 2600.0)
    gb = np.zeros((N9, N9), pkg.synth.GBUFFER_DTYPE)
    gb["normal"] = (0.0, 0.0, 1.0)
    return dict(mom=mom, hlen=np.ones((N9, N9), np.int32), gb=gb, variance=np.full((N9, N9), MARK, F))


def _both(pkg, orc, fr, K=6):
    """The estimate through the model, after the oracle's has been held to it on bits."""
    got = tm.spatial_variance(fr["variance"], fr["mom"], fr["hlen"], fr["gb"]["normal"], fr["gb"]["geomId"], K)
    ref = orc.spatial_variance(pkg, fr["variance"], fr["mom"], fr["hlen"], fr["gb"], K)
    assert same_bits(got, ref), "model and oracle"
    return got


def _expect(fr, taps, at=C9):
    """max(0, mean(m2) - mean(m1)^2) * boost over the named taps, in float32 scalar operations (the sums are exact)."""
    n = F(len(taps))
    s1, s2 = F(sum(float(fr["mom"][t][0]) for t in taps)), F(sum(float(fr["mom"][t][1]) for t in taps))
    with np.errstate(all="ignore"):
        m1, m2 = s1 / n, s2 / n
        v = m2 - m1 * m1
        return F((v if v > 0 else F(0)) * BOOST[int(fr["hlen"][at])])


def _without(taps, *gone):
    return [t for t in taps if t not in gone]


def test_case_the_loud_tap_shows(pkg, orc):
    fr = _frame(pkg)
    assert _both(pkg, orc, fr)[C9] == _expect(fr, WINDOW) != _expect(fr, _without(WINDOW, (4, 5))) and _expect(fr, WINDOW) > 0


def test_case_the_centre_counts_under_its_own_nan_normal(pkg, orc):
    fr = _frame(pkg)
    fr["gb"]["normal"][C9] = np.nan
    fr["mom"][C9] = (2.0, 9.0)
    assert _both(pkg, orc, fr)[C9] == _expect(fr, [C9]) == F(20.0)      # every neighbour rejected: (9 - 2^2) * 4


def test_case_a_neighbour_with_a_nan_normal_is_skipped(pkg, orc):
    for lane in range(3):
        fr = _frame(pkg)
        fr["gb"]["normal"][4, 5][lane] = np.nan
        assert _both(pkg, orc, fr)[C9] == _expect(fr, _without(WINDOW, (4, 5)))


def test_case_distance_of_exactly_a_tenth_is_accepted_and_the_next_float_rejected(pkg, orc):
    assert THRESHOLD_STEP[0] == F(0.1) and THRESHOLD_STEP[1] == np.nextafter(F(0.1), F(1)) == F(0.10000001)
    for lane in range(2):
        for step, taps in ((THRESHOLD_STEP[0], WINDOW), (THRESHOLD_STEP[1], _without(WINDOW, (4, 5))),
                           (-THRESHOLD_STEP[0], WINDOW), (-THRESHOLD_STEP[1], _without(WINDOW, (4, 5)))):
            fr = _frame(pkg)
            fr["gb"]["normal"][4, 5][lane] = step      # (0, 0, 1) and (step, 0, 1): sqrt(step^2) is step exactly
            assert _both(pkg, orc, fr)[C9] == _expect(fr, taps), (lane, step)


def test_case_another_geom_id_is_rejected(pkg, orc):
    fr = _frame(pkg)
    fr["gb"]["geomId"][4, 5] = 3
    assert _both(pkg, orc, fr)[C9] == _expect(fr, _without(WINDOW, (4, 5)))


def test_case_ray_misses_accept_each_other(pkg, orc):
    fr = _frame(pkg)
    fr["gb"]["geomId"][:] = -1
    assert _both(pkg, orc, fr)[C9] == _expect(fr, WINDOW)
    fr = _frame(pkg)
    fr["gb"]["geomId"][C9] = fr["gb"]["geomId"][4, 5] = fr["gb"]["geomId"][1, 1] = -1
    assert _both(pkg, orc, fr)[C9] == _expect(fr, [(1, 1), C9, (4, 5)])


def test_case_corner_and_edge_windows(pkg, orc):
    fr = _frame(pkg)
    got = _both(pkg, orc, fr)
    corners = {(0, 0): (range(0, 4), range(0, 4)), (8, 8): (range(5, 9), range(5, 9)), (0, 8): (range(0, 4), range(5, 9))}
    edges = {(0, 4): (range(0, 4), range(1, 8)), (4, 0): (range(1, 8), range(0, 4)), (8, 4): (range(5, 9), range(1, 8))}
    for n, cases in ((16, corners), (28, edges)):
        for at, (rows, cols) in cases.items():
            taps = [(y, x) for y in rows for x in cols]
            assert len(taps) == n and got[at] == _expect(fr, taps, at), at
    assert len({float(got[at]) for at in list(corners) + list(edges)}) > 3, "the windows differ"


def test_case_the_boost_by_history_length(pkg, orc):
    fr = _frame(pkg)
    base = None
    for hl, boost in ((1, 4.0), (2, 2.0), (3, 4.0 / 3.0), (4, 1.0), (5, 1.0)):
        fr["hlen"][C9] = hl
        got = _both(pkg, orc, fr)[C9]
        assert got == _expect(fr, WINDOW)
        base = got / F(4) if hl == 1 else base
        assert got == F(base * F(boost)), hl      # (base is a float32 value: a quarter of it times four is exact)
    assert base > 0


def test_case_a_nan_moment_in_the_window_gives_zero(pkg, orc):
    for lane in range(2):
        fr = _frame(pkg)
        fr["mom"][4, 5][lane] = np.nan
        got = _both(pkg, orc, fr)[C9]
        assert got == 0 and not np.signbit(got)


def test_case_a_1e20_neighbour_gives_inf(pkg, orc):
    fr = _frame(pkg)
    with np.errstate(over="ignore"):
        fr["mom"][4, 5] = (F(1e20), F(1e20) * F(1e20))      # what the temporal pass leaves of a luminance of 1e20: (1e20, +inf)
    assert np.isposinf(fr["mom"][4, 5][1])
    assert np.isposinf(_both(pkg, orc, fr)[C9])


def test_case_a_bright_flat_patch_never_goes_negative(pkg, orc):
    for lum in (F(1000.0), F(1000.1), F(999.9)):
        fr = _frame(pkg)
        fr["mom"][...] = (lum, lum * lum)
        got = _both(pkg, orc, fr)
        bound = (49 + 4) * U * 2.0 * float(lum) ** 2 * 4.0      # _restated's bound for 49 taps of (lum, lum^2), boost 4
        assert (got >= 0).all() and not np.signbit(got).any() and (got <= bound).all(), (lum, got.max(), bound)
    fr["mom"][...] = (F(1000.0), F(1000.0) * F(1000.0))           # every partial sum is exact: nothing is left
    assert (_both(pkg, orc, fr) == 0).all()


def test_case_a_history_of_k_frames_keeps_the_temporal_variance(pkg, orc):
    for K in (2, 3, 4, 6):
        fr = _frame(pkg)
        fr["hlen"][:, :5] = K
        fr["hlen"][:, 5:] = K - 1
        got = _both(pkg, orc, fr, K)
        assert (got[:, :5] == MARK).all() and (got[:, 5:] != MARK).all(), K
        fr["hlen"][:, :5] = K + 1
        assert (_both(pkg, orc, fr, K)[:, :5] == MARK).all(), K


def test_case_k_of_one_or_less_acts_on_nothing(pkg, orc):
    fr = _frame(pkg)
    for K in (1, 0, -3):
        assert (_both(pkg, orc, fr, K) == MARK).all(), K
    W, H = 67, 41
    for run in (lambda K: plain_model(pkg, orc, W, H, K), lambda K: oracle_run(pkg, orc, W, H, K)):
        off = run(0)
        for K in (1, -3):
            for f, (a, b) in enumerate(zip(run(K), off)):
                for name in ("hlen", "mom", "color", "variance"):
                    assert same_bits(a[name], b[name]), f"K {K}: {name}, frame {f}"


# ---- 2. CPU: the inputs act ------------------------------------------------------------------------------------------------------------------
def _threshold_pairs(gb, acted):
    """How many acted pixels have a right-hand neighbour of their geomId at a normal distance of exactly 0.1f (accepted), and how
    many at one above it by no more than 2^-20 of it (rejected)."""
    n, g = gb["normal"], gb["geomId"]
    with np.errstate(all="ignore"):
        d = n[:, :-1] - n[:, 1:]
        s = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
        dist = np.sqrt(s + d[..., 2] * d[..., 2])
        same = (g[:, :-1] == g[:, 1:]) & acted[:, :-1]
        return (int(np.count_nonzero(same & (dist == F(0.1)))),
                int(np.count_nonzero(same & (dist > F(0.1)) & (dist <= F(0.1) * F(1 + 2.0 ** -20)))))


@pytest.mark.parametrize("W,H", SIZES)
def test_model_every_cell_of_the_gpu_matrix_acts(pkg, orc, W, H):
    """Conditions, not measurements, on the last frame: a cell whose K left every pixel alone, or whose estimates were all 0,
    would hold a smaller kernel than it names."""
    last_gb = noisy_sequence(pkg, orc, W, H)[-1][1]
    for K in KS_GPU:
        r = plain_model(pkg, orc, W, H, K)[-1]
        acted = r["hlen"] < K
        est = r["variance"][acted]
        n_acted, n_left = int(acted.sum()), int((~acted).sum())
        n_pos, n_zero, n_inf = int((est > 0).sum()), int((est == 0).sum()), int(np.isposinf(est).sum())
        n_acc, n_rej = _threshold_pairs(last_gb, acted)
        print(f"{W}x{H} K {K}: acted {n_acted}, untouched {n_left}, estimate > 0 {n_pos}, = 0 {n_zero}, +inf {n_inf}, at hlen 5 "
              f"{int((r['hlen'][acted] == 5).sum())}, threshold pairs accepted {n_acc}, rejected {n_rej}")
        if K in (2, 3, 4):
            assert n_acted >= 20 and n_left >= 20
        if K == 6:
            assert int((r["hlen"][acted] == 5).sum()) >= 5, "the boost clamp"
        assert 2 * n_pos >= n_acted and n_zero >= 20 and n_inf >= 1
        assert n_acc >= 1 and n_rej >= 1
        # the same moments and history lengths, the texels without the threshold edits: the pairs are what moves the variance
        plain_gb = noisy_sequence(pkg, orc, W, H, threshold_edits=False)[-1][1]
        k0 = plain_model(pkg, orc, W, H, 0)[-1]
        other = tm.spatial_variance(k0["variance"], r["mom"], r["hlen"], plain_gb["normal"], plain_gb["geomId"], K)
        assert not same_bits(other, r["variance"]), "dropping the threshold edits changes some pixel's variance"


def test_the_estimate_reaches_the_levels_on_the_oracle(pkg, orc):
    for W, H in SIZES:
        seq = noisy_sequence(pkg, orc, W, H, finite=True)
        assert np.isfinite(np.stack([c for c, _, _, _ in seq])).all() and max(c.max() for c, _, _, _ in seq) == F(1000.0)
        on, off = plain_model(pkg, orc, W, H, LEVELS_K, finite=True)[-1], plain_model(pkg, orc, W, H, 0, finite=True)[-1]
        assert not same_bits(on["variance"], off["variance"]), "K = 4 changes the last frame's state 3"
        a, b = oracle_run(pkg, orc, W, H, LEVELS_K, LEVELS, finite=True)[-1], oracle_run(pkg, orc, W, H, 0, LEVELS, finite=True)[-1]
        assert same_bits(a["variance"], on["variance"])
        for K in (0, LEVELS_K):      # nothing non-finite in what the levels read or write, on any frame
            for r in oracle_run(pkg, orc, W, H, K, LEVELS, finite=True):
                assert np.isfinite(r["variance"]).all() and np.isfinite(r["mom"]).all() and np.isfinite(r["out"]).all()
        changed = float((a["out"] != b["out"]).any(axis=-1).mean())
        print(f"{W}x{H}: K = {LEVELS_K} changes {100 * changed:.1f} % of the oracle's output pixels")
        assert changed > 0.10


# ---- 3. GPU ------------------------------------------------------------------------------------------------------------------------------------
def _inputs(pkg, orc, W, H, **noisy):
    seq = noisy_sequence(pkg, orc, W, H, **noisy)
    return [(c, g) for c, g, _, _ in seq], [c for _, _, c, _ in seq]


def _run_cell(pkg, den, frames, cams, K, fmt=None, tol=0.0, radius=0, rank=0, scale=1.0, t_x=None, leg="aos", promised=False, **kw):
    """One cell on `den`: svgf_reset, every setting given anew, the frames.  K: one value or one per frame.  The plane, where one is
    used, is written on the device by svgf_motion_reproject with the same table (none: without)."""
    H, W = frames[0][1].shape
    Ks = [K] * len(frames) if np.isscalar(K) else list(K)
    params = [synth_params(pkg, W, H, reproj_position_tol=tol, spatial_variance_frames=k) for k in Ks]
    for p in params:
        p.inputs_ready = int(promised)
    den.reset()
    den.set_object_motion(t_x)
    den.set_history_clamp(radius, CLAMP_K[radius])
    den.set_firefly_filter(rank, scale)
    return run_gpu(pkg, den, frames, params, cams, leg=leg, plane_fmt=fmt,
                   plane_tables=None if t_x is None else [mixed_table()] * len(frames), **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("motion", list(MOTIONS))
@pytest.mark.parametrize("W,H", SIZES)
def test_kernel_equals_the_model_for_every_k_and_motion_input(pkg, orc, W, H, motion):
    frames, cams = _inputs(pkg, orc, W, H)
    fmt = MOTIONS[motion]
    den = pkg.Denoiser(W, H)
    try:
        for K in KS_GPU:
            got = _run_cell(pkg, den, frames, cams, K, fmt=fmt)
            assert_frames_equal(got, mixed_model(pkg, orc, W, H, fmt, 0.0, table=False, svf=K, noisy={}), f"{W}x{H} {motion} K {K}")
    finally:
        den.free()


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", SMALL_SIZES)
def test_kernel_equals_the_model_on_small_images(pkg, orc, W, H):
    """The window larger than the image, the exact block, the block plus one: AoS leg, camera path."""
    frames, cams = _inputs(pkg, orc, W, H)
    den = pkg.Denoiser(W, H)
    try:
        for K in KS_GPU:
            assert_frames_equal(_run_cell(pkg, den, frames, cams, K), plain_model(pkg, orc, W, H, K), f"{W}x{H} K {K}")
    finally:
        den.free()


@pytest.mark.gpu
@pytest.mark.parametrize("leg", ["aos", "planar", "promised"])
@pytest.mark.parametrize("W,H", SIZES)
def test_kernel_equals_the_model_with_everything_on(pkg, orc, W, H, leg):
    """Table on, tol 0.3, clamp and filter on (the temporal kernels of the matrix suite's diagonal), K = 3 and 6, through
    svgf_denoise, svgf_denoise_planar and a pipelined context with inputs_ready = 1 (the matrix suite's promised leg: the frames
    alternate between the context's two plane sets; with the levels off the promise itself is not taken up and they run on the
    caller's stream.  test_the_estimate_on_pipelined_frames has the promised frames on the context's own streams)."""
    frames, cams = _inputs(pkg, orc, W, H)
    den, t_x = pkg.Denoiser(W, H, 0, pipelined=leg == "promised"), device_table(mixed_table())
    try:
        if leg == "promised" and den.pipeline_status() == 2:
            pytest.skip("the context's two streams share a hardware queue: the promise is refused")
        for radius, rank, scale in DIAGONAL:
            for K in (3, 6):
                got = _run_cell(pkg, den, frames, cams, K, tol=0.3, radius=radius, rank=rank, scale=scale, t_x=t_x,
                                leg="planar" if leg == "planar" else "aos", promised=leg == "promised")
                ref = mixed_model(pkg, orc, W, H, None, 0.3, radius, CLAMP_K[radius], rank=rank, scale=scale, table=True, svf=K, noisy={})
                assert_frames_equal(got, ref, f"{W}x{H} {leg} radius {radius} rank {rank} scale {scale} K {K}")
        if leg == "promised":
            assert den.is_pipelined()
    finally:
        den.free()


@pytest.mark.gpu
@pytest.mark.parametrize("reset_before", [(), (3,)])
@pytest.mark.parametrize("W,H", SIZES)
def test_k_is_a_function_of_the_call(pkg, orc, W, H, reset_before):
    """K = 0, 4, 2, 6, 1, 3 over six frames of one context; with svgf_reset before frame 3 every history length is 1 there and
    K = 6 acts on every pixel."""
    frames, cams = _inputs(pkg, orc, W, H)
    ref = mixed_model(pkg, orc, W, H, None, 0.0, table=False, svf=CALL_KS, noisy={}, reset_before=reset_before)
    if reset_before:
        assert (ref[3]["hlen"] == 1).all() and CALL_KS[3] == 6
    den = pkg.Denoiser(W, H)
    try:
        assert_frames_equal(_run_cell(pkg, den, frames, cams, CALL_KS, reset_before=reset_before), ref, f"{W}x{H} K per call, reset {reset_before}")
    finally:
        den.free()


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", SIZES)
def test_k_that_acts_on_nothing_is_k_zero(pkg, orc, W, H):
    frames, cams = _inputs(pkg, orc, W, H)
    a, b = pkg.Denoiser(W, H), pkg.Denoiser(W, H)
    try:
        off = _run_cell(pkg, b, frames, cams, 0)
        assert_frames_equal(off, plain_model(pkg, orc, W, H, 0), f"{W}x{H} K 0")
        for K in (1, -3):
            for f, (g, r) in enumerate(zip(_run_cell(pkg, a, frames, cams, K), off)):
                for name in STATES:
                    assert same_bits(g[name], r[name]), f"{W}x{H} K {K} against K 0: {name}, frame {f}"
    finally:
        a.free(); b.free()


@pytest.mark.gpu
def test_debug_view_shows_the_estimate(pkg, orc):
    """right_view_option = 2 on frame 2, K = 4, 67x41: out = variance / 0.1f in three channels (correctly rounded on both sides)."""
    W, H, K = 67, 41, 4
    frames, cams = _inputs(pkg, orc, W, H)
    frames, cams = frames[:3], cams[:3]
    params = [synth_params(pkg, W, H, spatial_variance_frames=K, right_view_option=2 if f == 2 else 0) for f in range(3)]
    ref = plain_model(pkg, orc, W, H, K)[2]["variance"]
    assert int(np.count_nonzero(ref != plain_model(pkg, orc, W, H, 0)[2]["variance"])) > 20
    den, outs = pkg.Denoiser(W, H), []
    try:
        got = run_gpu(pkg, den, frames, params, cams, outputs=outs)
    finally:
        den.free()
    assert same_bits(got[2]["variance"], ref)
    with np.errstate(all="ignore"):
        want = (ref / F(0.1)).astype(F)
    assert same_bits(outs[2].reshape(H, W, 3), np.repeat(want[..., None], 3, axis=-1))


REFUSALS = set()      # (W, H, variant) that answer SVGF_ERR_UNSUPPORTED: none — steps 2, 4 and 8 are within every kernel's range at both sizes


def _levels_cell(pkg, orc, W, H, variant, leg="aos", pipelined=False):
    """spatial_enable = 1, three levels, K = 4, finite inputs, on one context: the output against the oracle at relerr <= 1e-4 (the
    bar of tests/test_f4_options.py); history lengths, moments and state 3 against the model on bits.  pipelined: a context
    created with the frame pipeline's resources, every frame promised (inputs_ready = 1)."""
    frames, cams = _inputs(pkg, orc, W, H, finite=True)
    params = synth_params(pkg, W, H, spatial_variance_frames=LEVELS_K, spatial_enable=1, atrous_nlevel=LEVELS, kernel_variant=variant,
                          inputs_ready=int(pipelined))
    ref, model = oracle_run(pkg, orc, W, H, LEVELS_K, LEVELS, finite=True), plain_model(pkg, orc, W, H, LEVELS_K, finite=True)
    den, outs = pkg.Denoiser(W, H, 0, pipelined=pipelined), []
    try:
        if pipelined and den.pipeline_status() == 2:
            pytest.skip("the context's two streams share a hardware queue: the promise is refused")
        if (W, H, variant) in REFUSALS:
            with pytest.raises(pkg.binding.SvgfError, match=f"-> {UNSUPPORTED}:"):
                run_gpu(pkg, den, frames[:1], params, cams[:1], leg=leg)
            return
        got = run_gpu(pkg, den, frames, params, cams, leg=leg, outputs=outs)
        if pipelined:
            assert den.is_pipelined()
    finally:
        den.free()
    for f in range(len(frames)):
        assert np.array_equal(got[f]["hlen"], model[f]["hlen"]) and same_bits(got[f]["mom"], model[f]["mom"]), f"frame {f}"
        assert same_bits(got[f]["variance"], model[f]["variance"]), f"state 3, frame {f}"
        e = float(relerr(outs[f].reshape(H, W, 3), ref[f]["out"]).max())
        print(f"{W}x{H} variant {variant} {leg}{' pipelined' if pipelined else ''} frame {f}: relerr {e:.3e}")
        assert e <= 1e-4, f"variant {variant} frame {f}: {e:.3e}"


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1, 2, 4])
@pytest.mark.parametrize("W,H", SIZES)
def test_the_estimate_reaches_the_levels(pkg, orc, W, H, variant):
    """Every kernel variant at both sizes.  A (size, variant) of REFUSALS answers SVGF_ERR_UNSUPPORTED before anything is
    enqueued and nothing else does: a refusal anywhere else fails the test."""
    _levels_cell(pkg, orc, W, H, variant)


@pytest.mark.gpu
@pytest.mark.parametrize("leg", ["aos", "planar"])
@pytest.mark.parametrize("W,H", SIZES)
def test_the_estimate_on_pipelined_frames(pkg, orc, W, H, leg):
    """The same frames promised on a pipelined context, where the frames alternate between two plane sets and two streams: the
    pass runs on the frame's own stream behind its temporal pass, and on the planar leg behind the ev_tdone record that lets the
    producer of the next frame's planes go on.  (With the levels off a promise is not taken up and the frame runs on the caller's
    stream, as in the promised leg of test_kernel_equals_the_model_with_everything_on.)"""
    _levels_cell(pkg, orc, W, H, 0, leg=leg, pipelined=True)
