"""The launch geometry of every a-trous kernel, pinned without a GPU.

csrc/svgf_atrous_geometry.hip turns (frame size, step, CU count) into a launch decision: can the kernel run the level, how is the
image cut into (strip, y-phase, segment) workgroups, how large are grid, block and LDS, and what does the automatic choice think the
launch costs.  The experiments build exports that arithmetic (svgf_exp_atrous_geometry, binding.atrous_geometry); it touches no
device, so it runs here.

golden/kernel_geometry_table.json.gz (JSON, gzipped) holds every returned field over the sweep below.  It was written by the code that computed the
geometry inside the kernel translation units, BEFORE that code moved into the geometry module, and is not regenerated with it: the
integers are compared exactly, the estimates to a relative 1e-12 (the one-segment costing of a lane level with fewer than three
lattice rows per phase was 1.857 * rounds * 10 * (nb + 6) / 10 and is 1.857 * rounds * (nb + 6): the last bits of the double may
differ), and the lane / strip choice that follows from the estimates exactly.

One kind of entry of the table is not an estimate: for the parked fused first level (experiments build only) on frames of fewer
than three lattice rows per phase (H <= 4) the old code returned 1.857 * -1, the "-1" of a segment search whose range 4 .. nb + 1 is
empty, where the plain lane level already costed its one segment.  With one search there is one rule, and such a launch is costed as
what it is: every strip is one workgroup of nb rows, the strips go to the 8 XCDs' max(n_cu / 8, 1) CUs each in
rounds = ceil(n_strips / max(n_cu // 8, 1)), so the estimate is 1.857 * rounds * (nb + 6).  The test expects that value, computed
here from the table's own n_strips, wherever the table holds the negative one.

`python tests/test_kernel_geometry.py --write` rewrites the table from the library in the tree: only for a change that MEANS to
change a launch, and then the diff of the table is the review."""
import gzip
import itertools
import json
import math
import os
import sys

import pytest

pytestmark = pytest.mark.experiments

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kernel_geometry_table.json.gz")      # gzip: 517 KB of JSON
KERNELS = ("lane", "strip", "lattice", "fused", "lane2y")
WIDTHS = (1, 5, 64, 300, 470, 640, 800, 1024, 1280, 1920, 2048, 2560, 3440, 3840, 4096)
HEIGHTS = (1, 3, 16, 40, 48, 72, 200, 300, 600, 1080, 2160)
STEPS = (1, 2, 4, 8, 16, 32, 64, 128)
N_CU = (8, 64, 104, 256, 304)
# beside the sweep (blur_variance = 1, the 4-byte variance plane present): what the lane kernel's chunked steps need of the variance
# plane, the 32-bit offset limit of all kernels, a step that is no power of two, a one-CU device; (kernel, W, H, step, blur_variance,
# has_variance_plane, n_cu)
EXTRA = [(k, w, h, s, bv, vp, 256) for k in ("lane", "strip") for (w, h) in ((1920, 1080), (64, 16)) for s in (8, 16, 32)
         for bv in (0, 1) for vp in (0, 1)] + \
        [(k, w, h, s, 1, 1, 256) for k in KERNELS for (w, h) in ((16384, 16383), (16384, 16384), (4095, 4096)) for s in (2, 16, 64)] + \
        [(k, 1920, 1080, s, 1, 1, n) for k in KERNELS for s in (3, 2, 64) for n in (1, 7)]
REL = 1e-12


def sweep():
    return list(itertools.product(WIDTHS, HEIGHTS, STEPS, N_CU))


def record(binding, kernel, W, H, step, bv=1, vp=1, n_cu=256):
    """[eight integers, estimate] or 0 where the kernel does not run such a level."""
    out, est = binding.atrous_geometry(kernel, W, H, step, bv, vp, n_cu)
    if not out[0]:
        assert not any(out) and est is None
        return 0
    return out + [est]


def compute(binding):
    return {"_comment": "written by tests/test_kernel_geometry.py --write; see its docstring before regenerating",
            "fields": ["supported", "n_strips", "seg_rows", "n_segs", "n_groups", "grid_blocks", "block_threads", "lds_bytes", "estimate_us"],
            "fields_lattice": ["supported", "log2k", "pstride", "band_rows", "n_bands", "grid_blocks", "block_threads", "lds_bytes", "estimate_us"],
            "order": "for W, for H, for step, for n_cu", "W": list(WIDTHS), "H": list(HEIGHTS), "step": list(STEPS), "n_cu": list(N_CU),
            "sweep": {k: [record(binding, k, W, H, s, n_cu=n) for W, H, s, n in sweep()] for k in KERNELS},
            "extra": [[list(e), record(binding, *e)] for e in EXTRA]}


def one_segment_fused_estimate(want, H, n_cu):
    """The table's record with the estimate of a one-segment launch in place of the old code's -1.857 (see the module docstring)."""
    if want == 0 or want[8] is None or want[8] >= 0:
        return want
    nb = (H + 1) // 2
    assert want[8] == -1.857 and nb < 3 and want[2:5] == [nb, 1, 1], want
    rounds = -(-want[1] // max(n_cu // 8, 1))
    return want[:8] + [1.857 * (rounds * (nb + 6))]


def same(got, want):
    """integers exactly, the estimate to REL; returns (equal, bit_equal)"""
    if got == 0 or want == 0:
        return got == want, got == want
    if got[:8] != want[:8] or (got[8] is None) != (want[8] is None):
        return False, False
    if got[8] is None:
        return True, True
    return math.isclose(got[8], want[8], rel_tol=REL, abs_tol=0.0), got[8] == want[8]


@pytest.fixture(scope="module")
def table():
    t = json.load(gzip.open(TABLE, "rt"))
    assert (t["W"], t["H"], t["step"], t["n_cu"]) == (list(WIDTHS), list(HEIGHTS), list(STEPS), list(N_CU)), "the table is of another sweep"
    assert [e for e, _ in t["extra"]] == [list(e) for e in EXTRA]
    return t


def test_every_field_of_every_launch_matches_the_table(pkg, table):
    b = pkg.binding
    cases = sweep()
    wrong, inexact = [], []
    for k in KERNELS:
        assert len(table["sweep"][k]) == len(cases)
        for (W, H, s, n), want in zip(cases, table["sweep"][k]):
            got = record(b, k, W, H, s, n_cu=n)
            if k == "fused":
                want = one_segment_fused_estimate(want, H, n)
            ok, bits = same(got, want)
            if not ok:
                wrong.append((k, W, H, s, n, got, want))
            elif not bits:
                inexact.append((k, W, H, s, n, got[8], want[8]))
    for e, want in table["extra"]:
        got = record(b, *e)
        if e[0] == "fused":
            want = one_segment_fused_estimate(want, e[2], e[6])
        if not same(got, want)[0]:
            wrong.append((*e, got, want))
    print(f"{len(cases) * len(KERNELS) + len(EXTRA)} launches; estimates equal to {REL} but not bit for bit: {len(inexact)}")
    for x in inexact:
        print("  ", x)
    assert not wrong, f"{len(wrong)} launches differ from the table, the first: {wrong[:5]}"
    # a lane level with fewer than three lattice rows per phase is the only place the estimate's arithmetic changed
    assert all(k == "lane" and (H + s - 1) // s < 3 for k, W, H, s, n, _, _ in inexact), inexact


def test_the_choice_between_lane_and_strip_matches_the_table(pkg, table):
    """lane_pays: the lane kernel runs where its estimate is not above the strip kernel's."""
    b = pkg.binding
    n = 0
    for (W, H, s, cu), lane, strip in zip(sweep(), table["sweep"]["lane"], table["sweep"]["strip"]):
        if lane == 0 or strip == 0:
            continue
        got_l, got_s = b.atrous_geometry("lane", W, H, s, 1, 1, cu)[1], b.atrous_geometry("strip", W, H, s, 1, 1, cu)[1]
        assert (got_l <= got_s) == (lane[8] <= strip[8]), f"{W}x{H} step {s} on {cu} CUs: lane {got_l} strip {got_s} us, table {lane[8]} / {strip[8]}"
        n += 1
    assert n == len(WIDTHS) * len(HEIGHTS) * 6 * len(N_CU)      # steps 1 .. 32: both kernels run them at every size of the sweep


def test_table_holds_the_geometry_the_recorded_workloads_ran(table):
    """1920x1080 and 3840x2160 on 256 CUs: the launches DESIGN.md describes and profiles/pmc_traffic.json was measured on."""
    at = {c: i for i, c in enumerate(sweep())}
    for s in (2, 4, 8, 16, 32):
        lane, strip = table["sweep"]["lane"][at[(1920, 1080, s, 256)]], table["sweep"]["strip"][at[(1920, 1080, s, 256)]]
        assert lane[1:3] == [4, 17] and strip[2] == 34, (s, lane, strip)
        assert lane[8] == pytest.approx(1.857 * (17 + 6)) and strip[8] == pytest.approx(1.162 * (34 + 8))
        lane4k = table["sweep"]["lane"][at[(3840, 2160, s, 256)]]
        assert lane4k[1:3] == [8, 68], (s, lane4k)
    assert table["sweep"]["strip"][at[(3840, 2160, 2, 256)]][2] == 136


def test_choice_table_of_the_gpu_test_follows_from_the_estimates(pkg):
    """CHOICE_256 of test_kernel_geometry_gpu.py (what a 256-CU device runs, level by level), from the two estimates alone."""
    from test_kernel_geometry_gpu import CHOICE_256
    b = pkg.binding
    for (W, H), want in CHOICE_256.items():
        got = ""
        for s in (2, 4, 8, 16, 32):
            (lane, lane_us), (strip, strip_us) = b.atrous_geometry("lane", W, H, s, 1, 1, 256), b.atrous_geometry("strip", W, H, s, 1, 1, 256)
            assert lane[0] and strip[0], f"{W}x{H} step {s}"
            got += "L" if lane_us <= strip_us else "s"
        assert got == want, f"{W}x{H}: {got}, CHOICE_256 says {want}"


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit(__doc__)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as ge
    ge.load_package().build.build_hip(experiments=True)
    with open(TABLE, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", compresslevel=9, mtime=0) as f:
        f.write((json.dumps(compute(ge.load_package().binding), separators=(",", ":")) + "\n").encode())
    print(TABLE, os.path.getsize(TABLE), "bytes")
