// svgf_atrous_geometry.hip — the launch geometry of the a-trous kernels and the cost model of the automatic kernel choice
// (svgf_atrous_geometry.h).  Host code only.
//
// Auto selection between the two fast a-trous kernels for steps 2-32.  The lane-marching kernel works on 480-column strips (at
// steps 16 / 32: 120 / 60 lattice columns of 4 / 8 x-phases), the strip kernel on 256-column strips; both cut the image into
// (strip, y-phase, segment) workgroups that run in rounds of one per CU, and both know what their launch will cost:
// rounds x (segment rows + fixed rows) x the time of a row (1.86 us lane, 1.16 us strip: 42.7 against 48.8 us at 1920x1080).
// The cheaper one runs (lane_pays, svgf_frame.hip).  Measured against that model at nine sizes (profiles/r03_exp_widths*.log): within
// 5 %, same choice as the stopwatch everywhere — lane at 1920, 3840, 1600, 3440, 800 (steps 2-8), 2560 and 1280 (steps 2-8, 32);
// strip at 1024, 2048, and at steps 16 of 800 / 1280 / 2560.  That holds for frames taller than about six lattice rows per level
// (H / step >= 6); shorter phases are one segment each on both kernels, and the one-round launches then favour the strip kernel's
// shorter rows at the coarse steps (tests/test_kernel_geometry_gpu.py holds the per-level table for a 256-CU device,
// tests/test_kernel_geometry.py every launch of a sweep of sizes, steps and CU counts).
#include "svgf_atrous_geometry.h"

#include <cstdio>

// time of one lattice row of a workgroup, us: 1920x1080 is one round of 34 + 8 rows = 48.8 us on the strip kernel, of 17 + 6 rows
// = 42.7 us on the lane kernel (profiles/r03_exp_widths*.log: within 5 % at eight other sizes)
static const double kStripRowUs = 1.162, kLaneRowUs = 1.857;
static const int kLaneFixedRows = 6;

static float sigma_slope(float sigma) { return (float)(1.4426950408889634 / ((double)sigma + 1e-6)); }

int atrous_step_log2(int step)
{
    int l = 0;
    while ((1 << l) < step) l++;
    return l;
}

long segment_search(int n_strips, int groups_per_strip, int nb_max, SegmentRange r, int capacity, int *best_L)
{
    if (r.L_lo > r.L_hi) r.L_lo = r.L_hi = nb_max;
    const long cap_xcd = capacity / 8 > 0 ? capacity / 8 : 1;        // (a device with fewer than 8 CUs: one workgroup per "XCD" at a time)
    long best_cost = -1;
    for (int L = r.L_lo; L <= r.L_hi; L++) {                 // L need not be a multiple of row_quantum: the last iteration idles rows
        const int segs_l = (nb_max + L - 1) / L;
        const long blocks_xcd = (long)n_strips * ((groups_per_strip * segs_l + 7) / 8);     // the busiest XCD: ceil(groups / 8) groups
        const long rounds = (blocks_xcd + cap_xcd - 1) / cap_xcd;
        const long cost = rounds * ((L + r.row_quantum - 1) / r.row_quantum * r.row_quantum + r.fixed_rows);
        if (best_cost < 0 || cost <= best_cost) { best_cost = cost; *best_L = L; }
    }
    return best_cost;
}

// (seg_rows searched, or forced by the tuning knob — the cost stays that of the searched length)
static long segment_geometry(const AtrousArgs &a, int n_strips, int groups_per_strip, SegmentRange r, int capacity, int forced_rows, SegmentGeom *gm)
{
    const int nb_max = (a.H + a.step - 1) / a.step;
    gm->n_strips = n_strips;
    const long cost = segment_search(n_strips, groups_per_strip, nb_max, r, capacity, &gm->seg_rows);
    if (forced_rows > 0) gm->seg_rows = forced_rows;
    gm->n_segs = (nb_max + gm->seg_rows - 1) / gm->seg_rows;
    gm->n_groups = groups_per_strip * gm->n_segs;
    gm->kn = sigma_slope(a.sigma_n);
    gm->kx = sigma_slope(a.sigma_x);
    gm->dbg = nullptr; gm->dbg_block = 0;
    return cost;
}

// ---- strip kernel -------------------------------------------------------------------------------------------------------------------

void strip_pick(int log2s, int &tx, int &rows)
{
    // 256 columns x 2 rows per workgroup everywhere (profiles/r01_exp_tx_rows.log):
    //  * 128-column strips (two workgroups per CU) run a lone S <= 8 level 3-4 % faster at 1080p (equal at 3840), but
    //    the whole frame gets slower (6.46 vs 6.94 Gpix/s) once the next frame's temporal pass shares the GPU with
    //    levels 2-3; at S >= 16 the 4S halo columns make narrow strips lose outright;
    //  * ROWS = 3 (12 compute waves) is correct but not faster: two compute waves already saturate a SIMD's VALU.
    tx = 256; rows = 2;
    if (const int v = SVGF_TUNE("strip_tx", 0); v == 128 || v == 256) tx = v;
    if (const int v = SVGF_TUNE("strip_rows", 0); v >= 1 && v <= 3) rows = v;
    if (rows == 3 && tx != 256) rows = 2;
    // LDS budget: ring + blur rows <= 160 KiB
    while (strip_shape::lds_bytes(1 << log2s, tx, rows) > 160 * 1024 && rows > 1) rows--;
}

long strip_geometry(const AtrousArgs &a, int tx, int rows, int n_cu, SegmentGeom *gm)
{
    // LDS and the 2048 threads of a CU admit `bpc` workgroups per CU
    int bpc = (int)((160 * 1024) / strip_shape::lds_bytes(a.step, tx, rows));
    const int threads = strip_shape::block_threads(tx, rows);
    if (bpc > 2048 / threads) bpc = 2048 / threads;
    if (bpc < 1) bpc = 1;
    const int nb_max = (a.H + a.step - 1) / a.step;
    static const int fixed_rows = SVGF_TUNE("strip_fixed_rows", 8);   // tuning only; the 4 halo rows + the exposed prologue latency
    return segment_geometry(a, (a.W + tx - 1) / tx, a.step, { rows * 4, nb_max + rows, rows, fixed_rows }, n_cu * bpc, SVGF_TUNE("strip_segrows", 0), gm);
}

bool atrous_strip_supported(const AtrousArgs &a)
{
    if (a.step < 1 || a.step > 32 || (a.step & (a.step - 1))) return false;      // step 1: SvgfParams::paper_steps
    if ((long long)a.W * a.H * 16 >= (1LL << 32)) return false;   // 32-bit element offsets in the kernel
    return true;
}

double atrous_strip_estimate_us(const AtrousArgs &a, int n_cu)
{
    int tx, rows;
    strip_pick(atrous_step_log2(a.step), tx, rows);
    SegmentGeom gm;
    return kStripRowUs * (double)strip_geometry(a, tx, rows, n_cu, &gm);
}

// ---- lane kernel --------------------------------------------------------------------------------------------------------------------

// strips: contiguous pixel columns (one x-phase per wave group), or (lattice-column strip, group of 8 x-phases) pairs (steps 16, 32)
int lane_strip_count(int W, int S, int YP)
{
    if (S <= 8) return (W + kLaneStripColumns / YP - 1) / (kLaneStripColumns / YP);
    return (((W + S - 1) / S + kLaneChunkColumns - 1) / kLaneChunkColumns) * (S / kLaneChunkPhases);
}

// one workgroup per CU (LDS-bound); a strip is cut into step / YP y-phase groups
long lane_geometry(const AtrousArgs &a, int YP, int n_cu, SegmentGeom *gm)
{
    const int nb_max = (a.H + a.step - 1) / a.step;
    return segment_geometry(a, lane_strip_count(a.W, a.step, YP), a.step / YP, { 4, nb_max + 1, 1, kLaneFixedRows }, n_cu,
                            SVGF_TUNE("lane_segrows", 0), gm);      // (the knob: tools/experiments/exp_small_frames.sh)
}

bool atrous_lane_supported(const AtrousArgs &a)
{
    if (!atrous_strip_supported(a)) return false;      // the same steps (1: SvgfParams::paper_steps) and 32-bit offsets
    return a.step <= 8 || a.var != nullptr || !a.blur_variance;      // steps 16, 32 (chunked x-phases): the loaders blur the variance from the 4-byte plane
}

double atrous_lane_estimate_us(const AtrousArgs &a, int n_cu)
{
    SegmentGeom gm;
    return kLaneRowUs * (double)lane_geometry(a, 1, n_cu, &gm);
}

// ---- lattice kernel -----------------------------------------------------------------------------------------------------------------

// Tile geometry.  K: the largest of 8, 4, 2, 1 phases per workgroup whose tile holds whole sub-images or at least
// 8-row bands within the LDS budget.  pstride: the row of one phase is padded so that the 16 lanes a b128 LDS access
// serves per cycle (K phases x 16/K consecutive columns, 12 dwords apart) fall on 16 distinct 4-bank groups:
// 12 * pstride mod 64 must be 32 (K = 2), 48 (K = 4) or 24 (K = 8).
bool lattice_geometry(const AtrousArgs &a, LatticeTiles &gm)
{
    if (a.step < 64 || (a.step & (a.step - 1))) return false;
    if ((long long)a.W * a.H * 16 >= (1LL << 32)) return false;     // 32-bit element offsets in the kernel
    const int log2s = atrous_step_log2(a.step);
    if (log2s > 12) return false;
    const int S = a.step;
    gm.log2s = log2s;
    gm.tw = (a.W + S - 1) / S + 4;
    const int mh_max = (a.H + S - 1) / S;
    int chosen = -1, rows_fit = 0;
    for (int log2k = 3; log2k >= 0 && chosen < 0; log2k--) {
        const int K = 1 << log2k;
        const int want = (K == 1) ? -1 : (K == 2 ? 32 : (K == 4 ? 48 : 24));
        int P = gm.tw;
        while (want >= 0 && (12 * P) % 64 != want) P++;
        const int fit = kLatticeLdsBudget / (K * P * kStagedPixelBytes) - 4;
        if (fit >= (mh_max < 8 ? mh_max : 8) || (K == 1 && fit >= 1)) { chosen = log2k; rows_fit = fit; gm.pstride = P; }
    }
    if (chosen < 0) return false;                                   // a single lattice row does not fit: gather kernel
    gm.log2k = chosen;
    if (rows_fit > mh_max) rows_fit = mh_max;
    gm.n_bands = (mh_max + rows_fit - 1) / rows_fit;
    gm.band_rows = (mh_max + gm.n_bands - 1) / gm.n_bands;          // equal bands
    if (((long long)S * S >> chosen) * gm.n_bands > (1LL << 30)) return false;
    gm.kn = sigma_slope(a.sigma_n);
    gm.kx = sigma_slope(a.sigma_x);
    return true;
}

bool atrous_lattice_supported(const AtrousArgs &a)
{
    LatticeTiles gm;
    return lattice_geometry(a, gm);
}

#ifdef SVGF_BUILD_EXPERIMENTS
// ---- experiments build: the parked fused kernel's estimate, the in-kernel timeline ------------------------------------------------

double atrous_fused_estimate_us(const AtrousArgs &a, int n_cu)
{
    SegmentGeom gm;
    return kLaneRowUs * (double)lane_geometry(a, 2, n_cu, &gm);
}

static const int kTimelineStamps = 16 * 16 * 8;      // waves x iterations x slots

bool SegmentTimeline::arm(const char *kernel, hipStream_t s, SegmentGeom *gm)
{
    char knob[32];
    snprintf(knob, sizeof(knob), "%s_dbg", kernel);
    const int block = SVGF_TUNE(knob, -1);
    if (block < 0) return false;
    if (!buf) (void)hipMalloc((void **)&buf, kTimelineStamps * sizeof(unsigned long long));
    (void)hipMemsetAsync(buf, 0, kTimelineStamps * sizeof(unsigned long long), s);
    gm->dbg = buf; gm->dbg_block = block;
    return true;
}

void SegmentTimeline::print(const char *kernel, hipStream_t s, const char *title, int max_prints, int max_iterations, const int waves[4], int first_loader,
                            const Span *prologue, const Span *compute, const Span *loader)
{
    char knob[32];
    snprintf(knob, sizeof(knob), "%s_dbg_skip", kernel);
    if (skip < 0) skip = SVGF_TUNE(knob, 0);      // warm launches only
    (void)hipStreamSynchronize(s);
    unsigned long long h[kTimelineStamps];
    (void)hipMemcpy(h, buf, sizeof(h), hipMemcpyDeviceToHost);
    if (skip > 0) { skip--; return; }
    if (prints++ >= max_prints) return;
    fprintf(stderr, "[%s dbg] %s\n", kernel, title);
    for (int si = 0; si < 4; si++) {
        const int w = waves[si];
        const unsigned long long *t = &h[w * 16 * 8];
        if (t[7]) {
            fprintf(stderr, "  wave %2d prologue:", w);
            for (const Span *p = prologue; p->label; p++) fprintf(stderr, " %s %6llu", p->label, t[p->to] - t[p->from]);
            fprintf(stderr, "\n");
        }
        for (int it = 0; it < max_iterations && t[it * 8]; it++) {
            fprintf(stderr, "  %s %2d it %2d: t0=%6llu", w >= first_loader ? "loader" : "wave", w, it, t[it * 8] - h[0]);
            for (const Span *p = w >= first_loader ? loader : compute; p->label; p++) fprintf(stderr, " %s %5llu", p->label, t[it * 8 + p->to] - t[it * 8 + p->from]);
            fprintf(stderr, "\n");
        }
    }
}
#endif
