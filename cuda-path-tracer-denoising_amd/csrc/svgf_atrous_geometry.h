// svgf_atrous_geometry.h — how an a-trous level is launched: which kernels can run it, how the image is cut into workgroups,
// and what the launch is estimated to cost.  Host arithmetic on (AtrousArgs, CU count) only — no kernel, no device call — so the
// planner (svgf_frame.hip), the launchers in the kernel files and, in the experiments build, svgf_exp_atrous_geometry
// (tests/test_kernel_geometry.py, which needs no GPU) all ask the same functions.  Internal, like svgf_kernels.h.
#pragma once
#include "svgf_kernels.h"

constexpr int kStagedPixelBytes = 48;      // the LDS record of a staged pixel, three 16-byte slots (all a-trous kernels)

// ---- strip and lane kernels: (strip, y-phase, segment) workgroups --------------------------------------------------------------
// A strip is a range of columns, a segment a range of the lattice rows of one y-phase.  (phase, segment) groups are dealt
// round-robin to the 8 XCDs (blockIdx % 8), all strips of a group to the same XCD, so that they share its L2.
struct SegmentGeom {
    int n_strips;   // strips of columns
    int n_segs;     // lattice-row segments per phase
    int seg_rows;   // lattice rows per segment
    int n_groups;   // (y-phase groups of a strip) * n_segs
    float kn, kx;   // log2(e) / (sigma_n + 1e-6), log2(e) / (sigma_x + 1e-6)
    unsigned long long *dbg;   // tuning only (SegmentTimeline below): s_memtime stamps of workgroup dbg_block, else null
    int dbg_block;
};
inline int segment_grid_blocks(const SegmentGeom &gm) { return (gm.n_groups + 7) / 8 * 8 * gm.n_strips; }

// Segment length.  Every (strip, phase, segment) is one workgroup and `capacity` of them run at a time, so the grid runs in rounds
// of equal-length workgroups, and the busiest XCD sets the number of rounds.  Returns the minimum over L_lo <= L <= L_hi of
// rounds * (L rounded up to row_quantum + fixed_rows) — in lattice rows; fixed_rows: the halo rows + the exposed prologue latency —
// and the segment length L that reaches it (ties: fewer, longer workgroups).  A phase too short for the range (L_lo > L_hi) is one
// segment of nb_max rows, costed like any other.
struct SegmentRange { int L_lo, L_hi, row_quantum, fixed_rows; };
long segment_search(int n_strips, int groups_per_strip, int nb_max, SegmentRange range, int capacity, int *best_L);

// The strip kernel's workgroup shape: what k_atrous_strip, its launcher and strip_geometry() all read.
#ifndef SVGF_LOADER_GROUPS
#define SVGF_LOADER_GROUPS 2
#endif
#ifndef SVGF_LOADER_DIV
#define SVGF_LOADER_DIV 2
#endif
namespace strip_shape {
// ROWS <= 2: SVGF_LOADER_GROUPS groups of TX / SVGF_LOADER_DIV threads take turns (issue / in flight / commit).
// ROWS == 3: 12 compute waves leave room for 4 loader waves (1024 threads): one group of TX threads that commits and
//            re-issues every iteration.
__host__ __device__ constexpr int loader_groups(int rows) { return rows >= 3 ? 1 : SVGF_LOADER_GROUPS; }
__host__ __device__ constexpr int loader_group(int tx, int rows) { return rows >= 3 ? tx : tx / SVGF_LOADER_DIV; }
__host__ __device__ constexpr int loader_threads(int tx, int rows) { return loader_groups(rows) * loader_group(tx, rows); }
constexpr int block_threads(int tx, int rows) { return tx * rows + loader_threads(tx, rows); }
constexpr size_t lds_bytes(int S, int tx, int rows) { return (size_t)(4 + 2 * rows) * (tx + 4 * S) * kStagedPixelBytes + (size_t)2 * rows * 2 * (tx + 2) * 4 + 16; }   // ring + blur rows
}  // namespace strip_shape
// columns x rows of a workgroup per dilation; svgf_exp_set("strip_tx" / "strip_rows") override it in the experiments build
void strip_pick(int log2s, int &tx, int &rows);
// fills *gm for workgroups of tx columns x rows rows; returns the launch's cost in lattice rows (what atrous_strip_estimate_us prices)
long strip_geometry(const AtrousArgs &a, int tx, int rows, int n_cu, SegmentGeom *gm);

// The lane kernel's strips: 480 contiguous pixel columns (8 waves x 60 output lanes; 240 with both y-phases in one workgroup), or,
// at steps 16 / 32, 60 lattice columns of 8 adjacent x-phases.  svgf_atrous_lane_impl.h holds these against its own layout.
constexpr int kLaneStripColumns = 480, kLaneChunkPhases = 8, kLaneChunkColumns = 60;
int lane_strip_count(int W, int S, int YP = 1);
// YP: y-phases per workgroup (2: the two-y-phase geometry of the parked variants, step 2 only); returns the cost in lattice rows
long lane_geometry(const AtrousArgs &a, int YP, int n_cu, SegmentGeom *gm);

// ---- lattice kernel (steps >= 64): K adjacent x-phases of one y-phase, in bands of lattice rows ----------------------------------
#ifndef SVGF_LATTICE_NT
#define SVGF_LATTICE_NT 1024
#define SVGF_LATTICE_LDS_KB 150
#endif
constexpr int kLatticeThreads = SVGF_LATTICE_NT;       // 1024 threads / 150 KB: one workgroup per CU, 16 waves
constexpr int kLatticeLdsBudget = SVGF_LATTICE_LDS_KB * 1024;
struct LatticeTiles {
    int log2s, log2k;
    int tw;          // staged lattice columns per phase row: ceil(W / S) + 4
    int pstride;     // records per phase row in LDS (>= tw, padded: see lattice_geometry())
    int band_rows;   // output lattice rows per workgroup
    int n_bands;     // bands per sub-image
    float kn, kx;    // log2(e) / (sigma_n + 1e-6), log2(e) / (sigma_x + 1e-6)
};
bool lattice_geometry(const AtrousArgs &a, LatticeTiles &gm);      // false: the lattice kernel does not run this level
inline size_t lattice_lds_bytes(const LatticeTiles &gm) { return (size_t)(gm.pstride << gm.log2k) * (gm.band_rows + 4) * kStagedPixelBytes; }
inline unsigned lattice_grid_blocks(const LatticeTiles &gm) { return ((1u << (2 * gm.log2s)) >> gm.log2k) * (unsigned)gm.n_bands; }

// ---- what the planner asks --------------------------------------------------------------------------------------------------------
int        atrous_step_log2(int step);                                  // steps are powers of two
bool       atrous_strip_supported(const AtrousArgs &a);
bool       atrous_lane_supported(const AtrousArgs &a);
bool       atrous_lattice_supported(const AtrousArgs &a);
double     atrous_strip_estimate_us(const AtrousArgs &a, int n_cu);    // launch-geometry cost model (automatic kernel choice)
double     atrous_lane_estimate_us(const AtrousArgs &a, int n_cu);
#ifdef SVGF_BUILD_EXPERIMENTS
double     atrous_fused_estimate_us(const AtrousArgs &a, int n_cu);    // the fused temporal + first-level kernel (two y-phases, step 2)

// In-kernel timeline of one workgroup of a strip / lane kernel built with -DSVGF_STRIP_TIMELINE / -DSVGF_LANE_TIMELINE: the kernel's
// stamp() writes s_memtime into dbg[(wave * 16 + iteration) * 8 + slot].  One object per launcher instantiation (a function-local
// static); `kernel` is "strip" or "lane": svgf_exp_set("<kernel>_dbg", <block>) names the workgroup, "<kernel>_dbg_skip" the number
// of (cold) launches not to print.
struct SegmentTimeline {
    struct Span { const char *label; int from, to; };      // stamp[to] - stamp[from], indices iteration * 8 + slot within one wave; label null: end
    unsigned long long *buf = nullptr;
    int skip = -1, prints = 0;
    bool arm(const char *kernel, hipStream_t s, SegmentGeom *gm);      // before the launch: clears the stamps; false: no timeline asked for
    // after the launch: waits for the stream and prints the prologue spans and, per iteration, the compute / loader spans of four waves
    void print(const char *kernel, hipStream_t s, const char *title, int max_prints, int max_iterations, const int waves[4], int first_loader,
               const Span *prologue, const Span *compute, const Span *loader);
};
#endif
