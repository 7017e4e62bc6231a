/* svgf_sah.h — row f25: the host builder's binned-SAH tree over the resident scene's triangles AS DRAWN, built on the device
 * (libsvgf_sah.so).
 *
 * Row f24 (include/svgf_lbvh.h) rebuilds a tree on the device in a millisecond, and that tree walks 1.10x - 2.40x slower than the
 * scene's own.  This library builds the tree svgf_scene_create would build from the triangles as they stand now - the same splits,
 * the same order[], the same boxes - in a fixed number of launches on the caller's stream, and hands it to the scene through
 * svgf_scene_adopt_tree.  It links against libsvgf_hip.so alone and reaches the scene through svgf_scene_view and
 * svgf_scene_adopt_tree and nothing else.
 *
 * svgf_sah_create(scene, p, out): validates before any device work - a NULL scene or out, p->max_leaf_tris outside 0..8, a scene
 *   without triangles: SVGF_ERR_INVALID_ARG (*out cleared) - then makes ONE device allocation that holds everything a build ever
 *   touches, the records at its start.  Allocates and synchronises: not under capture.
 * svgf_sah_build(t, stream): info.launches kernel launches on `stream` and nothing else - no allocation, no copy, no memset, no host
 *   wait; legal under stream capture.  The triangles and their padded boxes are re-read through svgf_scene_view on every call
 *   (svgf_scene_enable_pose moves them), their CONTENTS when the kernels run.  The same input gives the same bytes, padding included.
 *   Every error (a NULL tree, a scene whose triangle count changed) is answered before any device work.
 * svgf_sah_attach(t, scene): svgf_scene_adopt_tree(scene, records, order, 2 n_tris - 1, n_tris, depth_bound); `scene` must be the
 *   scene the tree was created for (otherwise SVGF_ERR_INVALID_ARG).  Host only.  Attach once; every later build rewrites the arrays
 *   the draws read, in stream order.  Detach (svgf_scene_adopt_tree with NULL nodes) before svgf_sah_destroy.
 * svgf_sah_read(t, which, host_dst, host_bytes): blocking (tests, debugging).  0 records (32 B * n_records), 1 order (4 B * n_tris),
 *   2 the SvgfSahCounts of the last build (16 B).  host_bytes must be the array's size exactly; otherwise, or for another kind or a
 *   NULL argument, SVGF_ERR_INVALID_ARG.
 * svgf_sah_destroy waits for the device first; NULL is accepted.
 *
 * Normative result - a function of the n_tris triangles as drawn (view.tris, view.tri_boxes) and L = max_leaf_tris alone; float32
 * where svgf_bvh_build_host is float32 and double where it is double, one rounding per operation, no contraction.
 * THE TREE is the tree of svgf_bvh_build_host(tris as drawn, { L, split = 0 }): the same order[] on every bit, the same nodes
 * (position range [b, e) and box), the same parent / child relation, left child first - in another layout (below).  Its rules
 * (csrc/svgf_bvh_build.cpp), for a node over order[b, e), n = e - b, at depth `level` (root 0):
 *   box            the union (min / max, no arithmetic) of the PADDED boxes (tri_boxes) of its triangles
 *   leaf           n <= L: first = b, count = n
 *   centroid       of a triangle, per axis: 0.5f * min3 + 0.5f * max3 of its three vertices
 *   centroid bounds  clo / chi = min / max of the node's centroids; ext = chi - clo; an axis is skipped when ext is not > 0 or
 *                  not finite
 *   bins           16 per axis; bin_of(v) = q = ((v - clo) / ext) * 16.0f;  !(q >= 0) ? 0 : (q >= 16 ? 15 : (int)q) - the comparisons
 *                  come before the cast, so the function is total (the host builder's clamp, for every value a finite triangle gives)
 *   bin boxes      per bin the count and the union of the PADDED boxes of its triangles
 *   cost           of the plane behind bin k = 0..14 with `left` triangles in bins 0..k (skipped when left is 0 or n):
 *                  area(left bins) * left + area(right bins) * (n - left) in double, area = x y + y z + z x from double differences
 *                  of the float32 box
 *   choice         the first strict minimum below +inf in the order axis 0..2, plane 0..14
 *   partition      stable, by bin_of(v on the chosen axis) <= the chosen bin: both sides keep their order; nl = left
 *   replacement    when no plane was usable (nl = 0), or nl or n - nl exceeds L << (47 - level): nl = (n + 1) / 2 BY POSITION, after the
 *                  partition has happened.  SvgfSahCounts.forced_splits counts the inner nodes where this rule acted.
 *   children       [b, b + nl) and [b + nl, e), at level + 1
 * LAYOUT - it needs no allocation and no scan.  Record 0 is the root.  An inner node over [b, e) whose left part holds nl triangles
 *   has first = 2 (b + nl) - 1, count = 0: its children are records 2 (b + nl) - 1 and 2 (b + nl).  Every inner node splits at a
 *   distinct position b + nl in 1 .. n_tris - 1, so no two collide.  A leaf has first = b, count = e - b.  There are n_records =
 *   2 n_tris - 1 records; those that no node owns are 32 zero bytes, written by a kernel on every build.  With L = 1 there is no
 *   padding.
 * ATTACH hands the scene the CAPACITY: n_nodes = 2 n_tris - 1, n_leaves = n_tris - what svgf_scene_adopt_tree's check
 *   (n_nodes == 2 n_leaves - 1) needs without a host wait.  The true n_nodes, n_leaves, the measured depth and forced_splits are the
 *   SvgfSahCounts record in device memory (svgf_sah_read kind 2).  The draws never read n_nodes (csrc/svgf_scene_bvh.hip) and the
 *   padding is unreachable from record 0.  svgf_scene_pose on an adopted tree skips its refit, as for row f24: the loop is pose,
 *   build, draw.
 * THE DEPTH BOUND, depth_bound = min(48, n_tris - 1).  A node with r levels left below it is only created with n <= L * 2^r: the root
 *   has n_tris <= 2^20 <= 1 * 2^48; an inner node at `level` has r = 48 - level, and the replacement rule makes both children hold at
 *   most L << (47 - level) = L * 2^(r - 1) (equal counts by position halve n <= L * 2^r).  A node with r = 0 holds n <= L triangles and
 *   is a leaf.  So depth <= 48 = SVGF_SCENE_MAX_DEPTH for EVERY input - the argument counts triangles and uses nothing about their
 *   values - and a binary tree over n_tris triangles is no deeper than n_tris - 1.
 * NON-FINITE VERTICES arrive only through a pose table (svgf_scene_create refuses them).  bin_of is total, the histogram pass and the
 *   partition pass use that one function and the left count comes from the same predicate, so the result is a permutation in this
 *   layout with leaves of 1..L, depth <= 48 and boxes that are the fminf / fmaxf unions (a NaN is ignored) of the padded boxes.
 *   Nothing else is promised there, and the host builder is not the oracle.
 * Device side (csrc/svgf_sah.hip): kernel boundaries are the only synchronisation between workgroups; no thread adds
 *   a float to another thread's - everything shared is an integer count or a min / max through the monotone integer view of the
 *   float's bits.  SVGF_SAH_SMALL = 256.  rounds = 0 for n_tris <= 256, else ceil(log2(n_tris / 256)) + 4.  A round splits every node
 *   of more than 256 triangles once: centroid bounds and box, 3 x 16 histogram (in LDS per workgroup, flushed once), one decision per
 *   node, count, stable scatter - five launches.  One more launch finishes every subtree of <= 256 triangles whole in LDS, one wave
 *   each, and - through global memory - whatever a round left larger.  launches = 2 + 5 * rounds.
 * INTEGRATION.md 5s has the frame loop and when to prefer the refit, row f24 or this. */
#ifndef SVGF_SAH_H_
#define SVGF_SAH_H_

#include "svgf.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct svgf_sah svgf_sah;
typedef struct SvgfSahParams { int max_leaf_tris; /* 1..8, 0 = 4: svgf_bvh_build_host's */ } SvgfSahParams;
typedef struct SvgfSahInfo {
    int n_tris, max_leaf_tris, n_records /* 2 n_tris - 1 */, depth_bound, launches;
    unsigned long long device_bytes;
} SvgfSahInfo;
typedef struct SvgfSahCounts { int n_nodes, n_leaves, depth, forced_splits; } SvgfSahCounts;   /* written by the build, in device memory */
#define SVGF_SAH_SMALL 256           /* triangles of a subtree that one wave finishes in LDS */

int  svgf_sah_create(const svgf_scene *scene, const SvgfSahParams *p /* NULL = defaults */, svgf_sah **out);
int  svgf_sah_build(svgf_sah *t, void *stream);
int  svgf_sah_attach(svgf_sah *t, svgf_scene *scene);
int  svgf_sah_info(const svgf_sah *t, SvgfSahInfo *out);
int  svgf_sah_read(const svgf_sah *t, int which, void *host_dst, unsigned long long host_bytes);   /* blocking: 0 records, 1 order, 2 SvgfSahCounts */
void svgf_sah_destroy(svgf_sah *t);
/* (SVGF_VERSION_MAJOR << 16) | SVGF_VERSION_MINOR of the svgf.h this library was compiled against, as svgf_trace_version. */
int  svgf_sah_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SVGF_SAH_H_ */
