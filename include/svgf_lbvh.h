/* svgf_lbvh.h — row f24: a linear BVH over the resident scene's triangles AS DRAWN, built on the device (libsvgf_lbvh.so).
 *
 * svgf_scene_create builds the scene's tree on the host and svgf_scene_pose refits it; neither changes its topology.  This library
 * builds a fresh tree from the padded triangle boxes the draws read at that moment (svgf_scene_view's tri_boxes: the posed boxes on a
 * posed scene) in a fixed number of launches on the caller's stream, and hands it to the scene through svgf_scene_adopt_tree.  Row
 * f14's frame is a gated brute force that every valid tree reproduces, so the adopted tree changes no pixel of any draw; what it
 * changes is how many nodes a ray visits.  The library links against libsvgf_hip.so alone and reaches the scene through
 * svgf_scene_view and svgf_scene_adopt_tree and nothing else.
 *
 * svgf_lbvh_create(scene, p, out): validates before any device work - a NULL scene or out, p->leaf_tris outside 0..8, a scene
 *   without triangles: SVGF_ERR_INVALID_ARG - then makes ONE device allocation that holds everything a build ever touches (two key
 *   arrays, the histograms, the partial bounds, the node ranges, slots and stamps, the top list, 2 * n_leaves nodes, n_tris order
 *   entries).  Allocates and synchronises: not under capture.
 * svgf_lbvh_build(t, stream): info.launches kernel launches on `stream` (5 + 3 * ceil(key_bits / 8): a function of n_tris and leaf_tris
 *   alone) and nothing else - no allocation, no copy, no memset, no host wait; legal under stream capture.  The triangle boxes are
 *   re-read through svgf_scene_view on every call (svgf_scene_enable_pose moves them), their CONTENTS when the kernels run.  The same
 *   boxes give the same bytes.  Every error (a NULL tree, a scene whose triangle count changed) is answered before any device work.
 * svgf_lbvh_attach(t, scene): svgf_scene_adopt_tree(scene, this tree's nodes, order, n_nodes, n_leaves, depth_bound); `scene` must be
 *   the scene the tree was created for (otherwise SVGF_ERR_INVALID_ARG).  Host only.  Attach once; every later build rewrites the
 *   arrays the draws read, in stream order.  Detach (svgf_scene_adopt_tree with NULL nodes) before svgf_lbvh_destroy.
 * svgf_lbvh_read(t, which, host_dst, host_bytes): blocking (tests, debugging).  0 nodes (32 B * n_nodes), 1 order (4 B * n_tris),
 *   2 the sorted keys (8 B * n_tris).  host_bytes must be the array's size exactly; otherwise, or for another kind or a NULL
 *   argument, SVGF_ERR_INVALID_ARG.
 * svgf_lbvh_destroy waits for the device first; NULL is accepted.
 * svgf_lbvh_build_host: the same function of the same input on the host, no device needed.  tri_boxes: n_tris SvgfBvhNode records
 *   (lo, hi read; first / count ignored); nodes has room for 2 * n_leaves, order for n_tris, keys (or NULL) for n_tris.
 *   SVGF_ERR_INVALID_ARG for a NULL tri_boxes, nodes, order or info, n_tris outside 1..SVGF_SCENE_MAX_TRIS, leaf_tris outside 0..8.
 *
 * Normative result - a function of the n_tris padded boxes and L = leaf_tris alone; float32, one rounding per operation, no contraction:
 *   centroid       c = (lo + hi) * 0.5f per axis
 *   bounds         bmin = fminf, bmax = fmaxf over all centroids, from +inf / -inf (a NaN is ignored; the fold is order-free)
 *   bits           idx_bits = max(1, ceil(log2(n_tris)));  axis_bits = min(10, (48 - idx_bits) / 3);  key_bits = 3 * axis_bits + idx_bits
 *   cell, M = 2^axis_bits, per axis:  ext = bmax - bmin;  q = ext > 0 ? (c - bmin) / ext : 0;  v = q * (float)M;
 *                  cell = !(v >= 0) ? 0 : (v >= (float)(M - 1) ? M - 1 : (int)v)     - the comparisons come before the cast: NaN and
 *                  inf are defined inputs
 *   Morton code    bit 3j + 2 = x's bit j, bit 3j + 1 = y's, bit 3j = z's
 *   key(i)         (morton << idx_bits) | i: unique, so the sorted order is unique; order[] = the low idx_bits of the sorted keys
 *   leaves         leaf k holds order[k L .. min(n_tris, k L + L)); its key is its first triangle's; n_leaves = ceil(n_tris / L)
 *   hierarchy      the binary radix tree of Karras 2012 over the leaf keys: delta(i, j) = the length of the common prefix of the two
 *                  keys within key_bits, -1 for j outside the array
 *   layout         internal radix node 0 is node 0; the children of internal node j are nodes 1 + 2j (left) and 2 + 2j (right); an
 *                  inner record has first = 1 + 2 * (the child's internal index), count = 0; a leaf record first = k L, count = 1..L;
 *                  n_nodes = 2 * n_leaves - 1, one leaf gives the single node 0
 *   boxes          a leaf = the fminf / fmaxf union of its triangles' stored boxes, an inner node = the union of its two children
 * The depth bound.  An internal node of the radix tree covers the leaves that share a key prefix, and its children share a strictly
 *   longer one.  The keys are distinct, so two leaves share at most key_bits - 1 bits: along a root-to-leaf path the internal nodes'
 *   prefix lengths grow strictly inside 0 .. key_bits - 1, there are at most key_bits of them, and a leaf stands at depth <= key_bits
 *   <= 48.  A tree of n_leaves leaves is no deeper than n_leaves - 1 either.  depth_bound = min(key_bits, n_leaves - 1) therefore
 *   bounds the depth for EVERY input - the argument uses the keys' distinctness (the index bits) and nothing about the boxes, so NaN
 *   and inf boxes are covered - and it never exceeds SVGF_SCENE_MAX_DEPTH, which is what keeps the draws' 48-level stack in bounds.
 * Device side: kernel boundaries are the only synchronisation between workgroups (DESIGN.md 5.4g's rule): an LSD radix sort with
 *   8-bit digits (count, scan, scatter per pass, on the 64-bit keys alone), one thread per internal node for the hierarchy, the boxes
 *   of the nodes inside a tile of 512 leaves by that tile's workgroup in LDS and the nodes that span tiles by ONE workgroup.
 * INTEGRATION.md 5r has the frame loop, DESIGN.md 5.4q the kernels and what they cost. */
#ifndef SVGF_LBVH_H_
#define SVGF_LBVH_H_

#include "svgf.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct svgf_lbvh svgf_lbvh;
typedef struct SvgfLbvhParams { int leaf_tris; /* 1..8, 0 = default 4 */ } SvgfLbvhParams;
typedef struct SvgfLbvhInfo {
    int n_tris, n_leaves, n_nodes, leaf_tris, idx_bits, axis_bits, key_bits, depth_bound, launches;
    unsigned long long device_bytes;
} SvgfLbvhInfo;
#define SVGF_LBVH_TILE 512           /* leaves per workgroup of the box pass */

int  svgf_lbvh_create(const svgf_scene *scene, const SvgfLbvhParams *p /* NULL = defaults */, svgf_lbvh **out);
int  svgf_lbvh_build(svgf_lbvh *t, void *stream);
int  svgf_lbvh_attach(svgf_lbvh *t, svgf_scene *scene);
int  svgf_lbvh_info(const svgf_lbvh *t, SvgfLbvhInfo *out);
int  svgf_lbvh_read(const svgf_lbvh *t, int which, void *host_dst, unsigned long long host_bytes);
void svgf_lbvh_destroy(svgf_lbvh *t);
/* (SVGF_VERSION_MAJOR << 16) | SVGF_VERSION_MINOR of the svgf.h this library was compiled against, as svgf_trace_version. */
int  svgf_lbvh_version(void);
int  svgf_lbvh_build_host(const SvgfBvhNode *tri_boxes, int n_tris, const SvgfLbvhParams *p, SvgfBvhNode *nodes, int *order,
                          unsigned long long *keys /* or NULL */, SvgfLbvhInfo *info);

#ifdef __cplusplus
}
#endif
#endif /* SVGF_LBVH_H_ */
