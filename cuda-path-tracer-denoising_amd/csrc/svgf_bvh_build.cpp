// svgf_bvh_build.cpp — the resident scene's BVH builder (row f14): plain C++, host only, no HIP call in this translation unit.
//
// svgf_bvh_build_host orders the triangles and writes SvgfBvhNode records: count > 0 a leaf over order[first .. first + count),
// count == 0 an inner node with children first and first + 1.  A node's box is the exact union (min / max, no arithmetic) of the
// PADDED boxes of the triangles below it; svgf_bvh_tri_box is the one place that computes a padded box (float32, one rounding per
// operation, contraction off), and the device reads what was stored here, never recomputes it.  That, with the slab test of
// svgf_scene_bvh.hip, is what makes the drawn frame independent of the tree (include/svgf.h, row f14).
//
// Split: binned SAH over the centroids (split 0) or equal counts along the widest centroid axis (split 1).  Depth bound: a node with
// n triangles and r levels left below it is only ever created with n <= max_leaf_tris * 2^r.  A split whose sides would break that
// for r - 1, or that is degenerate (all centroids equal, an empty side), is replaced by equal counts by POSITION in the list, which
// keeps the invariant; the root has 2^20 <= 1 * 2^48.  So depth <= SVGF_SCENE_MAX_DEPTH and every leaf holds <= max_leaf_tris
// triangles, for every input.  Everything is a function of the input alone (ties are broken by triangle index): two builds agree.
#include "../../include/svgf.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#pragma clang fp contract(off)

void svgf_bvh_tri_box(const float *T, float lo[3], float hi[3]);       // below; svgf_scene_bvh.hip uploads what it returns

namespace {

constexpr int kBins = 16;

struct Box { float lo[3], hi[3]; };

inline void box_empty(Box &b)
{
    for (int c = 0; c < 3; c++) { b.lo[c] = INFINITY; b.hi[c] = -INFINITY; }
}

inline void box_grow(Box &b, const Box &o)
{
    for (int c = 0; c < 3; c++) { b.lo[c] = o.lo[c] < b.lo[c] ? o.lo[c] : b.lo[c]; b.hi[c] = o.hi[c] > b.hi[c] ? o.hi[c] : b.hi[c]; }
}

inline double box_area(const Box &b)
{
    const double x = (double)b.hi[0] - b.lo[0], y = (double)b.hi[1] - b.lo[1], z = (double)b.hi[2] - b.lo[2];
    return x * y + y * z + z * x;
}

struct Builder {
    const Box *tb;              // padded box per triangle
    const float *cen;           // 3 per triangle: the centre of the vertices' box (finite for every finite triangle)
    int max_leaf, split;
    SvgfBvhNode *nodes;
    int n_nodes, depth;
    int *order;
    std::vector<int> tmp;

    // largest count a subtree with r levels below its root may hold
    long long room(int r) const { return r >= 40 ? (1LL << 62) : (long long)max_leaf << r; }

    // by (centroid on `axis`, triangle index descending): a total order.  Descending on purpose: triangles with equal centroids -
    // copies of one triangle above all - then meet the leaf loop against their index order, so the draw's "lowest index wins a tie"
    // is decided by its comparison and not by the order the builder happened to keep
    void sort_range(int b, int e, int axis)
    {
        const float *c = cen;
        std::sort(order + b, order + e, [c, axis](int i, int j) { const float x = c[3 * i + axis], y = c[3 * j + axis]; return x < y || (x == y && i > j); });
    }

    // number of triangles that go left, or 0 where the rule has no usable split; reorders order[b, e)
    int split_range(int b, int e)
    {
        const int n = e - b;
        float clo[3] = { INFINITY, INFINITY, INFINITY }, chi[3] = { -INFINITY, -INFINITY, -INFINITY };
        for (int k = b; k < e; k++)
            for (int c = 0; c < 3; c++) { const float v = cen[3 * order[k] + c]; clo[c] = v < clo[c] ? v : clo[c]; chi[c] = v > chi[c] ? v : chi[c]; }
        if (split == 1) {
            int axis = 0;
            for (int c = 1; c < 3; c++) if (chi[c] - clo[c] > chi[axis] - clo[axis]) axis = c;
            if (!(chi[axis] - clo[axis] > 0.0f)) return 0;
            sort_range(b, e, axis);
            return (n + 1) / 2;
        }
        double best_cost = INFINITY;
        int best_axis = -1, best_bin = 0, best_left = 0;
        for (int axis = 0; axis < 3; axis++) {
            const float ext = chi[axis] - clo[axis];
            if (!(ext > 0.0f) || !std::isfinite(ext)) continue;
            Box bb[kBins];
            int cnt[kBins] = { 0 };
            for (int k = 0; k < kBins; k++) box_empty(bb[k]);
            for (int k = b; k < e; k++) { const int j = bin_of(cen[3 * order[k] + axis], clo[axis], ext); cnt[j]++; box_grow(bb[j], tb[order[k]]); }
            double right_area[kBins];
            Box acc; box_empty(acc);
            for (int k = kBins - 1; k > 0; k--) { box_grow(acc, bb[k]); right_area[k] = box_area(acc); }
            box_empty(acc);
            int left = 0;
            for (int k = 0; k + 1 < kBins; k++) {       // the plane behind bin k
                box_grow(acc, bb[k]); left += cnt[k];
                if (left == 0 || left == n) continue;
                const double cost = box_area(acc) * left + right_area[k + 1] * (n - left);
                if (cost < best_cost) { best_cost = cost; best_axis = axis; best_bin = k; best_left = left; }
            }
        }
        if (best_axis < 0) return 0;
        const float lo = clo[best_axis], ext = chi[best_axis] - clo[best_axis];
        int nl = 0, nr = 0;                             // a stable partition: both sides keep their order
        for (int k = b; k < e; k++) {
            if (bin_of(cen[3 * order[k] + best_axis], lo, ext) <= best_bin) order[b + nl++] = order[k];
            else tmp[nr++] = order[k];
        }
        std::memcpy(order + b + nl, tmp.data(), sizeof(int) * (size_t)nr);
        return best_left;
    }

    static int bin_of(float v, float lo, float ext)
    {
        const int j = (int)(((v - lo) / ext) * (float)kBins);
        return j < 0 ? 0 : (j >= kBins ? kBins - 1 : j);
    }

    void build(int node, int b, int e, int level)
    {
        Box box; box_empty(box);
        for (int k = b; k < e; k++) box_grow(box, tb[order[k]]);
        SvgfBvhNode &nd = nodes[node];
        for (int c = 0; c < 3; c++) { nd.lo[c] = box.lo[c]; nd.hi[c] = box.hi[c]; }
        if (level > depth) depth = level;
        const int n = e - b;
        if (n <= max_leaf) { nd.first = b; nd.count = n; return; }
        const int below = SVGF_SCENE_MAX_DEPTH - level - 1;     // levels under each child
        int nl = split_range(b, e);
        if (nl <= 0 || nl >= n || nl > room(below) || n - nl > room(below)) nl = (n + 1) / 2;     // equal counts by position
        const int first = n_nodes;
        n_nodes += 2;
        nd.first = first; nd.count = 0;
        build(first, b, b + nl, level + 1);
        build(first + 1, b + nl, e, level + 1);
    }
};

}  // namespace

// The padded box of one triangle (T: 3 vertices x 8 floats, positions first).  include/svgf.h states the arithmetic.
void svgf_bvh_tri_box(const float *T, float lo[3], float hi[3])
{
#pragma clang fp contract(off)
    float mn[3], mx[3], ext = 0.0f;
    for (int c = 0; c < 3; c++) {
        mn[c] = std::fmin(std::fmin(T[c], T[8 + c]), T[16 + c]);
        mx[c] = std::fmax(std::fmax(T[c], T[8 + c]), T[16 + c]);
        const float e = mx[c] - mn[c];
        ext = e > ext ? e : ext;
    }
    for (int c = 0; c < 3; c++) {
        const float m = std::fmax(1.0f, std::fmax(std::fabs(mn[c]), std::fabs(mx[c])));
        const float pad = (ext * 0.00390625f) + (0.0000152587890625f * m);
        lo[c] = mn[c] - pad; hi[c] = mx[c] + pad;
    }
}

extern "C" int svgf_bvh_build_host(const float *tris, int n_tris, const SvgfSceneBuildParams *bp, SvgfBvhNode *nodes, int *n_nodes, int *order,
                                   int *depth)
{
    if (n_tris < 0 || n_tris > SVGF_SCENE_MAX_TRIS || (n_tris > 0 && (!tris || !order)) || !nodes || !n_nodes || !depth) return SVGF_ERR_INVALID_ARG;
    const int max_leaf = bp && bp->max_leaf_tris != 0 ? bp->max_leaf_tris : 4, split = bp ? bp->split : 0;
    if (max_leaf < 1 || max_leaf > 8 || split < 0 || split > 1) return SVGF_ERR_INVALID_ARG;
    for (size_t i = 0; i < (size_t)n_tris; i++)
        for (int v = 0; v < 3; v++)
            for (int c = 0; c < 3; c++)
                if (!std::isfinite(tris[24 * i + 8 * v + c])) return SVGF_ERR_INVALID_ARG;
    *n_nodes = 0; *depth = 0;
    if (n_tris == 0) return SVGF_OK;
    std::vector<Box> tb((size_t)n_tris);
    std::vector<float> cen(3 * (size_t)n_tris);
    for (size_t i = 0; i < (size_t)n_tris; i++) {
        svgf_bvh_tri_box(tris + 24 * i, tb[i].lo, tb[i].hi);
        const float *T = tris + 24 * i;
        for (int c = 0; c < 3; c++)
            cen[3 * i + c] = 0.5f * std::fmin(std::fmin(T[c], T[8 + c]), T[16 + c]) + 0.5f * std::fmax(std::fmax(T[c], T[8 + c]), T[16 + c]);
        order[i] = (int)i;
    }
    Builder bd;
    bd.tb = tb.data(); bd.cen = cen.data(); bd.max_leaf = max_leaf; bd.split = split;
    bd.nodes = nodes; bd.n_nodes = 1; bd.depth = 0; bd.order = order;
    bd.tmp.resize((size_t)n_tris);
    bd.build(0, 0, n_tris, 0);
    *n_nodes = bd.n_nodes; *depth = bd.depth;
    return SVGF_OK;
}
