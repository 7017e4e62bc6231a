// svgf_bvh_build.cpp — the resident scene's BVH builder (row f14): plain C++, host only, no HIP call in this translation unit.
//
// svgf_bvh_build_host orders the triangles and writes SvgfBvhNode records: count > 0 a leaf over order[first .. first + count),
// count == 0 an inner node with children first and first + 1.  A node's box is the exact union (min / max, no arithmetic) of the
// PADDED boxes of the triangles below it; svgf_bvh_tri_box is the one place that computes a padded box (float32, one rounding per
// operation, contraction off); a pose (row f15) restates it on the device with the same literals and nesting.  That, with the slab test of
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

void svgf_bvh_tri_box(const float *T, float lo[3], float hi[3]);       // below; svgf_scene_bvh.hip uploads what it returns (and restates it in k_scene_pose)

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

// ---- row f15: the refit plan of an animated resident scene, and the pose helper -----------------------------------------------------------
// The plan partitions the nodes for a refit without any traffic between workgroups: TREELETS (whole subtrees of at most `cap` nodes
// whose parent's subtree is larger; one workgroup sweeps one in LDS) and the TOP (every node whose subtree is larger than `cap`: the
// ancestors of treelet roots; one workgroup, deepest first).  It is a function of the nodes alone.  The layout it relies on - and
// checks - is the builder's: children in pairs behind their parent, a node's descendants in ONE index range that starts at its first
// child, so that a treelet is its root plus a range.
extern "C" int svgf_bvh_refit_plan_host(const SvgfBvhNode *nodes, int n_nodes, int cap, SvgfRefitTreelet *treelets, unsigned char *level,
                                        int *top, int *top_seg, SvgfRefitPlanInfo *info)
{
    if (!info || !top_seg || n_nodes < 0 || n_nodes > 2 * SVGF_SCENE_MAX_TRIS || cap < 1) return SVGF_ERR_INVALID_ARG;
    if (n_nodes > 0 && (!nodes || !treelets || !level || !top)) return SVGF_ERR_INVALID_ARG;
    *info = SvgfRefitPlanInfo{ 0, 0, 0, cap };
    top_seg[0] = 0;
    if (n_nodes == 0) return SVGF_OK;
    const size_t n = (size_t)n_nodes;
    std::vector<int> parent(n, -1), size(n, 1), depth(n, 0);
    for (int k = 0; k < n_nodes; k++) {
        const SvgfBvhNode &nd = nodes[k];
        if (nd.count < 0 || nd.first < 0) return SVGF_ERR_INVALID_ARG;
        if (nd.count > 0) continue;
        if (nd.first <= k || (long long)nd.first + 1 >= n_nodes) return SVGF_ERR_INVALID_ARG;       // children lie behind their parent
        for (int c = nd.first; c <= nd.first + 1; c++) {
            if (parent[c] != -1) return SVGF_ERR_INVALID_ARG;                                       // a tree: one parent per node
            parent[c] = k;
        }
    }
    for (int k = 1; k < n_nodes; k++) {
        if (parent[k] < 0) return SVGF_ERR_INVALID_ARG;                                             // ... and every node reached
        depth[k] = depth[parent[k]] + 1;                                                            // parent[k] < k: already set
        if (depth[k] > SVGF_SCENE_MAX_DEPTH) return SVGF_ERR_UNSUPPORTED;
    }
    for (int k = n_nodes - 1; k >= 1; k--) size[parent[k]] += size[k];
    for (int k = 0; k < n_nodes; k++) {                 // the builder's layout: descendants of k are [first, first + size - 1)
        if (nodes[k].count > 0) continue;
        const int a = nodes[k].first;
        if (k == 0 && a != 1) return SVGF_ERR_UNSUPPORTED;
        if (nodes[a].count == 0 && nodes[a].first != a + 2) return SVGF_ERR_UNSUPPORTED;
        if (nodes[a + 1].count == 0 && nodes[a + 1].first != a + 1 + size[a]) return SVGF_ERR_UNSUPPORTED;
    }
    int n_treelets = 0, n_top = 0, count_at[SVGF_SCENE_MAX_DEPTH + 1] = { 0 };
    for (int k = 0; k < n_nodes; k++) {
        if (size[k] > cap) { level[k] = (unsigned char)depth[k]; count_at[depth[k]]++; n_top++; continue; }
        if (k != 0 && size[parent[k]] <= cap) continue;                                             // inside a treelet
        SvgfRefitTreelet &t = treelets[n_treelets++];
        t.root = k; t.begin = nodes[k].count > 0 ? 0 : nodes[k].first; t.count = size[k] - 1;
        t.levels = nodes[k].count > 0 ? 0 : 1;
        level[k] = 0;
        for (int g = t.begin; g < t.begin + t.count; g++) {
            const int l = depth[g] - depth[k];
            level[g] = (unsigned char)l;
            if (nodes[g].count == 0 && l + 1 > t.levels) t.levels = l + 1;
        }
    }
    // the top list: deepest first, one segment per depth that occurs, so that a node's children are treelet roots or stand in an
    // earlier segment
    int at[SVGF_SCENE_MAX_DEPTH + 1], n_seg = 0, pos = 0;
    for (int d = SVGF_SCENE_MAX_DEPTH; d >= 0; d--) {
        at[d] = pos;
        if (count_at[d] > 0) { pos += count_at[d]; top_seg[++n_seg] = pos; }
    }
    for (int k = 0; k < n_nodes; k++)
        if (size[k] > cap) top[at[depth[k]]++] = k;
    *info = SvgfRefitPlanInfo{ n_treelets, n_top, n_seg, cap };
    return SVGF_OK;
}

// Rotation by angle_rad about `axis` through `pivot`, then `translate`: computed in double, each of the 24 values rounded once.
extern "C" int svgf_pose_rigid(const float axis[3], float angle_rad, const float pivot[3], const float translate[3], SvgfScenePose *out)
{
    if (!axis || !pivot || !translate || !out || !std::isfinite(angle_rad)) return SVGF_ERR_INVALID_ARG;
    for (int c = 0; c < 3; c++)
        if (!std::isfinite(axis[c]) || !std::isfinite(pivot[c]) || !std::isfinite(translate[c])) return SVGF_ERR_INVALID_ARG;
    const double len = std::sqrt((double)axis[0] * axis[0] + (double)axis[1] * axis[1] + (double)axis[2] * axis[2]);
    if (!(len > 0.0)) return SVGF_ERR_INVALID_ARG;
    const double u[3] = { axis[0] / len, axis[1] / len, axis[2] / len };
    const double c = std::cos((double)angle_rad), s = std::sin((double)angle_rad), v = 1.0 - c;
    const double R[3][3] = { { c + v * u[0] * u[0], v * u[0] * u[1] - s * u[2], v * u[0] * u[2] + s * u[1] },
                             { v * u[1] * u[0] + s * u[2], c + v * u[1] * u[1], v * u[1] * u[2] - s * u[0] },
                             { v * u[2] * u[0] - s * u[1], v * u[2] * u[1] + s * u[0], c + v * u[2] * u[2] } };
    double t[3];
    for (int r = 0; r < 3; r++) t[r] = ((double)pivot[r] - (R[r][0] * pivot[0] + R[r][1] * pivot[1] + R[r][2] * pivot[2])) + translate[r];
    for (int r = 0; r < 3; r++) {
        // "+ 0.0": a zero is +0 (angle 0 gives the identity on every bit, whatever the axis)
        for (int k = 0; k < 3; k++) { out->xf[4 * r + k] = (float)(R[r][k] + 0.0); out->inv[4 * r + k] = (float)(R[k][r] + 0.0); }
        out->xf[4 * r + 3] = (float)(t[r] + 0.0);
        out->inv[4 * r + 3] = (float)(0.0 - (R[0][r] * t[0] + R[1][r] * t[1] + R[2][r] * t[2]));      // (R^T, -R^T t): the analytic inverse
    }
    return SVGF_OK;
}
