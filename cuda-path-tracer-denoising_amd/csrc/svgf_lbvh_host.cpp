// svgf_lbvh_host.cpp — row f24: svgf_lbvh_build_host, include/svgf_lbvh.h's normative result computed on the host (no device, no HIP
// call): what the device builder of svgf_lbvh.hip is held to, and a builder for callers without a GPU at hand.  The arithmetic is
// svgf_lbvh_core.h's, the text the kernels compile; the order of work is the plain one - fold, keys, std::sort, one loop over the
// internal nodes, then the inner boxes in sweeps over the node array.
#include "../../include/svgf_lbvh.h"
#include "svgf_lbvh_core.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace {

struct HostKeys {
    const lbvh_key *sorted;
    int L;
    lbvh_key operator()(int k) const { return sorted[(size_t)k * L]; }
};

void leaf_record(const SvgfBvhNode *boxes, const lbvh_key *sorted, lbvh_key idx_mask, int n_tris, int L, int k, SvgfBvhNode &out)
{
    const int first = k * L, count = (n_tris - first < L) ? n_tris - first : L;
    const SvgfBvhNode &b0 = boxes[sorted[first] & idx_mask];
    for (int c = 0; c < 3; c++) { out.lo[c] = b0.lo[c]; out.hi[c] = b0.hi[c]; }
    for (int t = first + 1; t < first + count; t++) {
        const SvgfBvhNode &b = boxes[sorted[t] & idx_mask];
        for (int c = 0; c < 3; c++) { out.lo[c] = fminf(out.lo[c], b.lo[c]); out.hi[c] = fmaxf(out.hi[c], b.hi[c]); }
    }
    out.first = first; out.count = count;
}

}  // namespace

extern "C" int svgf_lbvh_build_host(const SvgfBvhNode *tri_boxes, int n_tris, const SvgfLbvhParams *p, SvgfBvhNode *nodes, int *order,
                                    unsigned long long *keys, SvgfLbvhInfo *info)
{
    if (!tri_boxes || !nodes || !order || !info || n_tris < 1 || n_tris > SVGF_SCENE_MAX_TRIS) return SVGF_ERR_INVALID_ARG;
    if (p && (p->leaf_tris < 0 || p->leaf_tris > 8)) return SVGF_ERR_INVALID_ARG;
    const int L = (p && p->leaf_tris) ? p->leaf_tris : 4;
    const LbvhBits bits = lbvh_bits(n_tris);
    const int n_leaves = (n_tris + L - 1) / L;
    float bmin[3] = { INFINITY, INFINITY, INFINITY }, bmax[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (int i = 0; i < n_tris; i++)
        for (int c = 0; c < 3; c++) {
            const float ctr = lbvh_centroid(tri_boxes[i].lo[c], tri_boxes[i].hi[c]);
            bmin[c] = fminf(bmin[c], ctr); bmax[c] = fmaxf(bmax[c], ctr);
        }
    std::vector<lbvh_key> sorted((size_t)n_tris);
    for (int i = 0; i < n_tris; i++) sorted[i] = lbvh_make_key(tri_boxes[i].lo, tri_boxes[i].hi, bmin, bmax, bits, i);
    std::sort(sorted.begin(), sorted.end());
    const lbvh_key idx_mask = ((lbvh_key)1 << bits.idx_bits) - 1;
    for (int i = 0; i < n_tris; i++) {
        order[i] = (int)(sorted[i] & idx_mask);
        if (keys) keys[i] = sorted[i];
    }
    const HostKeys key{ sorted.data(), L };
    if (n_leaves == 1) {
        leaf_record(tri_boxes, sorted.data(), idx_mask, n_tris, L, 0, nodes[0]);
    } else {
        nodes[0].first = 1; nodes[0].count = 0;
        for (int i = 0; i < n_leaves - 1; i++) {
            int lo, hi, gamma;
            lbvh_node(key, n_leaves, bits.key_bits, i, lo, hi, gamma);
            SvgfBvhNode &a = nodes[1 + 2 * (size_t)i], &b = nodes[2 + 2 * (size_t)i];
            if (lo == gamma) leaf_record(tri_boxes, sorted.data(), idx_mask, n_tris, L, gamma, a);
            else { a.first = 1 + 2 * gamma; a.count = 0; }
            if (hi == gamma + 1) leaf_record(tri_boxes, sorted.data(), idx_mask, n_tris, L, gamma + 1, b);
            else { b.first = 1 + 2 * (gamma + 1); b.count = 0; }
        }
        // Children need not stand behind their parent in this layout (a child's internal index may be lower than its parent's), so the
        // boxes are folded in sweeps: a node is finished once both children are; at most depth_bound + 1 sweeps.
        const int n_nodes = 2 * n_leaves - 1;
        std::vector<unsigned char> done((size_t)n_nodes);
        for (int k = 0; k < n_nodes; k++) done[k] = nodes[k].count > 0;
        for (bool pending = true; pending;) {
            pending = false;
            std::vector<int> ready;
            for (int k = 0; k < n_nodes; k++) {
                if (done[k]) continue;
                if (done[nodes[k].first] && done[nodes[k].first + 1]) ready.push_back(k);
                else pending = true;
            }
            for (int k : ready) {
                const SvgfBvhNode &a = nodes[nodes[k].first], &b = nodes[nodes[k].first + 1];
                for (int c = 0; c < 3; c++) { nodes[k].lo[c] = fminf(a.lo[c], b.lo[c]); nodes[k].hi[c] = fmaxf(a.hi[c], b.hi[c]); }
                done[k] = 1;
            }
            if (ready.empty()) break;
        }
    }
    const int depth_bound = bits.key_bits < n_leaves - 1 ? bits.key_bits : n_leaves - 1;
    *info = SvgfLbvhInfo{ n_tris, n_leaves, 2 * n_leaves - 1, L, bits.idx_bits, bits.axis_bits, bits.key_bits, depth_bound,
                          5 + 3 * lbvh_passes(bits.key_bits), 0ull };
    return SVGF_OK;
}
