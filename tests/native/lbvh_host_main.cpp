// lbvh_host_main.cpp — svgf_lbvh_build_host (row f24) as a stand-alone program, for a run under AddressSanitizer / UBSan
// (tests/test_lbvh.py compiles it with csrc/svgf_lbvh_host.cpp and -fsanitize=address,undefined).  Every case builds a tree into arrays
// of exactly the documented size, walks it (a binary tree over a permutation, leaves of 1..L triangles, depth within the bound, keys
// strictly increasing) and prints one line; "all trees hold" ends a clean run.
#include "svgf_lbvh.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static float uniform(float a, float b)
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return a + (b - a) * (float)((rng_state >> 40) & 0xFFFFFF) / 16777216.0f;
}

static int check(const char *name, const std::vector<SvgfBvhNode> &boxes, int L)
{
    const int n = (int)boxes.size(), Lq = L ? L : 4, n_leaves = (n + Lq - 1) / Lq;
    std::vector<SvgfBvhNode> nodes((size_t)2 * n_leaves);
    std::vector<int> order((size_t)n);
    std::vector<unsigned long long> keys((size_t)n);
    SvgfLbvhParams p = { L };
    SvgfLbvhInfo info;
    const int rc = svgf_lbvh_build_host(boxes.data(), n, &p, nodes.data(), order.data(), keys.data(), &info);
    if (rc != SVGF_OK) { std::printf("%s: rc %d\n", name, rc); return 1; }
    if (info.n_leaves != n_leaves || info.n_nodes != 2 * n_leaves - 1 || info.depth_bound > SVGF_SCENE_MAX_DEPTH || info.key_bits > 48) {
        std::printf("%s: info\n", name); return 1;
    }
    for (int i = 1; i < n; i++) if (!(keys[i] > keys[i - 1])) { std::printf("%s: keys not increasing at %d\n", name, i); return 1; }
    std::vector<int> hit((size_t)n, 0), seen((size_t)info.n_nodes, 0);
    for (int i = 0; i < n; i++) { if (order[i] < 0 || order[i] >= n || hit[order[i]]++) { std::printf("%s: order\n", name); return 1; } }
    std::vector<int> stack_node{ 0 }, stack_depth{ 0 };
    int depth = 0, covered = 0;
    while (!stack_node.empty()) {
        const int k = stack_node.back(), d = stack_depth.back();
        stack_node.pop_back(); stack_depth.pop_back();
        if (k < 0 || k >= info.n_nodes || seen[k]++) { std::printf("%s: node %d\n", name, k); return 1; }
        depth = d > depth ? d : depth;
        if (nodes[k].count > 0) {
            if (nodes[k].count > Lq || nodes[k].first < 0 || nodes[k].first + nodes[k].count > n) { std::printf("%s: leaf %d\n", name, k); return 1; }
            covered += nodes[k].count;
        } else {
            stack_node.push_back(nodes[k].first); stack_depth.push_back(d + 1);
            stack_node.push_back(nodes[k].first + 1); stack_depth.push_back(d + 1);
        }
    }
    if (covered != n || depth > info.depth_bound) { std::printf("%s: covered %d of %d, depth %d bound %d\n", name, covered, n, depth, info.depth_bound); return 1; }
    std::printf("%s: n %d L %d leaves %d key_bits %d depth %d <= %d\n", name, n, Lq, n_leaves, info.key_bits, depth, info.depth_bound);
    return 0;
}

static std::vector<SvgfBvhNode> random_boxes(int n, float spread)
{
    std::vector<SvgfBvhNode> b((size_t)n);
    for (int i = 0; i < n; i++)
        for (int c = 0; c < 3; c++) { const float x = uniform(-spread, spread); b[i].lo[c] = x - 0.01f; b[i].hi[c] = x + 0.01f; b[i].first = i; b[i].count = 1; }
    return b;
}

int main()
{
    int bad = 0;
    const int sizes[] = { 1, 2, 3, 4, 5, 8, 9, 257, 4097 };
    for (int n : sizes)
        for (int L : { 0, 1, 8 }) bad += check("random", random_boxes(n, 3.0f), L);
    std::vector<SvgfBvhNode> same(4096, random_boxes(1, 1.0f)[0]);
    bad += check("coincident", same, 1);
    std::vector<SvgfBvhNode> odd = random_boxes(300, 2.0f);
    odd[7].lo[0] = std::numeric_limits<float>::quiet_NaN(); odd[7].hi[2] = std::numeric_limits<float>::quiet_NaN();
    odd[11].lo[1] = -std::numeric_limits<float>::infinity(); odd[12].hi[1] = std::numeric_limits<float>::infinity();
    bad += check("nan and inf", odd, 4);
    std::vector<SvgfBvhNode> nan_all = random_boxes(33, 1.0f);
    for (auto &b : nan_all) for (int c = 0; c < 3; c++) b.lo[c] = b.hi[c] = std::numeric_limits<float>::quiet_NaN();
    bad += check("all nan", nan_all, 3);
    // refusals
    SvgfBvhNode one = random_boxes(1, 1.0f)[0], out[2];
    int ord[1];
    SvgfLbvhInfo info;
    SvgfLbvhParams p9 = { 9 }, pm = { -1 };
    bad += svgf_lbvh_build_host(nullptr, 1, nullptr, out, ord, nullptr, &info) != SVGF_ERR_INVALID_ARG;
    bad += svgf_lbvh_build_host(&one, 0, nullptr, out, ord, nullptr, &info) != SVGF_ERR_INVALID_ARG;
    bad += svgf_lbvh_build_host(&one, SVGF_SCENE_MAX_TRIS + 1, nullptr, out, ord, nullptr, &info) != SVGF_ERR_INVALID_ARG;
    bad += svgf_lbvh_build_host(&one, 1, &p9, out, ord, nullptr, &info) != SVGF_ERR_INVALID_ARG;
    bad += svgf_lbvh_build_host(&one, 1, &pm, out, ord, nullptr, &info) != SVGF_ERR_INVALID_ARG;
    bad += svgf_lbvh_build_host(&one, 1, nullptr, nullptr, ord, nullptr, &info) != SVGF_ERR_INVALID_ARG;
    bad += svgf_lbvh_build_host(&one, 1, nullptr, out, nullptr, nullptr, &info) != SVGF_ERR_INVALID_ARG;
    bad += svgf_lbvh_build_host(&one, 1, nullptr, out, ord, nullptr, nullptr) != SVGF_ERR_INVALID_ARG;
    bad += svgf_lbvh_build_host(&one, 1, nullptr, out, ord, nullptr, &info) != SVGF_OK;
    if (bad) { std::printf("%d failures\n", bad); return 1; }
    std::printf("all trees hold\n");
    return 0;
}
