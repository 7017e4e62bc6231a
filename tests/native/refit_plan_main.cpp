// refit_plan_main.cpp — svgf_bvh_refit_plan_host and svgf_pose_rigid on adversarial trees, as a stand-alone program: compiled with
// svgf_bvh_build.cpp under -fsanitize=address,undefined by tests/test_animated_scene.py and run as a child process.  Every output
// array is allocated at exactly the documented size, so a write past it is a sanitizer report; the plan's invariants are checked too.
#include "svgf.h"

#include <cstdio>
#include <cstdlib>
#include <functional>
#include <vector>

namespace {

// a node array in the builder's layout with one triangle per leaf; left_of(n): how many of a node's n leaves go left
std::vector<SvgfBvhNode> make_tree(int n_leaves, const std::function<int(int)> &left_of)
{
    std::vector<SvgfBvhNode> nodes((size_t)(2 * n_leaves - 1), SvgfBvhNode{});
    int used = 1, tri = 0;
    std::function<void(int, int)> build = [&](int k, int n) {
        if (n == 1) { nodes[k].first = tri++; nodes[k].count = 1; return; }
        const int a = used;
        used += 2;
        nodes[k].first = a; nodes[k].count = 0;
        const int nl = left_of(n);
        build(a, nl);
        build(a + 1, n - nl);
    };
    build(0, n_leaves);
    return nodes;
}

int fail(const char *what, int a, int b)
{
    std::printf("FAILED: %s (%d, %d)\n", what, a, b);
    return 1;
}

int check(const char *name, const std::vector<SvgfBvhNode> &nodes, int cap, int want_rc)
{
    const int n = (int)nodes.size();
    std::vector<SvgfRefitTreelet> treelets((size_t)n);
    std::vector<unsigned char> level((size_t)n);
    std::vector<int> top((size_t)n), seg(SVGF_SCENE_MAX_DEPTH + 2);
    SvgfRefitPlanInfo info;
    const int rc = svgf_bvh_refit_plan_host(nodes.data(), n, cap, treelets.data(), level.data(), top.data(), seg.data(), &info);
    if (rc != want_rc) return fail(name, rc, want_rc);
    if (rc != SVGF_OK) return 0;
    std::vector<int> owner((size_t)n, 0), done((size_t)n, 0);
    for (int t = 0; t < info.n_treelets; t++) {
        const SvgfRefitTreelet &tl = treelets[t];
        if (tl.count + 1 > cap || tl.root < 0 || tl.root >= n || tl.begin < 0 || tl.begin + tl.count > n) return fail("treelet out of range", t, tl.count);
        owner[tl.root]++; done[tl.root] = 1;
        for (int g = tl.begin; g < tl.begin + tl.count; g++) {
            owner[g]++; done[g] = 1;
            if (nodes[g].count == 0 && level[g] + 1 > tl.levels) return fail("an inner node below the last level", g, tl.levels);
        }
    }
    if (seg[0] != 0 || seg[info.n_top_depths] != info.n_top) return fail("segments", seg[0], info.n_top);
    for (int s = 0; s < info.n_top_depths; s++) {
        for (int i = seg[s]; i < seg[s + 1]; i++) {
            const int g = top[i];
            if (g < 0 || g >= n || nodes[g].count != 0) return fail("top entry", i, g);
            owner[g]++;
            if (!done[nodes[g].first] || !done[nodes[g].first + 1]) return fail("a top node before its children", g, s);
        }
        for (int i = seg[s]; i < seg[s + 1]; i++) done[top[i]] = 1;
    }
    for (int k = 0; k < n; k++)
        if (owner[k] != 1) return fail("a node in no or in two parts", k, owner[k]);
    std::printf("%s cap %d: %d nodes, %d treelets, %d top nodes in %d depths\n", name, cap, n, info.n_treelets, info.n_top, info.n_top_depths);
    return 0;
}

}  // namespace

int main()
{
    const int CAP = SVGF_SCENE_REFIT_CAP;
    int bad = 0;
    const auto half = [](int n) { return (n + 1) / 2; };
    const auto one = [](int) { return 1; };
    const auto rest = [](int n) { return n - 1; };
    const int caps[] = { CAP, 1, 2, 3, 7, 1022, 1023 };
    for (int cap : caps) {
        bad += check("chain48", make_tree(49, one), cap, SVGF_OK);
        bad += check("left_chain48", make_tree(49, rest), cap, SVGF_OK);
        bad += check("perfect_2cap-1", make_tree(CAP, half), cap, SVGF_OK);
        bad += check("1023_nodes", make_tree(512, half), cap, SVGF_OK);
        bad += check("1025_nodes", make_tree(513, half), cap, SVGF_OK);
        bad += check("single_leaf", make_tree(1, half), cap, SVGF_OK);
    }
    bad += check("chain49", make_tree(50, one), CAP, SVGF_ERR_UNSUPPORTED);
    bad += check("cap 0", make_tree(8, half), 0, SVGF_ERR_INVALID_ARG);
    {   // malformed arrays: refused, and nothing is written out of bounds on the way
        std::vector<SvgfBvhNode> t = make_tree(8, half);
        t[1].first = 1;
        bad += check("child at its parent", t, 4, SVGF_ERR_INVALID_ARG);
        t = make_tree(8, half); t[2].first = t[1].first;
        bad += check("two parents", t, 4, SVGF_ERR_INVALID_ARG);
        t = make_tree(8, half); t[0].first = (int)t.size() - 1;
        bad += check("children off the end", t, 4, SVGF_ERR_INVALID_ARG);
        t = make_tree(8, half); t[0].first = 0x7fffffff;
        bad += check("children far off the end", t, 4, SVGF_ERR_INVALID_ARG);
        t = make_tree(8, half); t[3].count = -1;
        bad += check("negative count", t, 4, SVGF_ERR_INVALID_ARG);
        t = make_tree(8, half); std::swap(t[1], t[2]);
        bad += check("not the builder's layout", t, 4, SVGF_ERR_UNSUPPORTED);
    }
    SvgfRefitPlanInfo info;
    int seg[SVGF_SCENE_MAX_DEPTH + 2];
    if (svgf_bvh_refit_plan_host(nullptr, 0, CAP, nullptr, nullptr, nullptr, seg, &info) != SVGF_OK || info.n_treelets != 0) bad += fail("no nodes", 0, 0);
    const float axis[3] = { 0.3f, -0.5f, 0.8f }, zero[3] = { 0, 0, 0 }, pivot[3] = { 1, -2, 0.5f };
    SvgfScenePose p;
    if (svgf_pose_rigid(axis, 2.9670597f, pivot, zero, &p) != SVGF_OK || svgf_pose_rigid(zero, 1.0f, pivot, zero, &p) != SVGF_ERR_INVALID_ARG) bad += fail("pose_rigid", 0, 0);
    if (bad) return 1;
    std::printf("all plans hold\n");
    return 0;
}
