// svgf_deform_check_rig_host (csrc/svgf_deform_rig.cpp, row f26) as a stand-alone program for AddressSanitizer / UBSan: the arrays are
// heap blocks of exactly the size the check may read, so that a read past a rig's end is an error and not a lucky value.
// tests/test_deform_scene.py compiles this file together with the library's source and runs it.
#include "svgf_deform.h"

#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

static int failures = 0;

static void expect(int got, int want, const char *what)
{
    if (got != want) { std::printf("FAIL %s: %d, expected %d\n", what, got, want); failures++; }
}

struct Rig {
    std::vector<int> tri;
    std::vector<unsigned short> bone;
    std::vector<float> weight;
    Rig(int n_skinned, int stride, int n_bones) : tri((size_t)n_skinned), bone(12 * (size_t)n_skinned), weight(12 * (size_t)n_skinned)
    {
        for (int s = 0; s < n_skinned; s++) tri[(size_t)s] = stride * s;
        for (size_t k = 0; k < bone.size(); k++) { bone[k] = (unsigned short)(k % (size_t)n_bones); weight[k] = 0.25f; }
    }
    int check(int n_tris, int n_bones) const { return svgf_deform_check_rig_host(n_tris, tri.data(), (int)tri.size(), bone.data(), weight.data(), n_bones); }
};

int main()
{
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    for (int n : { 1, 2, 255, 256, 257, 4097 }) {
        for (int n_bones : { 1, 7, SVGF_DEFORM_MAX_BONES }) {
            Rig r(n, 2, n_bones);
            expect(r.check(2 * n, n_bones), SVGF_OK, "a valid rig");
            expect(r.check(2 * n - 2, n_bones), SVGF_ERR_INVALID_ARG, "the last index == n_tris");
            expect(r.check(2 * n, 0), SVGF_ERR_INVALID_ARG, "n_bones 0");
            expect(r.check(2 * n, SVGF_DEFORM_MAX_BONES + 1), SVGF_ERR_INVALID_ARG, "n_bones above the limit");
            if (n_bones > 1 && 12 * n >= n_bones) expect(r.check(2 * n, n_bones - 1), SVGF_ERR_INVALID_ARG, "a bone index == n_bones");
            Rig last = r;
            last.bone.back() = (unsigned short)n_bones;
            expect(last.check(2 * n, n_bones), SVGF_ERR_INVALID_ARG, "the very last bone index out of range");
            for (float v : { -1.0f, -1e-38f, nan, inf, -inf }) {
                Rig w = r;
                w.weight.back() = v;
                expect(w.check(2 * n, n_bones), SVGF_ERR_INVALID_ARG, "the very last weight negative or not finite");
                w = r;
                w.weight.front() = v;
                expect(w.check(2 * n, n_bones), SVGF_ERR_INVALID_ARG, "the first weight negative or not finite");
            }
            Rig z = r;
            for (float &v : z.weight) v = 0.0f;
            z.weight[0] = -0.0f;
            expect(z.check(2 * n, n_bones), SVGF_OK, "weights of zero are finite and not negative");
            if (n > 1) {
                Rig o = r;
                o.tri[(size_t)n - 1] = o.tri[(size_t)n - 2];
                expect(o.check(2 * n, n_bones), SVGF_ERR_INVALID_ARG, "an index repeated");
                o.tri[(size_t)n - 1] = o.tri[(size_t)n - 2] - 1;
                expect(o.check(2 * n, n_bones), SVGF_ERR_INVALID_ARG, "an index below the one before it");
            }
            Rig neg = r;
            neg.tri[0] = -1;
            expect(neg.check(2 * n, n_bones), SVGF_ERR_INVALID_ARG, "a negative index");
            expect(svgf_deform_check_rig_host(2 * n, nullptr, n, r.bone.data(), r.weight.data(), n_bones), SVGF_ERR_INVALID_ARG, "NULL tri_index");
            expect(svgf_deform_check_rig_host(2 * n, r.tri.data(), n, nullptr, r.weight.data(), n_bones), SVGF_ERR_INVALID_ARG, "NULL bone");
            expect(svgf_deform_check_rig_host(2 * n, r.tri.data(), n, r.bone.data(), nullptr, n_bones), SVGF_ERR_INVALID_ARG, "NULL weight");
            expect(svgf_deform_check_rig_host(2 * n, r.tri.data(), 0, r.bone.data(), r.weight.data(), n_bones), SVGF_ERR_INVALID_ARG, "n_skinned 0");
            expect(svgf_deform_check_rig_host(n - 1, r.tri.data(), n, r.bone.data(), r.weight.data(), n_bones), SVGF_ERR_INVALID_ARG, "n_skinned > n_tris");
        }
    }
    Rig dense(300, 1, 3);                   // every triangle skinned
    expect(dense.check(300, 3), SVGF_OK, "a rig over every triangle");
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("all rigs hold\n");
    return 0;
}
