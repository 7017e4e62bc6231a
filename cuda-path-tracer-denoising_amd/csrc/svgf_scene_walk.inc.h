// svgf_scene_walk.inc.h — the two walks over the resident scene's BVH, shared as TEXT (as svgf_scene_pixel.inc.h is) by the kernels that
// trace rays through it: k_scene_bvh (svgf_scene_bvh.hip, the product library: the primary ray's closest hit and row f16's shadow
// rays) and k_scene_trace (svgf_scene_trace.hip, the companion library of row f17: the same two, and both again for the bounce).
// include/svgf.h states what they compute (a gated brute force that every tree reproduces); here is how.
//
// Both walks keep the current node in registers, descend into a child and park the other one on a per-lane stack in LDS:
// stk = stack + lane, entry `level` at stk[256 * level] (stack[level][lane], 48 levels x 256 lanes x 4 B = 48 KB per block), so that
// the 64 lanes of a wave always touch 64 consecutive words - no bank conflict, no runtime-indexed private array, no scratch.  A parked
// node is tested again when it is popped, which costs one 32-byte load of a node that was loaded as a child before.  Either walk
// leaves the stack empty.  float32, contraction off in every function.
// Include inside an anonymous namespace, after svgf_scene_pixel.inc.h.

struct SceneBvhArgs {
    SceneArgs s;
    const float4 *nodes;        // SvgfBvhNode as two float4: {lo, first}, {hi, count}
    const int *order;
    const float4 *tri_boxes;    // the padded box of triangle i, the same 32-byte layout: {lo, -}, {hi, -}
};

struct SceneRay { float o[3], d[3], inv[3]; bool flat[3]; };

// S(box, ray) of include/svgf.h
__device__ __forceinline__ bool scene_slab(const float4 &lo4, const float4 &hi4, const SceneRay &r, float &tn)
{
#pragma clang fp contract(off)
    const float lo[3] = { lo4.x, lo4.y, lo4.z }, hi[3] = { hi4.x, hi4.y, hi4.z };
    float tf = __builtin_huge_valf();
    bool pass = true;
    tn = 0.0f;
    for (int c = 0; c < 3; c++) {
        if (r.flat[c]) {
            pass = pass && (lo[c] <= r.o[c]) && (r.o[c] <= hi[c]);
        } else {
            const float t1 = (lo[c] - r.o[c]) * r.inv[c], t2 = (hi[c] - r.o[c]) * r.inv[c];
            tn = fmaxf(tn, fminf(t1, t2));
            tf = fminf(tf, fmaxf(t1, t2));
        }
    }
    return pass && (tn <= tf);
}

// The closest-hit walk: the counting triangle with the least t in t_lo < t < bt (the lower index at equal t) replaces (bt, best,
// bbx, bby); bt comes in as the nearest primitive's distance and best as -1.  The nearer child first, a node skipped iff its slab test
// fails or tn > bt.
__device__ __forceinline__ void scene_nearest(const SceneBvhArgs &b, const SceneRay &r, int *const stk, float t_lo, float &bt_io, int &best_io,
                                              float &bbx_io, float &bby_io)
{
#pragma clang fp contract(off)
    const SceneArgs &a = b.s;
    float bt = bt_io, bbx = bbx_io, bby = bby_io;
    int best = best_io;
    if (a.n_tris > 0) {
        int sp = 0;
        float4 nlo = b.nodes[0], nhi = b.nodes[1];
        float tn;
        bool go = scene_slab(nlo, nhi, r, tn) && !(tn > bt);
        while (go) {
            const int first = __float_as_int(nlo.w), count = __float_as_int(nhi.w);
            bool down = false;
            if (count > 0) {
                for (int k = first; k < first + count; k++) {
                    const int i = b.order[k];
                    float bx, by, t;
                    if (!scene_tri_test(a.tris + 24 * (size_t)i, r.o, r.d, bx, by, t) || !(t > t_lo)) continue;
                    float tni;
                    if (!scene_slab(b.tri_boxes[2 * (size_t)i], b.tri_boxes[2 * (size_t)i + 1], r, tni) || !(t >= tni)) continue;
                    if (t < bt || (t == bt && best >= 0 && i < best)) { bt = t; best = i; bbx = bx; bby = by; }
                }
            } else {
                const float4 alo = b.nodes[2 * (size_t)first], ahi = b.nodes[2 * (size_t)first + 1];
                const float4 blo = b.nodes[2 * (size_t)first + 2], bhi = b.nodes[2 * (size_t)first + 3];
                float ta, tb;
                const bool pa = scene_slab(alo, ahi, r, ta) && !(ta > bt), pb = scene_slab(blo, bhi, r, tb) && !(tb > bt);
                const bool a_first = pa && (!pb || ta <= tb);
                if (pa && pb) { stk[256 * sp] = a_first ? first + 1 : first; sp++; }
                if (pa || pb) { nlo = a_first ? alo : blo; nhi = a_first ? ahi : bhi; down = true; }
            }
            if (!down) {
                go = false;
                while (sp > 0 && !go) {
                    sp--;
                    const int cur = stk[256 * sp];
                    nlo = b.nodes[2 * (size_t)cur]; nhi = b.nodes[2 * (size_t)cur + 1];
                    go = scene_slab(nlo, nhi, r, tn) && !(tn > bt);
                }
            }
        }
    }
    bt_io = bt; best_io = best; bbx_io = bbx; bby_io = bby;
}

// The any-hit walk (row f16): true iff an occluder counts on the ray r with t_lo < t < t_hi - the primitives that do not emit, then
// the nodes, leaving at the first counting triangle.  Occlusion is an OR, so neither the visiting order nor the early exit can change
// it.
__device__ __forceinline__ bool scene_occluded(const SceneBvhArgs &b, const SceneRay &r, int *const stk, float t_lo, float t_hi)
{
#pragma clang fp contract(off)
    const SceneArgs &a = b.s;
    for (int k = 0; k < a.n_geoms; k++) {
        const SvgfSceneGeom &g = a.geoms[k];
        if (g.emittance != 0.0f) continue;
        bool hit;
        float tw, nw[3], pw[3];
        scene_primitive_test(g, r.o, r.d, hit, tw, nw, pw);
        if (hit && (tw > t_lo) && (tw < t_hi)) return true;
    }
    if (a.n_tris <= 0) return false;
    int sp = 0;
    float4 nlo = b.nodes[0], nhi = b.nodes[1];
    float tn;
    bool go = scene_slab(nlo, nhi, r, tn) && !(tn > t_hi);
    while (go) {
        const int first = __float_as_int(nlo.w), count = __float_as_int(nhi.w);
        bool down = false;
        if (count > 0) {
            for (int k = first; k < first + count; k++) {
                const int i = b.order[k];
                float bx, by, t;
                if (!scene_tri_test(a.tris + 24 * (size_t)i, r.o, r.d, bx, by, t) || !(t > t_lo) || !(t < t_hi)) continue;
                float tni;
                if (scene_slab(b.tri_boxes[2 * (size_t)i], b.tri_boxes[2 * (size_t)i + 1], r, tni) && (t >= tni)) return true;
            }
        } else {
            const float4 alo = b.nodes[2 * (size_t)first], ahi = b.nodes[2 * (size_t)first + 1];
            const float4 blo = b.nodes[2 * (size_t)first + 2], bhi = b.nodes[2 * (size_t)first + 3];
            float ta, tb;
            const bool pa = scene_slab(alo, ahi, r, ta) && !(ta > t_hi), pb = scene_slab(blo, bhi, r, tb) && !(tb > t_hi);
            if (pa && pb) { stk[256 * sp] = first + 1; sp++; }
            if (pa || pb) { nlo = pa ? alo : blo; nhi = pa ? ahi : bhi; down = true; }
        }
        if (!down) {
            go = false;
            while (sp > 0 && !go) {
                sp--;
                const int cur = stk[256 * sp];
                nlo = b.nodes[2 * (size_t)cur]; nhi = b.nodes[2 * (size_t)cur + 1];
                go = scene_slab(nlo, nhi, r, tn) && !(tn > t_hi);
            }
        }
    }
    return false;
}

// One f16 shadow sample of pixel p from `pos` (already in r.o): the light point from hash streams ku and kv, the ray to it in r, and
// whether an occluder counts on it.  !(dl > 0) forms no ray and is unoccluded.
__device__ __forceinline__ bool scene_shadow_sample(const SceneBvhArgs &b, const float edge_u[3], const float edge_v[3], SceneRay &r,
                                                    const float pos[3], int *const stk, int p, unsigned ku, unsigned kv)
{
#pragma clang fp contract(off)
    const SceneArgs &a = b.s;
    const float u = scene_hash(a.seed, a.frame, (unsigned)p, ku), v = scene_hash(a.seed, a.frame, (unsigned)p, kv);
    const float su = 2.0f * u - 1.0f, sv = 2.0f * v - 1.0f;
    float q[3];
    for (int c = 0; c < 3; c++) q[c] = ((a.light[c] + su * edge_u[c]) + sv * edge_v[c]) - pos[c];
    const float dl = sqrtf((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]);
    bool occluded = false;
    if (dl > 0.0f) {
        for (int c = 0; c < 3; c++) { r.d[c] = q[c] / dl; r.flat[c] = fabsf(r.d[c]) < 0x1p-100f; r.inv[c] = 1.0f / r.d[c]; }
        const float t_lo = 0x1p-10f * fmaxf(1.0f, dl);
        occluded = scene_occluded(b, r, stk, t_lo, dl - t_lo);
    }
    return occluded;
}
