// svgf_scene_gloss.inc.h — the glossy draw's pixel and its host-side preparation, shared as TEXT by two companion libraries, as
// svgf_scene_trace.inc.h is by the two before them: libsvgf_gloss.so (svgf_scene_gloss.hip: svgf_gloss_draw and svgf_gloss_draw_split,
// row f20) instantiates k_scene_gloss for SceneGlossArgs and SceneGlossSplitArgs, libsvgf_virtual.so (svgf_scene_virtual.hip: svgf_virtual_draw and
// svgf_virtual_draw_split, row f21) instantiates it for SceneVirtualArgs and SceneVirtualSplitArgs - every ray of every path the same statements, plus the GUIDE
// chain that replaces the first hit's normal, position and id in the stored texel where the first hit is purely specular
// (include/svgf_virtual.h); libsvgf_rough.so (svgf_scene_rough.hip: svgf_rough_draw and svgf_rough_draw_split, row f22) instantiates it for
// SceneRoughArgs and SceneRoughSplitArgs - the guide, and a GGX lobe (ROUGH) on the mirror vertices of objects with a roughness
// (include/svgf_rough.h); libsvgf_highlight.so (svgf_scene_highlight.hip: svgf_highlight_draw and svgf_highlight_draw_split, row f23)
// instantiates it for SceneHighlightArgs and SceneHighlightSplitArgs - the guide, the lobe, and the analytic light's GGX term (SHINE) at
// the rough vertices, through the shadow samples the diffuse vertices use (include/svgf_highlight.h).  Include inside an anonymous namespace, behind svgf_scene_trace.inc.h (whose text this one continues: the
// includer names both) and after svgf_path.h and svgf_gloss_table.h.
//
// k_scene_gloss: one thread per pixel, 256 per block, every ray of the pixel on the per-lane LDS stack stack[level][lane] (48 x 256 x 4 B;
// empty between rays).  Paths and vertices are runtime loops around ONE vertex body - classify, gather, throughput, roulette, next ray,
// nearest hit - so the code object holds one closest-hit walk and one any-hit walk behind the first hit whatever the counts and
// whatever the classes: the class selects how d', thr and acc are formed, not a second copy of a walk.  A path's state is scalars in
// registers - thr, acc, the vertex, its normal, albedo and id, the direction that arrived, the inside bit - no runtime-indexed private
// array, no scratch, no spinning, no traffic between workgroups.
// The guide (GUIDE only) is ONE MORE TURN of the path loop, behind the last path: the same classify, next ray and nearest hit with the
// class stream replaced by a constant and the gather, the throughput, the roulette and the sampler never reached.  It comes last so
// that nothing of it is live across the paths: what it leaves - a normal, an id, a length, a count - goes straight into the store.

// t (and for the split form s.t).bounce_samples carries `paths`
struct SceneGlossArgs {
    SceneTraceArgs t;
    int max_depth, rr_depth;
    const SvgfSurface *table;
    int n_table;
};

struct SceneGlossSplitArgs {
    SceneSplitArgs s;
    int max_depth, rr_depth;
    const SvgfSurface *table;
    int n_table;
};

// svgf_virtual_draw's and svgf_virtual_draw_split's: the glossy draw's arguments and the guide's own
struct SceneGuide {
    int max_chain, id_offset;
    int *out_chain;             // one int per pixel, or null
};

struct SceneVirtualArgs {
    SceneGlossArgs g;
    SceneGuide v;
};

struct SceneVirtualSplitArgs {
    SceneGlossSplitArgs g;
    SceneGuide v;
};

// svgf_rough_draw's and svgf_rough_draw_split's: the virtual draw's arguments and the roughness table's
struct SceneRough {
    const float *alpha;         // n values on the scene's device (null with n == 0)
    int n;
    float guide_alpha;
};

struct SceneRoughArgs {
    SceneVirtualArgs v;
    SceneRough r;
};

struct SceneRoughSplitArgs {
    SceneVirtualSplitArgs v;
    SceneRough r;
};

// svgf_highlight_draw's and svgf_highlight_draw_split's: the rough draw's arguments and the highlight's two parameters
struct SceneHighlight {
    int enable;
    float clamp;
};

struct SceneHighlightArgs {
    SceneRoughArgs r;
    SceneHighlight h;
};

struct SceneHighlightSplitArgs {
    SceneRoughSplitArgs r;
    SceneHighlight h;
};

__device__ __forceinline__ const SceneTraceArgs &trace_args(const SceneGlossArgs &a) { return a.t; }
__device__ __forceinline__ const SceneTraceArgs &trace_args(const SceneGlossSplitArgs &a) { return a.s.t; }
__device__ __forceinline__ const SceneGlossArgs &gloss_args(const SceneGlossArgs &a) { return a; }
__device__ __forceinline__ const SceneGlossSplitArgs &gloss_args(const SceneGlossSplitArgs &a) { return a; }
__device__ __forceinline__ const SceneGlossArgs &gloss_args(const SceneVirtualArgs &a) { return a.g; }
__device__ __forceinline__ const SceneGlossSplitArgs &gloss_args(const SceneVirtualSplitArgs &a) { return a.g; }
__device__ __forceinline__ const SceneGlossArgs &gloss_args(const SceneRoughArgs &a) { return a.v.g; }
__device__ __forceinline__ const SceneGlossSplitArgs &gloss_args(const SceneRoughSplitArgs &a) { return a.v.g; }
__device__ __forceinline__ const SceneGlossArgs &gloss_args(const SceneHighlightArgs &a) { return a.r.v.g; }
__device__ __forceinline__ const SceneGlossSplitArgs &gloss_args(const SceneHighlightSplitArgs &a) { return a.r.v.g; }
// the guide's arguments; a draw without a guide has none, and its kernel reads none
__device__ __forceinline__ SceneGuide gloss_guide(const SceneGlossArgs &) { return SceneGuide{ 0, 0, nullptr }; }
__device__ __forceinline__ SceneGuide gloss_guide(const SceneGlossSplitArgs &) { return SceneGuide{ 0, 0, nullptr }; }
__device__ __forceinline__ SceneGuide gloss_guide(const SceneVirtualArgs &a) { return a.v; }
__device__ __forceinline__ SceneGuide gloss_guide(const SceneVirtualSplitArgs &a) { return a.v; }
__device__ __forceinline__ SceneGuide gloss_guide(const SceneRoughArgs &a) { return a.v.v; }
__device__ __forceinline__ SceneGuide gloss_guide(const SceneRoughSplitArgs &a) { return a.v.v; }
__device__ __forceinline__ SceneGuide gloss_guide(const SceneHighlightArgs &a) { return a.r.v.v; }
__device__ __forceinline__ SceneGuide gloss_guide(const SceneHighlightSplitArgs &a) { return a.r.v.v; }
// the roughness table; only the ROUGH kernels read one
template <class Args> __device__ __forceinline__ SceneRough gloss_rough(const Args &) { return SceneRough{ nullptr, 0, 0.0f }; }
__device__ __forceinline__ SceneRough gloss_rough(const SceneRoughArgs &a) { return a.r; }
__device__ __forceinline__ SceneRough gloss_rough(const SceneRoughSplitArgs &a) { return a.r; }
__device__ __forceinline__ SceneRough gloss_rough(const SceneHighlightArgs &a) { return a.r.r; }
__device__ __forceinline__ SceneRough gloss_rough(const SceneHighlightSplitArgs &a) { return a.r.r; }
// the highlight's parameters; only the SHINE kernels read them
template <class Args> __device__ __forceinline__ SceneHighlight gloss_shine(const Args &) { return SceneHighlight{ 0, 0.0f }; }
__device__ __forceinline__ SceneHighlight gloss_shine(const SceneHighlightArgs &a) { return a.h; }
__device__ __forceinline__ SceneHighlight gloss_shine(const SceneHighlightSplitArgs &a) { return a.h; }

// the surface of object id g: the table's record, or the diffuse one (all fields 0) outside it
__device__ __forceinline__ SvgfSurface gloss_surface(const SvgfSurface *table, int n_table, int g)
{
    SvgfSurface S = { 0.0f, 0.0f, 0.0f, { 0.0f, 0.0f, 0.0f } };
    if (g >= 0 && g < n_table) S = table[g];
    return S;
}

// The class of a vertex with surface S and normal n, reached along d, from the stream value u: false = diffuse (dn, wgt = 1 and
// `moved` untouched or unused); true = specular, with the direction dn the path goes on in, the weight wgt of the lobe, and, for a
// transmission, `inside` toggled and `moved` set (the ray starts behind the surface, along -nn).  nn is written for a glass vertex.
__device__ __forceinline__ bool gloss_vertex(const SvgfSurface &S, bool triangle, const float d[3], const float n[3], float u, bool &inside,
                                             float dn[3], float wgt[3], float nn[3], bool &moved)
{
#pragma clang fp contract(off)
    moved = false;
    wgt[0] = 1.0f; wgt[1] = 1.0f; wgt[2] = 1.0f;
    const bool glass = S.refract > 0.0f && !triangle;
    const float dotn = (d[0] * n[0] + d[1] * n[1]) + d[2] * n[2];
    if (glass) {
        const bool flip = dotn > 0.0f;
        for (int c = 0; c < 3; c++) nn[c] = flip ? -n[c] : n[c];
        const float eta = inside ? S.ior : 1.0f / S.ior;
        const float dnn = (d[0] * nn[0] + d[1] * nn[1]) + d[2] * nn[2];
        const float cs = -dnn;
        const float r0 = (1.0f - eta) / (1.0f + eta), R0 = r0 * r0;
        const float m = 1.0f - cs;
        const float R = R0 + (1.0f - R0) * (((m * m) * (m * m)) * m);
        const float k2 = 1.0f - (eta * eta) * (1.0f - cs * cs);
        if (!(k2 >= 0.0f) || u < R) {
            const float f = 2.0f * dnn;
            for (int c = 0; c < 3; c++) { dn[c] = d[c] - f * nn[c]; wgt[c] = S.spec[c]; }
        } else {
            const float f = eta * cs - sqrtf(k2);
            for (int c = 0; c < 3; c++) dn[c] = eta * d[c] + f * nn[c];
            inside = !inside;
            moved = true;
        }
        normalise3(dn);
        return true;
    }
    if (u < S.reflect) {
        const float f = 2.0f * dotn;
        for (int c = 0; c < 3; c++) { dn[c] = d[c] - f * n[c]; wgt[c] = S.spec[c]; }
        normalise3(dn);
        return true;
    }
    return false;
}

// The GGX lobe of a ROUGH vertex (include/svgf_rough.h states this order of operations): a mirror vertex with roughness alpha > 0 and
// normal n, reached along d.  False: the vertex is not rough (v.n is not above 0) and dn and wgt stay gloss_vertex's.  True: dn is the
// direction d reflected about a normal h drawn from the visible normals, by the disc point the diffuse sampler would have drawn here
// (streams base + 0..7), wgt is wgt times G1(dn.n), and `absorbed` says that dn does not leave the surface.
__device__ __forceinline__ bool rough_vertex(const SceneArgs &a, int p, unsigned base, float alpha, const float d[3], const float n[3], float dn[3],
                                             float wgt[3], bool &absorbed)
{
#pragma clang fp contract(off)
    absorbed = false;
    const float s = copysignf(1.0f, n[2]), q = -1.0f / (s + n[2]), w = (n[0] * n[1]) * q;
    const float T[3] = { 1.0f + ((s * n[0]) * n[0]) * q, s * w, -(s * n[0]) };
    const float B[3] = { w, s + (n[1] * n[1]) * q, -n[1] };
    const float v[3] = { -d[0], -d[1], -d[2] };
    const float v_t = (v[0] * T[0] + v[1] * T[1]) + v[2] * T[2], v_b = (v[0] * B[0] + v[1] * B[1]) + v[2] * B[2];
    const float v_n = (v[0] * n[0] + v[1] * n[1]) + v[2] * n[2];
    if (!(v_n > 0.0f)) return false;
    // the disc point: trace_direction's bounded rejection
    float t1 = 0.0f, t2 = 0.0f;
    bool found = false;
#pragma unroll
    for (unsigned k = 0; k < 4; k++) {
        const float ak = 2.0f * scene_hash(a.seed, a.frame, (unsigned)p, base + 2 * k) - 1.0f;
        const float bk = 2.0f * scene_hash(a.seed, a.frame, (unsigned)p, base + 2 * k + 1) - 1.0f;
        const bool take = !found && (ak * ak + bk * bk < 1.0f);
        t1 = take ? ak : t1; t2 = take ? bk : t2;
        found = found || take;
    }
    float Vh[3] = { alpha * v_t, alpha * v_b, v_n };
    normalise3(Vh);
    const float lensq = Vh[0] * Vh[0] + Vh[1] * Vh[1];
    float T1x = 1.0f, T1y = 0.0f;
    if (lensq > 0.0f) {
        const float len = sqrtf(lensq);
        T1x = -Vh[1] / len; T1y = Vh[0] / len;
    }
    const float T2[3] = { -(Vh[2] * T1y), Vh[2] * T1x, Vh[0] * T1y - Vh[1] * T1x };
    const float sh = 0.5f * (1.0f + Vh[2]);
    const float one = 1.0f - t1 * t1;
    const float t2p = (1.0f - sh) * sqrtf(one) + sh * t2;
    const float cz = sqrtf(fmaxf(0.0f, one - t2p * t2p));
    const float Nh[3] = { (t1 * T1x + t2p * T2[0]) + cz * Vh[0], (t1 * T1y + t2p * T2[1]) + cz * Vh[1], t2p * T2[2] + cz * Vh[2] };
    float hl[3] = { alpha * Nh[0], alpha * Nh[1], fmaxf(0.0f, Nh[2]) };
    normalise3(hl);
    float h[3];
    for (int c = 0; c < 3; c++) h[c] = (hl[0] * T[c] + hl[1] * B[c]) + hl[2] * n[c];
    const float f = 2.0f * ((d[0] * h[0] + d[1] * h[1]) + d[2] * h[2]);
    for (int c = 0; c < 3; c++) dn[c] = d[c] - f * h[c];
    normalise3(dn);
    const float l_n = (dn[0] * n[0] + dn[1] * n[1]) + dn[2] * n[2];
    if (!(l_n > 0.0f)) { absorbed = true; return true; }
    const float a2 = alpha * alpha;
    const float G1 = (2.0f * l_n) / (l_n + sqrtf(a2 + (1.0f - a2) * (l_n * l_n)));
    for (int c = 0; c < 3; c++) wgt[c] = wgt[c] * G1;
    return true;
}

// The light's factor H at a ROUGH vertex (include/svgf_highlight.h states this order of operations): the point x with normal n and
// roughness alpha, reached along d, lit from the unit direction l.  E pi D G1(v) G1(l) / (4 v_n) of the GGX lobe rough_vertex samples,
// E the diffuse term's 30 / (4 + dist2) towards the light's centre; 0 unless l.n > 0; at most `clamp` where that is above 0.
__device__ __forceinline__ float shine_factor(const SceneArgs &a, float alpha, float clamp, const float d[3], const float n[3], const float x[3],
                                              const float l[3])
{
#pragma clang fp contract(off)
    const float l_n = (l[0] * n[0] + l[1] * n[1]) + l[2] * n[2];
    if (!(l_n > 0.0f)) return 0.0f;
    const float v[3] = { -d[0], -d[1], -d[2] };
    const float v_n = (v[0] * n[0] + v[1] * n[1]) + v[2] * n[2];
    float hv[3] = { v[0] + l[0], v[1] + l[1], v[2] + l[2] };
    normalise3(hv);
    const float h_n = (hv[0] * n[0] + hv[1] * n[1]) + hv[2] * n[2];
    const float a2 = alpha * alpha;
    const float t = (h_n * h_n) * (a2 - 1.0f) + 1.0f;
    float tl[3];
    for (int c = 0; c < 3; c++) tl[c] = a.light[c] - x[c];
    const float E = 30.0f / (4.0f + ((tl[0] * tl[0] + tl[1] * tl[1]) + tl[2] * tl[2]));
    const float G = (2.0f * l_n) / (l_n + sqrtf(a2 + (1.0f - a2) * (l_n * l_n)));
    float H = ((E * (a2 / (t * t))) * G) / (2.0f * (v_n + sqrtf(a2 + (1.0f - a2) * (v_n * v_n))));
    if (clamp > 0.0f) H = fminf(H, clamp);
    return H;
}

// Args = SceneGlossArgs: svgf_gloss_draw.  Args = SceneGlossSplitArgs: svgf_gloss_draw_split, the same rays with trace_store_split's tail.
// Args = SceneVirtualArgs, SceneVirtualSplitArgs: svgf_virtual_draw and svgf_virtual_draw_split, either with the guide (GUIDE).
// Args = SceneRoughArgs, SceneRoughSplitArgs: svgf_rough_draw and svgf_rough_draw_split, the guide and the rough lobe (ROUGH).
// Args = SceneHighlightArgs, SceneHighlightSplitArgs: svgf_highlight_draw and svgf_highlight_draw_split, those and the light's term (SHINE).
template <class AllArgs>
__global__ __launch_bounds__(256) void k_scene_gloss(AllArgs all_args)
{
#pragma clang fp contract(off)
    constexpr bool SHINE = std::is_same<AllArgs, SceneHighlightArgs>::value || std::is_same<AllArgs, SceneHighlightSplitArgs>::value;
    constexpr bool ROUGH = std::is_same<AllArgs, SceneRoughArgs>::value || std::is_same<AllArgs, SceneRoughSplitArgs>::value || SHINE;
    constexpr bool GUIDE = std::is_same<AllArgs, SceneVirtualArgs>::value || std::is_same<AllArgs, SceneVirtualSplitArgs>::value || ROUGH;
    constexpr bool SPLIT = std::is_same<AllArgs, SceneGlossSplitArgs>::value || std::is_same<AllArgs, SceneVirtualSplitArgs>::value ||
                           std::is_same<AllArgs, SceneRoughSplitArgs>::value || std::is_same<AllArgs, SceneHighlightSplitArgs>::value;
    __shared__ int stack[SVGF_SCENE_MAX_DEPTH * 256];
    const auto &args = gloss_args(all_args);
    const SceneGuide gd = gloss_guide(all_args);
    const SceneRough rg = gloss_rough(all_args);
    const SceneHighlight sh = gloss_shine(all_args);
    const SceneTraceArgs &arg = trace_args(args);
    const SceneBvhArgs &b = arg.b;
    const SceneArgs &a = b.s;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < a.W * a.H) {
        int *const stk = stack + threadIdx.x;
        // the first hit: k_scene_path's statements
        SceneRay r;
        scene_ray(a, p % a.W, p / a.W, r.o, r.d);
        const float d0[3] = { r.d[0], r.d[1], r.d[2] };
        SceneHit h;
        scene_primitives(a, r.o, r.d, h);
        trace_aim(r);
        int best = -1;
        float bt = h.t_best, bbx = 0.0f, bby = 0.0f;
        scene_nearest(b, r, stk, 0.0f, bt, best, bbx, bby);
        float pos[3];
        scene_surface(a, r.o, r.d, h, best, bt, bbx, bby, pos);

        float shade[3] = { h.emit, h.emit, h.emit };
        float first_term = h.emit, ind_term[3] = { 0.0f, 0.0f, 0.0f };
        float first3[3] = { h.emit, h.emit, h.emit };       // SHINE only: the first term per channel, the highlight in it
        bool bounced = false;
        // what the guide leaves: chain (0: none ran), and for chain > 0 the virtual hit's normal, id and unfolded position
        int chain = 0, vgid = 0;
        float vn[3] = { 0.0f, 0.0f, 0.0f }, vpos[3] = { 0.0f, 0.0f, 0.0f };
        if (!(h.emit > 0.0f)) {
            const bool casts = h.gid >= 0;
            // the diffuse share of the first hit's surface weighs the first term; a share of 0 casts no shadow ray
            const SvgfSurface S0 = gloss_surface(args.table, args.n_table, h.gid);
            const float w_d = (S0.refract > 0.0f && best < 0) ? 0.0f : 1.0f - S0.reflect;
            float first = 0.0f;
            // SHINE: a first hit that is rough for the highlight gathers the light through the very shadow samples of the first term
            bool lit0 = w_d != 0.0f, shine0 = false;
            float alpha0 = 0.0f, hsum = 0.0f;
            if constexpr (SHINE) {
                if (sh.enable != 0 && casts && !(S0.refract > 0.0f && best < 0) && S0.reflect > 0.0f) {
                    if (h.gid < rg.n) alpha0 = rg.alpha[h.gid];
                    const float v_n = (-d0[0] * h.n[0] + -d0[1] * h.n[1]) + -d0[2] * h.n[2];
                    shine0 = alpha0 > 0.0f && v_n > 0.0f;
                }
                lit0 = lit0 || shine0;
            }
            if (lit0) {
                int unoccluded = arg.samples;
                if (casts) {
                    unoccluded = 0;
                    for (int c = 0; c < 3; c++) r.o[c] = pos[c];
                    for (int s = 0; s < arg.samples; s++) {
                        if constexpr (SHINE) { r.d[0] = 0.0f; r.d[1] = 0.0f; r.d[2] = 0.0f; }      // a sample that forms no ray leaves them
                        const bool occluded = scene_shadow_sample(b, arg.edge_u, arg.edge_v, r, pos, stk, p, 8 + 2 * s, 9 + 2 * s);
                        unoccluded += occluded ? 0 : 1;
                        if constexpr (SHINE) {
                            if (shine0 && !occluded && (r.d[0] != 0.0f || r.d[1] != 0.0f || r.d[2] != 0.0f))
                                hsum = hsum + shine_factor(a, alpha0, sh.clamp, d0, h.n, pos, r.d);
                        }
                    }
                }
                if (!SHINE || w_d != 0.0f) {
                    const float vis = (float)unoccluded / (float)arg.samples;
                    first = w_d * (arg.ambient + vis * scene_direct(a, h.n, pos));
                }
            }
            shade[0] = first; shade[1] = first; shade[2] = first;
            first_term = first;
            if constexpr (SHINE) {
                const float hm = hsum / (float)arg.samples;
                for (int c = 0; c < 3; c++) {
                    first3[c] = shine0 ? first + (S0.reflect * S0.spec[c]) * hm : first;
                    shade[c] = first3[c];
                }
            }
            const int paths = arg.bounce_samples;
            // the guide's turn j == paths, where the first hit is a hit whose diffuse share is 0
            const int turns = (GUIDE && casts && w_d == 0.0f) ? paths + 1 : paths;
            if (casts && turns > 0) {
                float ind[3] = { 0.0f, 0.0f, 0.0f };
                for (int j = 0; j < turns; j++) {
                    const bool guide = GUIDE && j == paths;
                    float thr[3] = { 1.0f, 1.0f, 1.0f }, acc[3] = { 0.0f, 0.0f, 0.0f };
                    float x[3] = { pos[0], pos[1], pos[2] }, n[3] = { h.n[0], h.n[1], h.n[2] }, alb[3] = { h.alb[0], h.alb[1], h.alb[2] };
                    float d[3] = { d0[0], d0[1], d0[2] };
                    int gid = h.gid;
                    bool triangle = best >= 0, inside = false;
                    float L = h.t_best;                 // the guide's: the length of the chain so far
                    // cb: the class stream of vertex v.  Behind the first hit f19's base is cb - 11: the shadow ray of the vertex reads
                    // cb - 3 and cb - 2, its roulette cb - 1; the direction sampled AT vertex v reads cb + 117 + 0..7 (f19's next base)
                    unsigned cb = 139u + 16u * (unsigned)j;
                    for (int v = 0; ; v++, cb += 128u) {
                        // vertex v: a hit that is no emitter
                        const SvgfSurface S = gloss_surface(args.table, args.n_table, gid);
                        float dn[3] = { 0.0f, 0.0f, 0.0f }, wgt[3], nn[3] = { 0.0f, 0.0f, 0.0f };
                        bool moved;
                        // the guide reads no stream: glass transmits (u = 1), a full mirror reflects (u = 0), a partial one does not (u = 1)
                        float u = guide ? ((!(S.refract > 0.0f && !triangle) && S.reflect >= 1.0f) ? 0.0f : 1.0f)
                                        : scene_hash(a.seed, a.frame, (unsigned)p, cb);
                        // the roughness of the vertex; the guide does not follow a mirror rougher than guide_alpha
                        float alpha = 0.0f;
                        if constexpr (ROUGH) {
                            if (gid >= 0 && gid < rg.n) alpha = rg.alpha[gid];
                            if (guide && alpha > rg.guide_alpha) u = 1.0f;
                        }
                        const bool specular = gloss_vertex(S, triangle, d, n, u, inside, dn, wgt, nn, moved);
                        if constexpr (SHINE) {
                            // The highlight's kernels: the rough vertex, and the gather of a vertex behind the first hit - a diffuse one
                            // as below, a ROUGH one the light's GGX term - through ONE shadow sample on the streams of the vertex.
                            // A block of its own, so that the other kernels compile the text they compiled before it existed.  The gather
                            // comes AHEAD of the lobe's sample, whose direction and weight it does not need: an absorbed vertex has
                            // gathered, and dn and wgt are not live across the shadow walk (behind it the plain kernel kept 52 B of scratch).
                            const bool lobe = !guide && specular && alpha > 0.0f && !(S.refract > 0.0f && !triangle);
                            bool shines = false;
                            if (lobe && sh.enable != 0 && v >= 1) shines = ((-d[0] * n[0] + -d[1] * n[1]) + -d[2] * n[2]) > 0.0f;     // rough_vertex's v_n
                            if (!guide && v >= 1 && (!specular || shines)) {
                                bool occluded = false, formed = true;
                                if (arg.shadow_secondary) {
                                    for (int c = 0; c < 3; c++) { r.o[c] = x[c]; r.d[c] = 0.0f; }      // a sample that forms no ray leaves d
                                    occluded = scene_shadow_sample(b, arg.edge_u, arg.edge_v, r, x, stk, p, cb - 3u, cb - 2u);
                                    formed = r.d[0] != 0.0f || r.d[1] != 0.0f || r.d[2] != 0.0f;
                                } else if (shines) {                    // no ray is cast: the direction of the light's centre
                                    for (int c = 0; c < 3; c++) r.d[c] = a.light[c] - x[c];
                                    normalise3(r.d);
                                }
                                if (shines) {
                                    const float Hc = (formed && !occluded) ? shine_factor(a, alpha, sh.clamp, d, n, x, r.d) : 0.0f;
                                    for (int c = 0; c < 3; c++) acc[c] = acc[c] + thr[c] * (alb[c] * (S.spec[c] * Hc));
                                } else {
                                    const float Ld = arg.ambient + (occluded ? 0.0f : 1.0f) * scene_direct(a, n, x);
                                    for (int c = 0; c < 3; c++) acc[c] = acc[c] + thr[c] * (alb[c] * Ld);
                                }
                            }
                            if (lobe) {
                                bool absorbed;
                                rough_vertex(a, p, cb + 117u, alpha, d, n, dn, wgt, absorbed);
                                if (absorbed) break;
                            }
                        } else if constexpr (ROUGH) {
                            // a mirror vertex (not glass) of a rough object: the lobe's direction and weight in the smooth mirror's place
                            if (!guide && specular && alpha > 0.0f && !(S.refract > 0.0f && !triangle)) {
                                bool absorbed;
                                rough_vertex(a, p, cb + 117u, alpha, d, n, dn, wgt, absorbed);
                                if (absorbed) break;
                            }
                        }
                        if (guide) {
                            if (!specular) { chain = v; break; }                    // the virtual hit
                            if (v == gd.max_chain) { chain = -v; break; }           // the cap
                        } else if (v >= 1) {
                            if constexpr (!SHINE) {
                                if (!specular) {
                                    bool occluded = false;
                                    if (arg.shadow_secondary) {
                                        for (int c = 0; c < 3; c++) r.o[c] = x[c];
                                        occluded = scene_shadow_sample(b, arg.edge_u, arg.edge_v, r, x, stk, p, cb - 3u, cb - 2u);
                                    }
                                    const float Ld = arg.ambient + (occluded ? 0.0f : 1.0f) * scene_direct(a, n, x);
                                    for (int c = 0; c < 3; c++) acc[c] = acc[c] + thr[c] * (alb[c] * Ld);
                                }
                            }
                            if (v >= args.max_depth) break;
                            for (int c = 0; c < 3; c++) thr[c] = thr[c] * (alb[c] * wgt[c]);
                            if (args.rr_depth > 0 && v >= args.rr_depth) {
                                const float rq = fminf(fmaxf(fmaxf(thr[0], thr[1]), thr[2]), 1.0f);
                                if (!(rq > 0.0f && scene_hash(a.seed, a.frame, (unsigned)p, cb - 1u) < rq)) break;
                                for (int c = 0; c < 3; c++) thr[c] = thr[c] / rq;
                            }
                        } else {
                            for (int c = 0; c < 3; c++) thr[c] = wgt[c];        // the store applies the first hit's albedo
                        }
                        // the ray that leaves vertex v
                        const float t_lo = 0x1p-10f * fmaxf(1.0f, fmaxf(fmaxf(fabsf(x[0]), fabsf(x[1])), fabsf(x[2])));
                        if (specular) {
                            const float back = -(4.0f * t_lo);
                            for (int c = 0; c < 3; c++) { r.o[c] = moved ? x[c] + back * nn[c] : x[c]; r.d[c] = dn[c]; }
                        } else {
                            const float s = copysignf(1.0f, n[2]), q = -1.0f / (s + n[2]), w = (n[0] * n[1]) * q;
                            const float T[3] = { 1.0f + ((s * n[0]) * n[0]) * q, s * w, -(s * n[0]) };
                            const float B[3] = { w, s + (n[1] * n[1]) * q, -n[1] };
                            for (int c = 0; c < 3; c++) r.o[c] = x[c];
                            trace_direction(a, p, cb + 117u, n, T, B, r.d);
                        }
                        for (int c = 0; c < 3; c++) d[c] = r.d[c];
                        trace_aim(r);
                        SceneHit h2;
                        scene_primitives_beyond(a, r.o, r.d, t_lo, h2);
                        int best2 = -1;
                        float bt2 = h2.t_best, bbx2 = 0.0f, bby2 = 0.0f;
                        scene_nearest(b, r, stk, t_lo, bt2, best2, bbx2, bby2);
                        scene_surface(a, r.o, r.d, h2, best2, bt2, bbx2, bby2, x);
                        if (h2.gid < 0) {                       // a miss
                            if (guide) chain = -(v + 1);
                            break;
                        }
                        if (guide) L = L + h2.t_best;
                        if (h2.emit > 0.0f) {                   // an emitter, before its surface is looked at
                            if (guide) {
                                chain = v + 1;
                                for (int c = 0; c < 3; c++) n[c] = h2.n[c];
                                gid = h2.gid;
                            } else {
                                for (int c = 0; c < 3; c++) acc[c] = acc[c] + thr[c] * (h2.alb[c] * h2.emit);
                            }
                            break;
                        }
                        for (int c = 0; c < 3; c++) { n[c] = h2.n[c]; alb[c] = h2.alb[c]; }
                        gid = h2.gid;
                        triangle = best2 >= 0;
                    }
                    if (guide) {
                        // the path unfolded along the primary ray: a planar mirror's image of the seen point (include/svgf_virtual.h)
                        for (int c = 0; c < 3; c++) { vn[c] = n[c]; vpos[c] = a.o[c] + L * d0[c]; }
                        vgid = gid + gd.id_offset;
                    } else {
                        for (int c = 0; c < 3; c++) ind[c] = ind[c] + acc[c];
                    }
                }
                if (!GUIDE || paths > 0) {
                    for (int c = 0; c < 3; c++) { ind_term[c] = ind[c] / (float)paths; shade[c] = (SHINE ? first3[c] : first) + ind_term[c]; }
                    bounced = true;
                }
            }
        }
        if constexpr (GUIDE) {
            // the store tails unchanged: a hit whose n and gid are the virtual ones (albedo and emittance stay the first hit's)
            if (chain > 0) {
                for (int c = 0; c < 3; c++) { h.n[c] = vn[c]; pos[c] = vpos[c]; }
                h.gid = vgid;
            }
            if (gd.out_chain) gd.out_chain[p] = chain;
        }
        if constexpr (SPLIT && SHINE) trace_store_split3(args.s, p, h, pos, first3, ind_term, bounced, shade);
        else if constexpr (SPLIT) trace_store_split(args.s, p, h, pos, first_term, ind_term, bounced, shade);
        else scene_store(a, p, h, pos, shade[0], shade[1], shade[2]);
    }
}

// Every refusal of svgf_gloss_draw that needs no device, in its order, and the kernel's arguments: what svgf_virtual_draw repeats first
static inline int gloss_draw_args(SceneGlossArgs &t, int &device, const svgf_scene *scene, const svgf_gloss_table *table, void *out_rgb_dev,
                                  void *out_gbuffer_dev, const SvgfPlanarGBuffer *planes, int width, int height, const SvgfCamera *cam,
                                  const SvgfSynthParams *sp, const SvgfSceneLight *light, const SvgfPathParams *pp)
{
    const int rc = path_prepare(t.t, device, scene, out_rgb_dev, true, out_gbuffer_dev, planes, width, height, cam, sp, light, pp);
    if (rc != SVGF_OK) return rc;
    if (!path_params_ok(pp)) return SVGF_ERR_INVALID_ARG;
    if (table && table->device != device) return SVGF_ERR_INVALID_ARG;
    t.t.bounce_samples = pp->paths; t.max_depth = pp->max_depth; t.rr_depth = pp->rr_depth;
    t.table = table ? table->dev : nullptr; t.n_table = table ? table->n : 0;
    return SVGF_OK;
}

// the same for svgf_gloss_draw_split
static inline int gloss_draw_split_args(SceneGlossSplitArgs &s, int &device, const svgf_scene *scene, const svgf_gloss_table *table,
                                        void *out_direct_dev, void *out_indirect_dev, void *out_rgb_dev, void *out_gbuffer_dev,
                                        const SvgfPlanarGBuffer *planes, int width, int height, const SvgfCamera *cam, const SvgfSynthParams *sp,
                                        const SvgfSceneLight *light, const SvgfPathParams *pp)
{
    const int rc = path_prepare(s.s.t, device, scene, out_rgb_dev, false, out_gbuffer_dev, planes, width, height, cam, sp, light, pp);
    if (rc != SVGF_OK) return rc;
    if (!out_direct_dev || !out_indirect_dev || out_direct_dev == out_indirect_dev) return SVGF_ERR_INVALID_ARG;
    if (!path_params_ok(pp)) return SVGF_ERR_INVALID_ARG;
    if (table && table->device != device) return SVGF_ERR_INVALID_ARG;
    s.s.out_direct = static_cast<float *>(out_direct_dev); s.s.out_indirect = static_cast<float *>(out_indirect_dev);
    s.s.t.bounce_samples = pp->paths; s.max_depth = pp->max_depth; s.rr_depth = pp->rr_depth;
    s.table = table ? table->dev : nullptr; s.n_table = table ? table->n : 0;
    return SVGF_OK;
}

// What the draws behind svgf_gloss_draw add to its refusals, in their order - vp's, then rp's and the roughness table's device, then
// hp's - each with the kernel arguments it fills; compiled where the includer knows the header that declares the parameters.
#ifdef SVGF_VIRTUAL_H_
static inline int guide_args(SceneGuide &v, const SvgfVirtualParams *vp, void *out_chain_dev)
{
    if (!vp || vp->max_chain < 1 || vp->max_chain > SVGF_PATH_MAX_DEPTH || vp->id_offset < 0 || vp->id_offset > (1 << 24)) return SVGF_ERR_INVALID_ARG;
    v = SceneGuide{ vp->max_chain, vp->id_offset, static_cast<int *>(out_chain_dev) };
    return SVGF_OK;
}
#endif

#ifdef SVGF_ROUGH_TABLE_H_
static inline int rough_args(SceneRough &r, const SvgfRoughParams *rp, const svgf_rough_table *rough, int device)
{
    if (!rp || !std::isfinite(rp->guide_alpha) || rp->guide_alpha < 0.0f) return SVGF_ERR_INVALID_ARG;
    if (rough && rough->device != device) return SVGF_ERR_INVALID_ARG;
    r = SceneRough{ rough ? rough->dev : nullptr, rough ? rough->n : 0, rp->guide_alpha };
    return SVGF_OK;
}
#endif

#ifdef SVGF_HIGHLIGHT_H_
static inline int shine_args(SceneHighlight &h, const SvgfHighlightParams *hp)
{
    if (!hp || hp->enable < 0 || hp->enable > 1 || !std::isfinite(hp->clamp) || hp->clamp < 0.0f) return SVGF_ERR_INVALID_ARG;
    h = SceneHighlight{ hp->enable, hp->clamp };
    return SVGF_OK;
}
#endif

// The end of every draw of this text: the refusals' answer `rc`, else the device guard and one launch of k_scene_gloss<Args> on `stream`
template <class Args>
static inline int gloss_launch(int rc, const Args &args, int device, int width, int height, void *stream)
{
    if (rc != SVGF_OK) return rc;
    SvgfDeviceGuard dev_guard(device);
    if (!dev_guard.ok) return SVGF_ERR_NO_DEVICE;
    const int n = width * height;
    hipLaunchKernelGGL(k_scene_gloss<Args>, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), args);
    return hipGetLastError() == hipSuccess ? SVGF_OK : SVGF_ERR_HIP;
}
