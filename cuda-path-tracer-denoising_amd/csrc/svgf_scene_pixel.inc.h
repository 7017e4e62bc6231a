// svgf_scene_pixel.inc.h — the per-pixel body of the scene producer, shared as TEXT by its kernels (as svgf_temporal_pixel.inc.h
// is by the temporal kernels): k_scene_frame (svgf_scene.hip: every triangle for every pixel), k_scene_bvh (svgf_scene_bvh.hip:
// the resident scene's BVH walk, and in its shadowed form the shadow rays of row f16, which reuse the per-primitive test and the
// triangle test) and k_scene_trace (svgf_scene_trace.hip, the companion library of row f17: the same again for the bounce, and the
// tail with a shade per channel).  The ray, the primitives loop, the triangle test and everything behind the choice of the nearest
// triangle (corner weights, texture, shading, noise, the AoS / planar stores) live here, so both kernels compile the same
// arithmetic; only the loop that offers triangles to scene_tri_test differs.  float32, contraction off in every function.
// Include inside an anonymous namespace, after svgf.h and hip_runtime.h.

struct SceneArgs {
    float right[3], up[3], view[3], o[3];
    float light[3];
    float plx, ply, cx, cy;
    float noise, fireflies, chroma_amp;
    int W, H, frame, seed, n_geoms;
    const SvgfSceneGeom *geoms;
    const int *geom_ids;       // object index written as geomId for primitive k (null: k itself)
    int n_tris;                // world-space triangles of the scene's meshes (Scene::loadMesh, src/scene.cpp:234-311)
    const float *tris;         // n_tris x 3 vertices x {pos3, normal3, uv2}
    const int *tri_ids;        // object index of each triangle's mesh
    const float *tri_albedo;   // n_tris x rgb (the mesh's material colour)
    const int *tri_tex;        // texture index per triangle, -1 = untextured (null: no textures)
    const int *tex_desc;       // per texture {byte offset into tex, width, height}, 8-bit RGB rows top to bottom
    const unsigned char *tex;
    float *out_rgb;
    float *out_gbuf;           // AoS texels, or null: the planes below (svgf_planar_gbuffer)
    float *pl_nrm, *pl_pos, *pl_alb;
    int *pl_gid;
};

// what the primitives loop leaves and the triangle part may overwrite
struct SceneHit {
    float t_best;
    int gid;
    float n[3], ph[3], alb[3];
    float emit;
};

__device__ __forceinline__ float scene_hash(unsigned seed, unsigned frame, unsigned p, unsigned k)
{   // synth.py: hash_uniform
    unsigned x = p * 0x9E3779B1u + k * 0x85EBCA77u + frame * 0xC2B2AE3Du + seed * 0x27D4EB2Fu;
    x ^= x >> 15; x *= 0x2C1B3C6Du; x ^= x >> 12; x *= 0x297A2D39u; x ^= x >> 15;
    return (float)(x >> 8) * (1.0f / 16777216.0f);
}

#pragma clang fp contract(off)
__device__ __forceinline__ void apply34(const float *m, const float v[3], float w, float out[3])
{   // 3x4 row-major times (v, w): ((m0*v0 + m1*v1) + m2*v2) + m3*w
#pragma clang fp contract(off)
    for (int r = 0; r < 3; r++) out[r] = ((m[4 * r] * v[0] + m[4 * r + 1] * v[1]) + m[4 * r + 2] * v[2]) + m[4 * r + 3] * w;
}

__device__ __forceinline__ void normalise3(float v[3])
{
#pragma clang fp contract(off)
    const float l = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    v[0] = v[0] / l; v[1] = v[1] / l; v[2] = v[2] / l;
}

// the primary ray of pixel (x, y)
__device__ __forceinline__ void scene_ray(const SceneArgs &a, int x, int y, float o[3], float d[3])
{
#pragma clang fp contract(off)
    const float sx = a.plx * ((float)x - a.cx), sy = a.ply * ((float)y - a.cy);
    for (int c = 0; c < 3; c++) d[c] = (a.view[c] - a.right[c] * sx) - a.up[c] * sy;
    normalise3(d);
    o[0] = a.o[0]; o[1] = a.o[1]; o[2] = a.o[2];
}

// One primitive against the ray (o, d): the cube / sphere test of the reference, the world-space normal nw and point pw of the hit
// it reports, and tw, its distance from o measured in world space.  The text both users compile: scene_primitives (the nearest hit)
// and the shadow rays of svgf_scene_draw_shadowed (any hit inside an interval; nw and pw unused there).
__device__ __forceinline__ void scene_primitive_test(const SvgfSceneGeom &g, const float o[3], const float d[3], bool &hit, float &tw,
                                                     float nw[3], float pw[3])
{
#pragma clang fp contract(off)
    float qo[3], qd[3];
    apply34(g.inv, o, 1.0f, qo);
    apply34(g.inv, d, 0.0f, qd);
    normalise3(qd);
    float tt;
    if (g.type == 0) {      // unit cube: slab test, entering face (or leaving face when the origin is inside)
        float tmin = -1e38f, tmax = 1e38f;
        int amin = 0, amax = 0;
        for (int ax = 0; ax < 3; ax++) {
            const float t1 = (-0.5f - qo[ax]) / qd[ax], t2 = (0.5f - qo[ax]) / qd[ax];
            // glm::min / glm::max (src/intersections.h:65-66) as the reference's GLM defines them, x < y ? x : y and x > y ? x : y:
            // a NaN on either side (a ray in the plane of a face: 0/0) gives t2, where fminf / fmaxf give the other operand
            const float ta = t1 < t2 ? t1 : t2, tb = t1 > t2 ? t1 : t2;
            if (ta > 0.0f && ta > tmin) { tmin = ta; amin = ax; }
            if (tb < tmax) { tmax = tb; amax = ax; }
        }
        hit = (tmax >= tmin) && (tmax > 0.0f);
        const bool inside = tmin <= 0.0f;
        tt = inside ? tmax : tmin;
        const int axis = inside ? amax : amin;
        const float sgn = (qd[axis] < 0.0f) ? 1.0f : -1.0f;             // the face normal that looks at the ray
        const float no[3] = { axis == 0 ? sgn : 0.0f, axis == 1 ? sgn : 0.0f, axis == 2 ? sgn : 0.0f };
        apply34(g.xf, no, 0.0f, nw);
        normalise3(nw);
    } else {                // unit sphere, radius 0.5
        const float b = (qo[0] * qd[0] + qo[1] * qd[1]) + qo[2] * qd[2];
        const float rad = b * b - (((qo[0] * qo[0] + qo[1] * qo[1]) + qo[2] * qo[2]) - 0.25f);
        const float sq = sqrtf(fmaxf(rad, 0.0f));
        const float ta = -b + sq, tb = -b - sq;
        const bool both_pos = (ta > 0.0f) && (tb > 0.0f), both_neg = (ta < 0.0f) && (tb < 0.0f);
        tt = both_pos ? fminf(ta, tb) : fmaxf(ta, tb);
        hit = (rad >= 0.0f) && !both_neg;
        const float po[3] = { qo[0] + tt * qd[0], qo[1] + tt * qd[1], qo[2] + tt * qd[2] };
        for (int r = 0; r < 3; r++) nw[r] = (g.invT[3 * r] * po[0] + g.invT[3 * r + 1] * po[1]) + g.invT[3 * r + 2] * po[2];
        normalise3(nw);
    }
    const float po[3] = { qo[0] + tt * qd[0], qo[1] + tt * qd[1], qo[2] + tt * qd[2] };
    apply34(g.xf, po, 1.0f, pw);
    const float dv0 = o[0] - pw[0], dv1 = o[1] - pw[1], dv2 = o[2] - pw[2];
    tw = sqrtf((dv0 * dv0 + dv1 * dv1) + dv2 * dv2);                    // t is measured in world space
}

// nearest hit among the primitives beyond t_min (the primary ray: 1e-4, scene_primitives below)
__device__ __forceinline__ void scene_primitives_beyond(const SceneArgs &a, const float o[3], const float d[3], float t_min, SceneHit &h)
{
#pragma clang fp contract(off)
    h.t_best = __builtin_huge_valf();
    h.gid = -1;
    for (int c = 0; c < 3; c++) { h.n[c] = 0.0f; h.ph[c] = 0.0f; h.alb[c] = 0.0f; }
    h.emit = 0.0f;
    for (int k = 0; k < a.n_geoms; k++) {
        const SvgfSceneGeom &g = a.geoms[k];
        bool hit;
        float tw, nw[3], pw[3];
        scene_primitive_test(g, o, d, hit, tw, nw, pw);
        if (hit && (tw > t_min) && (tw < h.t_best)) {
            h.t_best = tw; h.gid = a.geom_ids ? a.geom_ids[k] : k;
            h.n[0] = nw[0]; h.n[1] = nw[1]; h.n[2] = nw[2];
            h.ph[0] = pw[0]; h.ph[1] = pw[1]; h.ph[2] = pw[2];
            h.alb[0] = g.albedo[0]; h.alb[1] = g.albedo[1]; h.alb[2] = g.albedo[2]; h.emit = g.emittance;
        }
    }
}

__device__ __forceinline__ void scene_primitives(const SceneArgs &a, const float o[3], const float d[3], SceneHit &h)
{
    scene_primitives_beyond(a, o, d, 1e-4f, h);
}

// glm::intersectRayTriangle (gtx/intersect.inl:37-74) on triangle T (24 floats): false where the reference's test leaves early,
// otherwise the barycentrics and t (which may still be <= 0: the caller's comparison rejects that)
__device__ __forceinline__ bool scene_tri_test(const float *T, const float o[3], const float d[3], float &bx, float &by, float &t)
{
#pragma clang fp contract(off)
    const float e1[3] = { T[8] - T[0], T[9] - T[1], T[10] - T[2] }, e2[3] = { T[16] - T[0], T[17] - T[1], T[18] - T[2] };
    const float pv[3] = { d[1] * e2[2] - e2[1] * d[2], d[2] * e2[0] - e2[2] * d[0], d[0] * e2[1] - e2[0] * d[1] };
    const float det = (e1[0] * pv[0] + e1[1] * pv[1]) + e1[2] * pv[2];
    if (det < 1.1920929e-7f) return false;
    const float f = 1.0f / det;
    const float sv[3] = { o[0] - T[0], o[1] - T[1], o[2] - T[2] };
    bx = f * ((sv[0] * pv[0] + sv[1] * pv[1]) + sv[2] * pv[2]);
    if (bx < 0.0f || bx > 1.0f) return false;
    const float q[3] = { sv[1] * e1[2] - e1[1] * sv[2], sv[2] * e1[0] - e1[2] * sv[0], sv[0] * e1[1] - e1[0] * sv[1] };
    by = f * ((d[0] * q[0] + d[1] * q[1]) + d[2] * q[2]);
    if (by < 0.0f || by + bx > 1.0f) return false;
    t = f * ((e2[0] * q[0] + e2[1] * q[1]) + e2[2] * q[2]);
    return true;
}

// The tail: the nearest triangle `best` (-1: none nearer than the primitives) at distance bt with barycentrics (bbx, bby) replaces
// the primitives' hit; then the miss position, shading, noise and the AoS / planar stores of pixel p.
// normal = n0 * b.x + n1 * b.y + n2 * (1 - b.x - b.y) normalised (Triangle::Intersect, src/sceneStructs.h:168-172, sic)
// It comes in two halves so that svgf_scene_draw_shadowed can cast its shadow rays from `pos` in between: scene_surface settles
// the hit and the position, scene_shade<SHADOWED> does the rest, with the light's term scaled by `vis` in the shadowed form only
// (the unshadowed instantiation compiles the statement it always did).  scene_shade is itself scene_direct (the light's term) and
// scene_store (noise, fireflies, chroma, stores), which the path-traced draw calls with a shade of its own.
__device__ __forceinline__ void scene_surface(const SceneArgs &a, const float o[3], const float d[3], SceneHit &h, int best, float bt,
                                              float bbx, float bby, float pos[3])
{
#pragma clang fp contract(off)
    if (best >= 0) {
        const float *T = a.tris + 24 * (size_t)best;
        const float w2 = 1.0f - bbx - bby;
        for (int c = 0; c < 3; c++) {
            h.n[c] = (T[3 + c] * bbx + T[11 + c] * bby) + T[19 + c] * w2;
            h.ph[c] = o[c] + bt * d[c];
            h.alb[c] = a.tri_albedo[3 * (size_t)best + c];
        }
        normalise3(h.n);
        const int tx = a.tri_tex ? a.tri_tex[best] : -1;
        if (tx >= 0) {      // Texture::getColor (src/sceneStructs.h:208-219) at the interpolated uv (Triangle::Intersect :162-164)
            const float u = (T[6] * w2 + T[14] * bbx) + T[22] * bby, v = (T[7] * w2 + T[15] * bbx) + T[23] * bby;
            const int tw = a.tex_desc[3 * tx + 1], th = a.tex_desc[3 * tx + 2];
            int X = (int)fminf(1.0f * (float)tw * u, 1.0f * (float)tw - 1.0f), Y = (int)fminf(1.0f * (float)th * (1.0f - v), 1.0f * (float)th - 1.0f);
            X = X < 0 ? 0 : X; Y = Y < 0 ? 0 : Y;                          // (the reference indexes out of bounds here)
            const unsigned char *px = a.tex + a.tex_desc[3 * tx] + 3 * ((size_t)Y * tw + X);
            for (int c = 0; c < 3; c++) h.alb[c] = 0.003921568627f * (float)px[c];
        }
        h.emit = 0.0f;
        h.gid = a.tri_ids[best];
        h.t_best = bt;
    }
    const bool miss = h.gid < 0;
    for (int c = 0; c < 3; c++) pos[c] = miss ? (o[c] + -1.0f * d[c]) : h.ph[c];    // t = -1 on a miss (src/pathtrace.cu:318)
}

// the light's term at `pos` with normal n, towards a.light: (30 lam) / (4 + dist2)
__device__ __forceinline__ float scene_direct(const SceneArgs &a, const float n[3], const float pos[3])
{
#pragma clang fp contract(off)
    float tl[3];
    for (int c = 0; c < 3; c++) tl[c] = a.light[c] - pos[c];
    const float dist2 = (tl[0] * tl[0] + tl[1] * tl[1]) + tl[2] * tl[2];
    const float dl = sqrtf(dist2);
    const float lam = fmaxf(((tl[0] / dl) * n[0] + (tl[1] / dl) * n[1]) + (tl[2] / dl) * n[2], 0.0f);
    return (30.0f * lam) / (4.0f + dist2);
}

// noise, fireflies, chroma and the AoS / planar stores of pixel p, whose surface is shaded `shade` per channel
__device__ __forceinline__ void scene_store(const SceneArgs &a, int p, const SceneHit &h, const float pos[3], float shade_r, float shade_g, float shade_b)
{
#pragma clang fp contract(off)
    const float *n = h.n, *alb = h.alb;
    const int gid = h.gid;
    const bool miss = gid < 0;
    const float shade[3] = { shade_r, shade_g, shade_b };

    const unsigned up = (unsigned)p;
    const float u = scene_hash(a.seed, a.frame, up, 0), v = scene_hash(a.seed, a.frame, up, 1);
    float mult = 1.0f + a.noise * (2.0f * u - 1.0f);
    if (v < a.fireflies) mult = mult * 6.0f;
    float col[3];
    for (int c = 0; c < 3; c++) {
        const float chroma = 1.0f + a.chroma_amp * (scene_hash(a.seed, a.frame, up, 2 + c) - 0.5f);
        col[c] = miss ? 0.0f : ((alb[c] * shade[c]) * mult) * chroma;
    }
    float *o_rgb = a.out_rgb + 3 * (size_t)p;
    o_rgb[0] = col[0]; o_rgb[1] = col[1]; o_rgb[2] = col[2];
    if (!a.out_gbuf) {        // planar: the denoiser's own current-frame planes; albedo * ialbedo with ialbedo == 1
        a.pl_nrm[3 * (size_t)p] = n[0]; a.pl_nrm[3 * (size_t)p + 1] = n[1]; a.pl_nrm[3 * (size_t)p + 2] = n[2];
        a.pl_pos[3 * (size_t)p] = pos[0]; a.pl_pos[3 * (size_t)p + 1] = pos[1]; a.pl_pos[3 * (size_t)p + 2] = pos[2];
        if (a.pl_alb) { a.pl_alb[3 * (size_t)p] = alb[0]; a.pl_alb[3 * (size_t)p + 1] = alb[1]; a.pl_alb[3 * (size_t)p + 2] = alb[2]; }
        a.pl_gid[p] = gid;
        return;
    }
    float *g = a.out_gbuf + 13 * (size_t)p;
    g[0] = n[0]; g[1] = n[1]; g[2] = n[2];
    g[3] = pos[0]; g[4] = pos[1]; g[5] = pos[2];
    g[6] = alb[0]; g[7] = alb[1]; g[8] = alb[2];
    g[9] = 1.0f; g[10] = 1.0f; g[11] = 1.0f;
    reinterpret_cast<int *>(g)[12] = gid;
}

template <bool SHADOWED>
__device__ __forceinline__ void scene_shade(const SceneArgs &a, int p, const SceneHit &h, const float pos[3], float vis)
{
#pragma clang fp contract(off)
    const float direct = scene_direct(a, h.n, pos);
    float shade = SHADOWED ? 0.15f + vis * direct : 0.15f + direct;
    if (h.emit > 0.0f) shade = h.emit;
    scene_store(a, p, h, pos, shade, shade, shade);
}

__device__ __forceinline__ void scene_finish(const SceneArgs &a, int p, const float o[3], const float d[3], SceneHit &h, int best, float bt,
                                             float bbx, float bby)
{
    float pos[3];
    scene_surface(a, o, d, h, best, bt, bbx, bby, pos);
    scene_shade<false>(a, p, h, pos, 1.0f);
}

// ---- host side, shared by svgf_scene_render* and the resident scene ---------------------------------------------------------------------
// The scene arguments of svgf_scene_render_mesh: SVGF_OK and the bytes of tex_data the descriptors reach, or SVGF_ERR_INVALID_ARG.
static inline int scene_check_inputs(const SvgfSceneGeom *geoms, int n_geoms, const float *tris, const int *tri_ids, const float *tri_albedo,
                                     int n_tris, const int *tri_tex, const int *tex_desc, const unsigned char *tex_data, int n_tex,
                                     size_t *n_texbytes_out)
{
    if (n_geoms < 0 || n_geoms > SVGF_SCENE_MAX_GEOMS || (n_geoms > 0 && !geoms)) return SVGF_ERR_INVALID_ARG;
    if (n_tris < 0 || n_tris > SVGF_SCENE_MAX_TRIS || (n_tris > 0 && (!tris || !tri_ids || !tri_albedo))) return SVGF_ERR_INVALID_ARG;
    if (n_tex < 0 || n_tex > 64 || (n_tex > 0 && (!tri_tex || !tex_desc || !tex_data || n_tris == 0))) return SVGF_ERR_INVALID_ARG;
    size_t n_texbytes = 0;              // bytes of tex_data the descriptors reach: that much is copied, not a byte more
    for (int k = 0; k < n_tex; k++) {
        if (tex_desc[3 * k] < 0 || tex_desc[3 * k + 1] <= 0 || tex_desc[3 * k + 2] <= 0) return SVGF_ERR_INVALID_ARG;
        const size_t end = (size_t)tex_desc[3 * k] + (size_t)3 * tex_desc[3 * k + 1] * tex_desc[3 * k + 2];
        if (end > n_texbytes) n_texbytes = end;
    }
    for (int i = 0; i < n_tris && n_tex > 0; i++)      // -1 = untextured; anything else must name one of the n_tex textures
        if (tri_tex[i] < -1 || tri_tex[i] >= n_tex) return SVGF_ERR_INVALID_ARG;
    *n_texbytes_out = n_texbytes;
    return SVGF_OK;
}

// camera, light, noise and frame size of one call
static inline void scene_frame_args(SceneArgs &a, int width, int height, const SvgfCamera *cam, const SvgfSynthParams *sp, const float light[3])
{
    for (int c = 0; c < 3; c++) { a.right[c] = cam->right[c]; a.up[c] = cam->up[c]; a.view[c] = cam->view[c]; a.o[c] = cam->position[c]; a.light[c] = light[c]; }
    a.plx = sp->pixel_length[0]; a.ply = sp->pixel_length[1];
    a.cx = (float)(width * 0.5 - 0.5); a.cy = (float)(height * 0.5 - 0.5);
    a.noise = sp->noise; a.fireflies = sp->fireflies; a.chroma_amp = 0.1f * sp->noise;
    a.W = width; a.H = height; a.frame = sp->frame; a.seed = sp->seed;
}
