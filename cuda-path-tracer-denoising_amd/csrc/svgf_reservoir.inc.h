// svgf_reservoir.inc.h — what a reservoir pass over a G-buffer of the resident scene is apart from its payload: the text svgf_restir.hip
// (row f27) and svgf_restir_gi.hip (row f28) share.  Included inside the anonymous namespace of a .hip behind its scene include
// (svgf_scene_walk.inc.h or svgf_scene_trace.inc.h: SceneArgs, SceneBvhArgs, scene_hash) and behind <cstring>, <new>, <vector>; no
// __global__ in it: each library keeps its three kernels, its argument struct and what a reservoir holds.
//   device  the 64 x 4 tile's pixel, the G-buffer reads, the id's emittance, the history tap's address and the arithmetic of
//           update() on the sums.  An argument struct `Args` has the fields gbuf, pl_nrm, pl_pos, pl_gid, motion, emit, n_ids,
//           prev_n, prev_gid and min_dot.  The neighbour pick and finish() stay in each .hip: as shared functions they moved
//           instructions of the spatial kernels.
//   host    ReservoirState (the fields behind both opaque handles), its create / read / info / destroy, scene_args, tile_grid.
// A later resampler includes this file, derives its handle from ReservoirState and writes its payload, its kernels and its reset.

// ---- device ---------------------------------------------------------------------------------------------------------------------------------
// the pixel of this thread on the 64 x 4 tile, or -1 outside the frame
__device__ __forceinline__ int tile_pixel(const SceneArgs &a, int &x, int &y)
{
    x = 64 * (int)blockIdx.x + ((int)threadIdx.x & 63);
    y = 4 * (int)blockIdx.y + ((int)threadIdx.x >> 6);
    return (x < a.W && y < a.H) ? y * a.W + x : -1;
}

template <class Args>
__device__ __forceinline__ int read_surface(const Args &a, int p, float n[3], float pos[3])
{
    if (a.gbuf) {
        const float *g = a.gbuf + 13 * (size_t)p;
        for (int c = 0; c < 3; c++) { n[c] = g[c]; pos[c] = g[3 + c]; }
        return reinterpret_cast<const int *>(g)[12];
    }
    for (int c = 0; c < 3; c++) { n[c] = a.pl_nrm[3 * (size_t)p + c]; pos[c] = a.pl_pos[3 * (size_t)p + c]; }
    return a.pl_gid[p];
}

template <class Args>
__device__ __forceinline__ void read_normal(const Args &a, int p, float n[3], int &gid)
{
    if (a.gbuf) {
        const float *g = a.gbuf + 13 * (size_t)p;
        for (int c = 0; c < 3; c++) n[c] = g[c];
        gid = reinterpret_cast<const int *>(g)[12];
        return;
    }
    for (int c = 0; c < 3; c++) n[c] = a.pl_nrm[3 * (size_t)p + c];
    gid = a.pl_gid[p];
}

template <class Args>
__device__ __forceinline__ float id_emittance(const Args &a, int gid) { return (gid >= 0 && gid < a.n_ids) ? a.emit[gid] : 0.0f; }

// the history tap of pixel p (id gid, normal n): true, and q the previous pixel its motion vector rounds to, unless that lies outside
// the frame, had another id, or a normal further from n than min_dot
template <class Args>
__device__ __forceinline__ bool history_tap(const Args &arg, const SceneArgs &a, int p, int gid, const float n[3], int &q)
{
#pragma clang fp contract(off)
    const float fx = floorf(arg.motion[2 * (size_t)p] + 0.5f), fy = floorf(arg.motion[2 * (size_t)p + 1] + 0.5f);
    if (fx >= 0.0f && fx < (float)a.W && fy >= 0.0f && fy < (float)a.H) {
        q = (int)fy * a.W + (int)fx;
        if (arg.prev_gid[q] == gid) {
            const float *m = arg.prev_n + 3 * (size_t)q;
            if ((n[0] * m[0] + n[1] * m[1]) + n[2] * m[2] >= arg.min_dot) return true;
        }
    }
    return false;
}

// update() on the sums: a sample of weight w that stands for M_s candidates enters; true where it is selected
__device__ __forceinline__ bool reservoir_add(float &w_sum, float &M, float w, float M_s, float xi)
{
#pragma clang fp contract(off)
    w = w > 0.0f ? w : 0.0f;
    const float before = w_sum;
    w_sum = w_sum + w;
    M = M + M_s;
    return w > 0.0f && (before == 0.0f || xi * w_sum < w);
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------------
constexpr int RESERVOIR_MAX_ID = (1 << 20) - 1;         // SVGF_RESTIR_MAX_ID and SVGF_RESTIR_GI_MAX_ID, asserted where they are known

// what both opaque handles are: one frame size over one resident scene, one allocation
struct ReservoirState {
    const svgf_scene *scene;
    int device, width, height, n_ids;
    unsigned long long reservoir_bytes;    // of one record: 32 (row f27) or 64 (row f28)
    char *dev;                  // the one allocation
    unsigned long long bytes;
    float4 *H, *T;
    float *prev_n;
    int *prev_gid;
    float *emit;
};

constexpr size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

dim3 tile_grid(int width, int height) { return dim3((unsigned)((width + 63) / 64), (unsigned)((height + 3) / 4)); }

// the scene's part of the kernel arguments, from the view of the moment
int scene_args(SceneBvhArgs &b, const svgf_scene *scene, int &device)
{
    SvgfSceneView v;
    if (!scene || svgf_scene_view(scene, &v) != SVGF_OK) return SVGF_ERR_INVALID_ARG;
    if (v.depth > SVGF_SCENE_MAX_DEPTH) return SVGF_ERR_UNSUPPORTED;        // the kernels' stack; svgf_scene_adopt_tree never lets it
    device = v.device;
    SceneArgs &a = b.s;
    a.n_geoms = v.n_geoms; a.geoms = v.geoms; a.geom_ids = v.geom_ids;
    a.n_tris = v.n_tris; a.tris = v.tris; a.tri_ids = v.tri_ids; a.tri_albedo = v.tri_albedo;
    a.tri_tex = v.tri_tex; a.tex_desc = v.tex_desc; a.tex = v.tex;
    b.nodes = reinterpret_cast<const float4 *>(v.nodes); b.order = v.order; b.tri_boxes = reinterpret_cast<const float4 *>(v.tri_boxes);
    return SVGF_OK;
}

// *_create of a handle `State` (a ReservoirState) whose records take reservoir_bytes each; `reset` is the library's own, since an empty
// reservoir is stored differently in each.  Refusals in order: NULL out; NULL scene or a size <= 0; a record index of 16-byte words
// past 2^31 (UNSUPPORTED); a scene without a view; ids outside 0 .. RESERVOIR_MAX_ID; one id naming surfaces of differing emittance.
template <class State>
int reservoir_state_create(const svgf_scene *scene, int width, int height, unsigned long long reservoir_bytes, int (*reset)(State *, void *), State **out)
{
    if (!out) return SVGF_ERR_INVALID_ARG;
    *out = nullptr;
    if (!scene || width <= 0 || height <= 0) return SVGF_ERR_INVALID_ARG;
    if ((long long)width * height >= (1LL << 31) / (long long)(reservoir_bytes / 2)) return SVGF_ERR_UNSUPPORTED;
    SvgfSceneView v;
    if (svgf_scene_view(scene, &v) != SVGF_OK) return SVGF_ERR_INVALID_ARG;
    SvgfDeviceGuard dev_guard(v.device);
    if (!dev_guard.ok) return SVGF_ERR_NO_DEVICE;
    // the table from geomId to emittance, from the view's own arrays
    std::vector<SvgfSceneGeom> geoms((size_t)v.n_geoms);
    std::vector<int> geom_ids(v.geom_ids ? (size_t)v.n_geoms : 0), tri_ids((size_t)v.n_tris);
    if (hipDeviceSynchronize() != hipSuccess) return SVGF_ERR_HIP;
    if (v.n_geoms > 0 && hipMemcpy(geoms.data(), v.geoms, geoms.size() * sizeof(SvgfSceneGeom), hipMemcpyDeviceToHost) != hipSuccess) return SVGF_ERR_HIP;
    if (!geom_ids.empty() && hipMemcpy(geom_ids.data(), v.geom_ids, geom_ids.size() * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return SVGF_ERR_HIP;
    if (v.n_tris > 0 && hipMemcpy(tri_ids.data(), v.tri_ids, tri_ids.size() * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return SVGF_ERR_HIP;
    int max_id = -1;
    for (int k = 0; k < v.n_geoms; k++) {
        const int id = geom_ids.empty() ? k : geom_ids[k];
        if (id < 0 || id > RESERVOIR_MAX_ID) return SVGF_ERR_INVALID_ARG;
        max_id = id > max_id ? id : max_id;
    }
    for (int i = 0; i < v.n_tris; i++) {
        if (tri_ids[i] < 0 || tri_ids[i] > RESERVOIR_MAX_ID) return SVGF_ERR_INVALID_ARG;
        max_id = tri_ids[i] > max_id ? tri_ids[i] : max_id;
    }
    const int n_ids = max_id + 1;
    std::vector<float> emit((size_t)(n_ids > 0 ? n_ids : 1), 0.0f);
    std::vector<char> seen(emit.size(), 0);
    for (int k = 0; k < v.n_geoms; k++) {
        const int id = geom_ids.empty() ? k : geom_ids[k];
        const float e = geoms[k].emittance > 0.0f ? geoms[k].emittance : 0.0f;
        if (seen[id] && emit[id] != e) return SVGF_ERR_INVALID_ARG;
        seen[id] = 1; emit[id] = e;
    }
    for (int i = 0; i < v.n_tris; i++) {
        if (seen[tri_ids[i]] && emit[tri_ids[i]] != 0.0f) return SVGF_ERR_INVALID_ARG;
        seen[tri_ids[i]] = 1;
    }
    // one allocation: [H | T | previous normals | previous ids | emittance], 16-byte aligned parts
    const size_t np = (size_t)width * height, rb = (size_t)reservoir_bytes;
    const size_t o_h = 0, o_t = o_h + rb * np, o_n = o_t + rb * np, o_g = o_n + align16(12 * np), o_e = o_g + align16(4 * np);
    const size_t bytes = o_e + align16(4 * emit.size());
    State *st = new (std::nothrow) State();
    if (!st) return SVGF_ERR_OOM;
    char *m = nullptr;
    if (hipMalloc(reinterpret_cast<void **>(&m), bytes) != hipSuccess) { (void)hipGetLastError(); delete st; return SVGF_ERR_OOM; }
    st->scene = scene; st->device = v.device; st->width = width; st->height = height; st->n_ids = n_ids;
    st->reservoir_bytes = reservoir_bytes; st->dev = m; st->bytes = (unsigned long long)bytes;
    st->H = reinterpret_cast<float4 *>(m + o_h); st->T = reinterpret_cast<float4 *>(m + o_t);
    st->prev_n = reinterpret_cast<float *>(m + o_n); st->prev_gid = reinterpret_cast<int *>(m + o_g); st->emit = reinterpret_cast<float *>(m + o_e);
    bool ok = hipMemset(m, 0, bytes) == hipSuccess && hipMemcpy(st->emit, emit.data(), 4 * emit.size(), hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && reset(st, nullptr) == SVGF_OK && hipDeviceSynchronize() == hipSuccess;
    if (!ok) { (void)hipGetLastError(); (void)hipFree(m); delete st; return SVGF_ERR_HIP; }
    *out = st;
    return SVGF_OK;
}

template <class Info>
int reservoir_state_info(const ReservoirState *st, Info *out)
{
    if (!st || !out) return SVGF_ERR_INVALID_ARG;
    *out = Info{ st->width, st->height, st->n_ids, 2, st->bytes };
    return SVGF_OK;
}

// *_read: 0 H, 1 T, 2 the previous normals, 3 the previous ids, into exactly the plane's bytes (blocking)
int reservoir_state_read(const ReservoirState *st, int which, void *host_dst, unsigned long long host_bytes)
{
    if (!st || which < 0 || which > 3 || !host_dst) return SVGF_ERR_INVALID_ARG;
    const unsigned long long np = (unsigned long long)st->width * st->height;
    const void *src[4] = { st->H, st->T, st->prev_n, st->prev_gid };
    const unsigned long long size[4] = { st->reservoir_bytes * np, st->reservoir_bytes * np, 12ull * np, 4ull * np };
    if (host_bytes != size[which]) return SVGF_ERR_INVALID_ARG;
    SvgfDeviceGuard dev_guard(st->device);
    if (!dev_guard.ok) return SVGF_ERR_NO_DEVICE;
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(host_dst, src[which], (size_t)host_bytes, hipMemcpyDeviceToHost) != hipSuccess) return SVGF_ERR_HIP;
    return SVGF_OK;
}

template <class State>
void reservoir_state_destroy(State *st)
{
    if (!st) return;
    SvgfDeviceGuard dev_guard(st->device);
    if (dev_guard.ok) { (void)hipDeviceSynchronize(); (void)hipFree(st->dev); }
    delete st;
}
