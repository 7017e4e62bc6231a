"""What the temporal-pass suites share (tests/test_motion_vectors.py, test_history_clamp.py, test_object_motion.py,
test_firefly_filter.py, test_temporal_matrix.py, test_spatial_variance.py): how frames are compared with tests/temporal_model.py, the parameter sets, the
input sequences (the synthetic scene as rendered and with mixed texels under a table of object motions, the block of box_room) and
the loop that runs a sequence through a context and reads its states back.  Test infrastructure only; not part of the package."""
import ctypes
import os

import numpy as np

import firefly_model as ff
import temporal_model as tm
from conftest import ROOT

F = np.float32
COORD, D32, D16 = tm.COORD, tm.D32, tm.D16
SCENE = os.path.join(ROOT, "tests", "golden", "scenes", "box_room.txt")
STATES = ("hlen", "mom", "color", "variance", "acc")      # svgf_read_state 0..4


# ---- comparison and parameters ----------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def assert_frames_equal(got, ref, what):
    """got: per frame the five states read from a context; ref: per frame the model's dict (acc = color with the spatial filter off)."""
    assert len(got) == len(ref)
    for f, (g, r) in enumerate(zip(got, ref)):
        for name in STATES:
            want = r["color" if name == "acc" else name]
            bad = "" if same_bits(g[name], want) else f"{np.count_nonzero(~np.isclose(g[name], want, rtol=0, atol=0, equal_nan=True))} values differ"
            assert not bad, f"{what}: {name}, frame {f}: {bad}"


def temporal_only(pkg, **kw):
    return pkg.reference_defaults().set(**{**dict(temporal_enable=1, spatial_enable=0), **kw})


def scales(pkg, W, H):
    """SvgfParams::reproj_scale that makes the reprojection exact at any aspect, (tan(FOVY) * W / H, tan(FOVY)): the reference's
    own mapping loses every pixel's history at 300x9, and nothing behind the reprojection would run there."""
    plx, ply = pkg.synth._pixel_length(W, H, 45.0)
    return float(plx) * W / 2.0, float(ply) * H / 2.0


def synth_params(pkg, W, H, **kw):
    p = temporal_only(pkg, **kw)
    p.reproj_scale[0], p.reproj_scale[1] = scales(pkg, W, H)
    return p


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def synth_sequence(pkg, orc, W, H, n=4, seed=31):
    """n frames of the synthetic scene under its moving camera, texels as rendered (finite positions): per frame
    (colour[H, W, 3], texels[H, W], camera, view matrix).  Computed once per session; callers that change a frame copy it."""
    cache = synth_sequence.__dict__.setdefault("cache", {})
    if (W, H, n, seed) not in cache:
        seq = []
        for f in range(n):
            col, gb, cam = pkg.synth.render_frame(W, H, f, seed=seed, moving=True, noise_model="hash")
            seq.append((np.asarray(col, F).reshape(H, W, 3), gb.reshape(H, W), cam, orc.view_matrix(pkg, cam)))
        cache[(W, H, n, seed)] = seq
    return cache[(W, H, n, seed)]


BLOCK, SIDE = 7, 96      # the turned block of box_room.txt; every box_room frame is SIDE x SIDE


def block_sequence(pkg, n, slide_x, turn_deg):
    """n frames of box_room at 96x96 under a static camera, the turned block (object 7) rotated by turn_deg about y and translated
    by slide_x in x per frame.  Returns (camera, [(colour[H, W, 3], texels[H, W], X float32[n_geoms, 12])]); X[g] = xf_prev[g] *
    inv_cur[g] composed in float64 and rounded: this frame's world space to the previous frame's (frame 0: identities).  Computed
    once per session."""
    cache = block_sequence.__dict__.setdefault("cache", {})
    if (n, slide_x, turn_deg) not in cache:
        sc = pkg.scene.parse_scene(open(SCENE).read())
        cam = pkg.scene.camera_for_frame(sc, 0, False)
        t0, r0 = tuple(sc.objects[BLOCK]["trans"]), tuple(sc.objects[BLOCK]["rotat"])
        frames, prev = [], None
        for f in range(n):
            o = sc.objects[BLOCK]
            o["trans"] = (t0[0] + slide_x * f,) + t0[1:]
            o["rotat"] = (r0[0], r0[1] + turn_deg * f, r0[2])
            g = pkg.scene.geom_array(sc)
            col, gb = pkg.scene.render_scene(SIDE, SIDE, f, g, cam, seed=3)
            X = np.tile(np.eye(3, 4).reshape(-1), (len(g), 1))
            if prev is not None:
                for k in range(len(g)):
                    a = np.vstack([prev[k]["xf"].astype(np.float64).reshape(3, 4), [0, 0, 0, 1]])
                    b = np.vstack([g[k]["inv"].astype(np.float64).reshape(3, 4), [0, 0, 0, 1]])
                    X[k] = (a @ b)[:3].reshape(-1)
            frames.append((np.asarray(col, F).reshape(SIDE, SIDE, 3), gb.reshape(SIDE, SIDE), X.astype(F)))
            prev = g
        cache[(n, slide_x, turn_deg)] = (cam, frames)
    return cache[(n, slide_x, turn_deg)]


MOVING_FRAMES = 6


def moving_block_sequence(pkg):
    """Six frames, the block translated by +0.4 in x per frame, no rotation."""
    return block_sequence(pkg, MOVING_FRAMES, 0.4, 0.0)


def rotation(axis, degrees):
    a = np.deg2rad(degrees)
    c, s = np.cos(a), np.sin(a)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis]


BAD_ROW = 6


def mixed_table():
    """Nine maps, indexed by the synthetic scene's geomIds 0..8: rotations of 0-12 degrees (svgf_normals_close rejects above about
    5.7) with translations of 0-0.45 (around the position tolerance 0.3); row 0 is the exact identity, row 6 holds NaN and inf."""
    spec = [("y", 0.0, (0.0, 0.0, 0.0)), ("y", 2.0, (0.05, 0.0, 0.0)), ("x", 4.0, (0.0, 0.02, 0.1)), ("z", 5.5, (0.0, 0.0, 0.0)),
            ("y", 6.0, (0.2, 0.0, 0.0)), ("x", 8.0, (0.0, 0.0, -0.3)), ("y", 1.0, (0.0, 0.0, 0.0)), ("y", 12.0, (0.4, 0.1, 0.0)),
            ("z", 0.0, (0.25, 0.0, 0.15))]
    X = np.stack([np.concatenate([rotation(ax, deg), np.array(t)[:, None]], axis=1).reshape(-1) for ax, deg, t in spec]).astype(F)
    X[BAD_ROW, 1], X[BAD_ROW, 7], X[BAD_ROW, 8] = np.nan, np.inf, -np.inf
    return X


def mixed_sequence(pkg, orc, W, H, n=4, finite=False):
    """n frames of the synthetic scene under its moving camera with the texels of tests/test_motion_vectors.py::_texels_for_helper:
    ray misses, ids beyond the table, non-finite and behind-the-camera positions.  Per frame (colour[H, W, 3], texels[H, W],
    camera, view matrix).
    finite: the same texels without the non-finite positions, for frames that run the a-trous levels.  A staged non-finite texel
    switches a workgroup of the lane a-trous kernel to its careful loop, and that switch is raced by the loader which stages the
    texel: the row computed meanwhile may round differently from run to run (tests/test_parity_gpu.py compares such frames bit
    for bit "only without non-finite texels"), so two contexts agree exactly only on finite texels.  The temporal pass, which
    is what these inputs are for, has no such race and is compared on the non-finite texels with the a-trous levels off."""
    cache = mixed_sequence.__dict__.setdefault("cache", {})
    if (W, H, n, finite) not in cache:
        seq = []
        for f, (col, gb, cam, M) in enumerate(synth_sequence(pkg, orc, W, H, n, seed=11)):
            gb = gb.copy()
            rng = np.random.default_rng(W * 1000 + H + 17 * f)
            flat = gb.reshape(-1)
            m = flat.size
            flat["geomId"][rng.integers(0, m, max(1, m // 7))] = -1
            flat["geomId"][rng.integers(0, m, max(1, m // 9))] = 40             # beyond the table: unmoved
            if m > 4:
                bad = rng.integers(0, m, 3)      # (drawn either way: the other texels are the same in both forms)
                if not finite:
                    flat["position"][bad] = (np.nan, np.inf, -1e30)
                flat["position"][rng.integers(0, m, 2)] = (0.0, 5.0, 60.0)      # behind the camera
            seq.append((col, gb, cam, M))
        cache[(W, H, n, finite)] = seq
    return cache[(W, H, n, finite)]


NOISY_FRAMES = 6
THRESHOLD_STEP = (F(0.1), np.nextafter(F(0.1), F(1)))      # 0.1f: the largest normal distance accepted; 0.10000001f: the next float


def noisy_sequence(pkg, orc, W, H, n=NOISY_FRAMES, finite=False, threshold_edits=True):
    """mixed_sequence made to act on the spatial variance estimate (k_spatial_variance), by seeded edits per frame:
    - every colour times one factor per pixel from [0.25, 1.75], plus noise per channel from [0, 0.2]: moments that differ from
      tap to tap (mixed_sequence's walls are flat, and a flat window's estimate is 0);
    - about 2 % of the normals NaN (such a pixel accepts its own tap alone, and is nobody's tap);
    - about 2 % of the pixels get a right-hand neighbour of their geomId with their normal + (0.1f, 0, 0), and about 2 % one with
      their normal + (0, 0.10000001f, 0): pairs at the threshold of the predicate, on either side of it where the pixel's own
      component is 0 (threshold_edits False leaves both out, nothing else changes: the draws are made either way);
    - two pixels each of colour 1e20 (its second moment overflows: an estimate of +inf), NaN and inf, and three of 1000.0.
    finite: on mixed_sequence's finite form (for frames that run the a-trous levels, see there) and without the edits that put a
    non-finite value into a plane the levels read: the NaN normals, the NaN and inf colours, and the 1e20 colours, which are
    inf edits by then (the temporal pass squares the luminance: a second moment of +inf, a variance of +inf or, from inf - inf,
    of 0, and the levels' kernels are held to the oracle on finite planes only).  The 1000.0 pixels stay.
    Per frame (colour[H, W, 3], texels[H, W], camera, view matrix)."""
    cache = noisy_sequence.__dict__.setdefault("cache", {})
    key = (W, H, n, finite, threshold_edits)
    if key not in cache:
        seq = []
        for f, (col, gb, cam, M) in enumerate(mixed_sequence(pkg, orc, W, H, n, finite)):
            rng = np.random.default_rng(7919 * W + 31 * H + 101 * f + 5)
            m = W * H
            col = (col.reshape(m, 3) * rng.uniform(0.25, 1.75, (m, 1)).astype(F) + rng.uniform(0.0, 0.2, (m, 3)).astype(F)).astype(F)
            gb = gb.copy()
            flat = gb.reshape(-1)
            nan_normals = rng.random(m) < 0.02
            step = rng.random((2, m))
            if not finite:
                flat["normal"][nan_normals] = np.nan
            if threshold_edits:
                for j, axis in enumerate((0, 1)):
                    src = np.flatnonzero((step[j] < 0.02) & (np.arange(m) % W != W - 1))
                    for i in src:      # in raster order: a pair laid down later may rewrite an earlier pair's neighbour
                        flat["geomId"][i + 1] = flat["geomId"][i]
                        nq = flat["normal"][i].copy()
                        nq[axis] = nq[axis] + THRESHOLD_STEP[j]
                        flat["normal"][i + 1] = nq
            special = rng.choice(m, min(9, m), replace=False)
            values = [F(1e20), F(1e20), F(1000.0), F(1000.0), F(1000.0), F(np.nan), F(np.nan), F(np.inf), F(np.inf)]
            for i, v in zip(special, values):
                if not finite or v == F(1000.0):
                    col[i] = v
            seq.append((col.reshape(H, W, 3), gb, cam, M))
        cache[key] = seq
    return cache[key]


def mixed_model(pkg, orc, W, H, fmt, tol, radius=0, k=0.0, rank=0, scale=1.0, table=True, svf=0, noisy=None, reset_before=()):
    """The model on mixed_sequence with mixed_table: fmt None = the camera path (the moved position projected through the previous
    frame's camera); otherwise through the plane svgf_motion_reproject(X) writes in that format, converted as the header says.
    rank, scale: the frames' colours go through firefly_model.firefly_filter first (svgf_set_firefly_filter; rank 0 leaves them as
    they are).  table False: no table at all, and the plane written without X.
    svf: SvgfParams::spatial_variance_frames, one K or one per frame.  noisy: None = mixed_sequence; otherwise the keyword
    arguments of noisy_sequence (a dict), whose frames the model then runs.  reset_before: as run_sequence's."""
    cache = mixed_model.__dict__.setdefault("cache", {})
    svf = svf if np.isscalar(svf) else tuple(svf)
    noisy_key = None if noisy is None else tuple(sorted(noisy.items()))
    key = (W, H, fmt, tol, radius, k, rank, scale if rank else None, table, svf, noisy_key, tuple(reset_before))
    if key not in cache:
        seq = mixed_sequence(pkg, orc, W, H) if noisy is None else noisy_sequence(pkg, orc, W, H, **noisy)
        X = mixed_table() if table else None
        sx, sy = scales(pkg, W, H)
        views = [seq[max(f - 1, 0)][3] for f in range(len(seq))]
        coords = None
        if fmt is not None:
            coords = [tm.coord_plane(tm.motion_plane(views[f], W, H, seq[f][1], X, fmt, F(sx), F(sy)), fmt, W, H) for f in range(len(seq))]
        cache[key] = tm.run_sequence([(ff.firefly_filter(c, rank, scale), g) for c, g, _, _ in seq], coords=coords,
                                     tables=[X] * len(seq) if table else None, views=views, scale=(sx, sy), pos_tol=tol, radius=radius, k=k,
                                     svf=svf, reset_before=tuple(reset_before))
    return cache[key]


# ---- the GPU side ---------------------------------------------------------------------------------------------------------------------
def _hip():
    """The HIP runtime already loaded into this process (torch's), for plain host-to-device copies into raw pointers."""
    for ln in open("/proc/self/maps"):
        if "libamdhip64" in ln:
            return ctypes.CDLL(ln.split()[-1])
    raise RuntimeError("no HIP runtime loaded")


def read_states(den):
    return {name: den.read_state(k) for k, name in enumerate(STATES)}


def device_table(X):
    import torch
    return torch.from_numpy(np.ascontiguousarray(X, dtype=F)).cuda()


def run_gpu(pkg, den, frames, params, cams, leg="aos", planes=None, fmt=COORD, plane_fmt=None, plane_tables=None, reset_before=(),
            outputs=None):
    """frames: [(colour, texels)]; cams: per frame; params: one SvgfParams, or one per frame.  The context's clamp and table are
    whatever the caller set.  The history is
    looked up through the camera path, or through a motion plane given in one of two ways:
    planes, fmt: per frame a host plane of format `fmt` (the model's), uploaded;
    plane_fmt, plane_tables: the plane svgf_motion_reproject writes on the device in that format for the previous frame's camera,
    params' reproj_scale and plane_tables[f] (None: no table).
    reset_before: the frames in front of which svgf_reset is called.  outputs: a list that receives each frame's `out` (host).
    Returns per frame the five states.  `leg`: aos | planar."""
    import torch
    assert planes is None or plane_fmt is None
    H, W = frames[0][1].shape
    den.set_capture(True)
    out, res, keep = torch.empty((H, W, 3), dtype=torch.float32, device="cuda"), [], []
    per_frame = list(params) if isinstance(params, (list, tuple)) else [params] * len(frames)
    for f, (col, gb) in enumerate(frames):
        params = per_frame[f]
        rs = (params.reproj_scale[0], params.reproj_scale[1])
        if f in reset_before:
            den.reset()
        t_c = torch.from_numpy(np.ascontiguousarray(col, dtype=F)).cuda()
        t_g = torch.from_numpy(np.ascontiguousarray(gb).view(np.uint8).reshape(-1).copy()).cuda()
        mv = None if planes is None else torch.from_numpy(np.ascontiguousarray(planes[f])).cuda()
        if plane_fmt is not None:
            fmt = plane_fmt
            mv = torch.empty((H, W, 2), dtype=torch.float16 if fmt == D16 else torch.float32, device="cuda")
            t_x = None if plane_tables is None or plane_tables[f] is None else device_table(plane_tables[f])
            pkg.binding.motion_reproject(mv, W, H, cams[max(f - 1, 0)], gbuffer=t_g, motion_format=fmt, reproj_scale=rs, geom_xf=t_x)
            keep.append(t_x)
        keep.append((t_c, t_g, mv))      # (a promised frame's inputs stay untouched until its work is done)
        torch.cuda.synchronize()
        if leg == "planar":
            g = den.planar_gbuffer()
            hip = _hip()
            hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
            flat = np.ascontiguousarray(gb).reshape(-1)
            for dst, arr in ((g.normal, flat["normal"]), (g.position, flat["position"]), (g.geom_id, flat["geomId"]),
                             (g.albedo, (flat["albedo"] * flat["ialbedo"]).astype(F))):
                arr = np.ascontiguousarray(arr)
                assert hip.hipMemcpy(dst, arr.ctypes.data, arr.nbytes, 1) == 0
            den.denoise_planar(out, t_c, cams[f], params, motion=mv, motion_format=fmt)
        else:
            den.denoise(out, t_c, t_g, cams[f], params, motion=mv, motion_format=fmt)
        den.sync()
        res.append(read_states(den))
        if outputs is not None:
            outputs.append(out.cpu().numpy())
    return res


def _whole_frames(pkg, den, params, frames, cam, tables=False):
    """The frames of a block_sequence through svgf_denoise, none waited for before the last is enqueued.  tables: each frame's X
    is set as the context's object motion table before the frame.  Returns (per frame the output, states 0-2 after the last)."""
    import torch
    H = W = SIDE
    keep = []
    for col, gb, X in frames:
        t_c = torch.from_numpy(col).cuda()
        t_g = torch.from_numpy(gb.view(np.uint8).reshape(-1).copy()).cuda()
        t_x = device_table(X) if tables else None      # one per frame: a promised frame's table stays untouched until the frame is done
        out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        keep.append((t_c, t_g, t_x, out))
        torch.cuda.synchronize()
        if tables:
            den.set_object_motion(t_x, X.shape[0])
        den.denoise(out, t_c, t_g, cam, params)
    den.sync()
    return [o.cpu().numpy() for _, _, _, o in keep], [den.read_state(k) for k in (0, 1, 2)]
