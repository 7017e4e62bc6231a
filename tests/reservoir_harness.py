"""What tests/test_restir.py (row f27) and tests/test_restir_gi.py (row f28) share: the comparison of reservoir planes, the inputs both
suites feed (the motion plane made for the taps, the tube in row f15's room, the lamps), the device buffers, and the one check of a
frame's state and output against a model's.  A plain module like tests/scene_harness.py: no test, no fixture."""
import functools
import subprocess

import numpy as np

import restir_model as rsm
import scene_harness as sh
import test_scene_model as tsm

F = np.float32
AMBIENT = 0.15


# ---- comparisons ---------------------------------------------------------------------------------------------------------------------------
def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def differing_records(a, b):
    """The records of two reservoir planes that differ in bits; NaNs in the same place are equal."""
    a, b = np.ascontiguousarray(a).reshape(-1), np.ascontiguousarray(b).reshape(-1)
    assert a.dtype == b.dtype and a.shape == b.shape
    bad = np.zeros(len(a), bool)
    for k in a.dtype.names:
        x, y = a[k].reshape(len(a), -1), b[k].reshape(len(b), -1)
        if x.dtype.kind == "f":
            nx, ny = np.isnan(x), np.isnan(y)
            bad |= ((nx != ny) | (~nx & ~ny & (x.view(np.uint32) != y.view(np.uint32)))).any(axis=1)
        else:
            bad |= (x != y).any(axis=1)
    return int(bad.sum())


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lamps(n, kind, seed=27):
    """n lights over the made stage: centres in a slab above the floor, `area` lights with half-edges of up to 0.4, powers per channel
    such that the sum over the lights stays near one light of 30."""
    rng = np.random.default_rng(seed + n)
    c = np.stack([rng.uniform(-5, 5, n), rng.uniform(1.5, 7.0, n), rng.uniform(-5, 5, n)], -1)
    eu = rng.uniform(-0.4, 0.4, (n, 3)) if kind == "area" else np.zeros((n, 3))
    ev = rng.uniform(-0.4, 0.4, (n, 3)) if kind == "area" else np.zeros((n, 3))
    lt = rsm.lights(c, eu, ev, rng.uniform(10.0, 50.0, (n, 3)) / min(n, 64) ** 0.5)
    lt.setflags(write=False)
    return lt


TUBE = dict(segments=8, sides=8, length=6.0, radius=0.5, base=(1.5, 0.1, 6.0))      # tests/test_deform_scene.py's tube in row f15's room
PIVOT, TUBE_ID = (1.5, 3.1, 6.0), 40


@functools.lru_cache(maxsize=None)
def tube_scene():
    import __graft_entry__ as ge
    pkg = ge.load_package()
    geoms, cam, lt = sh.example_scene()
    tris, bone, weight = pkg.deform.tube_rig(**TUBE)
    n = len(tris)
    s = dict(cam=cam, geoms=geoms, geom_ids=None, tris=tris, tri_ids=np.full(n, TUBE_ID, np.int32), tri_albedo=tsm._colours(n, 26), tri_tex=None,
             textures=None, light=lt["centre"])
    return s, (np.arange(n, dtype=np.int32), bone, weight)


def motion(W, H, f):
    """A SVGF_MOTION_PREV_COORD_F32 plane made for the taps: a shift that differs per frame and crosses object and face edges, and
    rows of pixels with NaN, +-inf and far off-screen values."""
    x, y = np.meshgrid(np.arange(W, dtype=F), np.arange(H, dtype=F))
    sign = F(-1.0 if f == 2 else 1.0)                                       # the second plane looks back the other way
    mv = np.stack([x + sign * F(1.3 + 2.1 * f), y - sign * F(0.6 + 0.9 * f)], -1).astype(F)
    flat = mv.reshape(-1, 2)
    n = W * H
    for k, bad in enumerate((np.nan, np.inf, -np.inf, -5.0, 1e9, -0.5001, W - 0.5)):
        flat[(7 * k + 3) % n::53, k % 2] = bad
    return mv


# ---- the libraries' surfaces, the device side --------------------------------------------------------------------------------------------------
def nm(path, flag):
    out = subprocess.run(["nm", "-D", flag, path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return sorted(ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("svgf_")), out


def planes_of(pkg, gb):
    """A G-buffer's normal, position and geomId as device planes: (SvgfPlanarGBuffer, the tensors that keep them alive)."""
    import torch
    t = [torch.from_numpy(np.ascontiguousarray(gb[f])).cuda() for f in ("normal", "position", "geomId")]
    return pkg.binding.SvgfPlanarGBuffer(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), None), t


def out(W, H):
    import torch
    return torch.full((H, W, 3), float("nan"), dtype=torch.float32, device="cuda")


def read(st):
    return dict(H=st.read(0), T=st.read(1), prev_n=st.read(2), prev_gid=st.read(3))


def assert_frame(st, out, want, key, what):
    """T and H as read back BEFORE the output plane `key` (D or I); expected and allowed differences: 0."""
    import torch
    torch.cuda.synchronize()
    got = read(st)
    bad = {k: differing_records(got[k], want[k]) for k in ("T", "H")}
    bad["prev_n"] = int(tsm.differing(got["prev_n"], want["prev_n"]).sum())
    bad["prev_gid"] = int((got["prev_gid"] != want["prev_gid"]).sum())
    print(f"{what}: differing records {bad} (expected and allowed: 0)")
    assert not any(bad.values()), f"{what}: {bad}"
    d = int(tsm.differing(out.cpu().numpy(), want[key]).sum())
    print(f"{what}: {key} differs on {d} pixels (expected and allowed: 0)")
    assert d == 0, f"{what}: {key} differs on {d} pixels"


def device_rp(pkg, rp):
    return pkg.restir.params(rp["candidates"], rp["temporal"], float(rp["m_cap"]), rp["neighbours"], float(rp["radius"]), float(rp["normal_min_dot"]))
