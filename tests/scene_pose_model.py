"""numpy model of the animated resident scene (include/svgf.h, row f15): posed triangles, their padded boxes, posed primitives, the
motion table and the refitted node boxes, float32 with one rounding per operation in the order the header writes them.  The frame of
a posed scene is tests/scene_model.py's on the posed arrays.  Also here: a replay of svgf_bvh_refit_plan_host's plan in numpy, and
hand-made node arrays in the builder's layout.  Test infrastructure only.

NaN: the model and the device place NaNs alike, but an x86 host and the GPU give a NaN they create different bits (sign, payload),
so comparisons "on bits" in the tests count NaNs in the same place as equal, like every other bit comparison of this suite.
"""
import numpy as np

import resident_scene_model as rm

F = np.float32
NODE = np.dtype([("lo", np.float32, 3), ("first", np.int32), ("hi", np.float32, 3), ("count", np.int32)])


def compose(A, B):
    """C = A o B of 3x4 row-major maps, float32[..., 12] each (broadcast)."""
    A, B = np.asarray(A, F).reshape(A.shape[:-1] + (3, 4)), np.asarray(B, F).reshape(B.shape[:-1] + (3, 4))
    shape = np.broadcast_shapes(A.shape, B.shape)
    C = np.zeros(shape, F)
    with np.errstate(all="ignore"):
        for r in range(3):
            for c in range(4):
                v = ((A[..., r, 0] * B[..., 0, c]).astype(F) + (A[..., r, 1] * B[..., 1, c]).astype(F)).astype(F)
                v = (v + (A[..., r, 2] * B[..., 2, c]).astype(F)).astype(F)
                C[..., r, c] = (v + A[..., r, 3]).astype(F) if c == 3 else v
    return C.reshape(shape[:-2] + (12,))


def _posed_mask(ids, n_objects):
    ids = np.asarray(ids)
    return (ids >= 0) & (ids < n_objects)


def posed_tris(tris, tri_ids, pose):
    """float32[n, 3, 8]: positions through pose[id].xf, normals through its linear block, uv untouched; an id outside the table is
    a bit copy."""
    T = np.array(tris, dtype=F).reshape(-1, 3, 8)
    m = _posed_mask(tri_ids, len(pose))
    if not m.any():
        return T
    M = pose["xf"][np.asarray(tri_ids)[m]].reshape(-1, 1, 3, 4)
    P, N = T[m][:, :, 0:3], T[m][:, :, 3:6]
    out = T[m]
    with np.errstate(all="ignore"):
        for r in range(3):
            p = ((M[..., r, 0] * P[..., 0]).astype(F) + (M[..., r, 1] * P[..., 1]).astype(F)).astype(F)
            p = (p + (M[..., r, 2] * P[..., 2]).astype(F)).astype(F)
            out[:, :, r] = (p + M[..., r, 3]).astype(F)
            q = ((M[..., r, 0] * N[..., 0]).astype(F) + (M[..., r, 1] * N[..., 1]).astype(F)).astype(F)
            out[:, :, 3 + r] = (q + (M[..., r, 2] * N[..., 2]).astype(F)).astype(F)
    T[m] = out
    return T


def posed_boxes(ptris):
    """(lo, hi) float32[n, 3]: the padded boxes of the posed triangles."""
    with np.errstate(all="ignore"):
        return rm.padded_boxes(ptris)


def posed_geoms(geoms, geom_ids, pose):
    """The primitives as drawn: xf' = pose.xf o xf, inv' = inv o pose.inv, invT' = transpose of inv's 3x3 block."""
    g = np.array(geoms)
    ids = np.arange(len(g)) if geom_ids is None else np.asarray(geom_ids)
    m = _posed_mask(ids, len(pose))
    if m.any():
        p = pose[ids[m]]
        xf, inv = compose(p["xf"], g["xf"][m]), compose(g["inv"][m], p["inv"])
        g["xf"][m], g["inv"][m] = xf, inv
        g["invT"][m] = inv.reshape(-1, 3, 4)[:, :, 0:3].transpose(0, 2, 1).reshape(-1, 9)
    return g


def motion_rows(held, pose):
    """float32[n_objects, 12]: held[k].xf o pose[k].inv."""
    return compose(held["xf"], pose["inv"])


def node_boxes(nodes, order, lo, hi):
    """(lo, hi) float32[n_nodes, 3]: per node the fmin / fmax union of the posed boxes of the triangles below it."""
    n = len(nodes)
    nlo, nhi = np.zeros((n, 3), F), np.zeros((n, 3), F)
    # the positions below a node are one range of `order` (leaves partition it in tree order): found bottom-up, and held against
    # resident_scene_model.leaves_below on every node of a small tree and on a sample of a large one
    first, count = nodes["first"].astype(np.int64), nodes["count"].astype(np.int64)
    b, e = np.where(count > 0, first, 0), np.where(count > 0, first + count, 0)
    for k in range(n - 1, -1, -1):
        if count[k] == 0:
            a = first[k]
            b[k], e[k] = min(b[a], b[a + 1]), max(e[a], e[a + 1])
    for k in (range(n) if n <= 300 else np.random.default_rng(n).choice(n, 100, replace=False).tolist() + [0]):
        assert sorted(rm.leaves_below(nodes, k)) == list(range(b[k], e[k])), f"node {k}"
    for k in range(n):
        ids = order[b[k]:e[k]]
        nlo[k], nhi[k] = np.fmin.reduce(lo[ids], axis=0), np.fmax.reduce(hi[ids], axis=0)
    return nlo, nhi


def state(s, pose, nodes, order):
    """Everything svgf_scene_read returns after one pose of scene dict `s`: tris, (lo, hi), node (lo, hi), geoms."""
    has = s["tris"] is not None and len(s["tris"])
    pt = posed_tris(s["tris"], s["tri_ids"], pose) if has else np.zeros((0, 3, 8), F)
    lo, hi = posed_boxes(pt) if has else (np.zeros((0, 3), F), np.zeros((0, 3), F))
    nlo, nhi = node_boxes(nodes, order, lo, hi) if has else (lo, hi)
    return dict(tris=pt, lo=lo, hi=hi, nlo=nlo, nhi=nhi, geoms=posed_geoms(s["geoms"], s["geom_ids"], pose))


def posed_scene(s, pose):
    """Scene dict `s` with posed triangles and primitives: what scene_model.render and svgf_scene_render_mesh are fed."""
    out = dict(s)
    if s["tris"] is not None and len(s["tris"]):
        out["tris"] = posed_tris(s["tris"], s["tri_ids"], pose)
    out["geoms"] = posed_geoms(s["geoms"], s["geom_ids"], pose)
    return out


# ---- the refit plan ---------------------------------------------------------------------------------------------------------------------
def replay_plan(plan, nodes, order, lo, hi):
    """Node boxes the way the kernels compute them from plan = binding.bvh_refit_plan_host(nodes, cap): per treelet the leaves from
    the triangle boxes, then its inner nodes level by level from the deepest; then the top list segment by segment.  Every node must
    be written exactly once."""
    n = len(nodes)
    nlo, nhi, written = np.full((n, 3), np.nan, F), np.full((n, 3), np.nan, F), np.zeros(n, int)
    level = plan["level"]

    def union(k):
        a = int(nodes[k]["first"])
        assert written[a] == 1 and written[a + 1] == 1, f"node {k} is computed before its children"
        nlo[k], nhi[k] = np.fmin(nlo[a], nlo[a + 1]), np.fmax(nhi[a], nhi[a + 1])
        written[k] += 1

    for t in plan["treelets"]:
        members = [int(t["root"])] + list(range(int(t["begin"]), int(t["begin"]) + int(t["count"])))
        for g in members:
            if nodes[g]["count"] > 0:
                ids = order[int(nodes[g]["first"]):int(nodes[g]["first"]) + int(nodes[g]["count"])]
                nlo[g], nhi[g] = np.fmin.reduce(lo[ids], axis=0), np.fmax.reduce(hi[ids], axis=0)
                written[g] += 1
        for L in range(int(t["levels"]) - 1, -1, -1):
            for g in members:
                if level[g] == L and nodes[g]["count"] == 0:
                    union(g)
    seg = plan["top_seg"]
    for s in range(len(seg) - 1):
        for g in plan["top"][seg[s]:seg[s + 1]]:
            union(int(g))
    assert (written == 1).all(), "a node is written more or less than once"
    return nlo, nhi


def tree(n_leaves, left_of):
    """A hand-made node array in the builder's layout (children in pairs behind their parent, descendants in one range) with one
    triangle per leaf: left_of(n) says how many of a node's n leaves go left.  Returns (nodes, order)."""
    nodes = np.zeros(2 * n_leaves - 1, NODE)
    used, tri = [1], [0]

    def build(k, n):        # depth-first, the left subtree completely before the right one
        if n == 1:
            nodes[k]["first"], nodes[k]["count"] = tri[0], 1
            tri[0] += 1
            return
        a = used[0]
        used[0] += 2
        nodes[k]["first"], nodes[k]["count"] = a, 0
        nl = left_of(n)
        build(a, nl)
        build(a + 1, n - nl)
    import sys
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 10000))
    try:
        build(0, n_leaves)
    finally:
        sys.setrecursionlimit(old)
    return nodes, np.arange(n_leaves, dtype=np.int32)


def chain(depth):
    """depth + 1 leaves, every inner node a leaf on the left and the rest on the right: depth `depth`."""
    return tree(depth + 1, lambda n: 1)


def balanced(n_leaves):
    return tree(n_leaves, lambda n: (n + 1) // 2)
