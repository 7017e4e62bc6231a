"""numpy model of row f24's linear BVH (include/svgf_lbvh.h, "Normative result"): keys from the padded triangle boxes in float32 with
one rounding per operation, numpy's sort, and the Karras radix tree built SEQUENTIALLY from the root down - a range [l, r] of sorted
leaf keys splits behind the last key whose highest differing bit is 0, the left part becomes internal node gamma (or leaf gamma), the
right part internal node gamma + 1 (or leaf gamma + 1) - which shares no line with the per-node search the library runs.  Also the
invariants every tree is held to.  Test infrastructure only.
"""
import bisect

import numpy as np

F = np.float32
NODE = np.dtype([("lo", np.float32, 3), ("first", np.int32), ("hi", np.float32, 3), ("count", np.int32)])
MAX_DEPTH = 48


def bits(n_tris):
    """(idx_bits, axis_bits, key_bits)"""
    idx = max(1, (int(n_tris) - 1).bit_length())
    axis = min(10, (48 - idx) // 3)
    return idx, axis, 3 * axis + idx


def boxes_of(lo, hi):
    b = np.zeros(len(lo), NODE)
    b["lo"], b["hi"], b["first"], b["count"] = lo, hi, np.arange(len(lo)), 1
    return b


def keys_of(boxes):
    n = len(boxes)
    idx, axis, _ = bits(n)
    M = 1 << axis
    with np.errstate(all="ignore"):
        c = ((boxes["lo"].astype(F) + boxes["hi"].astype(F)).astype(F) * F(0.5)).astype(F)
        bmin = np.fmin.reduce(c, axis=0, initial=F(np.inf)).astype(F)
        bmax = np.fmax.reduce(c, axis=0, initial=F(-np.inf)).astype(F)
        ext = (bmax - bmin).astype(F)
        q = np.where(ext > 0, ((c - bmin).astype(F) / ext).astype(F), F(0)).astype(F)
        v = (q * F(M)).astype(F)
        inside = (v >= 0) & (v < F(M - 1))
        cell = np.where(~(v >= 0), 0, np.where(v >= F(M - 1), M - 1, np.where(inside, v, 0).astype(np.int64))).astype(np.uint64)
    morton = np.zeros(n, np.uint64)
    for j in range(axis):
        for a, off in ((0, 2), (1, 1), (2, 0)):
            morton |= ((cell[:, a] >> np.uint64(j)) & np.uint64(1)) << np.uint64(3 * j + off)
    return (morton << np.uint64(idx)) | np.arange(n, dtype=np.uint64)


def _union(lo_a, hi_a, lo_b, hi_b):
    return np.fmin(lo_a, lo_b), np.fmax(hi_a, hi_b)


def build(boxes, leaf_tris=0):
    """dict(nodes NODE[n_nodes], order int32[n], keys uint64[n] sorted, info) of NODE[n] padded boxes."""
    boxes = np.ascontiguousarray(boxes, dtype=NODE)
    n, L = len(boxes), int(leaf_tris) or 4
    assert n >= 1 and 1 <= L <= 8
    idx, axis, kb = bits(n)
    keys = np.sort(keys_of(boxes))
    order = (keys & np.uint64((1 << idx) - 1)).astype(np.int32)
    n_leaves = -(-n // L)
    nodes = np.zeros(2 * n_leaves - 1, NODE)

    def leaf(k, at):
        tri = order[k * L:min(n, k * L + L)]
        nodes[at]["lo"] = np.fmin.reduce(boxes["lo"][tri], axis=0)
        nodes[at]["hi"] = np.fmax.reduce(boxes["hi"][tri], axis=0)
        nodes[at]["first"], nodes[at]["count"] = k * L, len(tri)

    lk = [int(x) for x in keys[::L]]
    if n_leaves == 1:
        leaf(0, 0)
    else:
        todo, inner = [(0, 0, n_leaves - 1, 0)], []           # (internal index, l, r, node)
        while todo:
            j, l, r, at = todo.pop()
            inner.append(at)
            nodes[at]["first"], nodes[at]["count"] = 1 + 2 * j, 0
            h = (lk[l] ^ lk[r]).bit_length() - 1
            g = bisect.bisect_right(lk, lk[l] | ((1 << h) - 1), l, r + 1) - 1
            assert l <= g < r
            for (cl, cr, ci, cat) in ((l, g, g, 1 + 2 * j), (g + 1, r, g + 1, 2 + 2 * j)):
                if cl == cr:
                    leaf(cl, cat)
                else:
                    todo.append((ci, cl, cr, cat))
        for at in reversed(inner):            # a parent is listed before its children
            f = nodes[at]["first"]
            nodes[at]["lo"], nodes[at]["hi"] = _union(nodes[f]["lo"], nodes[f]["hi"], nodes[f + 1]["lo"], nodes[f + 1]["hi"])
    info = dict(n_tris=n, n_leaves=n_leaves, n_nodes=2 * n_leaves - 1, leaf_tris=L, idx_bits=idx, axis_bits=axis, key_bits=kb,
                depth_bound=min(kb, n_leaves - 1), launches=5 + 3 * (-(-kb // 8)))
    return dict(nodes=nodes, order=order, keys=keys, info=info)


def same_values(a, b):
    """float arrays by value: -0 == +0, NaN equals NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def check_invariants(nodes, order, keys, boxes, leaf_tris, depth_bound):
    """A binary tree by the SvgfBvhNode rules over a permutation, leaves of 1..L triangles, exact boxes, strictly increasing keys.
    Returns the measured depth."""
    n, L, n_nodes = len(boxes), int(leaf_tris) or 4, len(nodes)
    assert sorted(order.tolist()) == list(range(n)), "order is no permutation"
    if keys is not None:
        assert np.all(keys[1:] > keys[:-1]), "keys not strictly increasing"
    seen, covered, depth = np.zeros(n_nodes, bool), np.zeros(n, np.int32), 0
    todo, post = [(0, 0)], []
    while todo:
        k, d = todo.pop()
        assert 0 <= k < n_nodes and not seen[k], f"node {k}: out of range or reached twice"
        seen[k] = True
        depth = max(depth, d)
        first, count = int(nodes[k]["first"]), int(nodes[k]["count"])
        if count > 0:
            assert 1 <= count <= L and 0 <= first and first + count <= n, f"leaf {k}: first {first} count {count}"
            covered[first:first + count] += 1
            tri = order[first:first + count]
            assert same_values(nodes[k]["lo"], np.fmin.reduce(boxes["lo"][tri], axis=0)) and \
                same_values(nodes[k]["hi"], np.fmax.reduce(boxes["hi"][tri], axis=0)), f"leaf {k}: box is not the union of its triangles"
        else:
            assert count == 0 and 0 < first and first + 1 < n_nodes, f"inner node {k}: first {first} count {count}"
            post.append(k)
            todo += [(first, d + 1), (first + 1, d + 1)]
    assert seen.all(), "unreached nodes"
    assert np.all(covered == 1), "a triangle in no leaf or in two"
    for k in post:
        f = int(nodes[k]["first"])
        lo, hi = _union(nodes[f]["lo"], nodes[f]["hi"], nodes[f + 1]["lo"], nodes[f + 1]["hi"])
        assert same_values(nodes[k]["lo"], lo) and same_values(nodes[k]["hi"], hi), f"inner node {k}: box is not the union of its children"
    assert depth <= depth_bound <= MAX_DEPTH, f"depth {depth}, bound {depth_bound}"
    return depth


def same_tree(got_nodes, got_order, got_keys, m, what):
    """A builder's result against the model's: keys, order, first / count on bits, boxes by value."""
    assert got_keys is None or np.array_equal(np.asarray(got_keys, np.uint64), m["keys"]), f"{what}: keys differ"
    assert np.array_equal(got_order, m["order"]), f"{what}: order differs"
    assert len(got_nodes) == len(m["nodes"]), f"{what}: {len(got_nodes)} nodes, model {len(m['nodes'])}"
    for f in ("first", "count"):
        bad = np.flatnonzero(got_nodes[f] != m["nodes"][f])
        assert bad.size == 0, f"{what}: {f} differs at nodes {bad[:8].tolist()} (of {bad.size})"
    for f in ("lo", "hi"):
        ok = (got_nodes[f] == m["nodes"][f]) | (np.isnan(got_nodes[f]) & np.isnan(m["nodes"][f]))
        bad = np.flatnonzero(~ok.all(axis=1))
        assert bad.size == 0, f"{what}: box {f} differs at nodes {bad[:8].tolist()} (of {bad.size})"
