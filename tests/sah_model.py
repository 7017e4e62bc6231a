"""numpy model of row f25's device SAH build (include/svgf_sah.h, "Normative result"): the binned-SAH tree of the triangles as drawn, in
the sparse layout the header states - record 0 the root, the children of an inner node that splits at position s at records 2 s - 1 and
2 s.  Sequential (one node at a time from an explicit list), float32 through numpy with one rounding per operation, the cost in Python
floats (IEEE double, no contraction); it shares no code with the library or with the host builder.  Also relayout(), which moves a tree
in the host builder's numbering into that layout, and the invariants of the sparse layout.  Test infrastructure only.
"""
import numpy as np

F = np.float32
NODE = np.dtype([("lo", np.float32, 3), ("first", np.int32), ("hi", np.float32, 3), ("count", np.int32)])
MAX_DEPTH = 48
BINS = 16
SMALL = 256
INF = float("inf")


def rounds(n_tris):
    """large-node rounds of the device plan: 0 up to SMALL triangles, else ceil(log2(n / SMALL)) + 4"""
    if n_tris <= SMALL:
        return 0
    r = 0
    while (SMALL << r) < n_tris:
        r += 1
    return r + 4


def info_of(n_tris, L):
    return dict(n_tris=n_tris, max_leaf_tris=int(L) or 4, n_records=2 * n_tris - 1, depth_bound=min(MAX_DEPTH, n_tris - 1), launches=2 + 5 * rounds(n_tris))


def centroids(tris):
    v = np.asarray(tris, F).reshape(-1, 3, 8)[:, :, 0:3]
    with np.errstate(all="ignore"):
        mn, mx = np.fmin.reduce(v, axis=1), np.fmax.reduce(v, axis=1)
        return ((F(0.5) * mn).astype(F) + (F(0.5) * mx).astype(F)).astype(F)


def bin_of(v, lo, ext):
    """total: the comparisons come before the cast"""
    with np.errstate(all="ignore"):
        q = (((v - lo).astype(F) / ext).astype(F) * F(BINS)).astype(F)
        inside = (q >= 0) & (q < F(BINS))
        return np.where(~(q >= 0), 0, np.where(q >= F(BINS), BINS - 1, np.where(inside, q, 0).astype(np.int64))).astype(np.int64)


def _area(lo, hi):
    x, y, z = (float(hi[c]) - float(lo[c]) for c in range(3))
    return x * y + y * z + z * x


def _room(L, below):
    return (1 << 62) if below >= 40 else (L << below)


def build(tris, boxes, max_leaf_tris=0):
    """dict(records NODE[2 n - 1], order int32[n], counts dict, info dict) of float32[n, 3, 8] triangles and their padded boxes (NODE[n] or
    a (lo, hi) pair)."""
    L = int(max_leaf_tris) or 4
    cen = centroids(tris)
    n = len(cen)
    assert n >= 1 and 1 <= L <= 8
    blo, bhi = (boxes["lo"], boxes["hi"]) if isinstance(boxes, np.ndarray) and boxes.dtype.names else boxes
    blo, bhi = np.asarray(blo, F), np.asarray(bhi, F)
    order, rec = np.arange(n, dtype=np.int32), np.zeros(2 * n - 1, NODE)
    counts = dict(n_nodes=0, n_leaves=0, depth=0, forced_splits=0)
    todo = [(0, 0, n, 0)]
    with np.errstate(all="ignore"):
        while todo:
            at, b, e, level = todo.pop()
            idx, m = order[b:e].copy(), e - b
            rec[at]["lo"], rec[at]["hi"] = np.fmin.reduce(blo[idx], axis=0, initial=F(np.inf)), np.fmax.reduce(bhi[idx], axis=0, initial=F(-np.inf))
            counts["n_nodes"] += 1
            counts["depth"] = max(counts["depth"], level)
            if m <= L:
                rec[at]["first"], rec[at]["count"] = b, m
                counts["n_leaves"] += 1
                continue
            c = cen[idx]
            clo, chi = np.fmin.reduce(c, axis=0, initial=F(np.inf)), np.fmax.reduce(c, axis=0, initial=F(-np.inf))
            best, best_axis, best_bin, best_left = INF, -1, 0, 0
            for axis in range(3):
                ext = F(chi[axis] - clo[axis])
                if not (ext > 0) or not np.isfinite(ext):
                    continue
                j = bin_of(c[:, axis], clo[axis], ext)
                cnt = np.bincount(j, minlength=BINS)
                lo = np.full((BINS, 3), np.inf, F)
                hi = np.full((BINS, 3), -np.inf, F)
                for k in range(BINS):
                    if cnt[k]:
                        lo[k], hi[k] = np.fmin.reduce(blo[idx[j == k]], axis=0, initial=F(np.inf)), np.fmax.reduce(bhi[idx[j == k]], axis=0, initial=F(-np.inf))
                left = 0
                for k in range(BINS - 1):               # the plane behind bin k
                    left += int(cnt[k])
                    if left == 0 or left == m:
                        continue
                    cost = _area(np.fmin.reduce(lo[:k + 1], axis=0), np.fmax.reduce(hi[:k + 1], axis=0)) * left + \
                        _area(np.fmin.reduce(lo[k + 1:], axis=0), np.fmax.reduce(hi[k + 1:], axis=0)) * (m - left)
                    if cost < best:
                        best, best_axis, best_bin, best_left = cost, axis, k, left
            nl = 0
            if best_axis >= 0:
                goes_left = bin_of(c[:, best_axis], clo[best_axis], F(chi[best_axis] - clo[best_axis])) <= best_bin
                order[b:e] = np.concatenate([idx[goes_left], idx[~goes_left]])          # stable
                nl = best_left
            room = _room(L, MAX_DEPTH - level - 1)
            if nl <= 0 or nl >= m or nl > room or m - nl > room:
                nl = (m + 1) // 2                       # by position, after the partition has happened
                counts["forced_splits"] += 1
            s = b + nl
            rec[at]["first"], rec[at]["count"] = 2 * s - 1, 0
            todo += [(2 * s, s, e, level + 1), (2 * s - 1, b, s, level + 1)]
    return dict(records=rec, order=order, counts=counts, info=info_of(n, L))


def relayout(nodes, n_tris):
    """A tree in the host builder's numbering (children in pairs at `first`) in the sparse layout: NODE[2 n_tris - 1]."""
    nodes = np.asarray(nodes, NODE)
    out = np.zeros(2 * n_tris - 1, NODE)

    first, count = nodes["first"].tolist(), nodes["count"].tolist()
    end = [0] * len(nodes)                              # the end of a node's position range: children stand behind their parent
    for k in range(len(nodes) - 1, -1, -1):
        end[k] = first[k] + count[k] if count[k] > 0 else end[first[k] + 1]
    todo = [(0, 0)]
    while todo:
        k, at = todo.pop()
        out[at]["lo"], out[at]["hi"] = nodes[k]["lo"], nodes[k]["hi"]
        if nodes[k]["count"] > 0:
            out[at]["first"], out[at]["count"] = nodes[k]["first"], nodes[k]["count"]
            continue
        f = int(nodes[k]["first"])
        s = end[f]
        assert out[2 * s - 1]["count"] == 0 and out[2 * s - 1]["first"] == 0 and out[2 * s]["count"] == 0 and out[2 * s]["first"] == 0, \
            f"two inner nodes split at position {s}"
        out[at]["first"], out[at]["count"] = 2 * s - 1, 0
        todo += [(f, 2 * s - 1), (f + 1, 2 * s)]
    return out


def same_values(a, b):
    """float arrays by value: -0 == +0, NaN equals NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def check_invariants(records, order, boxes, max_leaf_tris, depth_bound):
    """The reachable part a binary tree over a permutation, every inner node's children where the layout rule puts them, the padding all
    zero, leaves of 1..L triangles, exact boxes (fminf / fmaxf unions), depth <= bound.  Returns dict(n_nodes, n_leaves, depth)."""
    n, L = len(order), int(max_leaf_tris) or 4
    blo, bhi = (boxes["lo"], boxes["hi"]) if isinstance(boxes, np.ndarray) and boxes.dtype.names else boxes
    assert len(records) == 2 * n - 1, f"{len(records)} records for {n} triangles"
    assert sorted(np.asarray(order).tolist()) == list(range(n)), "order is no permutation"
    seen = np.zeros(len(records), bool)
    out = dict(n_nodes=0, n_leaves=0, depth=0)
    todo = [(0, 0, n, 0)]
    with np.errstate(all="ignore"):
        while todo:
            at, b, e, d = todo.pop()
            assert 0 <= at < len(records) and not seen[at], f"record {at}: out of range or reached twice"
            seen[at] = True
            out["n_nodes"] += 1
            out["depth"] = max(out["depth"], d)
            first, count = int(records[at]["first"]), int(records[at]["count"])
            tri = order[b:e]
            assert same_values(records[at]["lo"], np.fmin.reduce(blo[tri], axis=0, initial=F(np.inf))) and \
                same_values(records[at]["hi"], np.fmax.reduce(bhi[tri], axis=0, initial=F(-np.inf))), f"record {at}: box is not the union of [{b}, {e})"
            if count > 0:
                assert first == b and count == e - b and 1 <= count <= L, f"leaf {at} over [{b}, {e}): first {first} count {count}"
                out["n_leaves"] += 1
                continue
            assert count == 0 and first % 2 == 1, f"inner record {at}: first {first} count {count}"
            s = (first + 1) // 2
            assert b < s < e, f"inner record {at} over [{b}, {e}) splits at {s}"
            todo += [(first, b, s, d + 1), (first + 1, s, e, d + 1)]
    assert out["n_nodes"] == 2 * out["n_leaves"] - 1
    pad = np.asarray(records)[~seen]
    assert not np.frombuffer(pad.tobytes(), np.uint8).any(), "padding is not zero"
    if L == 1:
        assert seen.all(), "L = 1 leaves no padding"
    assert out["depth"] <= depth_bound <= MAX_DEPTH, f"depth {out['depth']}, bound {depth_bound}"
    return out


def same_tree(got_records, got_order, m_records, m_order, what, bytes_too=False):
    """A builder's result against another's: order, first / count on bits, boxes by value (or every byte)."""
    assert np.array_equal(got_order, m_order), f"{what}: order differs at {np.flatnonzero(np.asarray(got_order) != np.asarray(m_order))[:8].tolist()}"
    assert len(got_records) == len(m_records), f"{what}: {len(got_records)} records, expected {len(m_records)}"
    for f in ("first", "count"):
        bad = np.flatnonzero(got_records[f] != m_records[f])
        assert bad.size == 0, f"{what}: {f} differs at records {bad[:8].tolist()} (of {bad.size})"
    for f in ("lo", "hi"):
        ok = (got_records[f] == m_records[f]) | (np.isnan(got_records[f]) & np.isnan(m_records[f]))
        bad = np.flatnonzero(~ok.all(axis=1))
        assert bad.size == 0, f"{what}: box {f} differs at records {bad[:8].tolist()} (of {bad.size})"
    if bytes_too:
        assert np.asarray(got_records).tobytes() == np.asarray(m_records).tobytes(), f"{what}: records differ in their bytes (a zero's sign)"


def chain_set(cluster=300, seed=25):
    """float32[144 + cluster, 3, 8]: small triangles at +-32^i on each axis, i = 1..24, and `cluster` small triangles with corners in
    [0, 1e-3]^3: every split peels a few far triangles off the cluster's bin, so the depth rule (svgf_sah.h, "replacement") acts."""
    rng = np.random.default_rng(seed)
    far = np.zeros((144, 3, 8), F)
    k = 0
    for i in range(1, 25):
        for axis in range(3):
            for sign in (-1.0, 1.0):
                far[k, :, 0:3] = rng.uniform(0, 1e-3, (3, 3)).astype(F)
                far[k, :, axis] += F(sign * 32.0 ** i)
                k += 1
    near = np.zeros((cluster, 3, 8), F)
    near[:, :, 0:3] = rng.uniform(0, 1e-3, (cluster, 3, 3)).astype(F)
    return np.concatenate([far, near])
