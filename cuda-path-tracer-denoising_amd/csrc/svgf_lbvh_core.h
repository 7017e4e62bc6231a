// svgf_lbvh_core.h — row f24: the arithmetic of include/svgf_lbvh.h's normative text, shared as text by the device builder
// (svgf_lbvh.hip) and the host builder (svgf_lbvh_host.cpp, which a plain C++ compiler builds too): the bit budget, a triangle's key
// and one internal node of the Karras radix tree.  float32, contraction off (the build passes -ffp-contract=off as well).
#ifndef SVGF_LBVH_CORE_H_
#define SVGF_LBVH_CORE_H_

#if defined(__HIPCC__)
#define SVGF_LBVH_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SVGF_LBVH_HD inline
#endif

typedef unsigned long long lbvh_key;

struct LbvhBits { int idx_bits, axis_bits, key_bits; };

SVGF_LBVH_HD LbvhBits lbvh_bits(int n_tris)
{
    LbvhBits b;
    b.idx_bits = 1;
    while ((1 << b.idx_bits) < n_tris) b.idx_bits++;
    b.axis_bits = (48 - b.idx_bits) / 3 < 10 ? (48 - b.idx_bits) / 3 : 10;
    b.key_bits = 3 * b.axis_bits + b.idx_bits;
    return b;
}

SVGF_LBVH_HD int lbvh_passes(int key_bits) { return (key_bits + 7) / 8; }

SVGF_LBVH_HD float lbvh_centroid(float lo, float hi)
{
#pragma clang fp contract(off)
    return (lo + hi) * 0.5f;
}

// the cell of centroid c on one axis; M = 2^axis_bits
SVGF_LBVH_HD int lbvh_cell(float c, float bmin, float bmax, int M)
{
#pragma clang fp contract(off)
    const float ext = bmax - bmin;
    const float q = (ext > 0.0f) ? (c - bmin) / ext : 0.0f;
    const float v = q * (float)M;
    return !(v >= 0.0f) ? 0 : (v >= (float)(M - 1) ? M - 1 : (int)v);
}

// bit 3j + 2 = x's bit j, bit 3j + 1 = y's, bit 3j = z's
SVGF_LBVH_HD lbvh_key lbvh_morton(int cx, int cy, int cz, int axis_bits)
{
    lbvh_key m = 0;
    for (int j = 0; j < axis_bits; j++)
        m |= ((lbvh_key)((cx >> j) & 1) << (3 * j + 2)) | ((lbvh_key)((cy >> j) & 1) << (3 * j + 1)) | ((lbvh_key)((cz >> j) & 1) << (3 * j));
    return m;
}

SVGF_LBVH_HD lbvh_key lbvh_make_key(const float lo[3], const float hi[3], const float bmin[3], const float bmax[3], LbvhBits b, int i)
{
    int cell[3];
    for (int c = 0; c < 3; c++) cell[c] = lbvh_cell(lbvh_centroid(lo[c], hi[c]), bmin[c], bmax[c], 1 << b.axis_bits);
    return (lbvh_morton(cell[0], cell[1], cell[2], b.axis_bits) << b.idx_bits) | (lbvh_key)i;
}

// delta(i, j): the common-prefix length of leaf keys i and j within key_bits; -1 for j outside [0, n_leaves).  key(k) = leaf k's key;
// the keys are distinct, so for j != i the xor is not zero and the result is at most key_bits - 1.
template <class Key>
SVGF_LBVH_HD int lbvh_delta(const Key &key, int n_leaves, int key_bits, lbvh_key ki, int j)
{
    if (j < 0 || j >= n_leaves) return -1;
    const lbvh_key x = ki ^ key(j);
    if (x == 0) return key_bits;          // j == i only
    return __builtin_clzll(x) - (64 - key_bits);
}

// Internal node i (0 <= i < n_leaves - 1) of the radix tree: its leaf range [lo, hi] (i is one end of it) and its split gamma - the
// left child covers [lo, gamma] (the leaf gamma where lo == gamma, else internal node gamma), the right one [gamma + 1, hi] (the leaf
// gamma + 1 where that is hi, else internal node gamma + 1).  Karras 2012, algorithm of figure 4; every probe stays inside the array
// through delta's -1.
template <class Key>
SVGF_LBVH_HD void lbvh_node(const Key &key, int n_leaves, int key_bits, int i, int &lo, int &hi, int &gamma)
{
    const lbvh_key ki = key(i);
    const int d = lbvh_delta(key, n_leaves, key_bits, ki, i + 1) - lbvh_delta(key, n_leaves, key_bits, ki, i - 1) > 0 ? 1 : -1;
    const int dmin = lbvh_delta(key, n_leaves, key_bits, ki, i - d);
    int lmax = 2;
    while (lmax < 2 * n_leaves && lbvh_delta(key, n_leaves, key_bits, ki, i + lmax * d) > dmin) lmax *= 2;
    int l = 0;
    for (int t = lmax / 2; t >= 1; t /= 2)
        if (lbvh_delta(key, n_leaves, key_bits, ki, i + (l + t) * d) > dmin) l += t;
    const int j = i + l * d;
    const int dnode = lbvh_delta(key, n_leaves, key_bits, ki, j);
    int s = 0;
    for (int t = (l + 1) / 2;; t = (t + 1) / 2) {
        if (lbvh_delta(key, n_leaves, key_bits, ki, i + (s + t) * d) > dnode) s += t;
        if (t <= 1) break;
    }
    gamma = i + s * d + (d < 0 ? -1 : 0);
    lo = i < j ? i : j;
    hi = i < j ? j : i;
}

#endif
