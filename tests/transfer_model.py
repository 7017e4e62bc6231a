"""The float32 numpy model of the history transfer (include/svgf.h: svgf_transfer_history; csrc/svgf_transfer.hip:
k_transfer_history) - the yardstick of tests/test_history_transfer.py.  Test infrastructure only; not part of the package.

The state is the dict of temporal_model.empty_state (hlen, mom, color, normal, position, gid): what a context's next frame reads as
history, i.e. svgf_read_state kinds 0, 1, 2, 5, 6, 7.  The output history of svgf_set_output_taa is the pair (rgb, gid) of
taa_model.output_taa, i.e. kind 8 split into its colour and its geomId bits.

numpy rounds every array operation to float32 and never contracts a multiply and an add; sums are written as the kernel's
sequences of additions, in its order (taps k = 0..3)."""
import numpy as np

F = np.float32


def axis(n_d, n_s):
    """Per dst index: (floor of the src coordinate int64, fraction float32, anchor int64):
    u = ((float)i + 0.5f) * r - 0.5f, r = (float)n_s / (float)n_d; anchor = clamp(floor(u + 0.5f), 0, n_s - 1)."""
    r = F(n_s) / F(n_d)
    u = (np.arange(n_d).astype(F) + F(0.5)) * r - F(0.5)
    f = np.floor(u)
    a = np.clip(np.floor(u + F(0.5)).astype(np.int64), 0, n_s - 1)
    return f.astype(np.int64), (u - f).astype(F), a


def anchors(Ws, Hs, Wd, Hd):
    """(ya int64[Hd, 1], xa int64[1, Wd]): the src texel each dst pixel copies its G-buffer and history length from."""
    return axis(Hd, Hs)[2][:, None], axis(Wd, Ws)[2][None, :]


def _gather(gid_s, planes, Wd, Hd):
    """planes: list of float32[Hs, Ws, C].  Per plane the mean of the counted taps, or the anchor's value where sumw fails the test."""
    Hs, Ws = gid_s.shape
    fx, ax, xa = axis(Wd, Ws)
    fy, ay, ya = axis(Hd, Hs)
    fx, ax, xa, fy, ay, ya = fx[None, :], ax[None, :], xa[None, :], fy[:, None], ay[:, None], ya[:, None]
    one = F(1)
    w = [(one - ax) * (one - ay), ax * (one - ay), (one - ax) * ay, ax * ay]
    g = gid_s[ya, xa]
    acc = [np.zeros((Hd, Wd, p.shape[-1]), F) for p in planes]
    sumw = np.zeros((Hd, Wd), F)
    for k in range(4):
        tx, ty = fx + (k & 1), fy + (k >> 1)
        inside = np.broadcast_to((tx >= 0) & (tx < Ws) & (ty >= 0) & (ty < Hs), (Hd, Wd))
        qx, qy = np.broadcast_to(np.clip(tx, 0, Ws - 1), (Hd, Wd)), np.broadcast_to(np.clip(ty, 0, Hs - 1), (Hd, Wd))
        counted = inside & (gid_s[qy, qx] == g)
        wk = np.broadcast_to(w[k], (Hd, Wd)).astype(F)
        for i, p in enumerate(planes):
            acc[i] = np.where(counted[..., None], acc[i] + wk[..., None] * p[qy, qx], acc[i])
        sumw = np.where(counted, sumw + wk, sumw)
    ok = sumw.astype(np.float64) >= 0.01      # NaN fails
    return [np.where(ok[..., None], a / sumw[..., None], p[ya, xa]).astype(F) for a, p in zip(acc, planes)]


def transfer(state, Wd, Hd):
    """The state a context of Wd x Hd holds after svgf_transfer_history from a context holding `state`."""
    gid_s = np.asarray(state["gid"], np.int32)
    Hs, Ws = gid_s.shape
    if (Ws, Hs) == (Wd, Hd):      # the identity: bit copies
        return {k: np.array(v, copy=True) for k, v in state.items()}
    ya, xa = anchors(Ws, Hs, Wd, Hd)
    with np.errstate(all="ignore"):
        color, mom = _gather(gid_s, [np.asarray(state["color"], F), np.asarray(state["mom"], F)], Wd, Hd)
    return dict(hlen=np.asarray(state["hlen"], np.int32)[ya, xa].copy(), mom=mom, color=color,
                normal=np.asarray(state["normal"], F)[ya, xa].copy(), position=np.asarray(state["position"], F)[ya, xa].copy(),
                gid=gid_s[ya, xa].copy())


def transfer_output_history(prev, Wd, Hd):
    """prev: (rgb float32[Hs, Ws, 3], gid int32[Hs, Ws]), the output history with the geomId stored with it; the same pair at Wd x Hd."""
    rgb, gid_s = np.asarray(prev[0], F), np.asarray(prev[1], np.int32)
    Hs, Ws = gid_s.shape
    if (Ws, Hs) == (Wd, Hd):
        return rgb.copy(), gid_s.copy()
    ya, xa = anchors(Ws, Hs, Wd, Hd)
    with np.errstate(all="ignore"):
        out, = _gather(gid_s, [rgb], Wd, Hd)
    return out, gid_s[ya, xa].copy()
