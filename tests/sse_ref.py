"""Measured distortion, stated plainly: what hevcdbk_sse_device, hevcdbk_sse_device_sp and hevcdbk_sse_totals_device compute, in Python
integers and numpy uint64.  A square of a 16-bit difference is below 2^32 and a CTB holds at most 4096 of them, so a uint64 sum per
CTB is exact; the totals are sums modulo 2^64 by definition."""
import numpy as np

MASK64 = (1 << 64) - 1
MAX_SLICES = 600


def grid(w, h, lw, lh):
    """(CTB rows, CTB columns) of a plane, by ceiling"""
    return (h + (1 << lh) - 1) >> lh, (w + (1 << lw) - 1) >> lw


def sse_plane(rec, org, lw, lh):
    """(h, w) samples each -> (rows, cols) uint64: the sum of (org - rec)^2 over the samples of each CTB inside the plane"""
    rec, org = np.asarray(rec), np.asarray(org)
    assert rec.shape == org.shape and rec.ndim == 2
    d = org.astype(np.int64) - rec.astype(np.int64)
    sq = (d * d).astype(np.uint64)
    h, w = rec.shape
    rows, cols = grid(w, h, lw, lh)
    out = np.zeros((rows, cols), np.uint64)
    for cy in range(rows):
        for cx in range(cols):
            out[cy, cx] = sq[cy << lh: (cy + 1) << lh, cx << lw: (cx + 1) << lw].sum(dtype=np.uint64)
    return out


def sse_plane_loop(rec, org, lw, lh):
    """the same, sample by sample in Python integers"""
    h, w = np.asarray(rec).shape
    rows, cols = grid(w, h, lw, lh)
    out = [[0] * cols for _ in range(rows)]
    r, o = np.asarray(rec).tolist(), np.asarray(org).tolist()
    for y in range(h):
        for x in range(w):
            d = o[y][x] - r[y][x]
            out[y >> lh][x >> lw] += d * d
    return np.array(out, dtype=object)


def sse_pairs(rec, org, lg):
    """(h, 2 w) samples each, interleaved pairs -> (Cb's, Cr's): sse_plane of the even samples and of the odd samples"""
    rec, org = np.asarray(rec), np.asarray(org)
    return sse_plane(rec[:, 0::2], org[:, 0::2], lg, lg), sse_plane(rec[:, 1::2], org[:, 1::2], lg, lg)


def totals(sse, slice_idx, n_slices):
    """sse (rows, cols) uint64, slice_idx (rows, cols) or None (every CTB in slice 0) -> (slice totals (n_slices,) uint64, frame total):
    sums modulo 2^64; a CTB whose index is >= n_slices counts for the frame alone"""
    sse = np.asarray(sse)
    rows, cols = sse.shape
    st, ft = [0] * n_slices, 0
    for cy in range(rows):
        for cx in range(cols):
            v = int(sse[cy, cx])
            ft = (ft + v) & MASK64
            s = 0 if slice_idx is None else int(slice_idx[cy][cx])
            if s < n_slices:
                st[s] = (st[s] + v) & MASK64
    return np.array(st, np.uint64), np.uint64(ft)


def load_mode(sample_bytes, *operands):
    """the load path the entries choose from the addresses, pitches and frame strides (bytes) of both planes: 2 = 16 bytes per load,
    1 = four samples per load, 0 = sample by sample"""
    if all(v % 16 == 0 for v in operands):
        return 2
    return 1 if all(v % (4 * sample_bytes) == 0 for v in operands) else 0


def planes(w, h, bd, rng, n=1, err=None):
    """n frames of (rec, org): org anywhere in the depth's range, rec = org + an error of at most +-err (default: a quarter of the
    range) clipped to the range -- so that samples at both ends and errors of both signs occur"""
    hi = (1 << bd) - 1
    err = max(hi // 4, 1) if err is None else err
    dt = np.uint8 if bd == 8 else np.uint16
    org = rng.integers(0, hi + 1, (n, h, w))
    rec = np.clip(org + rng.integers(-err, err + 1, (n, h, w)), 0, hi)
    return rec.astype(dt), org.astype(dt)
