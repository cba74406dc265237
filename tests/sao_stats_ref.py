"""SAO parameter estimation: a per-sample numpy statement of the statistics hevcdbk_sao_stats_device gathers, and a plain-int
statement of the rule by which hevcdbk_sao_pick_device chooses hevcdbk_sao_ctb from them (include/hevc_deblock.h).

TEST INFRASTRUCTURE ONLY, parity unpinned like the rest of SAO.  Nothing of the library is mentioned here: the statistics are
stated per SAMPLE -- kept or not, its band, and per edge class whether both neighbours are available and which category it
falls in -- and the choice per CTB in Python ints.  The tests tie both to the SAO statements the suite already holds
(sao_borders_ref.sao_plane_by_bytes) through

    SSE(org, SAO(rec)) - SSE(org, rec) = sum over the bins the parameters use of (n o^2 - 2 o s)

which holds for ANY parameters on inputs where the final clip never acts.
"""
import numpy as np

import rext_oracle as ro
from sao_borders_ref import HV, NOX_BITS

STATS_DTYPE = np.dtype([("eo_count", "<i4", (4, 4)), ("eo_sum", "<i4", (4, 4)), ("bo_count", "<i4", (32,)), ("bo_sum", "<i4", (32,))])
assert STATS_DTYPE.itemsize == 384


def grid(w, h, lw, lh):
    """(rows, columns) of the CTB grid, by ceiling"""
    return -(-h >> lh), -(-w >> lw)


def stats_plane(rec, org, lw, lh, bit_depth, *, keep=None, nox=None):
    """the statistics of every CTB of one plane: (rows, cols) of STATS_DTYPE.  keep: one byte per 8x8 samples (by ceiling); nox:
    one HEVCDBK_SAO_NOX_* byte per CTB (columns beyond the grid are not looked at)"""
    rec = np.asarray(rec, np.int64)
    org = np.asarray(org, np.int64)
    h, w = rec.shape
    rows, cols = grid(w, h, lw, lh)
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = yy >> lh, xx >> lw
    ci = cy * cols + cx
    live = np.ones((h, w), bool) if keep is None else np.asarray(keep)[yy >> 3, xx >> 3] == 0
    byte = np.zeros((h, w), np.int64) if nox is None else np.asarray(nox, np.int64)[cy, cx]
    d = org - rec
    n = rows * cols

    def gather(sel, bins_per_ctb, bin_idx):
        at = (ci * bins_per_ctb + bin_idx)[sel]
        return (np.bincount(at, minlength=n * bins_per_ctb).reshape(rows, cols, bins_per_ctb),
                np.bincount(at, weights=d[sel].astype(np.float64), minlength=n * bins_per_ctb).round().astype(np.int64).reshape(rows, cols, bins_per_ctb))

    out = np.zeros((rows, cols), STATS_DTYPE)
    out["bo_count"], out["bo_sum"] = gather(live, 32, rec >> (bit_depth - 5))
    pad = np.pad(rec, 1, constant_values=-1)
    for k, nbs in HV.items():
        ok = live.copy()
        sign = np.zeros((h, w), np.int64)
        for dy, dx in nbs:
            ny, nx = yy + dy, xx + dx
            inside = (ny >= 0) & (ny < h) & (nx >= 0) & (nx < w)
            ncy, ncx = np.clip(ny, 0, h - 1) >> lh, np.clip(nx, 0, w - 1) >> lw
            bit = np.zeros((h, w), np.int64)       # the bit of THIS CTB's byte that speaks for the neighbour's CTB; 0 = the same CTB
            for (sy, sx), b in NOX_BITS.items():
                bit = np.where((np.sign(ncy - cy) == sy) & (np.sign(ncx - cx) == sx), b, bit)
            ok &= inside & ((byte & bit) == 0)
            sign += np.sign(rec - pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w])
        # edgeIdx = 2 + sign, remapped 0, 1, 2 -> 1, 2, 0 (8.7.3.2): categories 1 (valley), 2, 3, 4 (peak)
        cat = np.where(sign == -2, 1, np.where(sign == -1, 2, np.where(sign == 1, 3, np.where(sign == 2, 4, 0))))
        out["eo_count"][:, :, k, :], out["eo_sum"][:, :, k, :] = gather(ok & (cat > 0), 4, cat - 1)
    return out


# ---- the choice ---------------------------------------------------------------------------------------------------------------

def max_offset(bit_depth):
    return (1 << (min(bit_depth, 10) - 5)) - 1


def _bits(o, M, band):
    return (abs(o) + 1 if abs(o) < M else M) + (1 if band and o else 0)


def _offset(n, s, lo, hi, M, band, lam):
    """(o, cost, dd) of a bin"""
    if n == 0:
        return 0, lam * _bits(0, M, band), 0
    o0 = (2 * abs(s) + n) // (2 * n)
    o0 = min(max(-o0 if s < 0 else o0, lo), hi)
    best = None
    o = o0
    while True:
        dd = n * o * o - 2 * o * s
        c = dd * 256 + lam * _bits(o, M, band)
        if best is None or c <= best[1]:
            best = (o, c, dd)
        if o == 0:
            return best
        o += -1 if o > 0 else 1


def _bins(st, M, lam):
    """per component: edge[k][e] and band[b] as (o, cost, dd)"""
    edge = [[_offset(int(st["eo_count"][k][e]), int(st["eo_sum"][k][e]), 0 if e < 2 else -M, M if e < 2 else 0, M, False, lam) for e in range(4)]
            for k in range(4)]
    band = [_offset(int(st["bo_count"][b]), int(st["bo_sum"][b]), -M, M, M, True, lam) for b in range(32)]
    return edge, band


def pick_ctb(st_a, st_b, bit_depth, lam):
    """the choice of one CTB from its statistics (st_b: Cr beside Cb, or None): ((type, cls, offsets) per component, delta_d)"""
    M = max_offset(bit_depth)
    comps = [_bins(s, M, lam) for s in ((st_a,) if st_b is None else (st_a, st_b))]

    def edge(c, k):
        return c[0][k]

    def band(c, p):
        return [c[1][(p + j) & 31] for j in range(4)]

    cands = [(lam * 1, (0, None))]
    for k in range(4):
        cands.append((lam * 4 + sum(b[1] for c in comps for b in edge(c, k)), (2, k)))
    if st_b is None:
        for p in range(32):
            cands.append((lam * 7 + sum(b[1] for b in band(comps[0], p)), (1, (p,))))
    else:
        pos, cost = [], lam * 2
        for c in comps:
            costs = [sum(b[1] for b in band(c, p)) for p in range(32)]
            pos.append(costs.index(min(costs)))
            cost += lam * 5 + min(costs)
        cands.append((cost, (1, tuple(pos))))
    costs = [c[0] for c in cands]
    typ, arg = cands[costs.index(min(costs))][1]
    out, dd = [], 0
    for i, c in enumerate(comps):
        if typ == 0:
            out.append((0, 0, (0, 0, 0, 0)))
            continue
        chosen = edge(c, arg) if typ == 2 else band(c, arg[i])
        out.append((typ, arg if typ == 2 else arg[i], tuple(b[0] for b in chosen)))
        dd += sum(b[2] for b in chosen)
    return out, dd


def pick_plane(stats_a, stats_b, bit_depth, lam):
    """pick_ctb over a grid: (params_a, params_b or None, delta_d)"""
    rows, cols = stats_a.shape
    pa, pb = np.zeros((rows, cols), ro.SAO_CTB_DTYPE), None if stats_b is None else np.zeros((rows, cols), ro.SAO_CTB_DTYPE)
    dd = np.zeros((rows, cols), np.int64)
    for r in range(rows):
        for c in range(cols):
            out, dd[r, c] = pick_ctb(stats_a[r, c], None if stats_b is None else stats_b[r, c], bit_depth, lam)
            for p, o in zip((pa, pb), out):
                p[r, c] = (o[0], o[1], o[2])
    return pa, pb, dd


def predicted_delta(stats, params):
    """sum over the bins the parameters use of (n o^2 - 2 o s), per CTB"""
    rows, cols = stats.shape
    out = np.zeros((rows, cols), np.int64)
    for r in range(rows):
        for c in range(cols):
            p, st = params[r, c], stats[r, c]
            for j in range(4):
                o = int(p["offset"][j])
                if p["type"] == 2:
                    n, s = int(st["eo_count"][p["cls"] & 3][j]), int(st["eo_sum"][p["cls"] & 3][j])
                elif p["type"] == 1:
                    n, s = int(st["bo_count"][(p["cls"] + j) & 31]), int(st["bo_sum"][(p["cls"] + j) & 31])
                else:
                    continue
                out[r, c] += n * o * o - 2 * o * s
    return out


def sse_per_ctb(org, plane, lw, lh):
    d = np.asarray(org, np.int64) - np.asarray(plane, np.int64)
    h, w = d.shape
    rows, cols = grid(w, h, lw, lh)
    yy, xx = np.mgrid[0:h, 0:w]
    # int64 sums: (2^16)^2 * 2^12 per CTB is far inside
    out = np.zeros(rows * cols, np.int64)
    np.add.at(out, ((yy >> lh) * cols + (xx >> lw)).ravel(), (d * d).ravel())
    return out.reshape(rows, cols)


# ---- vectors ------------------------------------------------------------------------------------------------------------------

def planes(w, h, bit_depth, rng, *, n=1):
    """(rec, org), n frames each: blocky 8x8 content (a step at every x % 8 == 0 and y % 8 == 0) over the whole range plus noise; rec =
    org + coding noise + a bias per 8x8 block.  Every sample of rec stays one band plus M away from 0 and max: no offset |o| <= M
    ever reaches the clip"""
    max_v, band, M = (1 << bit_depth) - 1, 1 << (bit_depth - 5), max_offset(bit_depth)
    margin = band + M
    bh, bw = -(-h // 8), -(-w // 8)
    base = np.kron(rng.integers(margin, max_v - margin + 1, (n, bh, bw)), np.ones((8, 8), np.int64))[:, :h, :w]
    org = np.clip(base + rng.integers(-band, band + 1, (n, h, w)), margin, max_v - margin)
    bias = np.kron(rng.integers(-M, M + 1, (n, bh, bw)), np.ones((8, 8), np.int64))[:, :h, :w]
    rec = np.clip(org + rng.integers(-M, M + 1, (n, h, w)) + bias, margin, max_v - margin)
    dt = np.uint8 if bit_depth == 8 else np.uint16
    return rec.astype(dt), org.astype(dt)


def keep_map(w, h, rng):
    return (rng.integers(0, 6, (-(-h // 8), -(-w // 8))) == 0).astype(np.uint8)


# name -> (w, h, bit depth, log2 CTB width, log2 CTB height): the shapes the identity was first checked on
SHAPES = {"8b_72x40_ctb16": (72, 40, 8, 4, 4), "8b_68x36_ctb32": (68, 36, 8, 5, 5), "10b_96x136_ctb32x64": (96, 136, 10, 5, 6),
          "12b_136x72_ctb64": (136, 72, 12, 6, 6)}


# the vectors of tests/test_gpu_sao_stats.py (tests/sao_stats_sim walks the same): the four above, several workgroups with a cut last
# CTB, samples deeper than 12 bit, and a plane whose pitch is an odd number of samples
GPU_SHAPES = dict(SHAPES, **{"8b_200x136_ctb64": (200, 136, 8, 6, 6), "14b_72x40_ctb16": (72, 40, 14, 4, 4), "10b_76x44_ctb32_odd_pitch": (76, 44, 10, 5, 5)})


def pitch_of(name):
    """samples per row of the vector's planes in memory"""
    w = GPU_SHAPES[name][0]
    return w + 5 if name.endswith("odd_pitch") else w


def vector(name, seed=0):
    w, h, bd, lw, lh = GPU_SHAPES[name]
    rng = np.random.default_rng([seed, w, h, bd])
    rec, org = planes(w, h, bd, rng)
    rows, cols = grid(w, h, lw, lh)
    return {"w": w, "h": h, "bd": bd, "lw": lw, "lh": lh, "rec": rec[0], "org": org[0], "keep": keep_map(w, h, rng),
            "nox": rng.integers(0, 256, (rows, cols)).astype(np.uint8), "rng": rng}
