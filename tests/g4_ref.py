"""Planes sized in multiples of 4, not 8 (the _g4 entries: the 960x540 chroma planes of a 1920x1080 picture): vectors, the two
statements of what is expected, and the census that keeps a test from passing vacuously.

TEST INFRASTRUCTURE ONLY, PARITY UNPINNED like the rest of the spec-exact mode.  Nothing here is new arithmetic:
  statement 1  tests/rext_oracle.py (filter_chroma_plane, sao_plane) applied to the g4 plane as it is -- the file states 8.7.2 and
               8.7.3 for any plane size: edges at x = 8k, 0 < x < cw, a neighbour outside the h x w array is outside the picture;
               slice / tile borders through tests/sao_borders_ref.py, per-slice offsets through tests/slice_offsets_ref.py;
  statement 2  for 4:2:0, the C oracle (oracle/h265.py filter_plane, c_idx 1), which demands multiples of 8, by PAD AND CROP: the
               plane embedded in the next multiple of 8 with arbitrary content in the pad, the bS arrays embedded in the larger
               layout with arbitrary pad entries, filtered, cropped.  Exact, because segments are 4 samples long -- pad rows and
               columns form segments of their own -- the edge at 8 (W / 8) reads real samples only, and the padded plane's own
               boundary is never filtered.
For SAO padding is NOT exact -- 8.7.3.2 copies a sample whose neighbour is outside the picture, and in a padded plane the last row
and column have neighbours -- which is what padded_sao() is here to show: the census demands samples that the padded plane would
change and the g4 plane copies.
"""
import numpy as np

import rext_oracle as rx
import sao_borders_ref as B
import slice_offsets_ref as R

KEEP_P, KEEP_Q = 4, 8


def pad8(n):
    return (n + 7) // 8 * 8


def is_g4(w, h):
    return w >= 8 and h >= 8 and w % 4 == 0 and h % 4 == 0 and (w % 8 != 0 or h % 8 != 0)


def num_vert_bs(w, h):
    return (w // 8 + 1) * (h // 4)


def num_hor_bs(w, h):
    return (h // 8 + 1) * (w // 4)


# ---- content and operands -------------------------------------------------------------------------------------------------

def blocky_plane(w, h, depth, rng, step=None):
    """8 x 8 blocks of a constant each plus a little noise: steps at every edge of the 8-sample grid that the chroma filter moves"""
    maxv = (1 << depth) - 1
    step = (6 << (depth - 8)) if step is None else step
    by, bx = (h + 7) // 8, (w + 7) // 8
    base = rng.integers(maxv // 4, 3 * maxv // 4, (by, bx))
    base = base // max(step, 1) * max(step, 1)
    p = np.repeat(np.repeat(base, 8, 0), 8, 1)[:h, :w] + rng.integers(-step, step + 1, (h, w))
    return np.clip(p, 0, maxv).astype(np.uint8 if depth == 8 else np.uint16)


def noise_plane(w, h, depth, rng):
    return rng.integers(0, 1 << depth, (h, w)).astype(np.uint8 if depth == 8 else np.uint16)


def random_bs(w, h, rng, p2=0.6, p_keep=0.15):
    """4-sample-granular arrays of a w x h plane, every entry random -- the picture-boundary entries too, which nobody may read as
    an edge -- with KEEP flags, and KEEP_P / KEEP_Q on units of the last column and row of entries"""
    def draw(n):
        bs = np.where(rng.random(n) < p2, 2, rng.integers(0, 2, n))
        keep = np.where(rng.random(n) < p_keep, KEEP_P, 0) | np.where(rng.random(n) < p_keep, KEEP_Q, 0)
        return (bs | keep).astype(np.uint8)
    vb = draw(num_vert_bs(w, h)).reshape(h // 4, w // 8 + 1)
    hb = draw(num_hor_bs(w, h)).reshape(h // 8 + 1, w // 4)
    if (w // 8) * 8 < w and h >= 8:   # the new last vertical edge: a kept Q unit (4 x 4 samples) and a kept P unit on it
        vb[0, w // 8] = 2 | KEEP_Q
        vb[1, w // 8] = 2 | KEEP_P
    if (h // 8) * 8 < h and w >= 8:
        hb[h // 8, 0] = 2 | KEEP_Q
        hb[h // 8, 1] = 2 | KEEP_P
    return vb.ravel(), hb.ravel()


def random_qp_map(w, h, cf, unit_log2, rng, lo=20, hi=45):
    """QpY per (1 << unit_log2) luma samples of the picture whose chroma plane is w x h"""
    sx, sy = rx.SUB[cf]
    lw, lh = w * sx, h * sy
    return rng.integers(lo, hi + 1, (-(-lh >> unit_log2), -(-lw >> unit_log2))).astype(np.uint8)


# ---- deblocking: the two statements ---------------------------------------------------------------------------------------------

def deblock_direct(plane, vb, hb, cf, *, qp, qp_map=None, unit_log2=3, bit_depth=8, c_qp_offset=0, tc_offset_div2=0):
    """statement 1"""
    return rx.filter_chroma_plane(plane, vb, hb, cf, qp=qp, qp_map=qp_map, unit_log2=unit_log2, bit_depth=bit_depth,
                                  c_qp_offset=c_qp_offset, tc_offset_div2=tc_offset_div2)


def embed_plane(plane, rng, bit_depth):
    h, w = plane.shape
    out = rng.integers(0, 1 << bit_depth, (pad8(h), pad8(w))).astype(plane.dtype)
    out[:h, :w] = plane
    return out


def embed_bs(vb, hb, w, h, rng):
    """the arrays of the w x h plane inside those of the plane padded to multiples of 8, arbitrary entries elsewhere"""
    W, H = pad8(w), pad8(h)
    v = rng.integers(0, 16, (H // 4, W // 8 + 1)).astype(np.uint8)
    hh = rng.integers(0, 16, (H // 8 + 1, W // 4)).astype(np.uint8)
    v[: h // 4, : w // 8 + 1] = np.asarray(vb, np.uint8).reshape(h // 4, w // 8 + 1)
    hh[: h // 8 + 1, : w // 4] = np.asarray(hb, np.uint8).reshape(h // 8 + 1, w // 4)
    return v.ravel(), hh.ravel()


def embed_grid(a, rows, cols, rng, lo, hi):
    """a 2-D (or (rows, cols, k)) array inside a larger one of arbitrary entries lo..hi"""
    a = np.asarray(a)
    out = rng.integers(lo, hi + 1, (rows, cols) + a.shape[2:]).astype(a.dtype)
    out[: a.shape[0], : a.shape[1]] = a
    return out


def deblock_padcrop(plane, vb, hb, *, qp, qp_map=None, unit_log2=3, bit_depth=8, c_qp_offset=0, tc_offset_div2=0, seed=1):
    """statement 2 (4:2:0 only): the C oracle on the padded plane, cropped"""
    from oracle import h265
    rng = np.random.default_rng(seed)
    h, w = plane.shape
    big = embed_plane(plane, rng, bit_depth)
    v, hh = embed_bs(vb, hb, w, h, rng)
    m = None
    if qp_map is not None:
        m = embed_grid(qp_map, -(-2 * pad8(h) >> unit_log2), -(-2 * pad8(w) >> unit_log2), rng, 0, 51)
    out = h265.filter_plane(big, qp, v, hh, c_idx=1, bit_depth=bit_depth, qp_map=m, unit_log2=unit_log2,
                            tc_offset_div2=tc_offset_div2, c_qp_offset=c_qp_offset)
    return out[:h, :w].copy()


def deblock_sl(plane, vb, hb, cf, pairs, ctb_log2, *, qp, qp_map=None, unit_log2=3, bit_depth=8, c_qp_offset=0, seed=1):
    """per-slice offsets: the composition of tests/slice_offsets_ref.py -- as it is for 4:2:2 / 4:4:4 (it runs rext_oracle there),
    by pad and crop for 4:2:0 (it runs the C oracle there); pairs = (rows, cols, 2) of the LUMA CTB grid"""
    if cf != 1:
        return R.expected(plane, vb, hb, pairs, ctb_log2, qp=qp, c_idx=1, chroma_format=cf, qp_map=qp_map, unit_log2=unit_log2,
                          bit_depth=bit_depth, c_qp_offset=c_qp_offset)
    rng = np.random.default_rng(seed)
    h, w = plane.shape
    big = embed_plane(plane, rng, bit_depth)
    v, hh = embed_bs(vb, hb, w, h, rng)
    LW, LH = 2 * pad8(w), 2 * pad8(h)
    m = None if qp_map is None else embed_grid(qp_map, -(-LH >> unit_log2), -(-LW >> unit_log2), rng, 0, 51)
    pp = embed_grid(pairs, -(-LH >> ctb_log2), -(-LW >> ctb_log2), rng, -6, 6)
    out = R.expected(big, v, hh, pp, ctb_log2, qp=qp, c_idx=1, chroma_format=1, qp_map=m, unit_log2=unit_log2, bit_depth=bit_depth,
                     c_qp_offset=c_qp_offset)
    return out[:h, :w].copy()


def new_edge_changes(src, out):
    """(samples changed in the two columns at the new last vertical edge, in the two rows at the new last horizontal edge); 0 for
    a direction whose size is a multiple of 8"""
    h, w = src.shape
    d = np.asarray(src) != np.asarray(out)
    ex, ey = (w // 8) * 8, (h // 8) * 8
    cols = int(d[:, ex - 1: ex + 1].sum()) if ex < w else 0
    rows = int(d[ey - 1: ey + 1, :].sum()) if ey < h else 0
    return cols, rows


# ---- SAO --------------------------------------------------------------------------------------------------------------------

def ctb_grid(w, h, lw, lh):
    return -(-h >> lh), -(-w >> lw)


def keep_map(w, h, rng, p=0.12):
    """one byte per 8 x 8 samples, ceil(h / 8) x ceil(w / 8): the last byte of a row / column of a g4 plane speaks for 4 samples;
    one of those is set"""
    k = (rng.random(((h + 7) // 8, (w + 7) // 8)) < p).astype(np.uint8)
    if k.shape[0] > 1 and k.shape[1] > 1:
        k[-1, 0] = 1
        k[0, -1] = 1
    return k


def border_params(w, h, lw, lh, depth, frames, rng):
    """parameters per frame, constructed (random ones change nothing in the last row or column of small planes): the CTBs on the
    bottom and on the right border run through edge class 0, 1, 2, 3 and band offset -- CTB i of a border in frame f is kind
    (i + f) % 5 -- so that with five frames every border CTB has been everything; the others random.  Offsets are never zero."""
    rows, cols = ctb_grid(w, h, lw, lh)
    shift = min(max(depth - 10, 0), 4)   # above 14 bit: as far as the int8 entry holds the scaled value
    out = []
    for f in range(frames):
        p = rx.random_sao_params(w, h, lw, lh, rng, depth)
        border = [(rows - 1, i, i) for i in range(cols)] + [(i, cols - 1, cols + i) for i in range(rows - 1)]
        for (r, c, i) in border:
            kind = (i + f) % 5
            big = int((3 + (i % 4)) << shift)
            if kind == 4:
                p[r, c] = (1, 0, (big, -big, big, -big))   # band: the position is set by fit_bands()
            else:
                p[r, c] = (2, kind, (big, big, -big, -big))
        out.append(p)
    return out


def fit_bands(planes, params, lw, lh, depth):
    """band position of every band-offset CTB on the bottom / right border := the band of its last sample, so that the last row
    and column get an offset"""
    for pl, p in zip(planes, params):
        h, w = pl.shape
        rows, cols = p.shape
        for r in range(rows):
            for c in range(cols):
                if p[r, c]["type"] == 1 and (r == rows - 1 or c == cols - 1):
                    y = min(((r + 1) << lh), h) - 1
                    x = min(((c + 1) << lw), w) - 1
                    p[r, c]["cls"] = (int(pl[y, x]) >> (depth - 5)) & 31


def sao_direct(plane, params, lw, lh, *, bit_depth=8, keep=None, layout=None):
    if layout is None:
        return rx.sao_plane(plane, params, lw, lh, bit_depth=bit_depth, keep=keep)
    return B.sao_plane(plane, params, lw, lh, layout, bit_depth=bit_depth, keep=keep)


def padded_sao(plane, params, lw, lh, *, bit_depth=8, seed=3):
    """what a caller would get who padded the plane to a multiple of 8 (arbitrary pad content, the parameters' grid extended by
    repeating its last row / column), cropped: NOT what 8.7.3 says for the g4 plane"""
    rng = np.random.default_rng(seed)
    h, w = plane.shape
    big = embed_plane(plane, rng, bit_depth)
    rows, cols = ctb_grid(pad8(w), pad8(h), lw, lh)
    p = np.asarray(params)
    p = np.pad(p, ((0, rows - p.shape[0]), (0, cols - p.shape[1])), mode="edge")
    return rx.sao_plane(big, p, lw, lh, bit_depth=bit_depth)[:h, :w]


LOOKS_DOWN, LOOKS_RIGHT = (1, 2, 3), (0, 2, 3)


def sao_census(planes, params, lw, lh, depth):
    """what a set of frames (planes before SAO, per-frame parameters; no keep map, no borders) exercises at the picture edge:
      band_row / band_col        samples of band-offset CTBs in the last row / column that change
      copied_row[c] / copied_col[c]   samples of edge-offset CTBs of class c in the last row / column that the g4 plane copies
                                      and the plane padded to a multiple of 8 would change"""
    cen = {"band_row": 0, "band_col": 0, "copied_row": {c: 0 for c in range(4)}, "copied_col": {c: 0 for c in range(4)}}
    for pl, p in zip(planes, params):
        h, w = pl.shape
        want = sao_direct(pl, p, lw, lh, bit_depth=depth)
        padded = padded_sao(pl, p, lw, lh, bit_depth=depth)
        yy, xx = np.mgrid[0:h, 0:w]
        typ = p["type"][yy >> lh, xx >> lw]
        cls = p["cls"][yy >> lh, xx >> lw]
        last_row, last_col = yy == h - 1, xx == w - 1
        changed = want != pl
        cen["band_row"] += int((changed & (typ == 1) & last_row).sum())
        cen["band_col"] += int((changed & (typ == 1) & last_col).sum())
        differs = (padded != pl) & ~changed
        for c in range(4):
            cen["copied_row"][c] += int((differs & (typ == 2) & (cls == c) & last_row).sum())
            cen["copied_col"][c] += int((differs & (typ == 2) & (cls == c) & last_col).sum())
    return cen


def census_ok(cen, w, h):
    """the conditions every SAO case must meet on its expectation (in the directions in which the plane is not a multiple of 8 the
    difference to padding is demanded; the band offset in both)"""
    if not (cen["band_row"] > 0 and cen["band_col"] > 0):
        return False
    if h % 8 and not all(cen["copied_row"][c] > 0 for c in LOOKS_DOWN):
        return False
    if w % 8 and not all(cen["copied_col"][c] > 0 for c in LOOKS_RIGHT):
        return False
    return True


# ---- cases -------------------------------------------------------------------------------------------------------------------

# (name, plane width, plane height, bit depth, chroma_format_idc, QP map?, log2 of the SAO CTB width)
SMALL = [("12x12", 12, 12, 8, 1, False, 3), ("20x28", 20, 28, 8, 1, True, 3), ("28x20", 28, 20, 10, 1, True, 4),
         ("36x36_10", 36, 36, 10, 1, False, 4), ("64x44", 64, 44, 8, 1, True, 5), ("44x64_10", 44, 64, 10, 1, True, 5)]
WIDE = [("516x36", 516, 36, 8, 1, False, 5), ("2052x20", 2052, 20, 8, 1, True, 6), ("4100x12", 4100, 12, 10, 1, True, 6),
        ("8196x20", 8196, 20, 8, 1, False, 6)]
TILES8 = [("196x132", 196, 132, 8, 1, True, 5), ("388x124", 388, 124, 8, 1, False, 6), ("188x260", 188, 260, 8, 1, True, 4)]
TILES16 = [("132x132_10", 132, 132, 10, 1, True, 5), ("260x124_12", 260, 124, 12, 1, False, 6)]
P1080 = [("960x540_8", 960, 540, 8, 1, False, 5), ("960x540_8m", 960, 540, 8, 1, True, 5), ("960x540_10m", 960, 540, 10, 1, True, 5),
         ("960x540_12", 960, 540, 12, 1, True, 5)]
FORMATS = [("422_964x24", 964, 24, 8, 2, True, 4), ("422_964x24_10", 964, 24, 10, 2, False, 5), ("444_20x28", 20, 28, 8, 3, True, 3),
           ("444_20x28_10", 20, 28, 10, 3, False, 4)]
CASES = SMALL + WIDE + TILES8 + TILES16 + P1080 + FORMATS
# 4:2:2 / 4:4:4 planes just over 512 blocks per row, two block rows: the packed kernels' row-major map in the formats' own kernels
WIDE_FORMATS = [("422_4100x12", 4100, 12, 8, 2, True, 6), ("422_4100x12_10", 4100, 12, 10, 2, False, 6),
                ("444_4100x12", 4100, 12, 8, 3, False, 6), ("444_4100x12_10", 4100, 12, 10, 3, True, 6)]
# SAO above 12 bit: no packed procedure holds these samples, every 16-bit _g4 plane takes the sample-by-sample kernel on the
# renumbered grid (sao_g4_kernel<u16, true, false>).  Full-range content (sao_case(content="full")): the clip at max_v acts.
# The GPU test runs each with rows of a multiple of 16 bytes and of 8 bytes more; the entries refuse 16-bit rows that are no multiple
# of one 4-sample word (8 bytes), so no smaller misalignment reaches the kernel
DEEP = [("12x12_14", 12, 12, 14, 1, False, 3), ("28x20_14", 28, 20, 14, 1, False, 4), ("12x12_16", 12, 12, 16, 1, False, 3),
        ("28x20_16", 28, 20, 16, 1, False, 4)]
CQP, TC_DIV2, QP = 2, 1, 37
UNIT_LOG2 = 3
SL_CTB_LOG2 = 4
FRAMES = 5


def seed_of(name):
    return sum(ord(c) * (i + 1) for i, c in enumerate(name)) % 100003


def dbk_case(spec, frames=1):
    """one deblocking vector: `frames` blocky planes with per-frame bS; one QP or a per-8x8-luma QP map; (beta, tC) pairs per CTB of
    the luma grid for the per-slice runs (slices of three CTBs in raster order, tests/slice_offsets_ref.py)"""
    name, w, h, depth, cf, qmap, _ = spec
    rng = np.random.default_rng(seed_of(name))
    sx, sy = rx.SUB[cf]
    rows, cols = -(-h * sy >> SL_CTB_LOG2), -(-w * sx >> SL_CTB_LOG2)
    sidx = R.slices_raster(rows, cols, 3)
    c = {"name": name, "w": w, "h": h, "depth": depth, "sb": 1 if depth == 8 else 2, "cf": cf, "qp": QP,
         "planes": [blocky_plane(w, h, depth, rng) for _ in range(frames)], "bs": [random_bs(w, h, rng) for _ in range(frames)],
         "qp_map": random_qp_map(w, h, cf, UNIT_LOG2, rng) if qmap else None,
         "pairs": R.ctb_pairs(sidx, R.table_for(int(sidx.max()) + 1))}
    return c


def dbk_expected(c, f=0, sl=False, src=None):
    pl = c["planes"][f] if src is None else src
    vb, hb = c["bs"][f]
    kw = dict(qp=c["qp"], qp_map=c["qp_map"], unit_log2=UNIT_LOG2, bit_depth=c["depth"], c_qp_offset=CQP)
    if sl:
        return deblock_sl(pl, vb, hb, c["cf"], c["pairs"], SL_CTB_LOG2, **kw)
    return deblock_direct(pl, vb, hb, c["cf"], tc_offset_div2=TC_DIV2, **kw)


def sao_case(spec, frames=FRAMES, content="noise"):
    """one SAO vector: planes of noise (every sample is a local something: the constructed edge offsets then move nearly every
    sample), constructed parameters per frame, a keep map"""
    name, w, h, depth, cf, _, lw = spec
    lh = lw + (1 if cf == 2 else 0)
    rng = np.random.default_rng(seed_of(name) + 7)
    if content == "full":   # h265_vectors.sao_full_range (runs of 0 and max_v, ramps through every band, spikes) of the next multiple of 8, cropped
        import h265_vectors as hv
        planes = [np.ascontiguousarray(hv.sao_full_range(depth, lw, rng, w=pad8(w), h=pad8(h))[0][:h, :w]) for _ in range(frames)]
        for p in planes:   # the last sample one below max_v: in the frame in which the last CTB is a band-offset one (border_params),
            p[-1, -1] = (1 << depth) - 2   # fit_bands puts its first, positive offset on this sample's band, and the sum is clipped
    else:
        planes = [noise_plane(w, h, depth, rng) if content == "noise" else blocky_plane(w, h, depth, rng) for _ in range(frames)]
    params = border_params(w, h, lw, lh, depth, frames, rng)
    fit_bands(planes, params, lw, lh, depth)
    return {"name": name, "w": w, "h": h, "depth": depth, "sb": 1 if depth == 8 else 2, "cf": cf, "lw": lw, "lh": lh,
            "planes": planes, "params": params, "keep": [keep_map(w, h, rng) for _ in range(frames)]}


def sao_layout(c, seed=0):
    """slices and tiles on the plane's CTB grid (tests/sao_borders_ref.py)"""
    rows, cols = c["params"][0].shape
    return B._layout_of("mixed", rows, cols, np.random.default_rng(seed_of(c["name"]) + 11 + seed))
