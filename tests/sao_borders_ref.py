"""SAO at slice and tile boundaries that in-loop filtering must not cross: a per-sample numpy statement of ITU-T H.265
8.7.3.2, layout generators, the expected `nox` bytes of hevcdbk_h265_sao_borders_device, and a census of what a set of
vectors exercises.

TEST INFRASTRUCTURE ONLY, parity unpinned like the rest of the spec-exact mode.  The rule is stated per SAMPLE from per-sample
slice / tile membership; the library's CTB bytes and block masks appear nowhere in it.  For a sample of an edge-offset CTB
with neighbours at (x + hPos[k], y + vPos[k]), k = 0, 1 (Table 8-13), the sample is left as it is when for either neighbour
  1. the neighbour lies outside the picture, or
  2. it belongs to a different slice and -- the neighbour's slice earlier in decoding order -- the CURRENT sample's slice has
     slice_loop_filter_across_slices_enabled_flag == 0, or -- the neighbour's slice later -- the NEIGHBOUR's slice has, or
  3. loop_filter_across_tiles_enabled_flag == 0 and it belongs to a different tile.
The border-less result (rule 1 only) is rext_oracle.sao_plane.

A layout is a dict: slice_idx (CTB rows, CTB columns) = index of the CTB's slice in decoding order, slice_flags[s] = that
slice's flag, tile_idx (rows, columns), tiles_across = the PPS flag.
"""
import numpy as np

import rext_oracle as ro

HV = {0: ((0, -1), (0, 1)), 1: ((-1, 0), (1, 0)), 2: ((-1, -1), (1, 1)), 3: ((-1, 1), (1, -1))}  # class -> ((dy, dx), (dy, dx))
# the eight directions (dy, dx) and the bit HEVCDBK_SAO_NOX_* that speaks for each
NOX_BITS = {(0, -1): 0x01, (0, 1): 0x02, (-1, 0): 0x04, (1, 0): 0x08, (-1, -1): 0x10, (-1, 1): 0x20, (1, -1): 0x40, (1, 1): 0x80}
NOX_NAMES = {(0, -1): "L", (0, 1): "R", (-1, 0): "U", (1, 0): "D", (-1, -1): "UL", (-1, 1): "UR", (1, -1): "DL", (1, 1): "DR"}


def membership(layout, h, w, ctb_log2_w, ctb_log2_h):
    """per-sample slice index, that slice's flag and tile index of an h x w plane whose CTBs are (1 << ctb_log2_w) wide and
    (1 << ctb_log2_h) tall (a chroma plane: the luma CTB grid sub-sampled)"""
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = yy >> ctb_log2_h, xx >> ctb_log2_w
    S = np.asarray(layout["slice_idx"], np.int64)[cy, cx]
    F = np.asarray(layout["slice_flags"], np.int64)[S]
    T = np.asarray(layout["tile_idx"], np.int64)[cy, cx]
    return S, F, T


def neighbour_forbidden(S, F, T, tiles_across, dy, dx):
    """rule 2 / 3 for every sample's neighbour at (y + dy, x + dx): True where the neighbour is inside the picture and must not
    be looked at.  (Rule 1 is not in here: False where the neighbour is outside.)"""
    h, w = S.shape
    yy, xx = np.mgrid[0:h, 0:w]
    ny, nx = yy + dy, xx + dx
    ins = (ny >= 0) & (ny < h) & (nx >= 0) & (nx < w)
    nyc, nxc = np.clip(ny, 0, h - 1), np.clip(nx, 0, w - 1)
    s2, f2, t2 = S[nyc, nxc], F[nyc, nxc], T[nyc, nxc]
    rule2 = ((s2 < S) & (F == 0)) | ((S < s2) & (f2 == 0))
    rule3 = (t2 != T) if not tiles_across else np.zeros_like(ins)
    return ins & (rule2 | rule3)


def forbidden_map(params, layout, h, w, ctb_log2_w, ctb_log2_h):
    """True for the samples of edge-offset CTBs one of whose two neighbours falls under rule 2 / 3"""
    S, F, T = membership(layout, h, w, ctb_log2_w, ctb_log2_h)
    yy, xx = np.mgrid[0:h, 0:w]
    P = np.asarray(params, ro.SAO_CTB_DTYPE)
    typ = P["type"].astype(np.int64)[yy >> ctb_log2_h, xx >> ctb_log2_w]
    cls = P["cls"].astype(np.int64)[yy >> ctb_log2_h, xx >> ctb_log2_w]
    out = np.zeros((h, w), bool)
    for c, nbs in HV.items():
        for dy, dx in nbs:
            out |= neighbour_forbidden(S, F, T, layout["tiles_across"], dy, dx) & (typ == 2) & (cls == c)
    return out


def sao_plane(plane, params, ctb_log2_w, ctb_log2_h, layout, *, bit_depth=8, keep=None):
    """8.7.3 on one plane with the slices and tiles of `layout`; returns a new array"""
    src = np.asarray(plane)
    h, w = src.shape
    free = ro.sao_plane(src, params, ctb_log2_w, ctb_log2_h, bit_depth=bit_depth, keep=keep)
    return np.where(forbidden_map(params, layout, h, w, ctb_log2_w, ctb_log2_h), src, free).astype(src.dtype)


def expected_nox(layout):
    """the bytes hevcdbk_h265_sao_borders_device writes, gathered from the per-sample statement: the picture with CTBs of 2 x 2
    samples; bit d of a CTB = its sample in the corner / on the side that looks in direction d is forbidden to.  Bits that
    point outside the picture are 0."""
    rows, cols = np.asarray(layout["slice_idx"]).shape
    S, F, T = membership(layout, 2 * rows, 2 * cols, 1, 1)
    out = np.zeros((rows, cols), np.uint8)
    for (dy, dx), bit in NOX_BITS.items():
        m = neighbour_forbidden(S, F, T, layout["tiles_across"], dy, dx)
        # the sample of each CTB nearest to the neighbouring CTB in that direction (a side: either sample of that side)
        sy, sx = (1 if dy > 0 else 0), (1 if dx > 0 else 0)
        out |= np.where(m[sy::2, sx::2], bit, 0).astype(np.uint8)
    return out


def per_ctb(layout):
    """the producer's operands: slice_idx (uint16), slice_across (uint8, the flag of the CTB's slice), tile_idx (uint16)"""
    s = np.ascontiguousarray(layout["slice_idx"], np.uint16)
    a = np.ascontiguousarray(np.asarray(layout["slice_flags"], np.uint8)[np.asarray(layout["slice_idx"], np.int64)])
    return s, a, np.ascontiguousarray(layout["tile_idx"], np.uint16)


# ---- the rule stated from the bytes themselves ------------------------------------------------------------------------------

def look_bits(params, lw, lh, h, w):
    """per sample of an h x w plane: the bits of its CTB's byte that speak for its two neighbours (Table 8-13, by the CTB's
    class) -- the bit of direction (sign(cx' - cx), sign(cy' - cy)) for a neighbour inside the picture in another CTB
    (cx', cy'), nothing for a neighbour in the same CTB or outside the picture; 0 in CTBs without edge offset"""
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = yy >> lh, xx >> lw
    P = np.asarray(params, ro.SAO_CTB_DTYPE)
    edge = (P["type"] == 2)[cy, cx]
    cls = (P["cls"] & 3)[cy, cx]
    table = np.zeros((3, 3), np.uint8)              # [sign dy + 1, sign dx + 1] -> bit; (0, 0) = the same CTB -> 0
    for (dy, dx), bit in NOX_BITS.items():
        table[dy + 1, dx + 1] = bit
    out = np.zeros((h, w), np.uint8)
    for c, nbs in HV.items():
        bits = np.zeros((h, w), np.uint8)
        for dy, dx in nbs:
            ny, nx = yy + dy, xx + dx
            ins = (ny >= 0) & (ny < h) & (nx >= 0) & (nx < w)
            sy = np.sign((np.clip(ny, 0, h - 1) >> lh) - cy) + 1
            sx = np.sign((np.clip(nx, 0, w - 1) >> lw) - cx) + 1
            bits |= np.where(ins, table[sy, sx], 0).astype(np.uint8)
        out = np.where(edge & (cls == c), bits, out)
    return out


def sao_plane_by_bytes(plane, params, lw, lh, nox, *, bit_depth=8, keep=None, _free=None, _look=None):
    """8.7.3 on one plane with the boundaries given as hevcdbk_sao_borders bytes -- any bytes, not those of a layout: nox[cy, cx]
    is the byte of CTB (cx, cy) (columns beyond the grid are not looked at).  Per sample of an edge-offset CTB (cx, cy) and each
    of its two neighbours: the sample is copied if the neighbour is outside the plane; copied if the neighbour lies in a CTB
    (cx', cy') != (cx, cy) and THIS CTB's byte has the bit of direction (sign(cx' - cx), sign(cy' - cy)); else the edge offset
    applies.  No byte of another CTB is looked at.  CTBs of any (1 << lw) x (1 << lh), the last row / column cut by the plane or
    not.  Band offset and keep as in rext_oracle.sao_plane.  (_free, _look: the border-less result and look_bits of the same
    operands, for callers that go through many byte arrays.)"""
    src = np.asarray(plane)
    h, w = src.shape
    free = ro.sao_plane(src, params, lw, lh, bit_depth=bit_depth, keep=keep) if _free is None else _free
    look = look_bits(params, lw, lh, h, w) if _look is None else _look
    yy, xx = np.mgrid[0:h, 0:w]
    byte = np.asarray(nox, np.uint8)[yy >> lh, xx >> lw]
    return np.where((byte & look) != 0, src, free).astype(src.dtype)


def reconciled(nox):
    """what a library that "reconciled" the bytes would use: a CTB's bit also set when the neighbouring CTB in that direction
    has the bit that points back (the operand's definition says this never happens)"""
    b = np.asarray(nox, np.uint8)
    rows, cols = b.shape
    out = b.copy()
    for (dy, dx), bit in NOX_BITS.items():
        back = NOX_BITS[(-dy, -dx)]
        ys, xs = slice(max(0, -dy), rows - max(0, dy)), slice(max(0, -dx), cols - max(0, dx))
        yn, xn = slice(max(0, dy), rows - max(0, -dy)), slice(max(0, dx), cols - max(0, -dx))
        out[ys, xs] |= np.where(b[yn, xn] & back, bit, 0).astype(np.uint8)
    return out


# ---- layouts ------------------------------------------------------------------------------------------------------------

def one_slice(rows, cols):
    return {"slice_idx": np.zeros((rows, cols), np.int64), "slice_flags": np.array([1]), "tile_idx": np.zeros((rows, cols), np.int64),
            "tiles_across": True}


def tile_scan(rows, cols, col_starts=(), row_starts=()):
    """tile index and decoding order (CtbAddrRsToTs) of a tile grid whose columns / rows start at the given CTB positions"""
    cb = np.array(sorted(set([0] + [c for c in col_starts if 0 < c < cols])))
    rb = np.array(sorted(set([0] + [r for r in row_starts if 0 < r < rows])))
    tx = np.searchsorted(cb, np.arange(cols), side="right") - 1
    ty = np.searchsorted(rb, np.arange(rows), side="right") - 1
    tile = ty[:, None] * len(cb) + tx[None, :]
    order = np.zeros((rows, cols), np.int64)
    k = 0
    for t in range(len(cb) * len(rb)):            # tiles in raster order, CTBs in raster order inside a tile
        ys, xs = np.nonzero(tile == t)
        order[ys, xs] = k + np.arange(ys.size)
        k += ys.size
    return tile, order


def layout(rows, cols, rng, *, col_starts=(), row_starts=(), slice_starts=None, mean_run=6, flags=None, tiles_across=None):
    """tiles as a grid in tile-scan order, slices as runs of CTBs in decoding order (slice_starts = decoding-order addresses at
    which a slice starts; default: random, runs of about mean_run CTBs, down to one), flags drawn per slice"""
    tile, order = tile_scan(rows, cols, col_starts, row_starts)
    n = rows * cols
    if slice_starts is None:
        slice_starts = np.unique(rng.integers(1, max(n, 2), max(1, n // mean_run))) if n > 1 else []
    starts = np.array(sorted(set(int(s) for s in slice_starts if 0 < s < n)), np.int64)
    sl = np.searchsorted(starts, order, side="right")
    ns = int(sl.max()) + 1
    if flags is None:
        flags = rng.integers(0, 2, ns)
    flags = np.broadcast_to(np.asarray(flags, np.int64), (ns,)).copy()
    if tiles_across is None:
        tiles_across = bool(rng.integers(0, 2))
    return {"slice_idx": sl, "slice_flags": flags, "tile_idx": tile, "tiles_across": bool(tiles_across)}


def every_ctb(rows, cols):
    """each CTB a slice of its own with flag 0: every CTB border forbidden"""
    return layout(rows, cols, None, slice_starts=range(1, rows * cols), flags=0, tiles_across=True)


def coded_picture_layout(w, h, seed, ctb_log2=6):
    """the slices and tiles bs_vectors.coded_picture(w, h, seed, ctb_log2) draws (the same generator calls in the same order;
    test_sao_borders_cpu checks the units' NOX flags against it): slices as runs in RASTER order, tiles as a grid"""
    rng = np.random.default_rng(seed)
    uw, uh = w // 4, h // 4
    for _ in (0, 1):
        rng.integers(-(1 << 15), 1 << 15, (uh, uw, 2))
    for _ in (0, 1):
        rng.integers(-40, 40, (uh, uw))
    cs = 1 << (ctb_log2 - 2)
    cw, chh = -(-uw // cs), -(-uh // cs)
    n_ctb = cw * chh
    slice_of = np.zeros(n_ctb, np.int64)
    starts = np.unique(rng.integers(0, n_ctb, max(1, n_ctb // 6)))
    slice_of[starts] = 1
    slice_of = np.cumsum(slice_of).reshape(chh, cw)
    n_slices = int(slice_of.max()) + 1
    rng.integers(0, 5, n_slices)
    slice_nox = rng.integers(0, 2, n_slices) == 0
    tile_cols = set(int(x) for x in rng.integers(1, max(cw, 2), 2)) if cw > 2 else set()
    tile_rows = set(int(x) for x in rng.integers(1, max(chh, 2), 1)) if chh > 2 else set()
    tiles_nox = bool(rng.integers(0, 2))
    tile, _ = tile_scan(chh, cw, tile_cols, tile_rows)
    return {"slice_idx": slice_of, "slice_flags": (~slice_nox).astype(np.int64), "tile_idx": tile, "tiles_across": not tiles_nox}


# ---- parameters that make a layout bite -----------------------------------------------------------------------------------

def edge_params(rows, cols, rng, bit_depth=8, p_edge=0.75):
    """mostly edge-offset CTBs, every class, offsets of full size and never zero: on noise nearly every forbidden sample then
    differs from the border-less result"""
    p = np.zeros((rows, cols), ro.SAO_CTB_DTYPE)
    edge = rng.random((rows, cols)) < p_edge
    other = rng.integers(0, 2, (rows, cols))
    p["type"] = np.where(edge, 2, other)
    p["cls"] = np.where(edge, rng.integers(0, 4, (rows, cols)), rng.integers(0, 32, (rows, cols)))
    lim = (1 << (min(bit_depth, 10) - 5)) - 1
    off = rng.integers(1, lim + 1, (rows, cols, 4))
    off[..., 2:4] = -off[..., 2:4]
    band = p["type"] == 1
    off[band] = rng.integers(-lim, lim + 1, (int(band.sum()), 4))
    p["offset"] = off
    return p


# ---- census -----------------------------------------------------------------------------------------------------------------

def _empty():
    c = {"changed": 0}
    for cl, nbs in HV.items():
        for d in nbs:
            c[(cl, NOX_NAMES[d], "forbidden")] = 0   # samples looking there across a forbidden CTB border, byte changed
            c[(cl, NOX_NAMES[d], "allowed")] = 0     # samples looking there across an allowed CTB border, byte changed by SAO
    for cl in (2, 3):
        c[(cl, "corner_diag_only")] = 0              # diagonal CTB forbidden, both side CTBs allowed, byte changed
        c[(cl, "corner_sides_only")] = 0             # diagonal CTB allowed, a side CTB forbidden
    for k in ("slice_only", "tile_only", "both"):
        c[k] = 0
    return c


def merge(a, b):
    return {k: a[k] + b[k] for k in a}


def census(plane, params, ctb_log2_w, ctb_log2_h, lay, *, bit_depth=8):
    """what one vector exercises; counts are samples"""
    src = np.asarray(plane)
    h, w = src.shape
    c = _empty()
    S, F, T = membership(lay, h, w, ctb_log2_w, ctb_log2_h)
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = yy >> ctb_log2_h, xx >> ctb_log2_w
    P = np.asarray(params, ro.SAO_CTB_DTYPE)
    typ, cls = P["type"].astype(np.int64)[cy, cx], P["cls"].astype(np.int64)[cy, cx]
    free = ro.sao_plane(src, params, ctb_log2_w, ctb_log2_h, bit_depth=bit_depth)
    got = sao_plane(src, params, ctb_log2_w, ctb_log2_h, lay, bit_depth=bit_depth)
    c["changed"] = int((got != free).sum())
    one = dict(lay, tiles_across=True)
    s_only = neighbour_any(one, h, w, ctb_log2_w, ctb_log2_h, typ, cls)
    t_only = neighbour_any(dict(lay, slice_flags=np.ones_like(np.asarray(lay["slice_flags"]))), h, w, ctb_log2_w, ctb_log2_h, typ, cls)
    diff = got != free
    c["slice_only"] = int((diff & s_only & ~t_only).sum())
    c["tile_only"] = int((diff & t_only & ~s_only).sum())
    c["both"] = int((diff & t_only & s_only).sum())

    def other_ctb(dy, dx):
        ny, nx = yy + dy, xx + dx
        ins = (ny >= 0) & (ny < h) & (nx >= 0) & (nx < w)
        return ins & (((np.clip(ny, 0, h - 1) >> ctb_log2_h) != cy) | ((np.clip(nx, 0, w - 1) >> ctb_log2_w) != cx))

    for cl, nbs in HV.items():
        sel = (typ == 2) & (cls == cl)
        for d in nbs:
            forb = neighbour_forbidden(S, F, T, lay["tiles_across"], *d)
            c[(cl, NOX_NAMES[d], "forbidden")] = int((sel & forb & diff).sum())
            c[(cl, NOX_NAMES[d], "allowed")] = int((sel & other_ctb(*d) & ~forb & (free != src) & ~diff).sum())
    for cl in (2, 3):
        sel = (typ == 2) & (cls == cl)
        for dy, dx in HV[cl]:
            # the sample in the CTB's corner: its diagonal neighbour is in the diagonal CTB, (dy, 0) and (0, dx) are the side CTBs
            corner = other_ctb(dy, 0) & other_ctb(0, dx)
            diag = neighbour_forbidden(S, F, T, lay["tiles_across"], dy, dx)
            sides = neighbour_forbidden(S, F, T, lay["tiles_across"], dy, 0) | neighbour_forbidden(S, F, T, lay["tiles_across"], 0, dx)
            both_sides_free = ~neighbour_forbidden(S, F, T, lay["tiles_across"], dy, 0) & ~neighbour_forbidden(S, F, T, lay["tiles_across"], 0, dx)
            c[(cl, "corner_diag_only")] += int((sel & corner & diag & both_sides_free & diff).sum())
            c[(cl, "corner_sides_only")] += int((sel & corner & ~diag & sides & (free != src) & ~diff).sum())
    return c


def neighbour_any(lay, h, w, ctb_log2_w, ctb_log2_h, typ, cls):
    S, F, T = membership(lay, h, w, ctb_log2_w, ctb_log2_h)
    out = np.zeros((h, w), bool)
    for c, nbs in HV.items():
        for dy, dx in nbs:
            out |= neighbour_forbidden(S, F, T, lay["tiles_across"], dy, dx) & (typ == 2) & (cls == c)
    return out


# ---- the vectors of tests/test_gpu_sao_borders.py (the census of tests/test_sao_borders_cpu.py runs over the same list) ----------

def _layout_of(kind, rows, cols, rng):
    lay = _draw_layout(kind, rows, cols, rng)
    if kind != "none" and lay["slice_flags"].size > 1 and lay["slice_flags"].all():
        lay["slice_flags"][-1] = 0     # every flag drawn as 1: the last slice must not be looked into / out of
    return lay


def _draw_layout(kind, rows, cols, rng):
    if kind == "none":
        return one_slice(rows, cols)
    if kind == "every":
        return every_ctb(rows, cols)
    if kind == "tiles":    # a tile grid not to be crossed, slices inside it with drawn flags
        return layout(rows, cols, rng, col_starts=[max(cols // 2, 1)], row_starts=[max(rows // 2, 1)], mean_run=5, tiles_across=False)
    if kind == "slices":   # one tile: slices as runs in raster order, drawn flags
        return layout(rows, cols, rng, mean_run=4, tiles_across=True)
    if kind == "mixed":    # tiles that may be crossed, several slices per tile: a later slice up-right / down-left of an earlier one
        return layout(rows, cols, rng, col_starts=[max(cols // 3, 1), max(2 * cols // 3, 1)], row_starts=[max(rows // 2, 1)], mean_run=3,
                      tiles_across=True)
    if kind == "random":
        return layout(rows, cols, rng, col_starts=rng.integers(1, max(cols, 2), 2), row_starts=rng.integers(1, max(rows, 2), 1), mean_run=4)
    raise ValueError(kind)


def make_case(name, w, h, depth, lw, lh, kind, seed, *, sample_bytes=None, frames=1, keep=False, shared=True):
    """one vector: planes of noise (frames of them), edge-heavy parameters, a layout per frame (or one shared)"""
    rng = np.random.default_rng(seed)
    sb = sample_bytes or (1 if depth == 8 else 2)
    rows, cols = -(-h >> lh), -(-w >> lw)
    dt = np.uint8 if sb == 1 else np.uint16
    planes = [rng.integers(0, 1 << depth, (h, w)).astype(dt) for _ in range(frames)]
    params = [edge_params(rows, cols, rng, depth) for _ in range(frames)]
    lays = [_layout_of(kind, rows, cols, rng) for _ in range(1 if shared else frames)]
    keeps = [(rng.integers(0, 8, (h // 8, w // 8)) == 0).astype(np.uint8) for _ in range(frames)] if keep else None
    return {"name": name, "w": w, "h": h, "depth": depth, "sb": sb, "lw": lw, "lh": lh, "kind": kind, "planes": planes, "params": params,
            "layouts": lays, "keeps": keeps, "shared": shared}


def case_layout(c, f):
    return c["layouts"][0 if c["shared"] else f]


def case_expected(c, f):
    return sao_plane(c["planes"][f], c["params"][f], c["lw"], c["lh"], case_layout(c, f), bit_depth=c["depth"],
                     keep=None if c["keeps"] is None else c["keeps"][f])


SAO_CASES = [
    # name, w, h, depth, log2 CTB width, height, layout, seed, options
    ("8b_ctb64_tiles", 256, 192, 8, 6, 6, "tiles", 11, {}),
    ("8b_ctb64_slices", 320, 192, 8, 6, 6, "slices", 12, {}),
    ("8b_ctb64_mixed", 384, 256, 8, 6, 6, "mixed", 13, {}),
    ("8b_ctb64_every", 256, 128, 8, 6, 6, "every", 14, {}),
    ("8b_ctb32_mixed", 192, 160, 8, 5, 5, "mixed", 15, {}),
    ("8b_ctb16_random", 136, 72, 8, 4, 4, "random", 16, {}),          # not a multiple of the CTB size
    ("8b_ctb8_every", 64, 40, 8, 3, 3, "every", 17, {}),
    ("8b_ctb32x64_tiles", 160, 256, 8, 5, 6, "tiles", 18, {}),        # 4:2:2 chroma CTBs
    ("8b_ctb16x32_every", 64, 96, 8, 4, 5, "every", 19, {}),
    ("8b_w8", 8, 64, 8, 4, 4, "every", 20, {}),
    ("8b_w4096", 4096, 64, 8, 6, 6, "random", 21, {}),
    ("8b_partial_ctb", 200, 136, 8, 6, 6, "every", 22, {}),
    ("8b_batch_shared_keep", 256, 128, 8, 6, 6, "mixed", 23, {"frames": 3, "keep": True}),
    ("8b_batch_per_frame", 192, 128, 8, 5, 5, "random", 24, {"frames": 3, "shared": False}),
    ("8b_unaligned_pitch", 72, 48, 8, 4, 4, "every", 25, {}),          # run with a pitch that is not a multiple of 8: the 32-bit kernel
    ("8b_none", 192, 128, 8, 6, 6, "none", 26, {}),
    ("10b_ctb64_mixed", 256, 192, 10, 6, 6, "mixed", 69, {}),
    ("10b_ctb32_every", 128, 96, 10, 5, 5, "every", 32, {}),
    ("12b_ctb16_random", 136, 64, 12, 4, 4, "random", 33, {"keep": True}),
    ("12b_ctb32x64_tiles", 128, 192, 12, 5, 6, "tiles", 34, {}),
    ("10b_batch_per_frame", 192, 128, 10, 6, 6, "slices", 64, {"frames": 2, "shared": False}),
    ("16b_ctb32_mixed", 160, 96, 16, 5, 5, "mixed", 41, {}),           # deeper than 12 bit: the 32-bit kernel
    ("16b_ctb64_every", 200, 136, 14, 6, 6, "every", 42, {}),
    ("8b_2160p", 3840, 2160, 8, 6, 6, "tiles", 51, {}),
    ("10b_2160p", 3840, 2160, 10, 6, 6, "mixed", 52, {}),
]
SMALL_SAO_CASES = [c for c in SAO_CASES if c[1] * c[2] < 1000000]


def sao_case(spec):
    name, w, h, depth, lw, lh, kind, seed, opt = spec
    return make_case(name, w, h, depth, lw, lh, kind, seed, **opt)
