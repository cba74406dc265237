"""Vectors for the boundary-byte operand of SAO (hevcdbk_sao_borders.nox) taken as what the C ABI says it is: one ARBITRARY byte
per CTB, never reconciled with the neighbour's.  No slice / tile layout stands behind these bytes; the expected result is
sao_borders_ref.sao_plane_by_bytes.

"every byte" vectors: every CTB that is not on the rim of the CTB grid ("interior") has edge offset, and every pair (byte value
0..255, class 0..3) sits on an interior CTB at least once -- 1024 interior CTBs, spread over the frames of a batch with per-frame
bytes where the CTBs are large.  The CTBs on the rim carry random bytes (bits that point outside the picture among them) and
random types.  Content is low-amplitude noise around mid-grey in which the generator plants eight samples per CTB -- its four
corners and the middle of its four sides -- that are strict local extrema against ALL their eight neighbours: the top corners and
the middle of the top side LOW, the bottom ones HIGH, the middle of the left side HIGH, of the right side LOW, so that two planted
samples that are neighbours across a CTB border (the four corners that meet at a junction of CTBs along their diagonals, the two
side middles that face each other) always are one LOW and one HIGH.  Offsets are of full size and never zero, far from the clip:
every planted sample is changed by the edge offset of whatever class unless the byte forbids it, and so every bit that a class
looks at changes the CTB's output (test_sao_bytes_cpu.py asserts exactly that, for every interior CTB and bit).

"mixed" vectors: CTBs of 64, random bytes, random types (off / band / edge), full-range noise and a keep map; 8-bit ones are wide
enough for the aligned CTB pairs of the packed 8-bit SAO kernel (wide_pairs() counts which of its shapes the pairs take).

TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np

import rext_oracle as ro
import sao_borders_ref as R

NOX_POISON = 0xFF     # the bytes of a row of the byte array beyond the CTB columns (stride > columns): everything forbidden
STRIDE_EXTRA = 3

# class -> the bits its two neighbours can ask for: the two directions themselves and, for the diagonals, the sides a diagonal
# neighbour lies in when the sample is not in the CTB's corner
L, Rr, U, D, UL, UR, DL, DR = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80
RELEVANT = {0: L | Rr, 1: U | D, 2: L | U | UL | Rr | D | DR, 3: Rr | U | UR | L | D | DL}


def _plant(plane, lw, lh, rows, cols, low, high):
    h, w = plane.shape
    cw, ch = 1 << lw, 1 << lh
    for cy in range(rows):
        for cx in range(cols):
            x0, y0 = cx << lw, cy << lh
            x1, y1, xm, ym = x0 + cw - 1, y0 + ch - 1, x0 + cw // 2, y0 + ch // 2
            for (x, y, v) in ((x0, y0, low), (x1, y0, low), (xm, y0, low), (x0, y1, high), (x1, y1, high), (xm, y1, high),
                              (x0, ym, high), (x1, ym, low)):
                if x < w and y < h:
                    plane[y, x] = v


def every_byte(name, depth, lw, lh, rows, cols, frames, seed, *, cut_w=0, cut_h=0, sb=None):
    """one "every byte" vector: frames planes of ((cols << lw) - cut_w) x ((rows << lh) - cut_h) samples"""
    rng = np.random.default_rng(seed)
    sb = sb or (1 if depth == 8 else 2)
    dt = np.uint8 if sb == 1 else np.uint16
    w, h = (cols << lw) - cut_w, (rows << lh) - cut_h
    n_int = frames * (rows - 2) * (cols - 2)
    assert n_int >= 1024 and cut_w < (1 << lw) and cut_h < (1 << lh)
    pairs = rng.permutation(np.arange(n_int) % 1024).reshape(frames, rows - 2, cols - 2)    # byte | class << 8
    mid = 1 << (depth - 1)
    lim = (1 << (min(depth, 10) - 5)) - 1
    planes, params = [], []
    nox = np.full((frames, rows, cols + STRIDE_EXTRA), NOX_POISON, np.uint8)
    nox[:, :, :cols] = rng.integers(0, 256, (frames, rows, cols))
    nox[:, 1:-1, 1:cols - 1] = pairs & 255
    for f in range(frames):
        p = rng.integers(mid - 2, mid + 3, (h, w)).astype(dt)
        _plant(p, lw, lh, rows, cols, mid - 4, mid + 4)
        planes.append(p)
        prm = np.zeros((rows, cols), ro.SAO_CTB_DTYPE)
        prm["type"] = rng.integers(0, 3, (rows, cols))
        prm["type"][1:-1, 1:-1] = 2
        edge = prm["type"] == 2
        cls = rng.integers(0, 4, (rows, cols))
        cls[1:-1, 1:-1] = pairs[f] >> 8
        # band CTBs (on the rim only): the four bands start at or just below the content's band
        prm["cls"] = np.where(edge, cls, ((mid >> (depth - 5)) - rng.integers(0, 4, (rows, cols))) & 31)
        off = rng.integers(lim // 2 + 1, lim + 1, (rows, cols, 4))
        off[..., 2:4] = -off[..., 2:4]
        flip = rng.integers(0, 2, (rows, cols, 4)) * 2 - 1
        off = np.where(edge[..., None], off, np.abs(off) * flip)
        prm["offset"] = off
        params.append(prm)
    return {"name": name, "kind": "every", "w": w, "h": h, "depth": depth, "sb": sb, "lw": lw, "lh": lh, "rows": rows, "cols": cols,
            "planes": planes, "params": params, "keeps": None, "nox": nox}


def chroma_every_byte(name, luma, sx, sy, rot, seed):
    """a chroma plane that goes with the "every byte" vector `luma` in one picture: the luma plane's CTB grid and BYTES (one
    byte array serves the planes of a picture), CTBs and plane sub-sampled by (sx, sy), the classes of the interior CTBs the
    luma plane's turned by rot -- every (byte, class) pair again"""
    l = case(luma)
    c = every_byte(name, l["depth"], l["lw"] - (sx - 1), l["lh"] - (sy - 1), l["rows"], l["cols"], len(l["planes"]), seed)
    c["nox"] = l["nox"].copy()
    for pc, pl in zip(c["params"], l["params"]):
        pc["cls"][1:-1, 1:-1] = (pl["cls"][1:-1, 1:-1] + rot) & 3
    return c


def mixed(name, depth, w, h, frames, seed, *, lw=6, lh=6, sb=None):
    """random bytes, random types, full-range noise, a keep map; per-frame bytes"""
    rng = np.random.default_rng(seed)
    sb = sb or (1 if depth == 8 else 2)
    dt = np.uint8 if sb == 1 else np.uint16
    rows, cols = -(-h >> lh), -(-w >> lw)
    planes = [rng.integers(0, 1 << depth, (h, w)).astype(dt) for _ in range(frames)]
    params = [ro.random_sao_params(w, h, lw, lh, rng, depth) for _ in range(frames)]
    for prm in params:       # offsets never zero
        o = prm["offset"].astype(np.int64)
        edge = (prm["type"] == 2)[..., None]
        sign = np.where(edge, np.array([1, 1, -1, -1]), np.where(o < 0, -1, 1))
        prm["offset"] = np.where(o == 0, sign, o)
    keeps = [(rng.integers(0, 8, (h // 8, w // 8)) == 0).astype(np.uint8) for _ in range(frames)]
    nox = np.full((frames, rows, cols + STRIDE_EXTRA), NOX_POISON, np.uint8)
    nox[:, :, :cols] = rng.integers(0, 256, (frames, rows, cols))
    return {"name": name, "kind": "mixed", "w": w, "h": h, "depth": depth, "sb": sb, "lw": lw, "lh": lh, "rows": rows, "cols": cols,
            "planes": planes, "params": params, "keeps": keeps, "nox": nox}


def wide_pairs(c):
    """the aligned pairs of 64-sample CTBs (columns 2k, 2k + 1, whole inside the plane) by the shape the packed 8-bit SAO kernel
    gives them: counts of pairs on ONE path (both edge offset of one class, or neither edge offset) whose two bytes differ, and of
    pairs of one band-offset and one not-applied CTB (run as one band offset, the latter with offsets of zero)"""
    out = {"wide_bytes_differ": 0, "zero_band": 0}
    if c["lw"] != 6 or c["lh"] != 6:
        return out
    for f, prm in enumerate(c["params"]):
        for r in range(c["h"] >> 6):
            for k in range(0, (c["w"] >> 7) * 2, 2):
                a, b = prm[r, k], prm[r, k + 1]
                e0, e1 = a["type"] == 2, b["type"] == 2
                same = e0 == e1 and (not e0 or ((a["cls"] ^ b["cls"]) & 3) == 0)
                if same and c["nox"][f, r, k] != c["nox"][f, r, k + 1]:
                    out["wide_bytes_differ"] += 1
                if same and not e0 and (a["type"] == 1) != (b["type"] == 1):
                    out["zero_band"] += 1
    return out


# name -> (constructor, arguments).  Square CTBs of 8 / 16 / 32 / 64 at 8, 10 and 12 bit in the smallest shapes that hold 1024
# interior CTBs (34 x 34 CTBs in one plane; 4 frames of 18 x 18 with per-frame bytes for the large ones), CTBs twice as tall as
# wide (4:2:2 chroma), and planes whose last CTB column / row is cut to a multiple of 4 that is no multiple of 8 (the _g4 entries)
CASES = {}
_seed = 700
for _d in (8, 10, 12):
    for _l, (_r, _c, _n) in ((3, (34, 34, 1)), (4, (34, 34, 1)), (5, (18, 18, 4)), (6, (18, 18, 4))):
        _seed += 1
        CASES["every_%db_ctb%d" % (_d, 1 << _l)] = (every_byte, (_d, _l, _l, _r, _c, _n, _seed), {})
CASES["every_8b_ctb8x16"] = (every_byte, (8, 3, 4, 34, 34, 1, 731), {})
CASES["every_8b_ctb32x64"] = (every_byte, (8, 5, 6, 18, 18, 4, 732), {})
CASES["every_10b_ctb16x32"] = (every_byte, (10, 4, 5, 34, 34, 1, 733), {})
CASES["every_8b_g4_ctb8"] = (every_byte, (8, 3, 3, 34, 34, 1, 741), {"cut_w": 4, "cut_h": 4})
CASES["every_10b_g4_ctb16"] = (every_byte, (10, 4, 4, 34, 34, 1, 742), {"cut_w": 12, "cut_h": 4})
CASES["every_8b_g4_ctb8x16"] = (every_byte, (8, 3, 4, 34, 34, 1, 743), {"cut_w": 4})
# the chroma planes of pictures whose luma plane is one of the vectors above: 4:2:0, 4:2:2, 4:4:4
for _luma, _fmt, _sx, _sy in (("every_8b_ctb16", "420", 2, 2), ("every_8b_ctb16", "422", 2, 1), ("every_8b_ctb16", "444", 1, 1),
                              ("every_10b_ctb32", "420", 2, 2)):
    for _i, _pl in enumerate(("cb", "cr")):
        _seed += 1
        CASES["%s_%s%s" % (_luma, _pl, _fmt)] = (chroma_every_byte, (_luma, _sx, _sy, _i + 1, _seed), {})
CASES["mixed_8b"] = (mixed, (8, 512, 192, 2, 751), {})
CASES["mixed_10b"] = (mixed, (10, 384, 192, 2, 752), {})
CASES["mixed_12b"] = (mixed, (12, 256, 136, 2, 753), {})
del _seed, _d, _l, _r, _c, _n, _luma, _fmt, _sx, _sy, _i, _pl

EVERY = [n for n in CASES if n.startswith("every")]
MIXED = [n for n in CASES if n.startswith("mixed")]
TALL = ["every_8b_ctb8x16", "every_8b_ctb32x64", "every_10b_ctb16x32", "every_8b_g4_ctb8x16", "every_8b_ctb16_cb422",
        "every_8b_ctb16_cr422"]                     # CTBs twice as tall as wide (4:2:2 chroma)


@functools.lru_cache(maxsize=None)
def case(name):
    """the vector, built once per process; treat as read-only"""
    fn, args, kw = CASES[name]
    c = fn(name, *args, **kw)
    for a in c["planes"] + c["params"] + [c["nox"]] + (c["keeps"] or []):
        a.setflags(write=False)
    return c


def keep_of(c, f):
    return None if c["keeps"] is None else c["keeps"][f]


@functools.lru_cache(maxsize=None)
def free(name, f):
    """the border-less result (rext_oracle.sao_plane) of frame f"""
    c = case(name)
    out = ro.sao_plane(c["planes"][f], c["params"][f], c["lw"], c["lh"], bit_depth=c["depth"], keep=keep_of(c, f))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def look(name, f):
    c = case(name)
    return R.look_bits(c["params"][f], c["lw"], c["lh"], c["h"], c["w"])


def by_bytes(name, f, nox):
    """sao_plane_by_bytes of frame f under the bytes nox (rows x at least cols)"""
    c = case(name)
    return R.sao_plane_by_bytes(c["planes"][f], c["params"][f], c["lw"], c["lh"], nox, bit_depth=c["depth"], keep=keep_of(c, f),
                                _free=free(name, f), _look=look(name, f))


@functools.lru_cache(maxsize=None)
def expected(name, f):
    out = by_bytes(name, f, case(name)["nox"][f])
    out.setflags(write=False)
    return out
