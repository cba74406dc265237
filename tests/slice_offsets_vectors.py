"""Vectors of the per-slice deblocking offset tests (test_slice_offsets_cpu.py, test_gpu_slice_offsets.py): small pictures with
16-sample CTBs and slices of 5 CTBs in raster order, so that every 32 x 32 cell of every plane holds several slice boundaries, and
content made of flat 8 x 8 blocks with steps between them, so that the luma decisions switch the filter on and tC decides the
result.  The census of test_slice_offsets_cpu.py holds for every case; where a case's first seed failed it, the next one that
passes is recorded in SEED_OF."""
import zlib

import numpy as np

import rext_oracle as rx
import slice_offsets_ref as R

W, H, CTB_LOG2, RUN = 256, 192, 4, 5
ROWS, COLS = H >> CTB_LOG2, W >> CTB_LOG2
QPS = (24, 32, 40)
CQP = {0: 0, 1: 3, 2: -2}   # cQpPicOffset of Y, Cb, Cr

# (name, chroma_format, c_idx, bit depth, QP map?)
CASES = [("y_%db_%s" % (d, "map" if m else "qp"), 1, 0, d, m) for d in (8, 10, 12) for m in (False, True)]
CASES += [("%s_c%d_%db_%s" % ({1: "420", 2: "422", 3: "444"}[cf], c, d, "map" if m else "qp"), cf, c, d, m)
          for cf in (1, 2, 3) for d in (8, 10, 12) for m in (False, True) for c in (1, 2)]
# case name -> seed where the first one (first_seed) failed the census; the seeds tried go up in steps of 1000.  Both are 4:4:4 Cr
# planes with one QP (48 cells, one tC index for the whole plane but for the offsets): 927 and 1927, resp. 4, 1004, 2004, 3004 and
# 4004 left a cell equal to one of the uniform-pair pictures
SEED_OF = {"444_c2_8b_qp": 2927, "444_c2_10b_qp": 5004}


def first_seed(name):
    """a case's first seed: from its name, so that adding cases moves nobody's vectors"""
    return zlib.crc32(name.encode()) % 1000


def blocky(rng, h, w, depth):
    """flat 8 x 8 blocks of level 90..121 (8-bit scale): steps of up to +-31 between neighbours, +-1 of noise"""
    base = np.kron(rng.integers(90, 122, (h // 8, w // 8)), np.ones((8, 8), np.int64))
    v = (base << (depth - 8)) + rng.integers(-1, 2, (h, w)) * (1 << (depth - 8))
    return np.clip(v, 0, (1 << depth) - 1).astype(np.uint8 if depth == 8 else np.uint16)


def luma_bs(rng, w=W, h=H):
    """random bS 1 / 2 on every edge segment of the luma plane (the picture border is never filtered whatever the arrays hold)"""
    vb = rng.integers(1, 3, (h // 4) * (w // 8 + 1)).astype(np.uint8)
    hb = rng.integers(1, 3, (h // 8 + 1) * (w // 4)).astype(np.uint8)
    return vb, hb


def case(spec, frames=1, seed=None):
    """dict of one case: per frame a plane and a (ROWS, COLS, 2) pair array; shared bS, QP (map)"""
    name, cf, c_idx, depth, use_map = spec
    if seed is None:
        seed = SEED_OF.get(name, first_seed(name))
    rng = np.random.default_rng(1000 + seed)
    sx, sy = (1, 1) if c_idx == 0 else rx.SUB[cf]
    pw, ph = W // sx, H // sy
    vb, hb = luma_bs(rng)
    if c_idx:
        vb, hb = rx.chroma_bs(vb, hb, W, H, cf)
    qmap = rng.choice(QPS, (H // 8, W // 8)).astype(np.uint8) if use_map else None
    n_slices = -(-ROWS * COLS // RUN)
    sidx = R.slices_raster(ROWS, COLS, RUN)
    tables = [R.table_for(n_slices, shift=f) for f in range(frames)]
    return dict(name=name, cf=cf, c_idx=c_idx, depth=depth, sb=1 if depth == 8 else 2, pw=pw, ph=ph, vb=vb, hb=hb, qp=32, qp_map=qmap,
                c_qp_offset=CQP[c_idx], slice_idx=sidx, tables=tables, pairs=[R.ctb_pairs(sidx, t) for t in tables],
                planes=[blocky(rng, ph, pw, depth) for _ in range(frames)])


def expected(c, f=0, pairs=None, selector="q", plane=None):
    return R.expected(c["planes"][f] if plane is None else plane, c["vb"], c["hb"], c["pairs"][f] if pairs is None else pairs, CTB_LOG2,
                      qp=c["qp"], c_idx=c["c_idx"], chroma_format=c["cf"], qp_map=c["qp_map"], unit_log2=3, bit_depth=c["depth"],
                      c_qp_offset=c["c_qp_offset"], selector=selector)


def uniform(pair):
    p = np.zeros((ROWS, COLS, 2), np.int8)
    p[...] = pair
    return p


# ---- the clips of the two indices: Clip3(0, 51, qPL + 2 beta) and Clip3(0, 53, qPL + 2 (bS - 1) + 2 tc) at both ends ----

def clip_case(low, depth=8):
    """luma, bS 2, a QP map of QP 0..3 with (-6, -6) in half of the slices (low) or QP 48..51 with (+6, +6) (high); the other
    slices carry (0, 0)"""
    rng = np.random.default_rng(77 + int(low))
    vb = np.full((H // 4) * (W // 8 + 1), 2, np.uint8)
    hb = np.full((H // 8 + 1) * (W // 4), 2, np.uint8)
    qmap = rng.integers(0, 4, (H // 8, W // 8)).astype(np.uint8) + (0 if low else 48)
    sidx = R.slices_raster(ROWS, COLS, RUN)
    n_slices = -(-ROWS * COLS // RUN)
    e = (-6, -6) if low else (6, 6)
    table = np.array([e if i % 2 == 0 else (0, 0) for i in range(n_slices)], np.int8)
    return dict(name="clip_%s" % ("low" if low else "high"), cf=1, c_idx=0, depth=depth, sb=1 if depth == 8 else 2, pw=W, ph=H, vb=vb, hb=hb,
                qp=30, qp_map=qmap, c_qp_offset=0, slice_idx=sidx, tables=[table], pairs=[R.ctb_pairs(sidx, table)],
                planes=[blocky(rng, H, W, depth)])


def index_range(c, f=0):
    """(min, max) of the unclipped beta index and of the unclipped tC index over the luma edge segments of case c, with the pair of
    the CTB that holds q0,0: what the clips of 8.7.2.5.3 receive"""
    m = c["qp_map"].astype(np.int64)
    pr = c["pairs"][f].astype(np.int64)
    h, w = c["ph"], c["pw"]
    ib, it = [], []
    vb = c["vb"].reshape(h // 4, w // 8 + 1).astype(np.int64) & 3
    for y in range(0, h, 4):
        for x in range(8, w, 8):
            bs = vb[y // 4, x // 8]
            if bs:
                q = (m[y >> 3, x >> 3] + m[y >> 3, (x - 1) >> 3] + 1) >> 1
                ib.append(q + 2 * pr[y >> CTB_LOG2, x >> CTB_LOG2, 0])
                it.append(q + 2 * (bs - 1) + 2 * pr[y >> CTB_LOG2, x >> CTB_LOG2, 1])
    hb = c["hb"].reshape(h // 8 + 1, w // 4).astype(np.int64) & 3
    for y in range(8, h, 8):
        for x in range(0, w, 4):
            bs = hb[y // 8, x // 4]
            if bs:
                q = (m[y >> 3, x >> 3] + m[(y - 1) >> 3, x >> 3] + 1) >> 1
                ib.append(q + 2 * pr[y >> CTB_LOG2, x >> CTB_LOG2, 0])
                it.append(q + 2 * (bs - 1) + 2 * pr[y >> CTB_LOG2, x >> CTB_LOG2, 1])
    return (min(ib), max(ib)), (min(it), max(it))
