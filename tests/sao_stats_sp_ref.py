"""SAO statistics of a semi-planar chroma plane (hevcdbk_sao_stats_device_sp): the statement and the vectors.

THE STATEMENT contains no arithmetic of its own: the statistics of component c of an (h, w, 2) plane of Cb / Cr pairs are
sao_stats_ref.stats_plane of the (h, w) plane of that component -- the even samples of every row for Cb, the odd ones for Cr -- with
the same keep map (one byte per 8x8 PAIRS) and the same border bytes (one per CTB of the per-component grid).

THE VECTORS: Cb and Cr of rec and of org come from sao_stats_ref.planes with independent seeds, hence different content and a
different bias per 8x8 block, and no offset |o| <= M reaches the clip; the full-range vectors take h265_vectors.sao_full_range per
component with the two components in opposite phase (Cr is the complement, max - v, of its own draw: where Cb's planted borders hold
0 against max, Cr's hold max against 0).  census() states what every vector must satisfy, from the reference alone; a seed that
fails it is replaced by the next one and recorded in SEEDS.

TEST INFRASTRUCTURE ONLY, parity unpinned like the rest of SAO.  Everything is built once per process and handed out read-only."""
import functools

import numpy as np

import h265_vectors as hv
import sao_stats_ref as S

PLANES = ((132, 68), (8, 8), (12, 20), (72, 40))     # pairs: three regions by two with a 4-pair last block and block row; the minimal ones
CTBS = (3, 4, 5)
DEPTHS = {"8b": (8, 1), "8b_in_16": (8, 2), "10b": (10, 2), "12b": (12, 2), "14b": (14, 2), "16b": (16, 2)}      # name -> (bit depth, bytes per sample)
KINDS = ("planes", "full")

# every vector the tests use: (w, h, depth, kind, frames)
VECTORS = [(w, h, d, k, 1) for (w, h) in PLANES for d in ("8b", "8b_in_16", "10b", "14b", "16b") for k in KINDS] + \
          [(76, 44, "8b", "planes", 3), (76, 44, "10b", "planes", 3), (72, 40, "10b", "planes", 3), (72, 40, "8b", "planes", 2),
           (96, 136, "10b", "planes", 2), (136, 72, "12b", "planes", 2)]

# vector -> the first seed with which every frame passes census_fails() at every CTB size; 0 where not listed
SEEDS = {(8, 8, "8b_in_16", "full", 1): 2, (8, 8, "10b", "full", 1): 6, (8, 8, "14b", "full", 1): 6, (12, 20, "8b", "full", 1): 1,
         (72, 40, "16b", "full", 1): 1}


def stats_pairs(rec, org, lg, bd, *, keep=None, nox=None):
    """(Cb's, Cr's) statistics of (h, w, 2) planes: (rows, cols) of sao_stats_ref.STATS_DTYPE each"""
    return tuple(S.stats_plane(rec[..., c], org[..., c], lg, lg, bd, keep=keep, nox=nox) for c in (0, 1))


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def _draw(w, h, depth, kind, frames, seed):
    bd, sb = DEPTHS[depth]
    dt = np.uint8 if sb == 1 else np.uint16
    max_v = (1 << bd) - 1
    rec, org = np.zeros((frames, h, w, 2), dt), np.zeros((frames, h, w, 2), dt)
    for c in (0, 1):
        rng = np.random.default_rng([seed, w, h, bd, sb, frames, KINDS.index(kind), c])
        if kind == "planes":
            r, o = S.planes(w, h, bd, rng, n=frames)
            rec[..., c], org[..., c] = r, o
        else:
            w8, h8 = -(-w // 8) * 8, -(-h // 8) * 8
            for f in range(frames):
                p, _, _ = hv.sao_full_range(bd, 5, rng, w=w8, h=h8, stripe_cols=[x for k in range(8, w8, 8) for x in (k - 1, k)],
                                            stripe_rows=[y for k in range(8, h8, 8) for y in (k - 1, k)])
                rec[f, :, :, c] = (max_v - p if c else p)[:h, :w]
            org[..., c] = rng.integers(0, max_v + 1, (frames, h, w))
    return rec, org


@functools.lru_cache(maxsize=None)
def content(w, h, depth, kind="planes", frames=1):
    """(rec, org), frames x h x w x 2 each"""
    return _frozen(*_draw(w, h, depth, kind, frames, SEEDS.get((w, h, depth, kind, frames), 0)))


def census_fails(rec, org, bd, lg):
    """what a frame (h, w, 2) fails of the conditions on the vectors, per CTB of its borderless, nothing-kept statistics: the Cb entry
    differs from the Cr entry; every edge class has a non-empty category in both components; at least two bands are hit per component"""
    cb, cr = stats_pairs(rec, org, lg, bd)
    out = []
    same = (cb.view(np.int32).reshape(cb.shape + (96,)) == cr.view(np.int32).reshape(cr.shape + (96,))).all(axis=-1)
    if same.any():
        out.append(("Cb == Cr", np.argwhere(same)[:2].tolist()))
    for name, st in (("Cb", cb), ("Cr", cr)):
        empty = (st["eo_count"].sum(axis=-1) == 0).any(axis=-1)
        if empty.any():
            out.append((name + ": an edge class without a category", np.argwhere(empty)[:2].tolist()))
        few = (st["bo_count"] > 0).sum(axis=-1) < 2
        if few.any():
            out.append((name + ": fewer than two bands", np.argwhere(few)[:2].tolist()))
    return out


@functools.lru_cache(maxsize=None)
def keep_map(w, h, frames=1):
    rng = np.random.default_rng([w, h, frames, 11])
    return _frozen(np.stack([S.keep_map(w, h, rng) for _ in range(frames)]))


@functools.lru_cache(maxsize=None)
def border_bytes(w, h, lg, frames=1):
    rows, cols = S.grid(w, h, lg, lg)
    return _frozen(np.random.default_rng([w, h, lg, frames, 13]).integers(0, 256, (frames, rows, cols)).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def reference(w, h, depth, kind, lg, keep, nox, frames=1):
    """(frames, 2, rows, cols) statistics of content() under keep_map() / border_bytes() (keep, nox: bool); [:, 0] is Cb's"""
    rec, org = content(w, h, depth, kind, frames)
    k = keep_map(w, h, frames) if keep else None
    b = border_bytes(w, h, lg, frames) if nox else None
    return _frozen(np.stack([np.stack(stats_pairs(rec[f], org[f], lg, DEPTHS[depth][0], keep=None if k is None else k[f],
                                                  nox=None if b is None else b[f])) for f in range(frames)]))


def padded(a, cols, rows, poison):
    """(n, r, c) bytes -> (n, r + rows, c + cols) with poison in the excess: a stride beyond the columns, a frame stride with a gap"""
    a = np.asarray(a, np.uint8)
    out = np.full((a.shape[0], a.shape[1] + rows, a.shape[2] + cols), poison, np.uint8)
    out[:, : a.shape[1], : a.shape[2]] = a
    return out


KEEP_POISON, NOX_POISON = 1, 0xFF          # beyond the columns / rows of a padded operand: everything kept, everything forbidden

# the load choice: how the two planes lie in memory, in SAMPLES (offset of the base from an aligned address, pitch beyond the
# 2 * 76 samples of a row, extra frame stride).  Rows that start at a multiple of four pairs -- eight samples -- take wide loads
ALIGN_W, ALIGN_H, ALIGN_FRAMES, ALIGN_LG = 76, 44, 3, 4
ALIGNMENTS = {"aligned": {}, "aligned_pitches_differ": {"pitch": 160, "org_pitch": 168}, "rec_base_1_sample": {"rec_off": 1},
              "org_base_1_sample": {"org_off": 1}}
for _o in (1, 2, 3):                       # pairs
    ALIGNMENTS["rec_base_%d" % _o] = {"rec_off": 2 * _o}
    ALIGNMENTS["org_base_%d" % _o] = {"org_off": 2 * _o}
    ALIGNMENTS["rec_pitch_%d" % _o] = {"pitch": 152 + 2 * _o, "org_pitch": 152}
    ALIGNMENTS["org_pitch_%d" % _o] = {"pitch": 152, "org_pitch": 152 + 2 * _o}
    ALIGNMENTS["rec_frame_stride_%d" % _o] = {"rec_gap": 2 * _o}
    ALIGNMENTS["org_frame_stride_%d" % _o] = {"org_gap": 2 * _o}
del _o
WIDE_LOADS = ("aligned", "aligned_pitches_differ")


def takes_wide_loads(kw):
    """a condition on the vectors: which side of the load choice a case of ALIGNMENTS lies on"""
    pitch = kw.get("pitch", 2 * ALIGN_W)
    return all(v % 8 == 0 for v in (kw.get("rec_off", 0), kw.get("org_off", 0), kw.get("rec_gap", 0), kw.get("org_gap", 0), pitch,
                                    kw.get("org_pitch", pitch)))
