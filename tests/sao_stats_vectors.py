"""Vectors that take SAO parameter estimation (hevcdbk_sao_stats_device, hevcdbk_sao_pick_device) to its edges: every legal CTB
shape, full-range content with 0 against max across every block, CTB and region border, every boundary byte, padded and shared
small operands, every side of the vector / scalar load choice, and synthetic statistics tables -- extreme, tie-prone, sparse,
plain -- plus one hand-built table whose expected parameters are literals.  The expected statistics and parameters are those of
tests/sao_stats_ref.py; nothing here looks at the library.

TEST INFRASTRUCTURE ONLY.  Everything is built once per process and handed out read-only."""
import functools

import numpy as np

import h265_vectors as hv
import rext_oracle as ro
import sao_bytes_vectors as B
import sao_stats_ref as S

# ---- statistics ---------------------------------------------------------------------------------------------------------------

CTB_SHAPES = ((3, 3), (3, 4), (4, 4), (4, 5), (5, 5), (5, 6), (6, 6))            # every (log2 w, log2 h) the entry accepts
DEPTHS = {"8b": (8, 1), "8b_in_16": (8, 2), "10b": (10, 2), "16b": (16, 2)}      # name -> (bit depth, bytes per sample)
# more than one 64x64 region each way, a region whose first block is the 4-wide last one, a last block row of 4; and the minimal ones
PLANES = ((132, 68), (8, 8), (12, 20))
KEEP_POISON, NOX_POISON = 1, 0xFF          # beyond the columns / rows of a padded operand: everything kept, everything forbidden


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def content(w, h, depth, frames=1, seed=0):
    """(rec, org), frames x h x w each.  rec: h265_vectors.sao_full_range (ramps through every band, runs and checkers of 0 and
    max, plateaus with spikes, noise) with 0 against max across EVERY column and row that is a multiple of 8 -- hence of every CTB
    size and of 64; org: uniform over the whole range, with max against 0 and 0 against max planted once each where rec allows."""
    bd, sb = DEPTHS[depth]
    rng = np.random.default_rng([seed, w, h, bd, sb, frames])
    max_v = (1 << bd) - 1
    w8, h8 = -(-w // 8) * 8, -(-h // 8) * 8
    dt = np.uint8 if sb == 1 else np.uint16
    rec = np.zeros((frames, h, w), dt)
    for f in range(frames):
        p, _, _ = hv.sao_full_range(bd, 6, rng, w=w8, h=h8, stripe_cols=[c for k in range(8, w8, 8) for c in (k - 1, k)],
                                    stripe_rows=[r for k in range(8, h8, 8) for r in (k - 1, k)])
        rec[f] = p[:h, :w]
    org = rng.integers(0, max_v + 1, (frames, h, w)).astype(dt)
    for v in (0, max_v):
        at = np.argwhere(rec == v)
        if len(at):
            f, y, x = at[int(rng.integers(0, len(at)))]
            org[f, y, x] = max_v - v
    return _frozen(rec, org)


@functools.lru_cache(maxsize=None)
def keep_map(w, h, frames=1, seed=0):
    rng = np.random.default_rng([seed, w, h, 11])
    return _frozen(np.stack([S.keep_map(w, h, rng) for _ in range(frames)]))


@functools.lru_cache(maxsize=None)
def border_bytes(w, h, lw, lh, frames=1, seed=0):
    rows, cols = S.grid(w, h, lw, lh)
    return _frozen(np.random.default_rng([seed, w, h, lw, lh, 13]).integers(0, 256, (frames, rows, cols)).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def reference(w, h, depth, lw, lh, keep, nox, frames=1, seed=0):
    """(frames, rows, cols) statistics of content() under keep_map() / border_bytes() (keep, nox: bool)"""
    rec, org = content(w, h, depth, frames, seed)
    k = keep_map(w, h, frames, seed) if keep else None
    b = border_bytes(w, h, lw, lh, frames, seed) if nox else None
    return _frozen(np.stack([S.stats_plane(rec[f], org[f], lw, lh, DEPTHS[depth][0], keep=None if k is None else k[f], nox=None if b is None else b[f])
                             for f in range(frames)]))


def shape_set(depth, lw, lh):
    """the (w, h, keep) of one (shape, depth) set: every plane with and without a keep map, random bytes throughout"""
    return [(w, h, keep) for (w, h) in PLANES for keep in (False, True)]


def padded(a, cols, rows, poison):
    """(n, r, c) bytes -> (n, r + rows, c + cols) with poison in the excess: a stride beyond the columns, a frame stride with a gap"""
    a = np.asarray(a, np.uint8)
    out = np.full((a.shape[0], a.shape[1] + rows, a.shape[2] + cols), poison, np.uint8)
    out[:, : a.shape[1], : a.shape[2]] = a
    return out


# the alignment matrix: name -> how the two planes lie in memory, in SAMPLES (offset of the base from an aligned address, pitch
# beyond the 76 columns, extra frame stride).  "aligned" takes four samples per load; every other one must run sample by sample
ALIGN_W, ALIGN_H, ALIGN_FRAMES, ALIGN_SHAPE = 76, 44, 3, (4, 5)
ALIGNMENTS = {"aligned": {}}
for _o in (1, 2, 3):
    ALIGNMENTS["rec_base_%d" % _o] = {"rec_off": _o}
    ALIGNMENTS["org_base_%d" % _o] = {"org_off": _o}
ALIGNMENTS.update({"rec_pitch_odd": {"pitch": 77, "org_pitch": 76}, "org_pitch_odd": {"pitch": 76, "org_pitch": 77},
                   "aligned_pitches_differ": {"pitch": 80, "org_pitch": 84}, "rec_frame_stride": {"rec_gap": 2}, "org_frame_stride": {"org_gap": 1}})
del _o
VECTOR_LOADS = ("aligned", "aligned_pitches_differ")


# ---- every byte ---------------------------------------------------------------------------------------------------------------

# (log2 w, log2 h) -> (CTB rows, CTB columns, frames): 256 interior CTBs, one per byte value; frames where CTBs are large
EVERY_BYTE = {(3, 3): (18, 18, 1), (4, 5): (18, 18, 1), (6, 6): (6, 6, 16)}


@functools.lru_cache(maxsize=None)
def every_byte(lw, lh, depth="8b"):
    """the planted content of sao_bytes_vectors.every_byte (its eight strict extrema per CTB: four corners, four side middles) with
    every byte value 0..255 on a CTB that has all eight neighbours; the rim's bytes are random.  org: rec plus small noise"""
    rows, cols, frames = EVERY_BYTE[(lw, lh)]
    bd, sb = DEPTHS[depth]
    rng = np.random.default_rng([lw, lh, bd, 29])
    assert frames * (rows - 2) * (cols - 2) == 256
    dt = np.uint8 if sb == 1 else np.uint16
    mid = 1 << (bd - 1)
    w, h = cols << lw, rows << lh
    rec = rng.integers(mid - 2, mid + 3, (frames, h, w)).astype(dt)
    for f in range(frames):
        B._plant(rec[f], lw, lh, rows, cols, mid - 4, mid + 4)
    org = (rec.astype(np.int64) + rng.integers(-3, 4, rec.shape)).astype(dt)
    nox = rng.integers(0, 256, (frames, rows, cols)).astype(np.uint8)
    nox[:, 1:-1, 1:-1] = rng.permutation(256).reshape(frames, rows - 2, cols - 2)
    return {"w": w, "h": h, "bd": bd, "lw": lw, "lh": lh, "rows": rows, "cols": cols, "rec": _frozen(rec), "org": _frozen(org), "nox": _frozen(nox)}


@functools.lru_cache(maxsize=None)
def every_byte_reference(lw, lh, flip=0):
    """(frames, rows, cols) statistics of every_byte() with the bits `flip` turned over in every byte"""
    v = every_byte(lw, lh)
    return _frozen(np.stack([S.stats_plane(v["rec"][f], v["org"][f], lw, lh, v["bd"], nox=v["nox"][f] ^ np.uint8(flip)) for f in range(len(v["rec"]))]))


# ---- pick tables --------------------------------------------------------------------------------------------------------------

PICK_KINDS = ("extreme", "tie", "sparse", "plain")
PICK_DEPTHS = (8, 9, 10, 16)                # M = 7, 15, 31, 31
PICK_LAMBDAS = (0, 1, 255, 1024, 1 << 24)
PICK_GRID = (2, 3, 4)                       # frames, CTB rows, CTB columns
N_MAX, D_MAX = 4096, 65535                  # a bin of a 64x64 CTB at 16 bit: n = 4096, |s| = 4096 * 65535 = 268,431,360


@functools.lru_cache(maxsize=None)
def pick_table(kind, bd, comp=0):
    """PICK_GRID statistics of one component.  The kernel reads 16 edge and 32 band (n, s) pairs per CTB and nothing else: the
    tables need not be the statistics of any plane"""
    M = S.max_offset(bd)
    rng = np.random.default_rng([PICK_KINDS.index(kind), bd, comp, 41])
    frames, rows, cols = PICK_GRID
    t = np.zeros(PICK_GRID, S.STATS_DTYPE)
    for i in range(frames * rows * cols):
        n, s = np.zeros(48, np.int64), np.zeros(48, np.int64)            # 16 edge bins [class][category - 1], then 32 bands
        if kind == "extreme":
            n = rng.choice([0, 1, N_MAX], 48)
            s = n * rng.choice([D_MAX, -D_MAX, 1, -1, 0], 48)
        elif kind == "tie":
            # 2s = n (2o - 1): o and o - 1 cost the same at lambda 0; then whole classes and bands copied, so that candidates tie too
            n = 2 * rng.integers(1, 100, 48)
            o = rng.integers(-M, M + 2, 48)
            s = n * (2 * o - 1) // 2
            if i % 2:
                k0, k1 = rng.choice(4, 2, replace=False)
                n[4 * k1:4 * k1 + 4], s[4 * k1:4 * k1 + 4] = n[4 * k0:4 * k0 + 4], s[4 * k0:4 * k0 + 4]
            if i % 3:
                j = np.arange(32)
                n[16:], s[16:] = n[16 + (j & 7)], s[16 + (j & 7)]          # bands of period 8: four positions of every cost
        else:
            n = rng.integers(1, N_MAX + 1, 48)
            mean = rng.uniform(-1.5 * M, 1.5 * M, 48)
            if kind == "sparse":
                n = np.where(rng.integers(0, 8, 48) == 0, n, 0)
            elif i % 2:
                # a CTB whose four bands from position p on carry everything: p walks 29, 30, 31 first, and wraps
                p = (29 + i // 2) & 31 if i < 8 else int(rng.integers(0, 32))
                mean[:16] *= 0.05
                win = 16 + ((p + np.arange(4)) & 31)
                far = np.ones(48, bool)
                far[:16] = False
                far[win] = False
                n[far] = rng.integers(0, 3, int(far.sum()))
                mean[win] = rng.choice([-1, 1], 4) * rng.uniform(0.6 * M, 3 * M, 4)
            else:
                # an edge CTB: sums of the sign an encoder meets (valleys rise, peaks fall), bands weak
                e = np.arange(16)
                mean[:16] = np.where((e & 3) < 2, 1, -1) * np.abs(mean[:16])
                mean[16:] *= 0.1
            s = np.rint(n * mean).astype(np.int64)
        c = t.reshape(-1)[i]
        c["eo_count"], c["eo_sum"], c["bo_count"], c["bo_sum"] = n[:16].reshape(4, 4), s[:16].reshape(4, 4), n[16:], s[16:]
    assert int(np.abs(t["eo_sum"]).max()) <= N_MAX * D_MAX and int(np.abs(t["bo_sum"]).max()) <= N_MAX * D_MAX
    return _frozen(t)


@functools.lru_cache(maxsize=None)
def pick_expected(kind, bd, lam, joint):
    """per frame (params_a, params_b or None, delta_d) of pick_table(kind, bd) -- beside pick_table(kind, bd, 1) if joint -- by the
    plain-int statement"""
    a, b = pick_table(kind, bd), pick_table(kind, bd, 1) if joint else None
    return [S.pick_plane(a[f], None if b is None else b[f], bd, lam) for f in range(a.shape[0])]


def pick_census(joint):
    """over every random table, depth and lambda: CTBs per type, with a wrapped band position (29..31), with an offset of magnitude M"""
    out = {"type0": 0, "type1": 0, "type2": 0, "wrapped": 0, "offset_M": 0}
    for kind in PICK_KINDS:
        for bd in PICK_DEPTHS:
            for lam in PICK_LAMBDAS:
                for pa, pb, _ in pick_expected(kind, bd, lam, joint):
                    for p in (pa, pb) if joint else (pa,):
                        for t in range(3):
                            out["type%d" % t] += int((p["type"] == t).sum())
                        out["wrapped"] += int(((p["type"] == 1) & (p["cls"] >= 29)).sum())
                        out["offset_M"] += int(((p["type"] != 0) & (np.abs(p["offset"].astype(int)).max(axis=-1) == S.max_offset(bd))).sum())
    return out


# ---- the hand-built table -------------------------------------------------------------------------------------------------------
# Each case: bit depth, lambda_q8, the non-empty bins of Cb (and of Cr: a joint case), and the EXPECTED parameters and delta_d as
# literals worked out by hand from the text of include/hevc_deblock.h -- cost = (n o^2 - 2 o s) * 256 + lambda * bits(o), an empty
# bin costs lambda * 1 -- not from running anything.  Bins: ("e", class, category - 1) or ("b", band) -> (n, s).

def _case(bd, lam, a, want_a, dd, b=None, want_b=None):
    return {"bd": bd, "lam": lam, "a": a, "b": b, "want_a": want_a, "want_b": want_b, "dd": dd}


OFF = (0, 0, (0, 0, 0, 0))
# (n, s) = (10, 30): o0 = 70 / 20 = 3, delta(3) = 90 - 180 = -90, delta(2) = -80: offset 3.  (10, -30): offset -3, -90 likewise.
HAND = {
    # every candidate costs 0; "not applied" comes first
    "all_zero_lambda_0": _case(8, 0, {}, OFF, 0),
    # classes 1 and 3 cost -90 * 256 each: the earlier
    "equal_edge_classes": _case(8, 0, {("e", 1, 0): (10, 30), ("e", 3, 0): (10, 30)}, (2, 1, (3, 0, 0, 0)), -90),
    # class 2 and the band positions 2..5 cost the same: edge classes come before band positions
    "edge_equals_band": _case(8, 0, {("e", 2, 0): (10, 30), ("b", 5): (10, 30)}, (2, 2, (3, 0, 0, 0)), -90),
    # positions 7..10 and 17..20 cost the same: 7
    "equal_band_positions": _case(8, 0, {("b", 10): (10, 30), ("b", 20): (10, 30)}, (1, 7, (0, 0, 0, 3)), -90),
    # only position 30 holds band 30 and band 1: bands 30, 31, 0, 1
    "band_position_wraps": _case(8, 0, {("b", 30): (10, 30), ("b", 1): (10, -30)}, (1, 30, (3, 0, 0, -3)), -180),
    # lambda = 1.0.  (6, 7): o0 = 20 / 12 = 1, cost(1) = (6 - 14) * 256 + 256 * 2 = -1536 < cost(0) = 256.  Class 0:
    # 4 * 256 - 1536 + 3 * 256 = 256 = lambda * 1 exactly: not below "not applied"
    "cost_equals_not_applied": _case(8, 256, {("e", 0, 0): (6, 7)}, OFF, 0),
    # (6, 8): cost(1) = (6 - 16) * 256 + 512 = -2048, class 0 = 1024 - 2048 + 768 = -256 < 256
    "cost_one_step_below": _case(8, 256, {("e", 0, 0): (6, 8)}, (2, 0, (1, 0, 0, 0)), -10),
    # (2, 5): o0 = 12 / 4 = 3, delta(3) = 18 - 30 = -12 = delta(2) = 8 - 20, delta(1) = -8: the one nearer 0
    "offset_tie_nearer_0": _case(8, 0, {("e", 0, 0): (2, 5)}, (2, 0, (2, 0, 0, 0)), -12),
    "band_offset_tie_nearer_0": _case(8, 0, {("b", 8): (2, -5)}, (1, 5, (0, 0, 0, -2)), -12),
    # categories 1, 2 take 0..M and 3, 4 take -M..0: a sum of the other sign gives 0, whatever it would gain
    "wrong_sign_is_offset_0": _case(8, 0, {("e", 1, 0): (10, 30), ("e", 1, 1): (5, -20), ("e", 1, 2): (5, 20), ("e", 1, 3): (10, -30)},
                                    (2, 1, (3, 0, 0, -3)), -180),
    # the rounded mean is +-100; M = 7, 15, 31, 31 at depths 8, 9, 10 and 16: delta = M^2 - 200 M per bin
    "clamped_to_M_8b": _case(8, 0, {("e", 0, 0): (1, 100), ("e", 0, 3): (1, -100)}, (2, 0, (7, 0, 0, -7)), 2 * (49 - 1400)),
    "clamped_to_M_9b": _case(9, 0, {("e", 0, 0): (1, 100), ("e", 0, 3): (1, -100)}, (2, 0, (15, 0, 0, -15)), 2 * (225 - 3000)),
    "clamped_to_M_10b": _case(10, 0, {("b", 3): (1, 100), ("b", 4): (1, -100)}, (1, 1, (0, 0, 31, -31)), 2 * (961 - 6200)),
    "clamped_to_M_16b": _case(16, 0, {("e", 0, 0): (1, 100), ("e", 0, 3): (1, -100)}, (2, 0, (31, 0, 0, -31)), 2 * (961 - 6200)),
    # the largest legal bin under the largest lambda: delta(31) = 4096 * 961 - 62 * 268431360 = -16,638,808,064; the class costs
    # delta * 256 + lambda * (4 + 31 + 3), far below lambda
    "largest_bin_largest_lambda": _case(16, 1 << 24, {("e", 0, 0): (4096, 268431360)}, (2, 0, (31, 0, 0, 0)), -16638808064),
    "largest_bin_negative": _case(16, 1 << 24, {("b", 31): (4096, -268431360)}, (1, 28, (0, 0, 0, -31)), -16638808064),
    # Cb alone takes edge class 2 (-90), Cr alone band 12 ((10, 40): o0 = 90 / 20 = 4, delta(4) = 160 - 320 = -160, delta(3) = -150).
    # Together: class 2 costs -90 * 256, band -160 * 256: band for both, Cb's best position the lowest of 32 that cost 0
    "joint_cb_edge_cr_band": _case(8, 0, {("e", 2, 0): (10, 30)}, (1, 0, (0, 0, 0, 0)), -160, {("b", 12): (10, 40)}, (1, 9, (0, 0, 0, 4))),
    # (10, 60): offset 6, delta = 360 - 720 = -360 < -160: class 2 for both, Cr with nothing to gain from it
    "joint_cb_edge_wins": _case(8, 0, {("e", 2, 0): (10, 60)}, (2, 2, (6, 0, 0, 0)), -360, {("b", 12): (10, 40)}, (2, 2, (0, 0, 0, 0))),
    # per component the lowest of its tied positions
    "joint_band_ties": _case(8, 0, {("b", 10): (10, 30), ("b", 20): (10, 30)}, (1, 7, (0, 0, 0, 3)), -180,
                             {("b", 15): (10, 30), ("b", 5): (10, 30)}, (1, 2, (0, 0, 0, 3))),
    # both components' class 3 ties with both components' class 1; joint "not applied" at all-zero statistics
    "joint_equal_edge_classes": _case(8, 0, {("e", 1, 0): (10, 30), ("e", 3, 1): (10, 30)}, (2, 1, (3, 0, 0, 0)), -180,
                                      {("e", 1, 3): (10, -30), ("e", 3, 2): (10, -30)}, (2, 1, (0, 0, 0, -3))),
    "joint_all_zero": _case(8, 0, {}, OFF, 0, {}, OFF),
}


def hand_stats(bins):
    st = np.zeros((1, 1, 1), S.STATS_DTYPE)
    for key, (n, s) in bins.items():
        if key[0] == "e":
            st["eo_count"][0, 0, 0, key[1], key[2]], st["eo_sum"][0, 0, 0, key[1], key[2]] = n, s
        else:
            st["bo_count"][0, 0, 0, key[1]], st["bo_sum"][0, 0, 0, key[1]] = n, s
    return st


def hand_params(want):
    p = np.zeros((1, 1, 1), ro.SAO_CTB_DTYPE)
    p[0, 0, 0] = want
    return p
