"""The vectors of the tests of SAO estimation with log2_sao_offset_scale (tests/test_sao_scale_cpu.py, tests/test_gpu_sao_scale.py):
configurations of depths, scales and lambdas, the palette and the index grid of each, the tie vectors of the candidates' comparison,
and the reference's results (tests/sao_scale_ref.py) -- computed once per process and shared, never changed."""
import numpy as np

import sao_decide_ref as D
import sao_scale_ref as R
import sao_stats_ref as S
from sao_decide_vectors import N_RECORDS, grid

# name -> (luma depth, chroma depth, luma scale, chroma scale, lambda_q8 luma, lambda_q8 chroma, statistics at the int32 ends)
SCALE_CONFIGS = {
    "12b_12b_k2_k2": (12, 12, 2, 2, 4096, 1500, False),
    "11b_12b_k1_k2": (11, 12, 1, 2, 700, 9000, False),
    "12b_10b_k1_k0": (12, 10, 1, 0, 20000, 1024, False),
    "8b_12b_k0_k1": (8, 12, 0, 1, 1024, 60000, False),
    "14b_16b_k2_k1": (14, 16, 2, 1, 3000, 3000, False),
    "12b_12b_k2_lambdas_0_int32_ends": (12, 12, 2, 2, 0, 0, True),
    "16b_12b_k2_lambdas_2p24_int32_ends": (16, 12, 2, 2, 1 << 24, 1 << 24, True),
    "12b_16b_k2_lambdas_0_and_2p24_int32_ends": (12, 16, 2, 2, 0, 1 << 24, True),
}


def record(rng, bit_depth, k, kind, *, extreme=False):
    """one statistics record.  kind 0: nothing counted ("not applied"); 1: edge bins alone; 2: band bins alone; 3: both.  Ordinary: a
    few -- now and then very few -- samples per bin, each bin with a mean error of its own inside +-((M + 1) << k); about one bin in
    three sits exactly on a rounding tie of the scaled mean (2|s| an odd multiple of n << k).  extreme: counts and sums at the int32 ends, and sums of
    +-6, which 1 or 3 samples at a scale of 2 put on a rounding tie"""
    st = np.zeros((), S.STATS_DTYPE)
    M = R.max_offset(bit_depth)

    def filled(shape):
        if extreme:
            return rng.choice([0, 1, 3, D.INT32_MAX], shape), rng.choice([D.INT32_MIN, D.INT32_MAX, -1, 1, -6, 6], shape)
        n = np.where(rng.integers(0, 4, shape) == 0, rng.integers(0, 6, shape), rng.integers(0, 400, shape))
        s = np.rint(n * rng.uniform(-(M + 1) << k, (M + 1) << k, shape)).astype(np.int64) + rng.integers(-3, 4, shape)
        nk = n << k                                                         # a tie needs an even n << k
        tie = (2 * rng.integers(0, M + 1, shape) + 1) * (nk // 2) * rng.choice([-1, 1], shape)
        return n, np.where((rng.integers(0, 3, shape) == 0) & (nk % 2 == 0), tie, s)
    if kind in (1, 3):
        st["eo_count"], s = filled((4, 4))
        if not extreme:
            s[:, :2], s[:, 2:] = np.abs(s[:, :2]), -np.abs(s[:, 2:])      # valleys ask for positive offsets, peaks for negative ones
        st["eo_sum"] = s
    if kind in (2, 3):
        first = int(rng.integers(0, 32))
        n, s = filled(8)
        for j in range(8):
            st["bo_count"][(first + j) & 31], st["bo_sum"][(first + j) & 31] = n[j], s[j]
    return st


KINDS = (0, 1, 2, 3, 3, 3)   # of the six bases of a palette


def palette(rng, bd_luma, bd_chroma, k_luma, k_chroma, *, variants=3, extreme=False):
    """six bases (one per entry of KINDS) of `variants` records (S_y, S_cb, S_cr) each: a base, then records close to it"""
    out = []
    for kind in KINDS:
        base = [record(rng, bd, k, kind, extreme=extreme) for bd, k in ((bd_luma, k_luma), (bd_chroma, k_chroma), (bd_chroma, k_chroma))]
        out.append(tuple(base))
        for _ in range(variants - 1):
            if extreme:
                out.append(tuple(record(rng, bd, k, kind, extreme=True) for bd, k in ((bd_luma, k_luma), (bd_chroma, k_chroma), (bd_chroma, k_chroma))))
            else:
                out.append(tuple(D.nudged(b, rng) for b in base))
    assert len(out) == N_RECORDS
    return out


def decider(name, chroma):
    bl, bc, kl, kc, ll, lc, extreme = SCALE_CONFIGS[name]
    rng = np.random.default_rng([len(name), bl, bc, kl, kc])
    return R.Decider(palette(rng, bl, bc, kl, kc, extreme=extreme), bd_luma=bl, bd_chroma=bc, lam_luma=ll, lam_chroma=lc, chroma=chroma,
                     k_luma=kl, k_chroma=kc)


_cases = {}


def case(name, chroma, cols, rows, layout="none"):
    """(decider, index grid, slice_idx, tile_idx, the reference's result)"""
    key = (name, chroma, cols, rows, layout)
    if key not in _cases:
        dec = _cases.setdefault(("decider", name, chroma), decider(name, chroma))
        idx = grid(name, cols, rows)
        sl, tl = D.layout(rows, cols, layout)
        res = dec.decide(idx, sl, tl)
        for a in [idx, res["decision"]] + [p for p in res["params"] if p is not None]:
            a.setflags(write=False)
        _cases[key] = (dec, idx, sl, tl, res)
    return _cases[key]


def picks(name, cols, rows):
    """the reference's picks on the statistics of case(name, True, cols, rows): {"stats": [Y, Cb, Cr], "luma": (params, None, delta_d),
    "chroma": (params_cb, params_cr, delta_d)}"""
    key = ("picks", name, cols, rows)
    if key not in _cases:
        bl, bc, kl, kc, ll, lc, _ = SCALE_CONFIGS[name]
        dec, idx, _, _, _ = case(name, True, cols, rows)
        st = dec.stats(idx)
        _cases[key] = {"stats": st, "luma": R.pick_plane(st[0], None, bl, ll, kl), "chroma": R.pick_plane(st[1], st[2], bc, lc, kc)}
    return _cases[key]


# ---- the tie vectors of the candidates' comparison ---------------------------------------------------------------------------------

def _stats(**bins):
    st = np.zeros((), S.STATS_DTYPE)
    for field, entries in bins.items():
        for at, v in entries.items():
            st[field][at] = v
    return st


def tie_vectors():
    """name -> (st_a, st_b or None, bit depth, k, lambda_q8, the (type, cls) the rule must give per component)"""
    empty = np.zeros((), S.STATS_DTYPE)
    band = lambda b: _stats(bo_count={b: 50}, bo_sum={b: 50 * 40})                            # a mean error of 40: o = 40 at k = 2
    twins = _stats(eo_count={(1, 0): 30, (3, 0): 30, (1, 3): 7, (3, 3): 7}, eo_sum={(1, 0): 30 * 24, (3, 0): 30 * 24, (1, 3): -7 * 9, (3, 3): -7 * 9})
    e = _stats(eo_count={(2, 1): 10}, eo_sum={(2, 1): 200})                                     # the same bin as an edge bin and as a band
    b = _stats(bo_count={9: 10}, bo_sum={9: 200})
    eb = _stats(eo_count={(2, 1): 10}, eo_sum={(2, 1): 200}, bo_count={9: 10}, bo_sum={9: 200})
    return {
        "band_0_alone": (band(0), None, 12, 2, 1024, [(1, 0)]),                                 # positions 29, 30, 31 and 0 tie
        "band_5_alone": (band(5), None, 12, 2, 1024, [(1, 2)]),                                 # positions 2..5 tie
        "band_0_alone_joint": (band(0), band(5), 12, 2, 1024, [(1, 0), (1, 2)]),
        "twin_edge_classes": (twins, None, 12, 2, 1024, [(2, 1)]),
        "twin_edge_classes_joint": (twins, twins, 11, 1, 300, [(2, 1), (2, 1)]),
        "nothing_lambda_0": (empty, None, 12, 2, 0, [(0, 0)]),
        "nothing_lambda_0_joint": (empty, empty, 12, 2, 0, [(0, 0), (0, 0)]),
        "joint_band_equals_edge": (eb, empty, 12, 2, 0, [(2, 2), (2, 2)]),                      # lambda 0: costs are distortions alone
        "joint_band_equals_edge_split": (e, b, 12, 2, 0, [(2, 2), (2, 2)]),
    }


def biased(rng, n_records=24):
    """12-bit records whose bins carry a mean error of about +-100: more than 31 can take away, within reach of 31 << 2"""
    out = []
    for _ in range(n_records):
        st = np.zeros((), S.STATS_DTYPE)
        n = rng.integers(50, 400, (4, 4))
        mean = rng.uniform(85, 115, (4, 4)) * np.array([1, 1, -1, -1])
        st["eo_count"], st["eo_sum"] = n, np.rint(n * mean)
        first = int(rng.integers(0, 32))
        for j in range(6):
            m = int(rng.integers(50, 400))
            st["bo_count"][(first + j) & 31], st["bo_sum"][(first + j) & 31] = m, int(m * rng.uniform(85, 115) * rng.choice([-1, 1]))
        out.append(st)
    return out
