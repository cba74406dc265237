"""The vectors of the tests of the slice-level SAO flags (tests/test_sao_slice_flags_cpu.py, tests/test_gpu_sao_slice_flags.py): the
palettes of sao_decide_ref (ordinary and at the int32 ends; for a scale above 0 those of sao_scale_vectors), every record followed by
its variants with zeroed luma statistics, zeroed chroma statistics and all zero; the grids of sao_decide_vectors, in which slice s takes
variant s % 4 of every record -- so a slice is built to want the pair 3, 2, 1 or 0 --; and the reference's results
(tests/sao_slice_ref.py), computed once per process and shared, never changed."""
import numpy as np

import sao_decide_ref as D
import sao_decide_vectors as DV
import sao_scale_vectors as SV
import sao_slice_ref as R
import sao_stats_ref as S

# name -> (luma depth, chroma depth, luma scale, chroma scale, lambda_q8 luma, lambda_q8 chroma, statistics at the int32 ends)
CONFIGS = {
    "8b_equal": (8, 8, 0, 0, 1024, 1024, False),
    "10b_unequal": (10, 10, 0, 0, 40000, 1500, False),
    "12b_k2_unequal": (12, 12, 2, 2, 4096, 1500, False),
    "8b_lambdas_0": (8, 8, 0, 0, 0, 0, False),
    "10b_lambdas_2p24_int32_ends": (10, 10, 0, 0, 1 << 24, 1 << 24, True),
    "12b_k2_lambdas_2p20_2p24_int32_ends": (12, 12, 2, 2, 1 << 20, 1 << 24, True),
}
CENSUS = ("8b_equal", "10b_unequal")            # lambdas of 1024 and 40000: every pair is chosen on 5x7 and 61x34, `slices` and `both`
EXTREME = ("10b_lambdas_2p24_int32_ends", "12b_k2_lambdas_2p20_2p24_int32_ends")
LAYOUTS = ("slices", "tiles", "both", "ctb_slices")
MAX_SLICES = 600                                # of the choosing entry


def grown(palette):
    """every record followed by: luma zeroed, chroma zeroed, all zero"""
    zero = np.zeros((), S.STATS_DTYPE)
    out = []
    for sy, scb, scr in palette:
        out += [(sy, scb, scr), (zero, scb, scr), (sy, zero, zero), (zero, zero, zero)]
    return out


def decider(name, chroma):
    bl, bc, kl, kc, ll, lc, extreme = CONFIGS[name]
    rng = np.random.default_rng([len(name), bl, bc, kl])
    pal = D.palette(rng, bl, bc, extreme=extreme) if extreme or kl == 0 else SV.palette(rng, bl, bc, kl, kc)
    return R.Decider(grown(pal), bd_luma=bl, bd_chroma=bc, lam_luma=ll, lam_chroma=lc, chroma=chroma, k_luma=kl, k_chroma=kc)


def dealt(idx, sl):
    """the index grid over the grown palette: slice s takes variant s % 4"""
    return idx * 4 + (0 if sl is None else sl.astype(np.int64) % 4)


_cases = {}


def case(name, chroma, cols, rows, layout="none", short=False):
    """(decider, index grid, slice_idx, tile_idx, n_slices): n_slices is one more than the slices there are -- the last is empty --
    or, with short, one fewer: the CTBs of the last slice lie beyond n_slices"""
    key = (name, chroma, cols, rows, layout, short)
    if key not in _cases:
        dec = _cases.setdefault(("decider", name, chroma), decider(name, chroma))
        sl, tl = D.layout(rows, cols, layout)
        idx = dealt(DV.grid(name, cols, rows), sl)
        top = 0 if sl is None else int(sl.max())
        idx.setflags(write=False)
        _cases[key] = (dec, idx, sl, tl, max(top, 1) if short else top + 2)
    return _cases[key]


def chosen(name, chroma, cols, rows, layout="none", short=False):
    """the reference's choice on case(...): sao_slice_ref.Decider.choose"""
    key = ("chosen", name, chroma, cols, rows, layout, short)
    if key not in _cases:
        dec, idx, sl, tl, n = case(name, chroma, cols, rows, layout, short)
        res = dec.choose(idx, sl, tl, n)
        for a in [res["decision"]] + [p for p in res["params"] if p is not None]:
            a.setflags(write=False)
        _cases[key] = res
    return _cases[key]


def given_flags(n_slices, seed):
    """flag bytes for the decision under given flags: every pair, with higher bits set in some of them"""
    rng = np.random.default_rng([n_slices, seed])
    return (rng.integers(0, 4, n_slices) | (rng.integers(0, 2, n_slices) * 0xA4)).astype(np.uint8)
