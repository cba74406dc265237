"""The vectors of the SAO decision tests (tests/test_sao_decide_cpu.py, tests/test_gpu_sao_decide.py): configurations of depths and
lambdas, the palette and the index grid of each, and the reference's result (tests/sao_decide_ref.py) -- computed once per process and
shared, never changed."""
import numpy as np

import sao_decide_ref as D

# name -> (luma depth, chroma depth, lambda_q8 luma, lambda_q8 chroma, statistics at the int32 ends)
CONFIGS = {
    "8b_8b_equal": (8, 8, 1024, 1024, False),
    "10b_10b_unequal": (10, 10, 4096, 1500, False),
    "8b_12b_unequal": (8, 12, 700, 9000, False),
    "10b_8b_luma_lambda_0": (10, 8, 0, 5000, False),
    "8b_10b_lambdas_0": (8, 10, 0, 0, False),
    "10b_10b_lambdas_0_int32_ends": (10, 10, 0, 0, True),
    "10b_12b_lambdas_2p24_int32_ends": (10, 12, 1 << 24, 1 << 24, True),
    "8b_8b_lambdas_2p24_and_1_int32_ends": (8, 8, 1 << 24, 1, True),
}
CENSUS = ("8b_8b_equal", "10b_10b_unequal")      # the configurations whose 5x7 and 61x34 grids must show every outcome
LAYOUTS = ("slices", "tiles", "both", "ctb_slices")
N_RECORDS = 18                                   # six bases of three records each


def decider(name, chroma):
    bl, bc, ll, lc, extreme = CONFIGS[name]
    rng = np.random.default_rng([len(name), bl, bc])
    return D.Decider(D.palette(rng, bl, bc, extreme=extreme), bd_luma=bl, bd_chroma=bc, lam_luma=ll, lam_chroma=lc, chroma=chroma)


def grid(name, cols, rows):
    """blocks of the four kinds where the grid has room for them, bands of rows where it has not"""
    if cols * rows < 100:
        return D.banded(rows, cols, N_RECORDS)
    return D.grid_of(rows, cols, N_RECORDS, np.random.default_rng([cols, rows, len(name)]))


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
