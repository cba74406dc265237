"""The boundary-byte operand of SAO stated from the bytes themselves (sao_borders_ref.sao_plane_by_bytes), without a GPU: pinned
to the per-sample slice / tile statement on the bytes that layouts produce, and a census of the vectors of
tests/sao_bytes_vectors.py -- CONDITIONS on the reference alone, asserted here so that the GPU tests and the CPU simulator that
run on these vectors cannot pass with a rule that is wrong for some byte."""
import numpy as np
import pytest

import batch_vectors as bvx
import rext_oracle as rx
import sao_borders_ref as R
import sao_bytes_vectors as V


# ---- the by-byte statement is the layout statement wherever a layout stands behind the bytes ----------------------------------

@pytest.mark.parametrize("spec", R.SMALL_SAO_CASES, ids=[s[0] for s in R.SMALL_SAO_CASES])
def test_by_bytes_equals_the_layout_statement(spec):
    c = R.sao_case(spec)
    for f in range(len(c["planes"])):
        keep = None if c["keeps"] is None else c["keeps"][f]
        nox = R.expected_nox(R.case_layout(c, f))
        got = R.sao_plane_by_bytes(c["planes"][f], c["params"][f], c["lw"], c["lh"], nox, bit_depth=c["depth"], keep=keep)
        assert np.array_equal(got, R.case_expected(c, f)), (spec[0], f)
        assert np.array_equal(got, bvx.sao_plane_nox(c["planes"][f], c["params"][f], c["lw"], c["lh"], nox, bit_depth=c["depth"], keep=keep))


@pytest.mark.parametrize("w,h,lw,lh", [(268, 132, 4, 4), (268, 264, 4, 5), (100, 60, 5, 5), (36, 20, 3, 3), (44, 72, 3, 4)])
def test_by_bytes_equals_the_layout_statement_on_cut_ctbs(w, h, lw, lh):
    """planes whose last CTB column and row are cut (the ceil grid of the _g4 planes), square and 4:2:2 CTBs"""
    rng = np.random.default_rng(w + h)
    rows, cols = -(-h >> lh), -(-w >> lw)
    plane = rng.integers(0, 256, (h, w)).astype(np.uint8)
    for kind in ("every", "tiles", "mixed", "random"):
        prm = R.edge_params(rows, cols, rng)
        lay = R._layout_of(kind, rows, cols, rng)
        got = R.sao_plane_by_bytes(plane, prm, lw, lh, R.expected_nox(lay), bit_depth=8)
        assert np.array_equal(got, R.sao_plane(plane, prm, lw, lh, lay)), kind
    zero = np.zeros((rows, cols), np.uint8)
    assert np.array_equal(R.sao_plane_by_bytes(plane, prm, lw, lh, zero, bit_depth=8), rx.sao_plane(plane, prm, lw, lh))


@pytest.mark.parametrize("name", V.TALL)
def test_tall_ctbs_are_two_square_ones_with_rewritten_bytes(name):
    """the library turns CTBs twice as tall as wide into square ones (every parameter row twice, the bytes rewritten:
    batch_vectors.nox_rows_x2 states the rewrite).  On ARBITRARY bytes that is the by-byte result of the tall CTBs"""
    c = V.case(name)
    for f in range(len(c["planes"])):
        sq = R.sao_plane_by_bytes(c["planes"][f], bvx.rows_x2(c["params"][f]), c["lw"], c["lw"], bvx.nox_rows_x2(c["nox"][f]),
                                  bit_depth=c["depth"])
        assert np.array_equal(sq, V.expected(name, f)), (name, f)


# ---- census -------------------------------------------------------------------------------------------------------------------

def _per_ctb_any(diff, c):
    full = np.zeros((c["rows"] << c["lh"], c["cols"] << c["lw"]), bool)
    full[: c["h"], : c["w"]] = diff
    return full.reshape(c["rows"], 1 << c["lh"], c["cols"], 1 << c["lw"]).any(axis=(1, 3))


def _outward(rows, cols):
    """per CTB: the bits that point outside the picture"""
    o = np.zeros((rows, cols), np.uint8)
    o[0] |= V.U | V.UL | V.UR
    o[-1] |= V.D | V.DL | V.DR
    o[:, 0] |= V.L | V.UL | V.DL
    o[:, -1] |= V.Rr | V.UR | V.DR
    return o


def test_the_vectors_are_what_they_claim():
    for name in V.EVERY:
        c = V.case(name)
        rows, cols = c["rows"], c["cols"]
        seen = set()
        for f, prm in enumerate(c["params"]):
            assert prm.shape == (rows, cols) and (prm["type"][1:-1, 1:-1] == 2).all() and (prm["offset"] != 0).all()
            seen |= set(zip(c["nox"][f, 1:-1, 1:cols - 1].ravel().tolist(), prm["cls"][1:-1, 1:-1].ravel().tolist()))
            rim = np.ones((rows, cols), bool)
            rim[1:-1, 1:-1] = False
            assert (c["nox"][f, :, :cols][rim] & _outward(rows, cols)[rim]).any(), "no rim byte points outside the picture"
        assert seen == {(b, k) for b in range(256) for k in range(4)}, (name, len(seen))
        assert c["nox"].shape[2] > cols and (c["nox"][:, :, cols:] == V.NOX_POISON).all()
        assert len(c["planes"]) == 1 or not np.array_equal(c["nox"][0], c["nox"][1])      # per-frame bytes
        assert rows == -(-c["h"] >> c["lh"]) and cols == -(-c["w"] >> c["lw"])
        assert (c["lh"] == c["lw"] + 1) == (name in V.TALL) and c["lh"] - c["lw"] in (0, 1)
    for name in V.MIXED:
        c = V.case(name)
        assert c["lw"] == 6 and c["w"] >= 256 and c["keeps"] is not None and all((p["offset"] != 0).all() for p in c["params"])
        assert {0, 1, 2} == set(np.concatenate([p["type"].ravel() for p in c["params"]]).tolist())
        n = V.wide_pairs(c)
        assert n["wide_bytes_differ"] > 0 and n["zero_band"] > 0, (name, n)


@pytest.mark.parametrize("name", V.EVERY)
def test_census_every_relevant_bit_of_every_interior_ctb_bites(name):
    """Per interior CTB and bit: flipping a bit its class looks at changes the CTB's output (100 %: nothing left out), flipping
    any other bit changes nothing.  A CTB's samples depend on no byte but its own (the reference's definition; spot-checked
    below on single-CTB flips), so one run with the bit flipped in EVERY byte decides the question for every CTB at once."""
    c = V.case(name)
    rows, cols = c["rows"], c["cols"]
    interior = np.zeros((rows, cols), bool)
    interior[1:-1, 1:-1] = True
    rng = np.random.default_rng(len(name))
    for f in range(len(c["planes"])):
        base, nox = V.expected(name, f), c["nox"][f]
        cls = c["params"][f]["cls"].astype(np.int64)
        relevant = np.vectorize(V.RELEVANT.get)(cls & 3)
        for k in range(8):
            bit = np.uint8(1 << k)
            out = V.by_bytes(name, f, nox ^ bit)
            changed = _per_ctb_any(out != base, c)
            rel = (relevant & int(bit)) != 0
            assert changed[interior & rel].all(), (name, f, k, int((~changed[interior & rel]).sum()))
            assert not changed[interior & ~rel].any(), (name, f, k)
            # the same bit flipped in ONE interior CTB: that CTB's samples as above, every other sample as before
            cy, cx = int(rng.integers(1, rows - 1)), int(rng.integers(1, cols - 1))
            one = nox.copy()
            one[cy, cx] ^= bit
            single = V.by_bytes(name, f, one)
            ys, xs = slice(cy << c["lh"], (cy + 1) << c["lh"]), slice(cx << c["lw"], (cx + 1) << c["lw"])
            assert np.array_equal(single[ys, xs], out[ys, xs])
            single = single.copy()
            single[ys, xs] = base[ys, xs]
            assert np.array_equal(single, base)
        # bits of the rim CTBs that point outside the picture say nothing
        flipped = nox.copy()
        flipped[:, :cols] ^= _outward(rows, cols)
        assert np.array_equal(V.by_bytes(name, f, flipped), base), (name, f)
        # a reference that ORs the neighbour's reciprocal bit into a byte is another function on this vector, and so is one that
        # ignores the bytes
        assert (V.by_bytes(name, f, R.reconciled(nox[:, :cols])) != base).any(), (name, f)
        assert (base != V.free(name, f)).any(), (name, f)


@pytest.mark.parametrize("name", V.MIXED)
def test_census_mixed(name):
    c = V.case(name)
    for f in range(len(c["planes"])):
        base, nox = V.expected(name, f), c["nox"][f]
        assert (V.by_bytes(name, f, R.reconciled(nox[:, : c["cols"]])) != base).any(), (name, f)
        assert (base != V.free(name, f)).any(), (name, f)
        kept = np.repeat(np.repeat(c["keeps"][f], 8, axis=0), 8, axis=1) != 0
        assert kept.any() and np.array_equal(base[: kept.shape[0], : kept.shape[1]][kept], c["planes"][f][: kept.shape[0], : kept.shape[1]][kept])


def test_reconciled_is_what_it_says():
    nox = np.zeros((3, 3), np.uint8)
    nox[1, 1] = V.L | V.UR                      # the middle CTB forbids looking left and up-right
    r = R.reconciled(nox)
    assert r[1, 0] == V.Rr and r[0, 2] == V.DL and r[1, 1] == nox[1, 1] and int((r != 0).sum()) == 3
