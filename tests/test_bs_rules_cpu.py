"""bS derivation (H.265 8.7.2.4) at every edge of its rule and on decoder-shaped pictures, without a GPU.

Three statements of the rule are held against each other segment by segment: tests/bs_vectors.py (a statement about sets,
in Python ints and in numpy int64), oracle/h265_oracle.c::dbko_h265_derive_bs and the kernel's own h265_bs_of_edge compiled
for the CPU by tests/host_sim.  The census assertions are conditions on the vectors, not measurements: the generators are
built so that every leaf of the rule is reached, with every result it can give, in both directions, and so that every
vector comparison that decides a result is seen on both sides of the threshold.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bs_vectors as bv
import rext_oracle as rx
from conftest import ROOT

SIM_DIR = os.path.join(ROOT, "tests", "host_sim")
CODED = [(64, 64, 11, 4), (136, 72, 12, 5), (1920, 1080, 13, 6), (4096, 2176, 14, 6)]


@pytest.fixture(scope="module")
def h265():
    from oracle import h265 as h
    return h


@pytest.fixture(scope="module")
def sim():
    subprocess.check_call(["make", "-s", "-C", SIM_DIR])
    L = C.CDLL(os.path.join(SIM_DIR, "libdbk_hostsim.so"))
    L.host_sim_h265_derive_bs.restype = None
    return L


@pytest.fixture(scope="module")
def pictures():
    """name -> (units, w, h): the rule product and the extremes along both directions, and the small coded pictures"""
    out = {}
    for name, pics in (("product", bv.rule_product()), ("extreme", bv.extreme_cases())):
        for d, p in zip(("vert", "hor"), pics):
            out[name + "_" + d] = p
    for (w, h, seed, ctb) in CODED[:2]:
        out["coded_%dx%d" % (w, h)] = (bv.coded_picture(w, h, seed, ctb), w, h)
    return out


def num_vert(w, h):
    return (w // 8 + 1) * (h // 4)


def num_hor(w, h):
    return (h // 8 + 1) * (w // 4)


def sim_derive(sim, units, w, h):
    arrs = [np.ascontiguousarray(a, dt) for a, dt in zip(units, bv.UNIT_DTYPES)]
    vb = np.full(num_vert(w, h), 0xA5, np.uint8)
    hb = np.full(num_hor(w, h), 0xA5, np.uint8)
    sim.host_sim_h265_derive_bs(*[a.ctypes.data_as(C.c_void_p) for a in arrs], w, h, vb.ctypes.data_as(C.c_void_p),
                                hb.ctypes.data_as(C.c_void_p))
    return vb, hb


def assert_same(got, want, tag):
    for g, wnt, nm in zip(got, want, ("vert", "hor")):
        bad = np.flatnonzero(np.asarray(g) != np.asarray(wnt))
        assert not bad.size, (tag, nm, bad.size, bad[:8].tolist(), np.asarray(g)[bad[:8]].tolist(), np.asarray(wnt)[bad[:8]].tolist())


def test_set_statement_in_python_ints_equals_its_numpy_form(pictures):
    """segment_bs (Python ints, permutations of the entries) and derive_bs (int64, permutations of the list slots) on every
    segment of the rule product, the extremes and the small coded pictures"""
    for name, (units, w, h) in pictures.items():
        assert_same(bv.derive_bs(units, w, h), bv.derive_bs_scalar(units, w, h), name)


def test_reference_equals_oracle_and_kernel_rule(pictures, h265, sim):
    todo = dict(pictures)
    for (w, h, seed, ctb) in CODED[2:]:
        todo["coded_%dx%d" % (w, h)] = (bv.coded_picture(w, h, seed, ctb), w, h)
    for name, (units, w, h) in todo.items():
        want = bv.derive_bs(units, w, h)
        assert_same(h265.derive_bs(*units, w, h), want, ("oracle", name))
        assert_same(sim_derive(sim, units, w, h), want, ("kernel rule", name))
        assert any((np.asarray(a) & 3 == b).any() for a in want for b in (1, 2)), name


def test_hand_worked_motion_cases_on_a_horizontal_edge(h265, sim):
    """the horizontal twins of the motion cases test_h265_oracle.py::test_bs_rules works by hand on the vertical edge x = 8:
    a 16x16 picture, the edge y = 8 with four 4-column segments; rows 1 (P) and 2 (Q) of units"""
    w = h = 16

    def units():
        return [np.zeros((4, 4), np.uint16), np.zeros((4, 4, 2), np.int16), np.zeros((4, 4, 2), np.int16),
                np.zeros((4, 4), np.int32), np.zeros((4, 4), np.int32)]

    def hseg(u):
        res = [bv.derive_bs(u, w, h), bv.derive_bs_scalar(u, w, h), h265.derive_bs(*u, w, h), sim_derive(sim, u, w, h)]
        for r in res[1:]:
            assert_same(r, res[0], "hand")
        assert not res[0][0].any()
        return list(res[0][1].reshape(3, 4)[1])

    u = units()
    f, mv0, mv1, r0, r1 = u
    f[:] = bv.U_PRED_L0
    f[2, :] |= bv.U_TU_TOP | bv.U_PU_TOP
    f[1, 0] |= bv.U_INTRA                           # P intra -> 2
    f[2, 1] |= bv.U_CBF                             # coefficients on a transform edge -> 1
    mv0[2, 2] = (0, 3)                              # |dmv| = 3 < 4, same picture -> 0
    mv0[2, 3] = (-4, 0)                             # |dmv| = 4 -> 1
    assert hseg(u) == [2, 1, 0, 1]
    u = units()
    f, mv0, mv1, r0, r1 = u
    f[:] = bv.U_PRED_L0
    f[2, :] |= bv.U_PU_TOP
    f[2, 0] |= bv.U_CBF                             # no transform edge -> still 0
    r0[2, 1] = 7                                    # other picture -> 1
    f[1, 2] |= bv.U_INTRA | bv.U_KEEP               # 2 + keep P
    f[2, 3] |= bv.U_INTRA | bv.U_DBK_OFF            # deblocking disabled in Q's slice -> 0
    assert hseg(u) == [0, 1, 2 | bv.KEEP_P, 0]
    u = units()
    f, mv0, mv1, r0, r1 = u
    f[:] = bv.U_PRED_L0 | bv.U_PRED_L1
    f[2, :] |= bv.U_PU_TOP
    r0[:], r1[:] = 1, 2
    r0[2, 0], r1[2, 0] = 2, 1                       # Q swaps the lists with matching vectors -> 0
    mv0[1, 0], mv1[1, 0] = (5, 5), (-3, 2)
    mv0[2, 0], mv1[2, 0] = (-3, 2), (5, 5)
    mv1[2, 1] = (0, 4)                              # same pictures, list-1 vector differs by 4 -> 1
    f[2, 2] &= ~np.uint16(bv.U_PRED_L1)             # number of vectors differs -> 1
    r0[1, 3] = r1[1, 3] = r0[2, 3] = r1[2, 3] = 4   # one picture: needs BOTH pairings to be far
    mv0[1, 3], mv1[1, 3] = (0, 0), (0, 8)
    mv0[2, 3], mv1[2, 3] = (0, 8), (0, 0)           # straight pairing far, crossed pairing equal -> 0
    assert hseg(u) == [0, 1, 1, 0]
    mv1[2, 3] = (4, 0)                              # now the crossed pairing is far as well -> 1
    assert hseg(u)[3] == 1
    # what the hand-worked list leaves out: the switches and CBF on the P side only, KEEP on the Q side only, and
    # uni-predicted neighbours that hold the same picture in different lists
    u = units()
    f, mv0, mv1, r0, r1 = u
    f[:] = bv.U_INTRA
    f[2, :] |= bv.U_TU_TOP
    f[1, 0] |= bv.U_DBK_OFF                         # P's slice has the filter off: the edge is Q's -> still 2
    f[1, 1] |= bv.U_NOX_TOP | bv.U_NOX_LEFT         # P's own upper / left border is a slice border: nothing to this edge
    f[2, 2] |= bv.U_KEEP                            # 2 + keep Q
    f[2, 3] |= bv.U_NOX_LEFT                        # Q's LEFT border must not be crossed: nothing to its upper edge
    assert hseg(u) == [2, 2, 2 | bv.KEEP_Q, 2]
    u = units()
    f, mv0, mv1, r0, r1 = u
    f[1, :] = bv.U_PRED_L1
    f[2, :] = bv.U_PRED_L0 | bv.U_TU_TOP
    r1[1, :], r0[2, :] = -3, -3                     # P from list 1, Q from list 0, the same picture
    r0[1, :], r1[2, :] = 9, 8                       # the slots they do not use disagree
    mv1[1, :] = (-32768, 32767)
    mv0[2, :] = (-32768, 32767)
    mv0[1, :], mv1[2, :] = (100, 100), (-100, -100)
    f[1, 1] |= bv.U_CBF                             # cbf on the P side only, transform edge -> 1
    mv0[2, 2] = (-32765, 32767)                     # 3 away at the end of the range -> 0
    mv0[2, 3] = (32767, 32767)                      # 65535 away: 16-bit arithmetic would call it 1 apart
    assert hseg(u) == [0, 1, 0, 1]


def diff_keys(diff, leaf):
    keys = set()
    for (l, _c), hist in diff.items():
        if l == leaf:
            keys |= set(hist)
    return keys


def test_census_of_the_vectors(pictures):
    """every leaf at least 8 times with every result it can give, every deciding comparison on both sides of the threshold in
    both components, every KEEP combination on bS 1 and bS 2 -- per direction.  Nothing is filtered out after generation:
    the pictures counted here are the pictures the comparisons above and the GPU tests run, whole."""
    total = None
    for name, (units, w, h) in pictures.items():
        c = bv.census(units, w, h)
        n_v = sum(sum(x.values()) for x in c["vert"]["leaf"].values())
        n_h = sum(sum(x.values()) for x in c["hor"]["leaf"].values())
        assert n_v == (w // 8 - 1) * (h // 4) and n_h == (h // 8 - 1) * (w // 4), name   # every interior segment is in one leaf
        total = c if total is None else bv.merge_census(total, c)
    for d in ("vert", "hor"):
        c = total[d]
        for leaf in bv.LEAVES:
            assert set(c["leaf"][leaf]) == set(bv.LEAF_RESULTS[leaf]), (d, leaf, c["leaf"][leaf])
            for res in bv.LEAF_RESULTS[leaf]:
                assert c["leaf"][leaf][res] >= 8, (d, leaf, res, c["leaf"][leaf])
        assert c["off_grid"] >= 8 and c["boundary"] >= 8, d
        for bs in (1, 2):
            for kp in (0, 1):
                for kq in (0, 1):
                    assert c["keep"][(bs, kp, kq)] >= 8, (d, bs, kp, kq)
        assert not any(k[0] == 0 and (k[1] or k[2]) for k in c["keep"]), d
        for (leaf, comp), hist in c["diff"].items():
            for dxy in bv.THRESHOLD_DIFFS:
                assert hist[dxy] >= 1, (d, leaf, comp, dxy)
        # the ends of the ranges: a difference of 65535 and of 65533 in each component decided a one-vector result
        seen = diff_keys(c["diff"], "one_vector")
        for big in (65535, -65535, 65533, -65533):
            assert any(k[0] == big for k in seen) and any(k[1] == big for k in seen), (d, big)
    # the product alone satisfies the threshold conditions in the direction it is packed along (the other pictures add the
    # range ends and the decoder's shapes, not the thresholds)
    for d in ("vert", "hor"):
        units, w, h = pictures["product_" + d]
        c = bv.census(units, w, h)[d]
        for (leaf, comp), hist in c["diff"].items():
            assert all(hist[dxy] >= 1 for dxy in bv.THRESHOLD_DIFFS), (d, leaf, comp)


def test_coded_pictures_have_a_decoders_shapes():
    """what coded_picture promises: consistent flags, constant motion inside a block, inner prediction edges off the grid (from
    asymmetric partitions of 16x16 blocks and the halves of 8x8 blocks) and on it, bS 0 across real prediction edges
    (merged motion), slice and tile borders, DBK_OFF and KEEP blocks"""
    total = None
    for (w, h, seed, ctb) in CODED[:3]:
        units = bv.coded_picture(w, h, seed, ctb)
        f = units[0].astype(np.int64)
        c = bv.census(units, w, h)
        total = c if total is None else bv.merge_census(total, c)
        # a unit that flags no edge on its left continues its left neighbour's block: same prediction data
        inner = (f[:, 1:] & (bv.U_PU_LEFT | bv.U_TU_LEFT)) == 0
        same = bv.U_INTRA | bv.U_PRED_L0 | bv.U_PRED_L1 | bv.U_KEEP | bv.U_DBK_OFF | bv.U_CBF
        assert ((f[:, 1:] & same) == (f[:, :-1] & same))[inner].all()
        for l, bit in ((0, bv.U_PRED_L0), (1, bv.U_PRED_L1)):
            m = inner & ((f[:, 1:] & bit) != 0)
            assert (units[1 + l][:, 1:] == units[1 + l][:, :-1]).all(axis=-1)[m].all()
            assert (units[3 + l][:, 1:] == units[3 + l][:, :-1])[m].all()
        # the picture's left column and top row start blocks
        assert (f[:, 0] & bv.U_PU_LEFT).all() and (f[0, :] & bv.U_PU_TOP).all()
    for d in ("vert", "hor"):
        c = total[d]
        assert c["off_grid"] > 0 and c["leaf"]["nox"][0] > 0 and c["leaf"]["dbk_off"][0] > 0, d
        motion0 = sum(c["leaf"][l][0] for l in ("one_vector", "two_pictures_straight", "two_pictures_crossed", "one_picture"))
        assert motion0 > 0 and c["leaf"]["intra"][2] > 0 and c["leaf"]["cbf"][1] > 0 and c["leaf"]["pictures_differ"][1] > 0, d
        assert any(k[1] or k[2] for k in c["keep"]), d


def test_rule_is_invariant_under_its_symmetries(pictures, h265, sim):
    """no reference needed: transposing the picture transposes vert <-> hor; exchanging list 0 and list 1 in every unit,
    adding one constant to every reference id or one constant vector to every mv (nothing leaves int32 / int16) changes
    nothing -- for the new reference, the oracle and the kernel's rule alike"""
    implementations = (("reference", lambda u, w, h: bv.derive_bs(u, w, h)), ("oracle", lambda u, w, h: h265.derive_bs(*u, w, h)),
                       ("kernel rule", lambda u, w, h: sim_derive(sim, u, w, h)))
    shifted_mv = shifted_pic = 0
    for name, (units, w, h) in pictures.items():
        flags = units[0]
        used = [(flags & bit) != 0 for bit in (bv.U_PRED_L0, bv.U_PRED_L1)]
        mv = [units[1].astype(np.int64), units[2].astype(np.int64)]
        ref = [units[3].astype(np.int64), units[4].astype(np.int64)]

        def span(arrs):
            vals = np.concatenate([a[u].ravel() for a, u in zip(arrs, used)])
            return int(vals.min()), int(vals.max())

        # one constant for every vector / picture a unit USES, chosen so that nothing leaves int16 / int32 (the extremes
        # sit at both ends and cannot move); the slots a unit does not use keep what they hold
        lo, hi = span(mv)
        dv = np.array([min(37, bv.INT16_MAX - hi), -min(41, lo - bv.INT16_MIN)], np.int64)
        rlo, rhi = span(ref)
        dr = 12345 if rhi <= bv.INT32_MAX - 12345 else (-12345 if rlo >= bv.INT32_MIN + 12345 else 0)
        moved = [np.where(u[..., None], m + dv, m) for m, u in zip(mv, used)]
        repic = [np.where(u, r + dr, r) for r, u in zip(ref, used)]
        for m in moved:
            assert m.min() >= bv.INT16_MIN and m.max() <= bv.INT16_MAX
        for r in repic:
            assert r.min() >= bv.INT32_MIN and r.max() <= bv.INT32_MAX
        shifted = (flags, moved[0].astype(np.int16), moved[1].astype(np.int16), units[3], units[4])
        repoc = (flags, units[1], units[2], repic[0].astype(np.int32), repic[1].astype(np.int32))
        shifted_mv += bool(dv.all())
        shifted_pic += dr != 0
        for tag, fn in implementations:
            vb, hb = fn(units, w, h)
            tv, th = fn(bv.transpose_units(units), h, w)
            assert np.array_equal(np.asarray(tv).reshape(w // 4, h // 8 + 1), np.asarray(hb).reshape(h // 8 + 1, w // 4).T), (tag, name)
            assert np.array_equal(np.asarray(th).reshape(w // 8 + 1, h // 4), np.asarray(vb).reshape(h // 4, w // 8 + 1).T), (tag, name)
            assert_same(fn(bv.swap_lists(units), w, h), (vb, hb), (tag, name, "lists"))
            assert_same(fn(repoc, w, h), (vb, hb), (tag, name, "pictures + const"))
            assert_same(fn(shifted, w, h), (vb, hb), (tag, name, "mv + const"))
    assert shifted_mv >= 4 and shifted_pic >= 4     # the product and the coded pictures did move


@pytest.mark.parametrize("cf", [1, 2, 3])
def test_three_chroma_gathers_agree(cf, h265):
    """the chroma arrays of chroma_format_idc 1, 2, 3 from three restatements of "the luma entry at bS[xDk * SubWidthC][yDm *
    SubHeightC]", on pictures whose chroma planes have 1, 2 and many 8-sample columns (and rows)"""
    sx, sy = bv.SUB[cf]
    rng = np.random.default_rng(30 + cf)
    sizes = [(8 * sx, 8 * sy), (16 * sx, 16 * sy), (16 * sx, 8 * sy), (8 * sx, 16 * sy), (272, 144), (1920, 1088)]
    for (w, h) in sizes:
        # every entry its own value, so that a gather from the wrong place cannot go unnoticed
        vb = rng.integers(0, 256, num_vert(w, h)).astype(np.uint8)
        hb = rng.integers(0, 256, num_hor(w, h)).astype(np.uint8)
        a = bv.chroma_bs(vb, hb, w, h, cf)
        b = rx.chroma_bs(vb, hb, w, h, cf)
        assert a[0].size == num_vert(w // sx, h // sy) and a[1].size == num_hor(w // sx, h // sy)
        assert_same(b, a, ("rext", cf, w, h))
        if cf == 1:
            assert_same(h265.chroma_bs(vb, hb, w, h), a, ("oracle", w, h))
    # and on derived arrays of a coded picture
    w, h = 272, 144
    vb, hb = bv.derive_bs(bv.coded_picture(w, h, 5, 5), w, h)
    assert_same(rx.chroma_bs(vb, hb, w, h, cf), bv.chroma_bs(vb, hb, w, h, cf), ("coded", cf))
