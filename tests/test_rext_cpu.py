"""Chroma formats 4:2:2 / 4:4:4 of the spec-exact mode, without a GPU: the format-aware oracle (tests/rext_oracle.py) tied to
the 4:2:0 oracle (oracle/h265.py) where the two must agree, the QpC rule on a hand-worked case, and the kernels' new chroma
arithmetic (compiled for the CPU by tests/rext_sim) against the format-aware oracle."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import rext_oracle as rx

SIM_SRC = os.path.join(ROOT, "tests", "rext_sim", "rext_sim.cpp")


def _h265():
    from oracle import h265
    return h265


def _rand_bs(rng, w, h):
    """random 4-sample-granular arrays of a w x h plane: bS 0..2 with keep flags now and then"""
    nv, nh = (w // 8 + 1) * (h // 4), (h // 8 + 1) * (w // 4)
    v = rng.integers(0, 3, nv) | (rng.integers(0, 10, nv) == 0) * rx.KEEP_P | (rng.integers(0, 10, nv) == 0) * rx.KEEP_Q
    hh = rng.integers(0, 3, nh) | (rng.integers(0, 10, nh) == 0) * rx.KEEP_P | (rng.integers(0, 10, nh) == 0) * rx.KEEP_Q
    return v.astype(np.uint8), hh.astype(np.uint8)


def _blocky(rng, w, h, bit_depth):
    """flat 8x8 blocks with small steps between them and some noise: edges the chroma filter changes"""
    top = (1 << bit_depth) - 1
    base = rng.integers(top // 4, 3 * top // 4, (h // 8 + 1, w // 8 + 1))
    p = np.kron(base, np.ones((8, 8), np.int64))[:h, :w]
    p = p + rng.integers(-2, 3, (h, w)) * (1 << (bit_depth - 8))
    p[: h // 4, : w // 4] = rng.integers(0, top + 1, (h // 4, w // 4))
    return np.clip(p, 0, top).astype(np.uint8 if bit_depth == 8 else np.uint16)


# ---- (a) 4:2:0: the new oracle equals oracle/h265 ---------------------------------------------------------------------

def test_420_equals_existing_oracle_every_qpi():
    h265 = _h265()
    rng = np.random.default_rng(11)
    for (cw, ch) in [(8, 8), (16, 24), (40, 32), (64, 48)]:
        for bd in (8, 10):
            c = _blocky(rng, cw, ch, bd)
            vb, hb = _rand_bs(rng, cw, ch)
            for qp in range(0, 52):
                for c_off in (-12, 0, 12) if qp % 7 == 0 else (0,):
                    want = h265.filter_plane(c, qp, vb, hb, c_idx=1, bit_depth=bd, c_qp_offset=c_off, tc_offset_div2=qp % 5 - 2)
                    got = rx.filter_chroma_plane(c, vb, hb, 1, qp=qp, bit_depth=bd, c_qp_offset=c_off, tc_offset_div2=qp % 5 - 2)
                    assert np.array_equal(got, want), (cw, ch, bd, qp, c_off)


def test_420_qp_map_equals_existing_oracle():
    h265 = _h265()
    rng = np.random.default_rng(12)
    for (w, h) in [(64, 48), (96, 80)]:
        c = _blocky(rng, w // 2, h // 2, 8)
        vb, hb = _rand_bs(rng, w // 2, h // 2)
        for u in (3, 4, 5):
            m = rng.integers(0, 52, (-(-h >> u), -(-w >> u))).astype(np.uint8)
            want = h265.filter_plane(c, 0, vb, hb, c_idx=2, qp_map=m, unit_log2=u, c_qp_offset=5)
            got = rx.filter_chroma_plane(c, vb, hb, 1, qp_map=m, unit_log2=u, c_qp_offset=5)
            assert np.array_equal(got, want), (w, h, u)


def test_420_chroma_bs_equals_existing_oracle():
    h265 = _h265()
    for seed, (w, h) in enumerate([(16, 16), (64, 48), (96, 64)]):
        units = h265.random_units(w, h, seed)
        vb, hb = h265.derive_bs(*units, w, h)
        want = h265.chroma_bs(vb, hb, w, h)
        got = rx.chroma_bs(vb, hb, w, h, 1)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- (b) 4:4:4 and 4:2:2 where Table 8-10 is the identity: the existing oracle on transformed operands -------------------

def test_444_equals_existing_oracle_with_doubled_unit():
    """4:4:4 chroma at (x, y) reads the map at luma (x, y); the existing oracle reads (2x, 2y): one unit size up"""
    h265 = _h265()
    rng = np.random.default_rng(13)
    for (w, h) in [(32, 32), (64, 40), (48, 72)]:
        c = _blocky(rng, w, h, 8)
        vb, hb = _rand_bs(rng, w, h)
        for u in (3, 4):
            m = rng.integers(0, 26, (-(-h >> u), -(-w >> u))).astype(np.uint8)  # qPi <= 29 with the offsets below
            for c_off in (-4, 0, 3):
                want = h265.filter_plane(c, 0, vb, hb, c_idx=1, qp_map=m, unit_log2=u + 1, c_qp_offset=c_off)
                got = rx.filter_chroma_plane(c, vb, hb, 3, qp_map=m, unit_log2=u, c_qp_offset=c_off)
                assert np.array_equal(got, want), (w, h, u, c_off)
        for qp in range(0, 30):
            assert np.array_equal(rx.filter_chroma_plane(c, vb, hb, 3, qp=qp), h265.filter_plane(c, qp, vb, hb, c_idx=1))


def test_422_equals_existing_oracle_with_duplicated_rows():
    """4:2:2 chroma at (x, y) reads luma (2x, y); the existing oracle reads (2x, 2y): map rows duplicated"""
    h265 = _h265()
    rng = np.random.default_rng(14)
    for (cw, ch) in [(16, 32), (32, 40), (24, 64)]:
        c = _blocky(rng, cw, ch, 10)
        vb, hb = _rand_bs(rng, cw, ch)
        u = 3
        m = rng.integers(0, 28, (-(-ch >> u), -(-2 * cw >> u))).astype(np.uint8)
        m2 = np.repeat(m, 2, axis=0)
        want = h265.filter_plane(c, 0, vb, hb, c_idx=2, bit_depth=10, qp_map=m2, unit_log2=u)
        got = rx.filter_chroma_plane(c, vb, hb, 2, qp_map=m, unit_log2=u, bit_depth=10)
        assert np.array_equal(got, want), (cw, ch)


def test_422_sao_equals_existing_oracle_with_duplicated_rows():
    h265 = _h265()
    rng = np.random.default_rng(15)
    for (cw, ch, lw) in [(32, 64, 5), (40, 48, 4), (16, 32, 3)]:
        for bd in (8, 10):
            c = _blocky(rng, cw, ch, bd)
            prm = rx.random_sao_params(cw, ch, lw, lw + 1, rng, bd)
            keep = (rng.integers(0, 6, (ch // 8, cw // 8)) == 0).astype(np.uint8)
            sq = np.repeat(prm, 2, axis=0).astype(h265.SAO_CTB_DTYPE)
            want = h265.sao_plane(c, sq, lw, bit_depth=bd, keep=keep)
            got = rx.sao_plane(c, prm, lw, lw + 1, bit_depth=bd, keep=keep)
            assert np.array_equal(got, want), (cw, ch, lw, bd)
            # square CTBs: the two oracles directly
            prm_sq = rx.random_sao_params(cw, ch, lw, lw, rng, bd)
            assert np.array_equal(rx.sao_plane(c, prm_sq, lw, lw, bit_depth=bd),
                                  h265.sao_plane(c, prm_sq.astype(h265.SAO_CTB_DTYPE), lw, bit_depth=bd))


def test_422_and_444_chroma_bs_positions():
    h265 = _h265()
    w, h = 64, 32
    units = h265.random_units(w, h, 7)
    vb, hb = h265.derive_bs(*units, w, h)
    lv, lh = vb.reshape(h // 4, w // 8 + 1), hb.reshape(h // 8 + 1, w // 4)
    cv, chh = rx.chroma_bs(vb, hb, w, h, 2)  # 32 x 32 chroma plane
    cv, chh = cv.reshape(32 // 4, 32 // 8 + 1), chh.reshape(32 // 8 + 1, 32 // 4)
    for m in range(cv.shape[0]):
        for bx in range(cv.shape[1]):
            assert cv[m, bx] == lv[m, 2 * bx]       # vertical (y4, bx) <- luma (y4, 2 bx)
    for by in range(chh.shape[0]):
        for x4 in range(chh.shape[1]):
            assert chh[by, x4] == lh[by, 2 * x4]    # horizontal (by, x4) <- luma (by, 2 x4)
    c4 = rx.chroma_bs(vb, hb, w, h, 3)
    assert np.array_equal(c4[0], vb) and np.array_equal(c4[1], hb)


# ---- (c) qPi >= 30: the two QpC rules part ---------------------------------------------------------------------------

def test_qpc_rule_hand_worked():
    """qPi = 40: Table 8-10 gives QpC 36 (tC' at 36 + 2 = 38: 5), Min(qPi, 51) gives 40 (tC' at 42: 7).  A vertical edge with
    p1 = p0 = 100, q0 = q1 = 140: delta = ((40 << 2) + 100 - 140 + 4) >> 3 = 15, clipped to +-tC."""
    assert int(rx.chroma_qp(40, 1)) == 36 and int(rx.chroma_qp(40, 2)) == 40 and int(rx.chroma_qp(60, 3)) == 51
    assert int(rx.chroma_tc(40, 1)) == 5 and int(rx.chroma_tc(40, 2)) == 7 and int(rx.chroma_tc(40, 3)) == 7
    c = np.full((8, 16), 100, np.uint8)
    c[:, 8:] = 140
    vb = np.zeros((16 // 8 + 1) * 2, np.uint8).reshape(2, 3)
    vb[:, 1] = 2
    hb = np.zeros((8 // 8 + 1) * 4, np.uint8)
    f420 = rx.filter_chroma_plane(c, vb.ravel(), hb, 1, qp=40)
    f422 = rx.filter_chroma_plane(c, vb.ravel(), hb, 2, qp=40)
    f444 = rx.filter_chroma_plane(c, vb.ravel(), hb, 3, qp=40)
    assert (f420[:, 7] == 105).all() and (f420[:, 8] == 135).all()
    assert (f422[:, 7] == 107).all() and (f422[:, 8] == 133).all()
    assert np.array_equal(f422, f444)
    # the existing 4:2:0 oracle agrees with the Table 8-10 figure
    assert np.array_equal(_h265().filter_plane(c, 40, vb.ravel(), hb, c_idx=1), f420)


# ---- (d) the kernels' chroma arithmetic of the new formats, on the CPU ------------------------------------------------

@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rext_sim") / "librext_sim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", out, SIM_SRC])
    L = C.CDLL(out)
    L.rext_sim_filter_chroma.restype = C.c_int
    return L


def _run_sim(sim, plane, cf, vb, hb, *, qp=0, qp_map=None, unit_log2=3, bit_depth=8, tc_offset_div2=0, c_qp_offset=0, packed=0):
    out = np.ascontiguousarray(plane).copy()
    h, w = out.shape
    m = None if qp_map is None else np.ascontiguousarray(qp_map, np.uint8)
    vb, hb = np.ascontiguousarray(vb, np.uint8), np.ascontiguousarray(hb, np.uint8)
    rc = sim.rext_sim_filter_chroma(out.ctypes.data_as(C.c_void_p), w, h, C.c_long(out.strides[0]), out.itemsize, bit_depth, cf,
                                    vb.ctypes.data_as(C.c_void_p), hb.ctypes.data_as(C.c_void_p), int(qp),
                                    None if m is None else m.ctypes.data_as(C.c_void_p), 0 if m is None else m.shape[1], unit_log2,
                                    tc_offset_div2, c_qp_offset, packed)
    assert rc == 0
    return out


@pytest.mark.parametrize("cf", [2, 3])
def test_kernel_chroma_arithmetic_matches_oracle(sim, cf):
    rng = np.random.default_rng(20 + cf)
    sx, sy = rx.SUB[cf]
    for (w, h) in [(16, 8), (32, 16), (64, 48), (80, 40), (48, 72)]:  # luma picture
        cw, ch = w // sx, h // sy
        for bd in (8, 10, 12):
            c = _blocky(rng, cw, ch, bd)
            vb, hb = _rand_bs(rng, cw, ch)
            for qp in (20, 29, 30, 37, 45, 51):
                for tco, coff in ((0, 0), (2, 5), (-3, -7), (6, 12)):
                    want = rx.filter_chroma_plane(c, vb, hb, cf, qp=qp, bit_depth=bd, tc_offset_div2=tco, c_qp_offset=coff)
                    for packed in ((0, 1) if bd <= 12 else (0,)):
                        got = _run_sim(sim, c, cf, vb, hb, qp=qp, bit_depth=bd, tc_offset_div2=tco, c_qp_offset=coff, packed=packed)
                        assert np.array_equal(got, want), (w, h, bd, qp, tco, coff, packed)
            for u in (3, 4, 6):
                m = rng.integers(22, 52, (-(-h >> u), -(-w >> u))).astype(np.uint8)  # qPi on both sides of 30
                want = rx.filter_chroma_plane(c, vb, hb, cf, qp_map=m, unit_log2=u, bit_depth=bd, c_qp_offset=3)
                for packed in (0, 1):
                    got = _run_sim(sim, c, cf, vb, hb, qp_map=m, unit_log2=u, bit_depth=bd, c_qp_offset=3, packed=packed)
                    assert np.array_equal(got, want), (w, h, bd, u, packed)
