"""Spec-exact deblocking and SAO at their decision edges and over the full sample range, without a GPU.

The vectors come from tests/h265_vectors.py: segments solved to sit exactly on either side of every threshold of 8.7.2.5.3 /
8.7.2.5.6 / 8.7.2.5.7, clips at 0 and max_v, the largest legal normal-filter numerator, full-range SAO content.  Here:
  * a census proves the generator still reaches every case (so it cannot quietly degenerate into mid-range content),
  * the numpy luma restatement (h265_vectors.luma_reference) equals the C oracle, and rext_oracle equals it on chroma and SAO,
  * the kernels' block arithmetic (tests/host_sim: the 32-bit core, the packed-int16 core with its WIDE form at 12 bit, the
    mixed-bS form and the QP-map table form) equals the oracle on the same vectors.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import h265_vectors as hv
import rext_oracle as rx

BIT_DEPTHS = (8, 9, 10, 11, 12, 14, 16)
# (qp, tc_offset_div2, beta_offset_div2); qp None = a QP map holding every QP 0..51
# (17, 0, 0) and (16, 3, 0): beta 7 / 6 (beta >> 3 == 0 at 8 bit) with tC 1 at bS 2 -- and tC 0 at bS 1 for QP 17
OPERANDS = ((51, 0, 0), (37, 0, 0), (30, -6, 6), (45, 6, -6), (22, 3, -2), (17, 0, 0), (16, 3, 0), (None, 0, 0), (None, -4, 5),
            (None, 2, -3))


def _h265():
    from oracle import h265
    return h265


@functools.lru_cache(maxsize=None)
def luma_vectors(bd, w=528, h=32):
    """(plane, qp, vb, hb, qp_map, unit_log2, tc_offset_div2, beta_offset_div2) for every operand set, both edge directions"""
    rng = np.random.default_rng(1000 + bd)
    out = []
    for i, (qp, tco, bo) in enumerate(OPERANDS):
        for d in "vh":
            W, H = (w, h) if d == "v" else (h, w)
            u = 3 + i % 2
            m = None if qp is not None else hv.all_qp_map(W, H, u, rng)
            p, vb, hb = hv.luma_edge_plane(bd, qp or 0, tco, bo, rng, w=W, h=H, direction=d, qp_map=m, unit_log2=u)
            out.append((p, qp or 0, vb, hb, m, u, tco, bo))
    return out


def _achievable(bd):
    """the per-segment extras the tables allow at this bit depth"""
    sh = bd - 8
    betas = hv.BETA_TABLE << sh
    got = {"tc_max", "beta_max", "strong_sum_max", "max_ramp", "tc0_beta_pos"}
    if ((betas >> 3 == 0) & (betas > 0)).any():
        got.add("beta_sh3_0")
    if (betas >> 3 == 1).any():
        got.add("beta_sh3_1")
    if ((betas >> 2 == 0) & (betas > 0)).any():
        got.add("beta_sh2_0")
    if (betas >> 2 == 1).any():
        got.add("beta_sh2_1")
    return got


@pytest.mark.parametrize("bd", BIT_DEPTHS)
def test_luma_census(bd):
    """every label, every clip kind and every threshold at value - 1 and at value occurs in the generated luma planes"""
    st = hv.new_stats()
    for (p, qp, vb, hb, m, u, tco, bo) in luma_vectors(bd):
        hv.luma_reference(p, qp, vb, hb, bit_depth=bd, qp_map=m, unit_log2=u, tc_offset_div2=tco, beta_offset_div2=bo, stats=st)
    assert [k for k in hv.LABELS if not st["labels"][k]] == []
    assert [k for k in hv.CLIP_KINDS if not st["clips"][k]] == []
    assert [(n, s) for n in hv.THRESHOLDS for s in ("below", "at") if not st["events"][(n, s)]] == []
    assert [k for k in sorted(_achievable(bd)) if not st["extras"][k]] == []
    # samples cover the whole range
    lo = min(int(v[0].min()) for v in luma_vectors(bd))
    hi = max(int(v[0].max()) for v in luma_vectors(bd))
    assert (lo, hi) == (0, (1 << bd) - 1)


def test_luma_layout_uniform_mixed_and_keep_waves():
    """along a block row, each run of 64 blocks holds one bS kind: 2 (and 0), 1 (and 0), 1 and 2 mixed, or keep flags"""
    p, vb, hb = hv.luma_edge_plane(8, 37, 0, 0, np.random.default_rng(3), w=1056, h=32)
    v = vb.reshape(32 // 4, 1056 // 8 + 1)
    for y4 in range(v.shape[0]):
        for g in range(0, 132, 64):
            run = v[y4, max(g, 1): min(g + 64, 132)]
            mode = hv.WAVE_MODES[(y4 // 2 + g // 64) % 4]
            kinds = set(int(x) & 3 for x in run) - {0}
            keep = any(int(x) & 12 for x in run)
            want = {"bs2": {2}, "bs1": {1}, "mixed": {1, 2}, "keep": {1, 2}}[mode]
            if len(run) == 64 - (g == 0):   # full waves; the partial wave at the right edge is 4 blocks
                assert keep == (mode == "keep") and kinds == want, (y4, g, kinds)
            assert kinds <= want and (not keep or mode == "keep"), (y4, g, kinds)
    assert not hb.any()
    # the transposed twin: horizontal bS only
    th, tv, thb = hv.luma_edge_plane(10, 40, 0, 0, np.random.default_rng(4), w=64, h=528, direction="h")
    assert not tv.any() and thb.reshape(528 // 8 + 1, 64 // 4).any()


@pytest.mark.parametrize("bd", BIT_DEPTHS)
def test_luma_reference_equals_oracle(bd):
    """the numpy restatement and oracle/h265_oracle.c, bit for bit: both directions, keep flags, scalar QPs, QP maps with unit
    boundaries, tc / beta offsets from -6 to 6"""
    h265 = _h265()
    for k, (p, qp, vb, hb, m, u, tco, bo) in enumerate(luma_vectors(bd)):
        got, info = hv.luma_reference(p, qp, vb, hb, bit_depth=bd, qp_map=m, unit_log2=u, tc_offset_div2=tco, beta_offset_div2=bo)
        want = h265.filter_plane(p, qp, vb, hb, bit_depth=bd, qp_map=m, unit_log2=u, tc_offset_div2=tco, beta_offset_div2=bo)
        assert np.array_equal(got, want), (bd, k, qp, tco, bo, np.argwhere(got != want)[:4])
        assert not np.array_equal(got, p)
    # both passes on one plane: vertical segments of one plane and horizontal segments of another, overlaid
    rng = np.random.default_rng(bd)
    a, va, _ = hv.luma_edge_plane(bd, 40, 1, 1, rng, w=64, h=64)
    b, _, hb2 = hv.luma_edge_plane(bd, 40, 1, 1, rng, w=64, h=64, direction="h")
    mix = np.where((np.arange(64)[:, None] // 8 + np.arange(64)[None, :] // 8) % 2 == 0, a, b)
    for tco in range(-6, 7, 3):
        for bo in range(-6, 7, 4):
            got, _ = hv.luma_reference(mix, 40, va, hb2, bit_depth=bd, tc_offset_div2=tco, beta_offset_div2=bo)
            assert np.array_equal(got, h265.filter_plane(mix, 40, va, hb2, bit_depth=bd, tc_offset_div2=tco, beta_offset_div2=bo))


def test_luma_reference_known_answers():
    """the hand-worked segments of test_h265_oracle, through the numpy restatement, with their labels"""
    w, h = 16, 8
    vb = np.zeros((h // 4, w // 8 + 1), np.uint8)
    hb = np.zeros((h // 8 + 1) * (w // 4), np.uint8)
    plane = np.full((h, w), 100, np.uint8)
    plane[:, 8:] = 110
    vb[:, 1] = 2
    out, info = hv.luma_reference(plane, 37, vb.ravel(), hb)
    assert list(out[0, 4:12]) == [100, 101, 103, 104, 106, 108, 109, 110]
    assert list(info["vert"][:, 1]) == [hv.LABELS.index("strong")] * 2
    vb[:, 1] = 1
    out, info = hv.luma_reference(plane, 37, vb.ravel(), hb)
    assert list(out[0, 4:12]) == [100, 100, 102, 104, 106, 108, 110, 110]
    assert list(info["vert"][:, 1]) == [hv.LABELS.index("normal_p1q1")] * 2
    vb[:, 1] = 1 | hv.KEEP_P
    out, _ = hv.luma_reference(plane, 37, vb.ravel(), hb)
    assert list(out[0, 4:12]) == [100, 100, 100, 100, 106, 108, 110, 110]
    # the 12-bit maximal ramp p = 0, 1365, 2730, 4095 | q = 4095, 2730, 1365, 0: 9 * 4095 - 3 * (2730 - 1365) + 8 = 32768
    assert hv.max_ramp_numerator(12) == 32768


# ---- chroma ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def chroma_vectors(bd, cf):
    """(plane, vb, hb, kw) with kw the operands of rext_oracle.filter_chroma_plane"""
    rng = np.random.default_rng(2000 + 10 * bd + cf)
    sx, sy = rx.SUB[cf]
    out = []
    cw, ch = 264, 32
    for i, (qp, coff, tco) in enumerate(((27, 2, 0), (28, 2, 0), (41, 2, 0), (42, 2, 0), (51, 12, 6), (40, -12, -3), (None, 0, 0),
                                         (None, 12, 2), (None, -7, 1))):
        for d in "vh":
            W, H = (cw, ch) if d == "v" else (ch, cw)
            m = None if qp is not None else hv.all_qp_map(W * sx, H * sy, 3, rng, lo=16)
            p, vb, hb = hv.chroma_edge_plane(bd, rng, w=W, h=H, chroma_format=cf, qp=qp or 0, qp_map=m, c_qp_offset=coff,
                                             tc_offset_div2=tco, direction=d)
            out.append((p, vb, hb, dict(qp=qp or 0, qp_map=m, unit_log2=3, bit_depth=bd, c_qp_offset=coff, tc_offset_div2=tco)))
    return out


@pytest.mark.parametrize("cf", [1, 2, 3])
def test_chroma_census(cf):
    """delta clip at +-tC, Clip1 at 0 and max_v on both sides, and qPi at the Table 8-10 knees (4:2:0) or above the
    Min(qPi, 51) cap (4:2:2, 4:4:4)"""
    for bd in (8, 10, 12, 16):
        ev = hv.chroma_events(np.zeros((8, 8), np.uint8), np.zeros(4, np.uint8), cf)
        for (p, vb, hb, kw) in chroma_vectors(bd, cf):
            if kw["qp_map"] is None and not hb.any():
                ev.update(hv.chroma_events(p, vb, cf, **kw))
        for k in ("tc_clip_lo", "tc_clip_hi", "clip1_p0_lo", "clip1_p0_hi", "clip1_q0_lo", "clip1_q0_hi"):
            assert ev[k], (bd, cf, k)
        qpis = {k[1] for k in ev if isinstance(k, tuple)}
        assert {29, 30, 43, 44} <= qpis, (bd, cf, sorted(qpis))
        assert max(qpis) > 51, (bd, cf, sorted(qpis))   # 4:2:0: qPi - 6; 4:2:2 / 4:4:4: the Min(qPi, 51) cap


@pytest.mark.parametrize("bd", (8, 10, 12))
def test_chroma_rext_oracle_equals_oracle_420(bd):
    h265 = _h265()
    for k, (p, vb, hb, kw) in enumerate(chroma_vectors(bd, 1)):
        want = h265.filter_plane(p, kw["qp"], vb, hb, c_idx=1, bit_depth=bd, qp_map=kw["qp_map"], unit_log2=3,
                                 c_qp_offset=kw["c_qp_offset"], tc_offset_div2=kw["tc_offset_div2"])
        got = rx.filter_chroma_plane(p, vb, hb, 1, **kw)
        assert np.array_equal(got, want), (bd, k)
        assert not np.array_equal(got, p)


@pytest.mark.parametrize("cf", [2, 3])
def test_chroma_rext_oracle_equals_oracle_422_444(cf):
    """where Table 8-10 is the identity (qPi < 30) the formats' rule agrees with the 4:2:0 oracle on transformed operands
    (test_rext_cpu): 4:4:4 reads the map one unit size up, 4:2:2 reads it with duplicated rows"""
    h265 = _h265()
    rng = np.random.default_rng(30 + cf)
    sx, sy = rx.SUB[cf]
    for bd in (8, 12):
        for d in "vh":
            W, H = (264, 32) if d == "v" else (32, 264)
            m = rng.integers(0, 27, (-(-H * sy >> 3), -(-W * sx >> 3))).astype(np.uint8)   # qPi <= 29 with c_qp_offset <= 3
            p, vb, hb = hv.chroma_edge_plane(bd, rng, w=W, h=H, chroma_format=cf, qp_map=m, c_qp_offset=3, direction=d)
            got = rx.filter_chroma_plane(p, vb, hb, cf, qp_map=m, unit_log2=3, bit_depth=bd, c_qp_offset=3)
            if cf == 3:
                want = h265.filter_plane(p, 0, vb, hb, c_idx=1, bit_depth=bd, qp_map=m, unit_log2=4, c_qp_offset=3)
            else:
                want = h265.filter_plane(p, 0, vb, hb, c_idx=1, bit_depth=bd, qp_map=np.repeat(m, 2, axis=0), unit_log2=3, c_qp_offset=3)
            assert np.array_equal(got, want), (cf, bd, d)
            assert not np.array_equal(got, p)


# ---- the kernels' block arithmetic on the CPU -------------------------------------------------------------------------

SIM_DIR = os.path.join(ROOT, "tests", "host_sim")


@pytest.fixture(scope="module")
def sim():
    subprocess.check_call(["make", "-s", "-C", SIM_DIR])
    L = C.CDLL(os.path.join(SIM_DIR, "libdbk_hostsim.so"))
    L.host_sim_h265_filter_plane.restype = None
    assert L.host_sim_have_packed()
    return L


def sim_filter(sim, plane, qp, vb, hb, *, c_idx=0, bit_depth=8, qp_map=None, unit_log2=3, tc_off=0, beta_off=0, c_qp_off=0, packed=0):
    out = np.ascontiguousarray(plane).copy()
    h, w = out.shape
    vb, hb = np.ascontiguousarray(vb, np.uint8), np.ascontiguousarray(hb, np.uint8)
    m = None if qp_map is None else np.ascontiguousarray(qp_map, np.uint8)
    sim.host_sim_h265_filter_plane(
        out.ctypes.data_as(C.c_void_p), w, h, C.c_long(out.strides[0]), out.itemsize, bit_depth, c_idx,
        vb.ctypes.data_as(C.c_void_p), hb.ctypes.data_as(C.c_void_p), int(qp),
        None if m is None else m.ctypes.data_as(C.c_void_p), 0 if m is None else m.shape[1], unit_log2,
        tc_off, beta_off, c_qp_off, packed)
    return out


@pytest.mark.parametrize("bd", (8, 9, 10, 11, 12))
def test_host_sim_luma_equals_oracle(sim, bd):
    """32-bit core and packed core (12 bit: WIDE) with one QP, the packed core's mixed-bS form for every block, and the QP-map
    launches' table form, on the boundary vectors"""
    h265 = _h265()
    for k, (p, qp, vb, hb, m, u, tco, bo) in enumerate(luma_vectors(bd)):
        want = h265.filter_plane(p, qp, vb, hb, bit_depth=bd, qp_map=m, unit_log2=u, tc_offset_div2=tco, beta_offset_div2=bo)
        for packed in (0, 1):
            got = sim_filter(sim, p, qp, vb, hb, bit_depth=bd, qp_map=m, unit_log2=u, tc_off=tco, beta_off=bo, packed=packed)
            assert np.array_equal(got, want), (bd, k, qp, tco, bo, packed, np.argwhere(got != want)[:4])
        if m is None:
            sim.host_sim_h265_force_mixed(1)
            try:
                got = sim_filter(sim, p, qp, vb, hb, bit_depth=bd, tc_off=tco, beta_off=bo, packed=1)
            finally:
                sim.host_sim_h265_force_mixed(0)
            assert np.array_equal(got, want), ("mixed form", bd, k, np.argwhere(got != want)[:4])


@pytest.mark.parametrize("bd", (8, 10, 12))
def test_host_sim_chroma_equals_oracle(sim, bd):
    h265 = _h265()
    for k, (p, vb, hb, kw) in enumerate(chroma_vectors(bd, 1)):
        want = h265.filter_plane(p, kw["qp"], vb, hb, c_idx=1, bit_depth=bd, qp_map=kw["qp_map"], unit_log2=3,
                                 c_qp_offset=kw["c_qp_offset"], tc_offset_div2=kw["tc_offset_div2"])
        for packed in (0, 1):
            got = sim_filter(sim, p, kw["qp"], vb, hb, c_idx=1, bit_depth=bd, qp_map=kw["qp_map"], unit_log2=3,
                             tc_off=kw["tc_offset_div2"], c_qp_off=kw["c_qp_offset"], packed=packed)
            assert np.array_equal(got, want), (bd, k, packed)


# ---- SAO ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bd", BIT_DEPTHS)
def test_sao_full_range(bd):
    """the two SAO restatements agree on full-range content with scaled and int8-limit offsets; the census shows every band
    position (and the wrap of 29..31), every edge class and category, clipping at both ends and the offset magnitudes"""
    h265 = _h265()
    rng = np.random.default_rng(3000 + bd)
    tags = set()
    for ctb_log2, (w, h) in ((4, (320, 256)), (5, (320, 256)), (6, (1056, 272))):
        p, prm, keep = hv.sao_full_range(bd, ctb_log2, rng, w=w, h=h)
        for k in (None, keep):
            want = h265.sao_plane(p, prm, ctb_log2, bit_depth=bd, keep=k)
            got = rx.sao_plane(p, prm, ctb_log2, ctb_log2, bit_depth=bd, keep=k)
            assert np.array_equal(got, want), (bd, ctb_log2, k is None)
            tags |= hv.sao_census(p, prm, ctb_log2, bd, k)
        for c in hv.FUSED_COLS:
            assert {0, (1 << bd) - 1} <= set(np.unique(p[:, c]).tolist())
        for r in hv.FUSED_ROWS:
            assert {0, (1 << bd) - 1} <= set(np.unique(p[r]).tolist())
    missing = [("band", b) for b in range(32) if ("band", b) not in tags]
    missing += [("wrap", b) for b in (29, 30, 31) if ("wrap", b) not in tags]
    missing += [("edge", c, e) for c in range(4) for e in range(1, 5) if ("edge", c, e) not in tags]
    missing += [t for t in ("clip_lo", "clip_hi") if t not in tags]
    offs = {t[1] for t in tags if t[0] == "offset"}
    missing += [("offset", v) for v in [127, -128] + [s * L for L in hv.sao_offset_limits(bd) for s in (1, -1)] if v not in offs]
    assert missing == [], (bd, missing)


@pytest.mark.parametrize("bd", (11, 12, 14))
def test_random_sao_params_scaled_offsets(bd):
    """random_sao_params draws log2OffsetScale 0 .. Max(0, bitDepth - 10) (within int8), with the edge offset signs"""
    h265 = _h265()
    p = h265.random_sao_params(1024, 1024, 4, seed=bd, bit_depth=bd)
    off = p["offset"].astype(int)
    top = max(hv.sao_offset_limits(bd))
    assert np.abs(off).max() == top and (np.abs(off) > 31).any()
    eo = p["type"] == 2
    assert (off[eo][:, :2] >= 0).all() and (off[eo][:, 2:] <= 0).all()
    r = rx.random_sao_params(1024, 1024, 4, 4, np.random.default_rng(bd), bd)
    assert np.abs(r["offset"].astype(int)).max() == top
    # up to 10 bit the draws are those of before
    a = h265.random_sao_params(64, 64, 4, seed=5, bit_depth=10)
    assert np.abs(a["offset"].astype(int)).max() <= 31
