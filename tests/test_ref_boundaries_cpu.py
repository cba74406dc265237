"""Reference-exact deblocking at its decision edges and over the full sample range, without a GPU.

The vectors come from tests/ref_vectors.py: segments solved to sit exactly on either side of every threshold of cpu.h's luma
filter (d < beta, the three strong-filter conditions on lines 0 and 3, cond5 / cond6, |delta| < 10 tc), on its clips, the
range extremes and the picture border, and chroma segments on the +-tc clips and Clip2.  Here:
  * a census proves the generator still reaches every case (so it cannot quietly degenerate into mid-range content),
  * the numpy restatement (ref_vectors.reference_plane) equals the C oracle, 8..16 bit, with scalar QPs, custom tables and QP
    maps,
  * the kernels' block arithmetic (tests/host_sim: the 32-bit core, the packed 8-bit and 16-bit cores, the WIDE 12-bit core,
    the QP-map operand table) equals the oracle on the same vectors,
  * the boundary frames of tests/golden/make_golden.py reproduce the reference's recorded outputs (and oracle/_ref's, live).
"""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, sha256
import ref_vectors as rv

BIT_DEPTHS = (8, 9, 10, 11, 12, 14, 16)
SIZES = ((8, 8), (24, 16), (120, 24), (504, 16), (520, 24))   # ragged widths: 1, 3, 15, 63, 65 blocks
CHROMA_WAVES = ("v", "h", "default")


@functools.lru_cache(maxsize=None)
def vectors(bd):
    """(name, plane, filter_plane keyword arguments) for every operand set at bit depth bd"""
    rng = np.random.default_rng(4000 + bd)
    out = []
    for qp in range(52):   # every QP of the reference tables, planes of every shape and wave
        w, h = SIZES[qp % len(SIZES)]
        p, vb, hb = rv.luma_plane(bd, rng, w=w, h=h, wave=rv.WAVES[qp % 3], qp=qp)
        out.append(("qp%d" % qp, p, dict(qp=qp, vert_bs=vb, hor_bs=hb)))
        c, cvb, chb = rv.chroma_plane(bd, rng, w=w, h=h, wave=CHROMA_WAVES[qp % 3], qp=qp)
        out.append(("c_qp%d" % qp, c, dict(qp=qp, is_chroma=True, vert_bs=cvb, hor_bs=chb)))
    for name, tct, bt in rv.custom_tables():
        for wave in ("v", "h"):
            p, vb, hb = rv.luma_plane(bd, rng, w=248, h=32, wave=wave, qp=40, tc_table=tct, beta_table=bt)
            out.append((name, p, dict(qp=40, vert_bs=vb, hor_bs=hb, tc_table=tct, beta_table=bt)))
        c, cvb, chb = rv.chroma_plane(bd, rng, w=120, h=24, wave="v", qp=40, tc_table=tct)
        out.append(("c_" + name, c, dict(qp=40, is_chroma=True, vert_bs=cvb, hor_bs=chb, tc_table=tct, beta_table=bt)))
    # the operand-range edge of the packed luma core: the largest entry it holds, and one more
    edge = rv.fits_edge(bd)
    for e in (edge, edge + 1):
        if edge < 0 or e > 255:
            continue
        tct, bt = np.full(52, e, np.int64), np.full(52, 255, np.int64)
        for wave in ("v", "h"):
            p, vb, hb = rv.luma_plane(bd, rng, w=120, h=24, wave=wave, qp=40, tc_table=tct, beta_table=bt)
            out.append(("fits%d" % e, p, dict(qp=40, vert_bs=vb, hor_bs=hb, tc_table=tct, beta_table=bt)))
    for lg in range(3, 9):   # QP maps with every QP, unit borders on 8-sample edges up to 256-sample units
        m = rv.all_qp_map(264, 48, lg, rng)
        for wave in ("v", "h"):
            p, vb, hb = rv.luma_plane(bd, rng, w=264, h=48, wave=wave, qp_map=m, ctu_log2=lg)
            out.append(("map%d" % lg, p, dict(qp=0, vert_bs=vb, hor_bs=hb, qp_map=m, ctu_log2=lg)))
        cm = rv.all_qp_map(264, 48, lg, rng)
        c, cvb, chb = rv.chroma_plane(bd, rng, w=132 // 8 * 8, h=24, wave=CHROMA_WAVES[lg % 3], qp_map=cm, ctu_log2=lg)
        out.append(("c_map%d" % lg, c, dict(qp=0, is_chroma=True, vert_bs=cvb, hor_bs=chb, qp_map=cm, ctu_log2=lg)))
    return out


@functools.lru_cache(maxsize=None)
def reference_outputs(bd):
    """the numpy reference on vectors(bd): outputs and the luma / chroma census"""
    lst, cst = rv.new_stats(), rv.new_stats()
    outs = []
    for name, p, kw in vectors(bd):
        got, _ = rv.reference_plane(p, bit_depth=bd, stats=cst if kw.get("is_chroma") else lst, **kw)
        outs.append(got)
    return outs, lst, cst


@pytest.mark.parametrize("bd", BIT_DEPTHS)
def test_census(bd):
    """every threshold on both sides, every label and clip, border segments on all four sides, hor2 segments with their Q taps
    in the padding and the chroma guard's shifted read occur in the generated planes"""
    _, st, cst = reference_outputs(bd)
    assert [k for k in rv.LABELS[:-1] if not st["labels"][k]] == []
    assert [k for k in rv.LUMA_CLIPS if not st["clips"][k]] == []
    assert [(n, s) for n in rv.LUMA_THRESHOLDS for s in ("below", "at") if not st["events"][(n, s)]] == []
    want = ["border_" + b for b in rv.BORDERS] + ["hor2", "hor2_q_padding", "max_ramp", "strong_sum_max"]
    assert [k for k in want if not st["extras"][k]] == []
    assert cst["labels"]["chroma"] > 0
    assert [k for k in rv.CHROMA_CLIPS if not cst["clips"][k]] == []
    assert [(n, s) for n in rv.CHROMA_THRESHOLDS for s in ("below", "at") if not cst["events"][(n, s)]] == []
    want = ["border_" + b for b in rv.BORDERS] + ["hor2", "chroma_round", "chroma_shifted_read"]
    assert [k for k in want if not cst["extras"][k]] == []
    # samples cover the whole range
    assert min(int(p.min()) for _, p, _ in vectors(bd)) == 0
    assert max(int(p.max()) for _, p, _ in vectors(bd)) == (1 << bd) - 1


def test_labels_hold_as_solved():
    """in vertical-only and horizontal-only waves no two enabled segments share a tap, so every segment is decided on the
    samples it was solved with: the solver's targets show up as solved, segment by segment"""
    rng = np.random.default_rng(5)
    for wave in ("v", "h"):
        p, vb, hb = rv.luma_plane(8, rng, w=120, h=40, wave=wave, qp=37)
        _, info = rv.reference_plane(p, 37, vert_bs=vb, hor_bs=hb)
        lab = info["labels"]
        on = lab != rv.NOT_FILTERED
        if wave == "v":
            assert not on[:, :, 2:].any() and on[:, :, :2].any()
        else:
            assert not on[:, :, :2].any() and on[:, :, 2:].any()
            # hor1 and hor2 of one block are never both enabled (they share their Q taps)
            assert not (on[:, :, 2] & on[:, :, 3]).any()
        # a segment's samples are untouched by every other segment: filtering it alone gives the same label
        for by, bx, s in zip(*np.nonzero(on)):
            one_v, one_h = np.zeros_like(vb), np.zeros_like(hb)
            if s == 0:
                one_v[(by - 1) * (120 // 8 + 1) + bx] = 1
            elif s == 1:
                one_v[by * (120 // 8 + 1) + bx] = 1
            elif s == 2:
                one_h[by * (120 // 8) + bx - 1] = 1
            else:
                one_h[by * (120 // 8) + bx] = 1
            _, i1 = rv.reference_plane(p, 37, vert_bs=one_v, hor_bs=one_h)
            assert i1["labels"][by, bx, s] == lab[by, bx, s], (wave, by, bx, s)


def test_reference_known_answers():
    """hand-worked segments of cpu.h through the numpy restatement, with their labels"""
    w, h = 16, 8
    vb = np.zeros(3 * 1, np.uint8)
    hb = np.zeros(2 * 2, np.uint8)
    plane = np.full((h, w), 100, np.uint8)
    plane[:, 8:] = 104
    vb[1] = 2   # vert entry (row 0, x = 8): ver2 of block (1, 0) and ver1 of block (1, 1)
    out, info = rv.reference_plane(plane, 37, vert_bs=vb, hor_bs=hb)
    # QP 37: beta 36, tc 4; d = 0, |p0 - q0| = 4 < 5 * 4 / 2 = 10, beta / 8 = 4 > 0: strong, c = 8
    # p0' = 100 + ((100 + 200 - 600 + 208 + 104 + 4) >> 3) = 102, p1' = 100 + ((100 - 300 + 100 + 104 + 2) >> 2) = 101,
    # p2' = 100 + ((200 - 500 + 100 + 100 + 104 + 4) >> 3) = 101; q0' = 104 + (-8 >> 3) = 103, q1' = 104 + (-2 >> 2) = 103
    assert list(out[0, 4:12]) == [100, 101, 101, 102, 103, 103, 104, 104]
    assert info["labels"][0, 1, 1] == rv.LABELS.index("strong") and info["labels"][1, 1, 0] == rv.LABELS.index("strong")
    # QP 30: beta 22, tc 2: a step of 6 fails |p0 - q0| < 5 * 2 / 2 -> normal filter, 0 < 3 * 22 / 16 on both sides;
    # delta = (9 * 6 - 3 * 6 + 8) >> 4 = 2 < 10 * 2, clip(2, 4) = 2; dp1 = (100 - 100 + 2) >> 1 = 1, dq1 = (106 - 106 - 2) >> 1 = -1
    plane[:, 8:] = 106
    out, info = rv.reference_plane(plane, 30, vert_bs=vb, hor_bs=hb)
    assert list(out[0, 4:12]) == [100, 100, 101, 102, 104, 105, 106, 106]
    assert info["labels"][0, 1, 1] == rv.LABELS.index("normal_p1q1")
    # chroma (Q8): p0 = 100, q0 = 110, p1 = q1 = 100: dp = (-40 + 4) >> 3 = -5, dq = (40 + 4) >> 3 = 5, both clipped at tc 4
    c = np.full((8, 16), 100, np.uint8)
    c[:, 8] = 110
    c[:, 9:] = 100
    cvb = np.array([0, 2, 0], np.uint8)
    out, info = rv.reference_plane(c, 37, is_chroma=True, vert_bs=cvb, hor_bs=np.zeros(4, np.uint8))
    assert list(out[0, 6:10]) == [100, 96, 106, 100]
    # the rounding case: 4 (p0 - q0) + p1 - q1 = -12 == 4 (mod 8): dp = -1, dq = 2
    c[:, 7], c[:, 8], c[:, 6], c[:, 9] = 100, 103, 100, 100
    out, _ = rv.reference_plane(c, 37, is_chroma=True, vert_bs=cvb, hor_bs=np.zeros(4, np.uint8))
    assert list(out[0, 6:10]) == [100, 99, 101, 100]


@pytest.mark.parametrize("bd", BIT_DEPTHS)
def test_reference_equals_oracle(bd, oracle):
    """the numpy restatement and oracle/deblock_oracle.c, bit for bit: luma and chroma, scalar QPs 0..51, custom tables, the
    packed core's operand-range edge, QP maps with units of 8 .. 256 samples"""
    outs, _, _ = reference_outputs(bd)
    changed = 0
    for (name, p, kw), got in zip(vectors(bd), outs):
        want = oracle.filter_plane(p, bit_depth=bd, **kw)
        assert np.array_equal(got, want), (bd, name, np.argwhere(got != want)[:4])
        changed += not np.array_equal(got, p)
    assert changed > len(outs) // 2


# ---- the kernels' block arithmetic (tests/host_sim) --------------------------------------------------------------------

SIM_DIR = os.path.join(ROOT, "tests", "host_sim")


@pytest.fixture(scope="module")
def sim():
    subprocess.check_call(["make", "-s", "-C", SIM_DIR])
    L = C.CDLL(os.path.join(SIM_DIR, "libdbk_hostsim.so"))
    L.host_sim_filter_plane.restype = None
    if not L.host_sim_have_packed():
        pytest.fail("the host simulator was built without the packed core")
    return L


def run_sim(sim, plane, *, qp, packed, bit_depth=8, sample_bytes=None, is_chroma=False, vert_bs=None, hor_bs=None,
            qp_map=None, ctu_log2=6, tc_table=None, beta_table=None):
    dt = np.uint8 if (sample_bytes or (1 if bit_depth == 8 else 2)) == 1 else np.uint16
    out = np.ascontiguousarray(plane, dt).copy()
    h, w = out.shape
    tct, bt = (np.ascontiguousarray(t, np.uint8) for t in rv.tables_of(tc_table, beta_table))
    q, sh = min(qp, 51), bit_depth - 8
    vb, hb = np.ascontiguousarray(vert_bs, np.uint8), np.ascontiguousarray(hor_bs, np.uint8)
    m = None if qp_map is None else np.ascontiguousarray(qp_map, np.uint8)
    sim.host_sim_filter_plane(
        out.ctypes.data_as(C.c_void_p), w, h, C.c_long(out.strides[0]), out.itemsize, int(is_chroma),
        vb.ctypes.data_as(C.c_void_p), hb.ctypes.data_as(C.c_void_p), int(tct[q]) << sh, int(bt[q]) << sh, (1 << bit_depth) - 1,
        None if m is None else m.ctypes.data_as(C.c_void_p), 0 if m is None else m.shape[1], ctu_log2,
        tct.ctypes.data_as(C.c_void_p), bt.ctypes.data_as(C.c_void_p), sh, packed)
    return out


def _packed_ok(bd, kw):
    """the operands the launcher hands to the packed cores: up to 12 bit, luma tc within packed_luma_tc_fits"""
    if bd > 12:
        return False
    if kw.get("is_chroma"):
        return True
    tct, _ = rv.tables_of(kw.get("tc_table"), kw.get("beta_table"))
    tmax = int(tct.max()) if kw.get("qp_map") is not None else int(tct[min(kw["qp"], 51)])
    return rv.packed_tc_fits((1 << bd) - 1, tmax << (bd - 8))


@pytest.mark.parametrize("bd", BIT_DEPTHS)
def test_host_sim_equals_oracle(bd, sim):
    """generic (32-bit) core at every depth; packed cores where the launcher takes them: 8-bit bytes, 16-bit containers up to
    11 bit, the WIDE core at 12 bit -- scalar QP and QP-map (operand table) forms -- and 8-bit data in 16-bit containers"""
    outs, _, _ = reference_outputs(bd)
    n_packed = 0
    for (name, p, kw), want in zip(vectors(bd), outs):
        got = run_sim(sim, p, packed=0, bit_depth=bd, **kw)
        assert np.array_equal(got, want), (bd, name, "generic", np.argwhere(got != want)[:4])
        if _packed_ok(bd, kw):
            n_packed += 1
            got = run_sim(sim, p, packed=1, bit_depth=bd, **kw)
            assert np.array_equal(got, want), (bd, name, "packed", np.argwhere(got != want)[:4])
            if bd == 8:   # 8-bit data in 16-bit containers through the packed16 core
                got = run_sim(sim, p, packed=1, bit_depth=8, sample_bytes=2, **kw)
                assert np.array_equal(got, want.astype(np.uint16)), (name, "packed16@8")
    assert n_packed >= (len(outs) // 2 if bd <= 12 else 0)


def test_packed_operand_range_edge(sim):
    """packed_luma_tc_fits (deblock_packed.h) is the documented range of the 16-bit fields, for every scaled tc a table can
    produce, at every depth the packed cores take; the largest table entry it admits is 255 up to 10 bit and 128 at 11 / 12"""
    for bd in range(8, 13):
        max_v, sh = (1 << bd) - 1, bd - 8
        for t in range(0, (255 << sh) + 1):
            assert bool(sim.host_sim_packed_luma_tc_fits(max_v, t)) == rv.packed_tc_fits(max_v, t), (bd, t)
        assert rv.fits_edge(bd) == (255 if bd <= 10 else 128)


# ---- the pinned boundary frames ----------------------------------------------------------------------------------------

def _make_golden():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(GOLDEN, "make_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_boundary_frames_against_reference(oracle):
    """the boundary frames (make_golden.boundary_cases: 8-bit 4:2:0, scalar QP, luma bS override, default chroma bS) through
    the C oracle reproduce the reference's outputs recorded in tests/golden/ref_boundaries.json, and oracle/_ref's live where
    it is built; the numpy restatement agrees plane by plane"""
    with open(os.path.join(GOLDEN, "ref_boundaries.json")) as fh:
        rec = json.load(fh)["cases"]
    if not oracle.have_ref() and os.path.exists(oracle.REF_HEADER):
        oracle.build(ref=True)
    live = oracle.have_ref()
    cases = list(_make_golden().boundary_cases())
    assert len(cases) == len(rec) == 20
    for (w, h, qp, wave, buf, vb, hb), want in zip(cases, rec):
        assert (w, h, qp, wave, sha256(buf)) == (want["width"], want["height"], want["qp"], want["wave"], want["input_sha256"])
        got = oracle.filter_yuv420(buf, w, h, qp, vb, hb)
        assert sha256(got) == want["sha256"], (w, h, qp, wave)
        if live:
            assert got == oracle.ref_filter_yuv420(buf, w, h, qp, vb, hb), (w, h, qp, wave)
        y, u, v = oracle.split_yuv420(buf, w, h)
        gy, gu, gv = oracle.split_yuv420(got, w, h)
        assert np.array_equal(rv.reference_plane(y, qp, vert_bs=vb, hor_bs=hb)[0], gy)
        for c, g in ((u, gu), (v, gv)):
            assert np.array_equal(rv.reference_plane(c, qp, is_chroma=True)[0], g)
