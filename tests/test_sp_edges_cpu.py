"""The semi-planar kernels' per-lane procedures at the decision edges, over the full sample range and over every boundary byte,
without a GPU: the vectors of tests/sp_edge_vectors.py through the existing simulations (tests/sp_sim, tests/sao_sp_sim, tests/fused_sp_sim)
against the existing statements (sp_ref.deblock, rext_oracle.sao_plane / sao_borders_ref.sao_plane_by_bytes per component, the chain of the
two), and the CONDITIONS on the vectors that keep tests/test_gpu_sp_edges.py, which runs the same vectors through the kernels, from
passing vacuously: what each vector reaches is asserted here, on the reference alone."""
import ctypes as C
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

import rext_oracle as rx
import sao_borders_ref as B
import sao_bytes_vectors as V
import sp_edge_vectors as E
import sp_ref as S
from test_fused_sp_cpu import run_sim as fused_run_sim
from test_sao_sp_cpu import run_sim as sao_run_sim

OPS = [o[0] for o in E.OPERANDS]
BIG = [s for s in S.DBK if s[1] >= 36 and s[2] >= 20]     # every shape from 36x36 up: each meets the census on its own
FUSED_OPS = ["q51", "allqp", "slices"]                    # one QP, the all-QP map, per-slice pairs


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def diff(got, want):
    return int((got != want).sum()), np.argwhere(got != want)[:4].tolist()


# ---- the simulations -------------------------------------------------------------------------------------------------------------------

def _shared(tmp_path_factory, name, restype_of):
    from conftest import ROOT
    out = str(tmp_path_factory.mktemp(name) / ("lib%s.so" % name))
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", out,
                           os.path.join(ROOT, "tests", name, name + ".cpp")])
    lib = C.CDLL(out)
    getattr(lib, restype_of).restype = C.c_int
    return lib


@pytest.fixture(scope="module")
def dbk_sim(tmp_path_factory):
    return _shared(tmp_path_factory, "sp_sim", "sp_sim_filter_plane")


@pytest.fixture(scope="module")
def sao_sim(tmp_path_factory):
    return _shared(tmp_path_factory, "sao_sp_sim", "sao_sp_sim_plane")


@pytest.fixture(scope="module")
def fused_sim(tmp_path_factory):
    from conftest import ROOT
    out = str(tmp_path_factory.mktemp("fused_sp_sim")) + os.sep
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "fused_sp_sim"), "OUT=" + out, "all"])
    return out


def forms(c):
    return (0, 1) if c["depth"] <= 12 else (0,)


def run_dbk(sim, c, f, form):
    out = np.ascontiguousarray(c["planes"][f]).copy()
    vb, hb = (np.ascontiguousarray(x) for x in c["bs"][f])
    m = c["qp_map"]
    pr = None if c["pairs"] is None else np.ascontiguousarray(c["pairs"], np.int8)
    rc = sim.sp_sim_filter_plane(vp(out), c["w"], c["h"], C.c_long(out.strides[0]), out.itemsize, c["depth"], vp(vb), vp(hb), c["qp"], vp(m),
                                 0 if m is None else m.shape[1], E.UNIT_LOG2, c["cb"], c["cr"], c["tc_div2"], vp(pr),
                                 0 if pr is None else pr.shape[1], E.SL_CTB_LOG2, form)
    assert rc == 0
    return out


def run_sao(sim, c, f, keep, borders, form):
    """test_sao_sp_cpu.run_sim (the plane inside a larger, poisoned array) with the vector's arbitrary bytes"""
    return sao_run_sim(sim, c, f, keep, None, form, 0xEE, nox=c["nox"][f] if borders else None)


def run_fused(sim, c, f, borders):
    """test_fused_sp_cpu.run_sim (the stand-alone program that drives the pair body tile by tile) under the case's own operands"""
    m, pr = c["qp_map"], c["pairs"]
    job = dict(c, qp_map=np.zeros((1, 1), np.uint8) if m is None else m, pairs=np.zeros((1, 1, 2), np.int8) if pr is None else pr)
    return fused_run_sim(sim, job, f, m is not None, pr is not None, None, 0xC3, 0xEE, nox=c["nox"][f] if borders else None)


# ---- deblocking: the block procedure on the vectors --------------------------------------------------------------------------------------

@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("spec", S.DBK, ids=lambda s: s[0])
def test_deblocking_block_procedure(dbk_sim, spec, op):
    """the three frames (vertical, horizontal, both); the per-sample form and, up to 12 bit, the packed form"""
    c = E.dbk_case(spec, op)
    for f in range(3):
        want = E.dbk_expected(c, f)
        for form in forms(c):
            got = run_dbk(dbk_sim, c, f, form)
            assert np.array_equal(got, want), (c["name"], E.FRAMES[f], form) + diff(got, want)


# ---- deblocking: what the vectors reach -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dbk_censuses():
    return {(s[0], op): E.dbk_census(E.dbk_case(s, op)) for s in S.DBK for op in OPS}


@pytest.mark.parametrize("spec", S.DBK, ids=lambda s: s[0])
def test_deblocking_vectors_reach_every_clip(dbk_censuses, spec):
    """Per component and direction, summed over the operand sets: the delta clip at -tC and at +tC, Clip1 of p0 and of q0 at 0 and at
    max_v.  Every shape from 36x36 up meets this on its own -- so does the union of the shapes that run each kernel (the 32-bit
    kernel: all; the packed 8-bit kernel: the 8-bit ones; the packed 16-bit kernel: the 10-bit ones).  Under every operand set
    whose tC is not 0 both components change in every frame; on 16x16 and 12x12, with four and two segments per row, over the three
    frames (their all-QP maps hold the highest QPs, so tC is not 0 there either); the new last edge moves samples of both."""
    name, w, h, _ = spec
    for k in range(2):
        for d in ("v", "h"):
            tot = Counter()
            for op in OPS:
                tot.update({e: n for e, n in dbk_censuses[(name, op)][k][d].items() if isinstance(e, str)})
            if spec in BIG:
                assert all(tot[e] > 0 for e in E.EVENTS), (name, k, d, dict(tot))
        for op in OPS:
            cen = dbk_censuses[(name, op)][k]
            c = E.dbk_case(spec, op)
            if op not in ("allqp", "slices") and E.tc_of(c, k, c["qp"])[1] == 0:   # "q0", and the even samples of "q20"
                assert cen["changed"] == [0, 0, 0], (name, op, k, cen["changed"])
            else:
                assert all(n > 0 for n in cen["changed"]) if spec in BIG else sum(cen["changed"]) > 0, (name, op, k, cen["changed"])
                assert (w % 8 == 0 or cen["new_cols"] > 0) and (h % 8 == 0 or cen["new_rows"] > 0), (name, op, k, cen)
    assert {s[3] for s in BIG} == {8, 10, 14} and len(BIG) == len(S.DBK) - 2


def test_deblocking_vectors_reach_the_knees_of_table_8_10(dbk_censuses):
    """qPi = ((QpQ + QpP + 1) >> 1) + cQpPicOffset of the filtered segments: 29 and 30, 43 and 44, a negative one, 63 -- on every shape
    from 36x36 up, per depth"""
    for spec in BIG:
        seen = set()
        for op in OPS:
            for k in range(2):
                for d in ("v", "h"):
                    seen |= {e[1] for e in dbk_censuses[(spec[0], op)][k][d] if not isinstance(e, str)}
        assert {29, 30, 43, 44, 63} <= seen and min(seen) < 0, (spec[0], sorted(seen))
    # the all-QP map puts segments on both sides of each knee in one launch
    seen = {e[1] for k in range(2) for d in ("v", "h") for e in dbk_censuses[("1032x24", "allqp")][k][d] if not isinstance(e, str)}
    assert {29, 30, 43, 44} <= seen and min(seen) < 0 and max(seen) > 51, sorted(seen)


def test_tc_zero_changes_nothing_and_q_is_clipped_to_53():
    """the second operand set: Q = Clip3(0, 53, QpC + 2 - 12) is 0 and 2, tC = 0 -- NOTHING changes although bS is 2 on extreme content;
    the first: QpC + 2 + 12 = 71, clipped to 53, tC' = 24"""
    for spec in S.DBK:
        c = E.dbk_case(spec, "q0")
        assert [E.tc_of(c, k, 0) for k in range(2)] == [(-22, 0), (2, 0)]
        for f in range(3):
            vb, hb = c["bs"][f]
            assert ((vb & 3) == 2).any() == (f != 1) and ((hb & 3) == 2).any() == (f != 0), (spec[0], f)
            assert np.array_equal(E.dbk_expected(c, f), c["planes"][f]), (spec[0], f)
        c = E.dbk_case(spec, "q51")
        (q0, t0), (q1, t1) = E.tc_of(c, 0, 51), E.tc_of(c, 1, 51)
        assert q0 == 71 and t0 == 24 << (c["depth"] - 8) and q1 == 49 and t1 == 16 << (c["depth"] - 8)


@pytest.mark.parametrize("spec", S.DBK, ids=lambda s: s[0])
def test_exchanging_the_offsets_changes_both_components(dbk_censuses, spec):
    """wherever the two cQpPicOffsets give different tC (not "q0": tC 0 twice; not "q36": qPi 29 and 30 are both QpC 29) the expectation
    with the offsets exchanged differs in BOTH components"""
    for op in OPS:
        c = E.dbk_case(spec, op)
        cen = dbk_censuses[(spec[0], op)]
        if op in ("q0", "q36"):
            assert E.tc_of(c, 0, c["qp"])[1] == E.tc_of(c, 1, c["qp"])[1]
            assert cen[0]["swap"] == 0 and cen[1]["swap"] == 0
        else:
            assert cen[0]["swap"] > 0 and cen[1]["swap"] > 0, (spec[0], op, cen[0]["swap"], cen[1]["swap"])


def test_per_slice_pairs_and_the_both_way_frame():
    """the per-slice set holds every tC offset of SLICE_VALUES where the plane has five slices, and the call's own offsets are 0, so no
    sum leaves -6 .. 6; the third frame has entries in both directions; the components' contents differ"""
    for spec in S.DBK:
        c = E.dbk_case(spec, "slices")
        assert c["tc_div2"] == 0 and set(np.unique(c["pairs"])) <= set(E.SLICE_VALUES)
        if c["pairs"].shape[0] * c["pairs"].shape[1] >= 15:
            assert set(np.unique(c["pairs"][..., 1])) == set(E.SLICE_VALUES), spec[0]
        for op in OPS:
            c = E.dbk_case(spec, op)
            assert not np.array_equal(c["planes"][0][..., 0], c["planes"][0][..., 1])
            vb, hb = c["bs"][2]
            assert ((hb & 3) == 2).any() and ((vb & 3) == 2).any()


# ---- SAO: the block procedures on the vectors -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spec", E.SAO, ids=lambda s: s[0])
def test_sao_block_procedures_full_range(sao_sim, spec):
    """every frame x {no keep map, keep map} x {no borders, ARBITRARY bytes}; the per-sample form and, up to 12 bit, the packed form"""
    c = E.sao_case(spec)
    for f in range(len(c["planes"])):
        for keep in (False, True):
            for borders in (False, True):
                want = E.sao_expected(c, f, keep, borders)
                for form in forms(c):
                    got = run_sao(sao_sim, c, f, keep, borders, form)
                    assert np.array_equal(got, want), (spec[0], f, keep, borders, form) + diff(got, want)


@pytest.mark.parametrize("name", list(E.BYTES))
def test_sao_block_procedures_every_byte(sao_sim, name):
    c = E.bytes_case(name)
    for f in range(len(c["planes"])):
        want = E.bytes_expected(name, f)
        for form in forms(c):
            got = run_sao(sao_sim, c, f, False, True, form)
            assert np.array_equal(got, want), (name, f, form) + diff(got, want)


# ---- SAO: what the vectors reach -----------------------------------------------------------------------------------------------------------

def test_sao_vectors_reach_the_range_and_every_class():
    """per component, on EVERY shape (12x12 and 72x24 at 14 bit, the per-sample kernel's own, among them): SAO clips at 0 and at
    max_v, offsets -128 and 127 are applied, a band wraps; the spec-legal scaled limit of the depth is applied from 72 columns up;
    over the set every band position 0..31 and every edge class x category"""
    bands, edges = [set(), set()], [set(), set()]
    for spec in E.SAO:
        c = E.sao_case(spec)
        tags = E.sao_tags(c)
        for k in range(2):
            bands[k] |= {t[1] for t in tags[k] if isinstance(t, tuple) and t[0] == "band"}
            edges[k] |= {t[1:] for t in tags[k] if isinstance(t, tuple) and t[0] == "edge"}
            offs = {t[1] for t in tags[k] if isinstance(t, tuple) and t[0] == "offset"}
            assert "clip_lo" in tags[k] and "clip_hi" in tags[k], (spec[0], k)
            assert {-128, 127} <= offs, (spec[0], k, sorted(offs))
            assert any(isinstance(t, tuple) and t[0] == "wrap" for t in tags[k]), (spec[0], k)
            if spec[1] >= 72:
                lim = max(E.hv.sao_offset_limits(c["depth"]))
                assert {-lim, lim} <= offs, (spec[0], k, lim)
    for k in range(2):
        assert bands[k] == set(range(32)), (k, sorted(bands[k]))
        assert edges[k] == {(c, e) for c in range(4) for e in range(1, 5)}, (k, sorted(edges[k]))


@pytest.mark.parametrize("spec", [s for s in E.SAO if s[1] >= 72], ids=lambda s: s[0])
def test_sao_vectors_change_samples_on_both_sides_of_every_border(spec):
    """the columns and rows on both sides of the SAO wave and strip and of the fused tiles hold 0 next to max_v, and samples change in
    every one of them, in both components"""
    c = E.sao_case(spec)
    want_cols = {1: {63, 64, 95, 96, 191, 192, 255, 256}, 2: {63, 64, 127, 128, 191, 192, 255, 256}}[c["sb"]]
    assert set(c["cols"]) == {x for x in want_cols if x < c["w"]} and c["rows"] == tuple(y for y in (63, 64, 127, 128) if y < c["h"])
    max_v = (1 << c["depth"]) - 1
    for k, cen in enumerate(E.sao_border_changes(c)):
        assert all(n > 0 for n in cen.values()), (spec[0], k, dict(cen))
        for x in c["cols"][::2]:
            pl = c["planes"][0][..., k].astype(np.int64)
            assert (np.abs(pl[:, x] - pl[:, x + 1]) == max_v).any(), (spec[0], k, x)


@pytest.mark.parametrize("spec", E.SAO, ids=lambda s: s[0])
def test_sao_parameters_agree_in_more_than_half_of_the_ctbs(spec):
    c = E.sao_case(spec)
    n, same, types, classes = E.sao_agreement(c)
    assert 2 * same > n and types > 0, (spec[0], n, same, types, classes)
    if n > 2 * 4:
        assert classes > 0, (spec[0], n, same, types, classes)
    # the keep map and the bytes both bite (in every frame of the shapes with an interior wave), and the bytes are no layout's
    kept = [(E.sao_expected(c, f, True, False) != E.sao_expected(c, f, False, False)).any() for f in range(len(c["planes"]))]
    byted = [(E.sao_expected(c, f, False, True) != E.sao_expected(c, f, False, False)).any() for f in range(len(c["planes"]))]
    assert (all(kept) and all(byted)) if spec[1] >= 140 else (any(kept) and any(byted)), (spec[0], kept, byted)
    for f in range(len(c["planes"])):
        nox = c["nox"][f][:, : c["pcb"][f].shape[1]]
        assert not np.array_equal(B.reconciled(nox), nox)


# ---- every byte -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(E.BYTES))
def test_every_byte_pairs_are_what_they_claim(name):
    """every (byte, class) pair on an interior CTB of EACH component, one byte array for both; per interior CTB and component, each bit
    its class looks at changes that CTB's output and no other bit does (the assertion of test_sao_bytes_cpu.py, per component)"""
    c = E.bytes_case(name)
    rows, cols = c["grid"]
    lg = c["lg"]
    assert rows == -(-c["h"] >> lg) and cols == -(-c["w"] >> lg) and (name != "bytes_8b_g4_ctb8" or (c["w"] % 8 == 4 and c["h"] % 8 == 4))
    interior = np.zeros((rows, cols), bool)
    interior[1:-1, 1:-1] = True
    for k, key in enumerate(("pcb", "pcr")):
        seen = set()
        for f, prm in enumerate(c[key]):
            assert (prm["type"][1:-1, 1:-1] == 2).all()
            seen |= set(zip(c["nox"][f, 1:-1, 1:cols - 1].ravel().tolist(), prm["cls"][1:-1, 1:-1].ravel().tolist()))
        assert seen == {(b, cl) for b in range(256) for cl in range(4)}, (name, k, len(seen))
    assert all((b["cls"][1:-1, 1:-1] != r["cls"][1:-1, 1:-1]).all() for b, r in zip(c["pcb"], c["pcr"]))

    def per_ctb(d):
        full = np.zeros((rows << lg, cols << lg), bool)
        full[: c["h"], : c["w"]] = d
        return full.reshape(rows, 1 << lg, cols, 1 << lg).any(axis=(1, 3))

    for f in range(len(c["planes"])):
        base, nox = E.bytes_expected(name, f), c["nox"][f]
        for k, key in enumerate(("pcb", "pcr")):
            comp, prm = np.ascontiguousarray(c["planes"][f][..., k]), c[key][f]
            free = rx.sao_plane(comp, prm, lg, lg, bit_depth=c["depth"])
            look = B.look_bits(prm, lg, lg, c["h"], c["w"])
            relevant = np.vectorize(V.RELEVANT.get)(prm["cls"].astype(np.int64) & 3)
            assert (base[..., k] != free).any()
            for bit in range(8):
                out = B.sao_plane_by_bytes(comp, prm, lg, lg, nox ^ np.uint8(1 << bit), bit_depth=c["depth"], _free=free, _look=look)
                changed = per_ctb(out != base[..., k])
                rel = (relevant & (1 << bit)) != 0
                assert changed[interior & rel].all() and not changed[interior & ~rel].any(), (name, f, k, bit)


# ---- deblocking + SAO: the pair body tile by tile -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("op", FUSED_OPS)
@pytest.mark.parametrize("name", E.FUSED)
def test_pair_body_on_decision_edges_under_full_range_sao(fused_sim, name, op):
    """the deblocking vectors with full-range SAO content over every third 16 x 16 block; with and without the arbitrary bytes; both
    stages do something in both components"""
    c = E.chain_case(name, op)
    for f in range(E.SAO_FRAMES):
        for borders in (False, True):
            dbk, want = E.chain_expected(c, f, borders)
            for k in range(2):
                assert (dbk[..., k] != c["planes"][f][..., k]).any() and (want[..., k] != dbk[..., k]).any()
            got = run_fused(fused_sim, c, f, borders)
            assert np.array_equal(got, want), (name, op, f, borders) + diff(got, want)


@pytest.mark.parametrize("name", list(E.BYTES))
def test_pair_body_every_byte(fused_sim, name):
    """bS all 0: deblocking is the identity and the SAO stage sees every byte"""
    c = dict(E.bytes_case(name), qp=30, cb=-3, cr=4, tc_div2=0, qp_map=None, pairs=None)
    c["bs"] = E.bytes_bs(c)
    for f in range(len(c["planes"])):
        got = run_fused(fused_sim, c, f, True)
        want = E.bytes_expected(name, f)
        assert np.array_equal(got, want), (name, f) + diff(got, want)
