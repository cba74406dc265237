"""The SAO decision per CTB without a GPU: the entry exists everywhere it must and refuses bad operands with the documented codes in
the documented order; the serial statement of the rule (tests/sao_decide_ref.py) does by construction what merging is for, and its
vectors exercise what they claim to; and csrc/sao_decide.h, compiled into a stand-alone program (plain and under the address and
undefined-behaviour sanitizers) that walks the anti-diagonals in chunks of 256 as the kernel does, reproduces the reference byte for
byte -- lambdas of 0 and 2^24 on sums at the int32 ends included, where only an exact 128-bit comparison agrees."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import rext_oracle as ro
import sao_decide_ref as D
import sao_stats_ref as S
from sao_decide_vectors import CENSUS, CONFIGS, LAYOUTS, case, decider

CSRC = os.path.join(ROOT, "gpu_video_codec_amd", "csrc")
SIM_SRC = os.path.join(ROOT, "tests", "sao_decide_sim", "sao_decide_sim.cpp")


@pytest.fixture(scope="module")
def L():
    from gpu_video_codec_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


# ---- the entry and its codes ----------------------------------------------------------------------------------------------------

def test_entry_is_exported_declared_and_bound(L):
    from gpu_video_codec_amd import _lib, deblock
    hdr = open(os.path.join(ROOT, "include", "hevc_deblock.h")).read()
    sym = "hevcdbk_sao_decide_device"
    assert re.search(r"\b%s\s*\(" % sym, hdr)
    assert sym in _lib.EXPORTS and hasattr(L, sym) and getattr(L, sym).argtypes is not None
    assert "typedef struct hevcdbk_sao_decision" in hdr
    assert C.sizeof(_lib.SaoDecision) == 32 and np.dtype(_lib.SAO_DECISION_DTYPE) == D.DECISION_DTYPE
    assert [f[0] for f in _lib.SaoDecision._fields_] == list(D.DECISION_DTYPE.names)
    assert callable(deblock.Context.sao_decide_device)


def test_documented_codes_and_their_order_without_a_device(L):
    """a context that no device stands behind (a zeroed block of memory: never looked into): every bad operand is refused with the
    documented code before the device is asked for anything; of two faults the one the header lists first decides the code"""
    from gpu_video_codec_amd import _lib
    ctx = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    ARG, DIM = _lib.ERR_ARG, _lib.ERR_DIMENSIONS
    SY, SCB, SCR, PY, PCB, PCR, DEC, IDX = (0x100000 * k for k in range(1, 9))      # 4 x 4 grids: 6 KiB of statistics at the most

    def call(ctx=ctx, sy=SY, scb=SCB, scr=SCR, stride=4, sfs=0, cx=4, cy=4, n=1, bl=8, bc=8, ll=1024, lc=1024, sl=None, tl=None, istride=0,
             py=PY, pcb=PCB, pcr=PCR, pstride=4, pfs=0, dec=DEC, dstride=4, dfs=0):
        return L.hevcdbk_sao_decide_device(ctx, sy, scb, scr, stride, sfs, cx, cy, n, bl, bc, ll, lc, sl, tl, istride, 0, py, pcb, pcr, pstride, pfs,
                                           dec, dstride, dfs, None)

    assert call(ctx=None) == ARG and call(sy=None) == ARG and call(py=None) == ARG and call(dec=None) == ARG
    assert call(scb=None) == ARG and call(scr=None) == ARG                         # exactly one of the two
    assert call(pcb=None) == ARG and call(pcr=None) == ARG                         # chroma statistics without a chroma output
    for d in (7, 17):
        assert call(bl=d) == ARG and call(bc=d) == ARG
    assert call(ll=(1 << 24) + 1) == ARG and call(lc=(1 << 24) + 1) == ARG
    assert call(cx=0) == DIM and call(cy=0) == DIM and call(cx=65536) == DIM and call(cy=65536) == DIM
    assert call(stride=3) == ARG and call(pstride=3) == ARG and call(dstride=3) == ARG
    assert call(sl=IDX, istride=3) == ARG and call(tl=IDX, istride=3) == ARG
    assert call(n=2, sfs=16, pfs=15, dfs=16) == ARG and call(n=2, sfs=16, pfs=16, dfs=15) == ARG
    assert call(n=65536, sfs=0, pfs=16, dfs=16) == ARG
    assert call(sy=SY + 2) == ARG and call(dec=DEC + 4) == ARG and call(sl=IDX + 1, istride=4) == ARG
    for kw in (dict(pcb=PY), dict(pcr=PY + 6 * 15), dict(pcb=PCR), dict(dec=PY + 8), dict(py=SY + 384 * 15 + 378), dict(pcr=SCB), dict(dec=SCR)):
        assert call(**kw) == ARG, kw                                               # an output on another output or on the statistics
    # without chroma the four chroma operands are not looked at
    luma = dict(scb=None, scr=None)
    assert call(ctx=None, **luma) == ARG                                            # ... and the call gets as far as the others do
    assert call(cx=0, pcb=None, pcr=None, bc=0, lc=1 << 30, **luma) == DIM
    # order: pointers and pairing, depths and lambdas, dimensions, then strides, frame strides, frames and overlaps
    assert call(bl=7, cx=0) == ARG and call(ll=1 << 25, cy=0) == ARG and call(pcb=None, cx=0) == ARG
    assert call(cx=0, stride=0) == DIM and call(cy=0, n=65536) == DIM and call(cx=0, pcb=PY) == DIM and call(cx=65536, dec=DEC + 4) == DIM


# ---- the reference: what merging is for -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("chroma", [False, True])
def test_identical_records_merge_left_stripes_merge_up_and_a_change_is_new(chroma):
    for name in ("8b_8b_equal", "10b_10b_unequal", "10b_12b_lambdas_2p24_int32_ends"):
        dec = decider(name, chroma)
        n = len(dec.palette)
        row = dec.decide(np.zeros((1, 12), np.int64) + 5)["decision"]["merge"]
        assert row[0, 0] == 0 and (row[0, 1:] == 1).all(), (name, row)
        stripes = dec.decide(np.broadcast_to(np.arange(0, 12) * 3 % n, (6, 12)).copy())["decision"]["merge"]
        assert (stripes[0] == 0).all() and (stripes[1:] == 2).all(), (name, stripes)
        # two runs: the first CTB of the second run has a left candidate that fits it badly
        res = dec.decide(np.array([[0] * 5 + [9] * 5]))
        assert res["decision"]["merge"][0].tolist() == [0, 1, 1, 1, 1, 0, 1, 1, 1, 1], name
        assert res["decision"]["cand"][0].tolist() == [0] + [1] * 9
    # also where NEW is "not applied": statistics of nothing
    empty = np.zeros((), S.STATS_DTYPE)
    dec = D.Decider([(empty, empty, empty)], bd_luma=8, lam_luma=1024, chroma=chroma)
    res = dec.decide(np.zeros((3, 4), np.int64))
    assert (res["params"][0]["type"] == 0).all() and res["decision"]["merge"].tolist() == [[0, 1, 1, 1]] + [[2, 1, 1, 1]] * 2


@pytest.mark.parametrize("name", CENSUS)
@pytest.mark.parametrize("cols,rows", [(5, 7), (61, 34)])
def test_census_of_the_vectors(name, cols, rows):
    """conditions on the vectors, asserted on the reference's own output, not measurements of the library"""
    _, _, _, _, res = case(name, True, cols, rows)
    c = D.census(res)
    print(name, cols, rows, c)
    assert min(c["share"]) >= 0.10, c
    assert c["left_chain"] >= 3 and c["up_of_merged"], c
    d = res["decision"]
    assert (d["zero"] == 0).all() and (res["j"] <= res["j_new"]).all()
    assert (d["flag_bits"][d["merge"] == 0] == (d["cand"][d["merge"] == 0] & 1) + (d["cand"][d["merge"] == 0] >> 1)).all()
    # a merged CTB holds a copy of its neighbour's triple
    for p in res["params"]:
        left, up = d["merge"] == 1, d["merge"] == 2
        assert (p[:, 1:][left[:, 1:]] == p[:, :-1][left[:, 1:]]).all() and (p[1:][up[1:]] == p[:-1][up[1:]]).all()


@pytest.mark.parametrize("kind", ["slices", "tiles"])
def test_a_boundary_changes_the_outcome(kind):
    hits = 0
    for cols, rows in ((5, 7), (61, 34)):
        _, _, _, _, free = case("8b_8b_equal", True, cols, rows)
        _, _, _, _, cut = case("8b_8b_equal", True, cols, rows, kind)
        lost = cut["decision"]["cand"] != free["decision"]["cand"]
        assert lost.any() and (cut["decision"]["cand"][lost] & ~free["decision"]["cand"][lost] == 0).all()
        hits += int((lost & (cut["decision"]["merge"] != free["decision"]["merge"])).sum())
        # and past the boundary: a CTB whose candidates are the same inherits something else
        assert any((cut["params"][c] != free["params"][c])[~lost].any() for c in range(3)) or cols == 5
    assert hits > 0


def test_128_bits_are_needed():
    """the vectors at the int32 ends with lambdas of 2^24: J leaves 64 bits, and J taken modulo 2^64 would decide otherwise"""
    _, _, _, _, res = case("10b_12b_lambdas_2p24_int32_ends", True, 61, 34)
    big = max(abs(int(j)) for j in res["j"].ravel())
    assert big >= 1 << 64, big
    class Wrapped(D.Decider):
        def J(self, c_y, c_c, F):
            return ((D.Decider.J(self, c_y, c_c, F) + (1 << 63)) % (1 << 64)) - (1 << 63)

    for name in ("10b_12b_lambdas_2p24_int32_ends", "8b_8b_lambdas_2p24_and_1_int32_ends"):
        bl, bc, ll, lc, _ = CONFIGS[name]
        dec, idx, _, _, res = case(name, True, 61, 34)
        short = Wrapped(dec.palette, bd_luma=bl, bd_chroma=bc, lam_luma=ll, lam_chroma=lc).decide(idx)
        assert (short["decision"]["merge"] != res["decision"]["merge"]).sum() >= 10, name


def test_no_candidate_is_the_two_picks():
    for name in ("8b_12b_unequal", "10b_12b_lambdas_2p24_int32_ends"):
        bl, bc, ll, lc, _ = CONFIGS[name]
        dec, idx, _, _, res = case(name, True, 5, 7, "ctb_slices")
        sy, scb, scr = dec.stats(idx)
        py, _, dy = S.pick_plane(sy, None, bl, ll)
        pcb, pcr, dc = S.pick_plane(scb, scr, bc, lc)
        for got, want in zip(res["params"], (py, pcb, pcr)):
            assert got.tobytes() == want.tobytes(), name
        d = res["decision"]
        assert not d["merge"].any() and not d["cand"].any() and not d["flag_bits"].any() and np.array_equal(d["delta_d"], dy + dc)


# ---- csrc/sao_decide.h on the CPU -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=["plain", "sanitized"])
def sim(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("sao_decide_sim_" + request.param)
    exe = str(d / "sao_decide_sim")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas"] + flags + ["-I", CSRC, "-o", exe, SIM_SRC])
    return exe, str(d)


def run_sim(sim, name, dec, idx, sl, tl):
    exe, d = sim
    bl, bc, ll, lc, _ = CONFIGS[name]
    rows, cols = idx.shape
    n = rows * cols
    st = dec.stats(idx)
    blob = np.array([cols, rows, int(dec.chroma), bl, bc, ll, lc, int(sl is not None), int(tl is not None)], "<i4").tobytes()
    blob += b"".join(s.tobytes() for s in (st if dec.chroma else st[:1]))
    blob += b"".join(np.ascontiguousarray(a, "<u2").tobytes() for a in (sl, tl) if a is not None)
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    open(fin, "wb").write(blob)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw = open(fout, "rb").read()
    k = 3 if dec.chroma else 1
    assert len(raw) == n * (6 * k + 32)
    params = [np.frombuffer(raw[c * n * 6: (c + 1) * n * 6], ro.SAO_CTB_DTYPE).reshape(rows, cols) for c in range(k)]
    return params, np.frombuffer(raw[k * n * 6:], D.DECISION_DTYPE).reshape(rows, cols)


def same(got, res, tag):
    params, dec = got
    for c, p in enumerate(params):
        assert p.tobytes() == res["params"][c].tobytes(), (tag, "params", c, np.argwhere(p != res["params"][c])[:4].tolist())
    assert dec.tobytes() == res["decision"].tobytes(), (tag, [f for f in D.DECISION_DTYPE.names if not np.array_equal(dec[f], res["decision"][f])],
                                                        np.argwhere(dec["merge"] != res["decision"]["merge"])[:4].tolist())


@pytest.mark.parametrize("chroma", [False, True])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_procedure_reproduces_the_reference(sim, name, chroma):
    for cols, rows in D.GRIDS:
        dec, idx, sl, tl, res = case(name, chroma, cols, rows)
        same(run_sim(sim, name, dec, idx, sl, tl), res, (name, chroma, cols, rows))


@pytest.mark.parametrize("chroma", [False, True])
@pytest.mark.parametrize("kind", LAYOUTS)
def test_procedure_under_slices_and_tiles(sim, kind, chroma):
    for name in ("8b_8b_equal", "10b_12b_lambdas_2p24_int32_ends"):
        for cols, rows in ((9, 1), (5, 7), (61, 34)):
            dec, idx, sl, tl, res = case(name, chroma, cols, rows, kind)
            same(run_sim(sim, name, dec, idx, sl, tl), res, (name, chroma, cols, rows, kind))
            if kind == "ctb_slices":
                assert not res["decision"]["merge"].any()


def test_a_diagonal_longer_than_a_chunk(sim):
    """300 x 290 CTBs, luma alone: diagonals of up to 290 CTBs, so a second chunk of the 256 runs"""
    dec, idx, sl, tl, res = case("8b_8b_equal", False, 300, 290)
    same(run_sim(sim, "8b_8b_equal", dec, idx, sl, tl), res, "300x290")
    assert D.census(res)["left_chain"] >= 3
