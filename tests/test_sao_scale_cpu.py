"""SAO estimation with log2_sao_offset_scale without a GPU: hevcdbk_sao_pick_device_os and hevcdbk_sao_decide_device_os exist
everywhere they must and refuse bad operands with the documented codes in the documented order; the plain-int statement of the rule
(tests/sao_scale_ref.py) is the existing references' at a scale of 0, its vectors meet the conditions they are built for, and its tie
vectors come out as the rule says; and csrc/sao_pick_os.h, compiled into a stand-alone program (plain and under the address and
undefined-behaviour sanitizers) that runs every step for all 64 lanes of a wave and then walks the anti-diagonals, reproduces the
reference byte for byte."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import rext_oracle as ro
import sao_decide_ref as D
import sao_decide_vectors as DV
import sao_scale_ref as R
import sao_scale_vectors as V
import sao_stats_ref as S

CSRC = os.path.join(ROOT, "gpu_video_codec_amd", "csrc")
SIM_SRC = os.path.join(ROOT, "tests", "sao_scale_sim", "sao_scale_sim.cpp")
PICK, DECIDE = "hevcdbk_sao_pick_device_os", "hevcdbk_sao_decide_device_os"


@pytest.fixture(scope="module")
def L():
    from gpu_video_codec_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


# ---- the entries and their codes -------------------------------------------------------------------------------------------------

def test_entries_are_exported_declared_and_bound(L):
    import inspect
    from gpu_video_codec_amd import _lib, deblock
    hdr = open(os.path.join(ROOT, "include", "hevc_deblock.h")).read()
    for sym, base, extra in ((PICK, "hevcdbk_sao_pick_device", 1), (DECIDE, "hevcdbk_sao_decide_device", 2)):
        assert re.search(r"\b%s\s*\(" % sym, hdr)
        assert sym in _lib.EXPORTS and hasattr(L, sym)
        assert len(getattr(L, sym).argtypes) == len(getattr(L, base).argtypes) + extra
    assert re.search(r"unsigned bit_depth, unsigned log2_offset_scale, unsigned lambda_q8", hdr)
    assert re.search(r"unsigned\s+bit_depth_chroma, unsigned log2_offset_scale_luma, unsigned log2_offset_scale_chroma,\s+unsigned lambda_q8_luma", hdr)
    assert inspect.signature(deblock.Context.sao_pick_device).parameters["log2_offset_scale"].default is None
    sig = inspect.signature(deblock.Context.sao_decide_device).parameters
    assert sig["log2_offset_scale"].default is None and sig["log2_offset_scale_chroma"].default is None


def test_pick_codes_and_their_order_without_a_device(L):
    """a context that no device stands behind (a zeroed block of memory: never looked into): the refusals of hevcdbk_sao_pick_device in
    its order, the illegal scale with the depth and the lambda, the legal scale beyond int8_t last"""
    from gpu_video_codec_amd import _lib
    ctx = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    ARG, DIM, UNS = _lib.ERR_ARG, _lib.ERR_DIMENSIONS, _lib.ERR_UNSUPPORTED
    SA, SB, PA, PB, DD = (0x100000 * k for k in range(1, 6))

    def call(ctx=ctx, sa=SA, sb=SB, stride=4, sfs=0, cx=4, cy=4, n=1, bd=12, k=2, lam=1024, pa=PA, pb=PB, pstride=4, pfs=0, dd=DD):
        return L.hevcdbk_sao_pick_device_os(ctx, sa, sb, stride, sfs, cx, cy, n, bd, k, lam, pa, pb, pstride, pfs, dd, None)

    assert call(ctx=None) == ARG and call(sa=None) == ARG and call(pa=None) == ARG and call(sb=None) == ARG and call(pb=None) == ARG
    assert call(bd=7) == ARG and call(bd=17, k=0) == ARG and call(lam=(1 << 24) + 1) == ARG
    for bd, k in ((8, 1), (10, 1), (11, 2), (12, 3), (13, 4), (16, 7)):
        assert call(bd=bd, k=k) == ARG, (bd, k)                                   # no stream codes it
    for bd, k in ((13, 3), (14, 4), (16, 3), (16, 6)):
        assert call(bd=bd, k=k) == UNS, (bd, k)                                   # legal, beyond int8_t
    assert call(cx=0) == DIM and call(cy=0) == DIM and call(cy=65536) == DIM and call(n=65536) == DIM
    assert call(stride=3) == ARG and call(pstride=3) == ARG and call(sa=SA + 2) == ARG and call(dd=DD + 4) == ARG
    assert call(n=2, sfs=16, pfs=15) == ARG
    # the order: the illegal scale before the grid, the unsupported one after everything else
    assert call(bd=12, k=3, cx=0) == ARG and call(bd=16, k=3, cx=0) == DIM
    assert call(bd=16, k=3, stride=3) == ARG and call(bd=16, k=3, n=2, sfs=16, pfs=15) == ARG and call(bd=16, k=3, dd=DD + 4) == ARG
    assert call(bd=7, k=9) == ARG and call(ctx=None, bd=16, k=3) == ARG


def test_decide_codes_and_their_order_without_a_device(L):
    from gpu_video_codec_amd import _lib
    ctx = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    ARG, DIM, UNS = _lib.ERR_ARG, _lib.ERR_DIMENSIONS, _lib.ERR_UNSUPPORTED
    SY, SCB, SCR, PY, PCB, PCR, DEC, IDX = (0x100000 * k for k in range(1, 9))      # 4 x 4 grids: 6 KiB of statistics at the most

    def call(ctx=ctx, sy=SY, scb=SCB, scr=SCR, stride=4, sfs=0, cx=4, cy=4, n=1, bl=12, bc=12, kl=2, kc=2, ll=1024, lc=1024, sl=None, tl=None,
             istride=0, py=PY, pcb=PCB, pcr=PCR, pstride=4, pfs=0, dec=DEC, dstride=4, dfs=0):
        return L.hevcdbk_sao_decide_device_os(ctx, sy, scb, scr, stride, sfs, cx, cy, n, bl, bc, kl, kc, ll, lc, sl, tl, istride, 0, py, pcb, pcr,
                                              pstride, pfs, dec, dstride, dfs, None)

    # the refusals of hevcdbk_sao_decide_device, as tests/test_sao_decide_cpu.py lists them
    assert call(ctx=None) == ARG and call(sy=None) == ARG and call(py=None) == ARG and call(dec=None) == ARG
    assert call(scb=None) == ARG and call(scr=None) == ARG and call(pcb=None) == ARG and call(pcr=None) == ARG
    for d in (7, 17):
        assert call(bl=d, kl=0) == ARG and call(bc=d, kc=0) == ARG
    assert call(ll=(1 << 24) + 1) == ARG and call(lc=(1 << 24) + 1) == ARG
    assert call(cx=0) == DIM and call(cy=0) == DIM and call(cx=65536) == DIM and call(cy=65536) == DIM
    assert call(stride=3) == ARG and call(pstride=3) == ARG and call(dstride=3) == ARG
    assert call(sl=IDX, istride=3) == ARG and call(tl=IDX, istride=3) == ARG
    assert call(n=2, sfs=16, pfs=15, dfs=16) == ARG and call(n=2, sfs=16, pfs=16, dfs=15) == ARG
    assert call(n=65536, sfs=0, pfs=16, dfs=16) == ARG
    assert call(sy=SY + 2) == ARG and call(dec=DEC + 4) == ARG and call(sl=IDX + 1, istride=4) == ARG
    for kw in (dict(pcb=PY), dict(pcr=PY + 6 * 15), dict(pcb=PCR), dict(dec=PY + 8), dict(py=SY + 384 * 15 + 378), dict(pcr=SCB), dict(dec=SCR)):
        assert call(**kw) == ARG, kw
    # the scales: illegal for the depth of its component -- with the depths and lambdas; legal above 2 -- last
    assert call(kl=3) == ARG and call(kc=3) == ARG and call(bl=10, kl=1) == ARG and call(bc=11, kc=2) == ARG and call(bl=8, kl=1, bc=16) == ARG
    assert call(bl=16, kl=3) == UNS and call(bc=16, kc=3) == UNS and call(bl=13, kl=3, bc=13, kc=3) == UNS and call(bl=16, kl=6) == UNS
    assert call(bl=12, kl=3, cx=0) == ARG and call(bl=16, kl=3, cx=0) == DIM and call(bc=12, kc=3, cy=0) == ARG and call(bc=16, kc=3, cy=0) == DIM
    for kw in (dict(stride=3), dict(n=2, sfs=16, pfs=15, dfs=16), dict(n=65536, pfs=16, dfs=16), dict(dec=DEC + 4), dict(pcb=PY), dict(dec=SCR)):
        assert call(bl=16, kl=3, **kw) == ARG, kw                                  # everything else comes before UNSUPPORTED
    assert call(bl=7, kl=9) == ARG and call(ctx=None, bl=16, kl=3) == ARG and call(scb=None, bl=16, kl=3) == ARG
    # without chroma the chroma scale is not looked at, like the other chroma operands
    luma = dict(scb=None, scr=None, pcb=None, pcr=None)
    assert call(cx=0, bc=0, lc=1 << 30, kc=99, **luma) == DIM and call(bl=16, kl=3, kc=99, **luma) == UNS and call(bl=16, kl=2, kc=99, cx=0, **luma) == DIM


# ---- the reference at a scale of 0 ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(DV.CONFIGS))
def test_scale_0_is_the_existing_references(name):
    bl, bc, ll, lc, _ = DV.CONFIGS[name]
    for chroma in (False, True):
        for cols, rows in D.GRIDS:
            dec, idx, sl, tl, res = DV.case(name, chroma, cols, rows)
            mine = R.Decider(dec.palette, bd_luma=bl, bd_chroma=bc, lam_luma=ll, lam_chroma=lc, chroma=chroma, k_luma=0, k_chroma=0).decide(idx)
            assert mine["decision"].tobytes() == res["decision"].tobytes(), (name, chroma, cols, rows)
            for c in range(3 if chroma else 1):
                assert mine["params"][c].tobytes() == res["params"][c].tobytes(), (name, chroma, cols, rows, c)
    dec, idx, _, _, _ = DV.case(name, True, 61, 34)
    sy, scb, scr = dec.stats(idx)
    for got, want in zip(R.pick_plane(sy, None, bl, ll, 0) + R.pick_plane(scb, scr, bc, lc, 0), S.pick_plane(sy, None, bl, ll) + S.pick_plane(scb, scr, bc, lc)):
        assert (got is None and want is None) or got.tobytes() == want.tobytes(), name


# ---- conditions on the vectors, asserted on the reference's own output: caps, not measurements ------------------------------------

def scaled_components(name):
    """(statistics of the distinct records, depth, scale, lambda) of every component of a configuration that has a scale above 0"""
    bl, bc, kl, kc, ll, lc, _ = V.SCALE_CONFIGS[name]
    pal = V.decider(name, True).palette
    out = []
    for c, (bd, k, lam) in enumerate(((bl, kl, ll), (bc, kc, lc), (bc, kc, lc))):
        if k > 0:
            out.append(([rec[c] for rec in pal], bd, k, lam))
    return out


def bins_of(st, bd, k, lam):
    """(n, s, lo, hi, trace) of the 48 bins of one record"""
    M = R.max_offset(bd)
    edge, band = R.bins(st, M, k, lam)
    out = [(int(st["eo_count"][c][e]), int(st["eo_sum"][c][e])) + R.bin_limits(e, M) + (edge[c][e],) for c in range(4) for e in range(4)]
    return out + [(int(st["bo_count"][b]), int(st["bo_sum"][b]), -M, M, band[b]) for b in range(32)]


@pytest.mark.parametrize("name", list(V.SCALE_CONFIGS))
def test_conditions_on_the_vectors(name):
    bl, bc, kl, kc, ll, lc, _ = V.SCALE_CONFIGS[name]
    pk = V.picks(name, 61, 34)
    n_ctb = 61 * 34
    for which, st_a, st_b, bd, lam, k in (("luma", pk["stats"][0], None, bl, ll, kl), ("chroma", pk["stats"][1], pk["stats"][2], bc, lc, kc)):
        if k == 0:
            continue
        pa, pb, _ = pk[which]
        share = np.bincount(pa["type"].ravel(), minlength=3) / n_ctb
        flat = R.pick_plane(st_a, st_b, bd, lam, 0)
        differs = (pa != flat[0]) if pb is None else ((pa != flat[0]) | (pb != flat[1]))
        reach = max(int(np.abs(p["offset"].astype(int)).max()) for p in (pa, pb) if p is not None)
        print(name, which, "types", share.round(3).tolist(), "differ from k = 0", float(differs.mean()), "largest |o|", reach)
        assert share.min() >= 0.10, (name, which, share)
        assert differs.mean() >= 0.25, (name, which)
        assert reach == 31 << k, (name, which, reach)
        for p in (pa, pb):
            assert p is None or (p["offset"].astype(int) % (1 << k) == 0).all()
    ties = other = other_negative = walked = 0
    for records, bd, k, lam in scaled_components(name):
        for st in records:
            for n, s, lo, hi, t in bins_of(st, bd, k, lam):
                if n == 0:
                    continue
                nk = n << k
                if 2 * abs(s) % nk == 0 and (2 * abs(s) // nk) % 2 == 1 and lo <= t["q0"] <= hi:
                    ties += 1                                                  # half away from zero or not: another start
                naive = (R.sign(s) * ((2 * abs(s) + n) // (2 * n))) >> k       # round(s / n) >> k
                if min(max(naive, lo), hi) != t["start"]:
                    other += 1
                    other_negative += s < 0
                walked += t["q"] != t["start"]
    print(name, "ties", ties, "round-then-shift differs", other, "of them s < 0", other_negative, "walked", walked)
    assert ties >= 10 and other >= 10 and other_negative >= 1 and walked >= 10, (name, ties, other, other_negative, walked)


def test_a_scale_takes_away_what_31_cannot():
    """12-bit bins with a mean error of about +-100: the summed predicted delta_d at k = 2 is below that at k = 0"""
    st = np.array(V.biased(np.random.default_rng(12)), S.STATS_DTYPE).reshape(4, 6)
    dd = {k: int(R.pick_plane(st, None, 12, 4096, k)[2].sum()) for k in (0, 1, 2)}
    print(dd)
    assert dd[2] < dd[1] < dd[0] < 0


@pytest.mark.parametrize("name", list(V.tie_vectors()))
def test_tie_vectors_in_the_reference(name):
    st_a, st_b, bd, k, lam, want = V.tie_vectors()[name]
    out, _, _ = R.pick_ctb(st_a, st_b, bd, lam, k)
    assert [(o[0], o[1]) for o in out] == want, (name, out)
    if name == "joint_band_equals_edge":           # the tie is one: the band form costs what the edge class costs
        M = R.max_offset(bd)
        edge, band = R.bins(st_a, M, k, lam)
        assert sum(b["cost"] for b in edge[2]) == min(sum(band[(p + j) & 31]["cost"] for j in range(4)) for p in range(32)) < 0


# ---- csrc/sao_pick_os.h on the CPU ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=["plain", "sanitized"])
def sim(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("sao_scale_sim_" + request.param)
    exe = str(d / "sao_scale_sim")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas"] + flags + ["-I", CSRC, "-o", exe, SIM_SRC])
    return exe, str(d)


def run_sim(sim, st, chroma, bl, bc, kl, kc, ll, lc, sl=None, tl=None, mode=0):
    """st: the statistics arrays, (rows, cols) each -- mode 0: [Y] or [Y, Cb, Cr]; mode 1: [a] or [a, b].  Returns (params per
    component, records) or (params per component, delta_d)"""
    exe, d = sim
    rows, cols = st[0].shape
    n = rows * cols
    blob = np.array([cols, rows, int(chroma), bl, bc, ll, lc, int(sl is not None), int(tl is not None), kl, kc, mode], "<i4").tobytes()
    blob += b"".join(np.ascontiguousarray(s).tobytes() for s in st)
    blob += b"".join(np.ascontiguousarray(a, "<u2").tobytes() for a in (sl, tl) if a is not None)
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    open(fin, "wb").write(blob)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw = open(fout, "rb").read()
    k = len(st)
    assert len(raw) == n * (6 * k + (32 if mode == 0 else 8))
    params = [np.frombuffer(raw[c * n * 6: (c + 1) * n * 6], ro.SAO_CTB_DTYPE).reshape(rows, cols) for c in range(k)]
    return params, np.frombuffer(raw[k * n * 6:], D.DECISION_DTYPE if mode == 0 else "<i8").reshape(rows, cols)


def sim_case(sim, name, dec, idx, sl, tl):
    bl, bc, kl, kc, ll, lc, _ = V.SCALE_CONFIGS[name]
    st = dec.stats(idx)
    return run_sim(sim, st if dec.chroma else st[:1], dec.chroma, bl, bc, kl, kc, ll, lc, sl, tl)


def same(got, res, tag):
    params, dec = got
    for c, p in enumerate(params):
        assert p.tobytes() == res["params"][c].tobytes(), (tag, "params", c, np.argwhere(p != res["params"][c])[:4].tolist())
    assert dec.tobytes() == res["decision"].tobytes(), (tag, [f for f in D.DECISION_DTYPE.names if not np.array_equal(dec[f], res["decision"][f])],
                                                        np.argwhere(dec["merge"] != res["decision"]["merge"])[:4].tolist())


@pytest.mark.parametrize("chroma", [False, True])
@pytest.mark.parametrize("name", list(V.SCALE_CONFIGS))
def test_procedure_reproduces_the_reference(sim, name, chroma):
    for cols, rows in D.GRIDS:
        dec, idx, sl, tl, res = V.case(name, chroma, cols, rows)
        same(sim_case(sim, name, dec, idx, sl, tl), res, (name, chroma, cols, rows))


@pytest.mark.parametrize("chroma", [False, True])
@pytest.mark.parametrize("name", list(DV.CONFIGS))
def test_procedure_at_scale_0_reproduces_the_existing_reference(sim, name, chroma):
    bl, bc, ll, lc, _ = DV.CONFIGS[name]
    for cols, rows in D.GRIDS:
        dec, idx, sl, tl, res = DV.case(name, chroma, cols, rows)
        st = dec.stats(idx)
        same(run_sim(sim, st if chroma else st[:1], chroma, bl, bc, 0, 0, ll, lc), res, (name, chroma, cols, rows))


@pytest.mark.parametrize("chroma", [False, True])
@pytest.mark.parametrize("kind", DV.LAYOUTS)
def test_procedure_under_slices_and_tiles(sim, kind, chroma):
    for name in ("12b_12b_k2_k2", "16b_12b_k2_lambdas_2p24_int32_ends"):
        for cols, rows in D.GRIDS:
            dec, idx, sl, tl, res = V.case(name, chroma, cols, rows, kind)
            same(sim_case(sim, name, dec, idx, sl, tl), res, (name, chroma, cols, rows, kind))
            if kind == "ctb_slices":
                assert not res["decision"]["merge"].any()


@pytest.mark.parametrize("name", list(V.SCALE_CONFIGS))
def test_pick_procedure_reproduces_the_reference(sim, name):
    bl, bc, kl, kc, ll, lc, _ = V.SCALE_CONFIGS[name]
    for cols, rows in ((5, 7), (61, 34)):
        pk = V.picks(name, cols, rows)
        params, dd = run_sim(sim, pk["stats"][:1], False, bl, bl, kl, kl, ll, ll, mode=1)
        assert params[0].tobytes() == pk["luma"][0].tobytes() and np.array_equal(dd, pk["luma"][2]), (name, cols, rows)
        params, dd = run_sim(sim, pk["stats"][1:], True, bc, bc, kc, kc, lc, lc, mode=1)
        assert params[0].tobytes() == pk["chroma"][0].tobytes() and params[1].tobytes() == pk["chroma"][1].tobytes(), (name, cols, rows)
        assert np.array_equal(dd, pk["chroma"][2]), (name, cols, rows)


def test_pick_procedure_on_the_tie_vectors(sim):
    for name, (st_a, st_b, bd, k, lam, want) in V.tie_vectors().items():
        st = [np.array(s, S.STATS_DTYPE).reshape(1, 1) for s in ((st_a,) if st_b is None else (st_a, st_b))]
        params, dd = run_sim(sim, st, st_b is not None, bd, bd, k, k, lam, lam, mode=1)
        out, ref_dd, _ = R.pick_ctb(st_a, st_b, bd, lam, k)
        for p, o, w in zip(params, out, want):
            assert (int(p[0, 0]["type"]), int(p[0, 0]["cls"])) == w and p[0, 0]["offset"].tolist() == list(o[2]), (name, p, o)
        assert int(dd[0, 0]) == ref_dd, name
