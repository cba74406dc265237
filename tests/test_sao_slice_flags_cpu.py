"""slice_sao_luma_flag / slice_sao_chroma_flag in SAO estimation without a GPU: hevcdbk_sao_decide_device_sf,
hevcdbk_sao_slice_flags_device and hevcdbk_sao_slice_flags_workspace exist everywhere they must and refuse bad operands with the
documented codes in the documented order; the plain-int statement of the rule (tests/sao_slice_ref.py) agrees with itself and with
sao_scale_ref.Decider, and its vectors meet the conditions they are built for; and csrc/sao_slice.h, compiled into a stand-alone
program (plain and under the address and undefined-behaviour sanitizers) that runs the NEW step for all 64 lanes of a wave and the
walk diagonal by diagonal with the limb sums and the carry step, reproduces the reference byte for byte."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import rext_oracle as ro
import sao_decide_ref as D
import sao_scale_ref as SR
import sao_slice_ref as R
import sao_slice_vectors as V

CSRC = os.path.join(ROOT, "gpu_video_codec_amd", "csrc")
SIM_SRC = os.path.join(ROOT, "tests", "sao_slice_sim", "sao_slice_sim.cpp")
SF, CHOOSE, SIZE = "hevcdbk_sao_decide_device_sf", "hevcdbk_sao_slice_flags_device", "hevcdbk_sao_slice_flags_workspace"


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
    n_os = len(L.hevcdbk_sao_decide_device_os.argtypes)
    for sym, extra in ((SF, 3), (CHOOSE, 7)):
        assert re.search(r"\b%s\s*\(" % sym, hdr)
        assert sym in _lib.EXPORTS and hasattr(L, sym)
        assert len(getattr(L, sym).argtypes) == n_os + extra
    assert re.search(r"size_t\s+%s\s*\(" % SIZE, hdr) and SIZE in _lib.EXPORTS and L.hevcdbk_sao_slice_flags_workspace.restype is C.c_size_t
    assert re.search(r"const uint8_t \*slice_flags, unsigned n_slices,\s+size_t slice_flags_frame_stride, void \*hip_stream", hdr)
    assert "the caller's to set" not in hdr
    assert C.sizeof(_lib.SaoSliceRecord) == 72 == np.dtype(_lib.SAO_SLICE_RECORD_DTYPE).itemsize == R.SLICE_RECORD_DTYPE.itemsize
    assert np.dtype(_lib.SAO_SLICE_RECORD_DTYPE) == R.SLICE_RECORD_DTYPE
    sig = inspect.signature(deblock.Context.sao_decide_device).parameters
    assert sig["slice_flags_ptr"].default is None and sig["n_slices"].default is None and sig["slice_flags_frame_stride"].default == 0
    assert hasattr(deblock.Context, "sao_slice_flags_device") and hasattr(deblock.Context, "sao_slice_flags_workspace")


SY, SCB, SCR, PY, PCB, PCR, DEC, IDX, FL, REC, WS = (0x100000 * k for k in range(1, 12))     # 4 x 4 grids: 6 KiB of statistics at the most


def test_given_flags_codes_and_their_order_without_a_device(L):
    """a context that no device stands behind (a zeroed block of memory: never looked into)"""
    from gpu_video_codec_amd import _lib
    ctx = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    ARG, DIM, UNS = _lib.ERR_ARG, _lib.ERR_DIMENSIONS, _lib.ERR_UNSUPPORTED

    def call(ctx=ctx, sy=SY, scb=SCB, scr=SCR, stride=4, sfs=0, cx=4, cy=4, n=1, bl=12, bc=12, kl=2, kc=2, ll=1024, lc=1024, sl=None, tl=None,
             istride=0, py=PY, pcb=PCB, pcr=PCR, pstride=4, pfs=0, dec=DEC, dstride=4, dfs=0, fl=FL, ns=4, ffs=0):
        return L.hevcdbk_sao_decide_device_sf(ctx, sy, scb, scr, stride, sfs, cx, cy, n, bl, bc, kl, kc, ll, lc, sl, tl, istride, 0, py, pcb, pcr,
                                              pstride, pfs, dec, dstride, dfs, fl, ns, ffs, None)

    # the refusals of hevcdbk_sao_decide_device_os, as tests/test_sao_scale_cpu.py lists them
    assert call(ctx=None) == ARG and call(sy=None) == ARG and call(py=None) == ARG and call(dec=None) == ARG
    assert call(scb=None) == ARG and call(scr=None) == ARG and call(pcb=None) == ARG and call(pcr=None) == ARG
    for d in (7, 17):
        assert call(bl=d, kl=0) == ARG and call(bc=d, kc=0) == ARG
    assert call(ll=(1 << 24) + 1) == ARG and call(lc=(1 << 24) + 1) == ARG and call(kl=3) == ARG and call(bc=11, kc=2) == ARG
    assert call(cx=0) == DIM and call(cy=0) == DIM and call(cx=65536) == DIM and call(cy=65536) == DIM
    assert call(stride=3) == ARG and call(pstride=3) == ARG and call(dstride=3) == ARG and call(sl=IDX, istride=3) == ARG
    assert call(n=2, sfs=16, pfs=15, dfs=16) == ARG and call(n=2, sfs=16, pfs=16, dfs=15) == ARG and call(n=65536, pfs=16, dfs=16) == ARG
    assert call(sy=SY + 2) == ARG and call(dec=DEC + 4) == ARG and call(sl=IDX + 1, istride=4) == ARG
    for kw in (dict(pcb=PY), dict(pcr=PCB + 6 * 15), dict(dec=PY + 8), dict(pcr=SCB), dict(dec=SCR)):
        assert call(**kw) == ARG, kw
    assert call(bl=16, kl=3) == UNS and call(bc=16, kc=3) == UNS
    # the additions: n_slices with the strides, the frame stride of the flags with the frame strides, the flags against the outputs
    assert call(ns=0) == ARG and call(ns=65537) == ARG
    assert call(n=2, sfs=16, pfs=16, dfs=16, ffs=3) == ARG
    for kw in (dict(fl=PY + 5), dict(fl=DEC + 32 * 15 + 31), dict(fl=PCR - 3), dict(fl=PCB - 4, ns=5)):
        assert call(**kw) == ARG, kw
    assert call(fl=PY + 6 * 16, bl=16, kl=3) == UNS and call(fl=PY - 4, bl=16, kl=3) == UNS      # beside an output, not in it
    # the order: DIMENSIONS before the additions, UNSUPPORTED after them
    assert call(ns=0, cx=0) == DIM and call(ns=0, kl=3) == ARG and call(ns=0, bl=16, kl=3) == ARG and call(ns=65537, bl=16, kl=3, cx=0) == DIM
    assert call(n=2, sfs=16, pfs=16, dfs=16, ffs=3, bl=16, kl=3) == ARG and call(fl=PY + 5, bl=16, kl=3) == ARG
    assert call(n=2, sfs=16, pfs=16, dfs=16, ffs=0, bl=16, kl=3) == UNS and call(n=2, sfs=16, pfs=16, dfs=16, ffs=4, bl=16, kl=3) == UNS
    # slice_flags == NULL is the _os entry itself: n_slices and the frame stride are not looked at
    assert call(fl=None, ns=0, ffs=1, n=2, sfs=16, pfs=16, dfs=16, bl=16, kl=3) == UNS and call(fl=None, ns=99999, cx=0) == DIM
    # without chroma the chroma operands are not looked at
    luma = dict(scb=None, scr=None, pcb=None, pcr=None)
    assert call(bl=16, kl=3, kc=99, bc=0, **luma) == UNS and call(ns=0, bl=16, kl=3, **luma) == ARG


def test_choosing_codes_and_their_order_without_a_device(L):
    from gpu_video_codec_amd import _lib
    ctx = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    ARG, DIM, UNS = _lib.ERR_ARG, _lib.ERR_DIMENSIONS, _lib.ERR_UNSUPPORTED
    need = lambda cx=4, cy=4, n=1, ns=4: L.hevcdbk_sao_slice_flags_workspace(cx, cy, n, ns)

    def call(ctx=ctx, sy=SY, scb=SCB, scr=SCR, stride=4, sfs=0, cx=4, cy=4, n=1, bl=12, bc=12, kl=2, kc=2, ll=1024, lc=1024, sl=None, tl=None,
             istride=0, py=PY, pcb=PCB, pcr=PCR, pstride=4, pfs=0, dec=DEC, dstride=4, dfs=0, ns=4, fl=FL, ffs=0, rec=REC, rfs=0, ws=WS, wb=None):
        wb = need(cx, cy, n, ns) if wb is None else wb
        return L.hevcdbk_sao_slice_flags_device(ctx, sy, scb, scr, stride, sfs, cx, cy, n, bl, bc, kl, kc, ll, lc, sl, tl, istride, 0, py, pcb, pcr,
                                                pstride, pfs, dec, dstride, dfs, ns, fl, ffs, rec, rfs, ws, wb, None)

    two = dict(n=2, sfs=16, pfs=16, dfs=16, ffs=4, rfs=4)
    ok = dict(bl=16, kl=3)                                   # everything else in order: the unsupported scale answers
    assert call(**ok) == UNS and call(**two, **ok) == UNS and call(rec=None, **ok) == UNS
    # those of the entry under given flags
    assert call(ctx=None) == ARG and call(sy=None) == ARG and call(scb=None) == ARG and call(pcr=None) == ARG and call(bl=7, kl=0) == ARG
    assert call(lc=(1 << 24) + 1) == ARG and call(kl=3) == ARG and call(cx=0) == DIM and call(cy=65536) == DIM
    assert call(stride=3) == ARG and call(sl=IDX, istride=3) == ARG and call(ns=0) == ARG and call(ns=65537) == ARG
    assert call(**dict(two, pfs=15)) == ARG and call(**dict(two, n=65536)) == ARG and call(dec=DEC + 4) == ARG and call(pcb=PY) == ARG
    # an output cannot be shared: the flag bytes and the slice records of more than one frame
    assert call(**dict(two, ffs=0), **ok) == ARG and call(**dict(two, ffs=3), **ok) == ARG and call(**dict(two, rfs=3), **ok) == ARG
    assert call(**dict(two, rfs=0), rec=None, **ok) == UNS
    # then the operands of its own
    assert call(fl=None, **ok) == ARG and call(ws=None, **ok) == ARG and call(ws=WS + 8, **ok) == ARG and call(rec=REC + 4, **ok) == ARG
    assert call(wb=need() - 1, **ok) == ARG and call(wb=0, **ok) == ARG and call(wb=need() + 1000, **ok) == UNS
    for kw in (dict(fl=PY + 5), dict(fl=WS + 7), dict(rec=DEC + 8), dict(rec=FL - 64), dict(ws=PCR - 16), dict(ws=SY + 16), dict(fl=SCR + 100),
               dict(rec=WS + need() - 8), dict(ws=REC + 64)):
        assert call(**kw, **ok) == ARG, kw
    # last: more slices than the choosing entry takes -- after the unsupported scale, after every ARG
    assert call(ns=600, **ok) == UNS and call(ns=601) == UNS and call(ns=65536, rec=None) == UNS and call(ns=601, cx=0) == DIM
    assert call(ns=601, fl=None) == ARG and call(ns=601, wb=0) == ARG and call(ns=601, ws=PCR - 16) == ARG and call(ns=601, kl=3) == ARG
    assert call(**dict(two, ffs=600, rfs=601, ns=601)) == ARG and call(**dict(two, ffs=601, rfs=601, ns=601)) == UNS
    luma = dict(scb=None, scr=None, pcb=None, pcr=None)
    assert call(kc=99, bc=0, **luma, **ok) == UNS and call(ns=601, kc=99, **luma) == UNS and call(fl=None, **luma) == ARG


def test_the_size_function(L):
    f = L.hevcdbk_sao_slice_flags_workspace
    assert f(1, 1, 1, 1) > 0 and f(1, 1, 1, 1) % 16 == 0
    for a, b in (((5, 7, 1, 5), (6, 7, 1, 5)), ((5, 7, 1, 5), (5, 8, 1, 5)), ((5, 7, 1, 5), (5, 7, 2, 5)), ((5, 7, 1, 5), (5, 7, 1, 600)),
                 ((240, 135, 64, 8), (240, 135, 64, 135))):
        assert f(*a) <= f(*b), (a, b)
    assert f(5, 7, 2, 5) > f(5, 7, 1, 5) and f(61, 34, 1, 1) >= 61 * 34 * 3 * (32 + 18)
    assert f(65535, 65535, 65535, 600) > f(65535, 65535, 65534, 600) > 1 << 50            # no wrap at the largest operands


# ---- the reference alone ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(V.CONFIGS))
def test_all_flags_3_is_the_decision_without_flags(name):
    bl, bc, kl, kc, ll, lc, _ = V.CONFIGS[name]
    for chroma in (False, True):
        for cols, rows, lay in ((1, 1, "none"), (5, 7, "slices"), (61, 34, "both")):
            dec, idx, sl, tl, n = V.case(name, chroma, cols, rows, lay)
            want = SR.Decider(dec.palette, bd_luma=bl, bd_chroma=bc, lam_luma=ll, lam_chroma=lc, chroma=chroma, k_luma=kl, k_chroma=kc).decide(idx, sl, tl)
            for flags in (3, [3] * n, [0xFF] * n):
                got = dec.decide(idx, sl, tl, flags, n)
                assert got["decision"].tobytes() == want["decision"].tobytes() and (got["j"] == want["j"]).all(), (name, chroma, cols, rows)
                for c in range(3 if chroma else 1):
                    assert got["params"][c].tobytes() == want["params"][c].tobytes()


@pytest.mark.parametrize("chroma", [False, True])
@pytest.mark.parametrize("name", list(V.CONFIGS))
def test_the_choice_agrees_with_uniform_runs(name, chroma):
    """T_c of the record is the sum of J of a run with every slice under c; the final outputs are, slice by slice, those of the run
    under the slice's pair (a candidate never leaves the slice) and, as a whole, the decider under the chosen flags"""
    for cols, rows, lay in ((5, 7, "slices"), (9, 1, "both"), (61, 34, "slices")):
        dec, idx, sl, tl, n = V.case(name, chroma, cols, rows, lay)
        res = V.chosen(name, chroma, cols, rows, lay)
        rec = R.records(res)
        uniform = {c: dec.decide(idx, sl, tl, c, n) for c in (0, 1, 2, 3)}
        for s in range(n):
            mine = sl == s
            assert rec[s]["n_ctbs"] == mine.sum() and rec[s]["flags"] == res["flags"][s] and rec[s]["cost_lo"][0] == 0 == rec[s]["cost_hi"][0]
            for c in (1, 2, 3) if chroma else (1,):
                total = sum(int(j) for j in uniform[c]["j"][mine])
                assert total == res["T"][s][c] == (int(rec[s]["cost_hi"][c]) << 64) + int(rec[s]["cost_lo"][c]), (name, s, c)
            best = min(res["T"][s][: 4 if chroma else 2])
            assert res["T"][s][res["flags"][s]] == best and all(t > best for t in res["T"][s][: res["flags"][s]])
            u = uniform[res["flags"][s]]
            assert res["decision"][mine].tobytes() == u["decision"][mine].tobytes()
            for c in range(3 if chroma else 1):
                assert res["params"][c][mine].tobytes() == u["params"][c][mine].tobytes()
        again = dec.decide(idx, sl, tl, res["flags"], n)
        assert again["decision"].tobytes() == res["decision"].tobytes()
        assert not uniform[0]["decision"].view(np.uint8).any() and not any(p.view(np.uint8).any() for p in uniform[0]["params"] if p is not None)


def test_a_slices_choice_does_not_depend_on_another_slice():
    dec, idx, sl, tl, n = V.case("8b_equal", True, 61, 34, "slices")
    res = V.chosen("8b_equal", True, 61, 34, "slices")
    other = idx.copy()
    other[sl == 3] = (other[sl == 3] + 4 * 7 + 1) % len(dec.palette)       # other records, another variant, in slice 3 alone
    moved = dec.choose(other, sl, tl, n)
    assert moved["T"][3] != res["T"][3]
    for s in range(n):
        if s != 3:
            assert moved["T"][s] == res["T"][s] and moved["flags"][s] == res["flags"][s]
            assert moved["decision"][sl == s].tobytes() == res["decision"][sl == s].tobytes()


# ---- conditions on the vectors, from the reference alone: not measurements ----------------------------------------------------------

@pytest.mark.parametrize("name", V.CENSUS)
def test_every_pair_is_chosen(name):
    for cols, rows in ((5, 7), (61, 34)):
        for lay in ("slices", "both"):
            res = V.chosen(name, True, cols, rows, lay)
            n = np.bincount(res["flags"], minlength=4)
            print(name, cols, rows, lay, "slices per pair", n.tolist())
            assert (n > 0).all(), (name, cols, rows, lay, n)
            luma = np.bincount(V.chosen(name, False, cols, rows, lay)["flags"], minlength=2)
            assert (luma > 0).all() and len(luma) == 2


@pytest.mark.parametrize("name", V.EXTREME)
def test_totals_wrapped_to_64_bits_choose_otherwise(name):
    dec, idx, sl, tl, n = V.case(name, True, 5, 7, "slices")
    res = V.chosen(name, True, 5, 7, "slices")
    wrapped = dec.choose(idx, sl, tl, n, wrap=64)
    differ = sum(a != b for a, b in zip(res["flags"], wrapped["flags"]))
    bits = max(abs(t) for T in res["T"] for t in T).bit_length()
    print(name, res["flags"], wrapped["flags"], "largest total: %d bits" % bits)
    assert differ >= 1 and 64 < bits <= 127


def test_further_conditions_on_the_vectors():
    dec, idx, sl, tl, n = V.case("8b_equal", True, 61, 34, "slices")
    m = [dec.decide(idx, sl, tl, c, n)["decision"]["merge"] for c in (1, 2, 3)]
    assert (m[2] != m[0]).any() and (m[2] != m[1]).any()                    # a CTB merges otherwise under pair 3 than under 1 or 2
    res = V.chosen("8b_lambdas_0", True, 5, 7, "slices")                     # chroma at lambdas of 0: every J is 0, every slice ties to 0
    assert res["flags"] == [0] * len(res["T"]) and all(T == [0, 0, 0, 0] for T in res["T"]) and max(res["n_ctbs"]) > 1
    res = V.chosen("8b_lambdas_0", False, 5, 7, "slices")                    # without chroma J is not cleared: luma still gains
    assert 1 in res["flags"]
    for lay in ("slices", "both"):                                           # an empty slice: the last, and gaps in `both`
        res = V.chosen("8b_equal", True, 5, 7, lay)
        assert res["n_ctbs"][-1] == 0 and res["flags"][-1] == 0
    assert 0 in V.chosen("8b_equal", True, 5, 7, "both")["n_ctbs"][:-1]
    dec, idx, sl, tl, n = V.case("8b_equal", True, 5, 7, "slices", short=True)   # CTBs beyond n_slices
    res = V.chosen("8b_equal", True, 5, 7, "slices", short=True)
    beyond = sl >= n
    assert beyond.any() and not res["decision"][beyond].view(np.uint8).any() and sum(res["n_ctbs"]) == (~beyond).sum()
    assert len(V.case("8b_equal", True, 61, 34, "ctb_slices")[2].ravel()) > V.MAX_SLICES


# ---- csrc/sao_slice.h on the CPU ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=["plain", "sanitized"])
def sim(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("sao_slice_sim_" + request.param)
    exe = str(d / "sao_slice_sim")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas"] + flags + ["-I", CSRC, "-o", exe, SIM_SRC])
    return exe, str(d)


def run_sim(sim, dec, idx, sl, tl, n_slices, name, flags=None):
    """flags: the bytes of the decision under given flags, or None = the choice.  Returns (params per component, records) and, for the
    choice, (flag bytes, slice records)"""
    exe, d = sim
    bl, bc, kl, kc, ll, lc, _ = V.CONFIGS[name]
    rows, cols = idx.shape
    n = rows * cols
    st = dec.stats(idx)
    st = st if dec.chroma else st[:1]
    blob = np.array([cols, rows, int(dec.chroma), bl, bc, ll, lc, int(sl is not None), int(tl is not None), kl, kc, int(flags is None), n_slices],
                    "<i4").tobytes()
    blob += b"".join(np.ascontiguousarray(s).tobytes() for s in st)
    blob += b"".join(np.ascontiguousarray(a, "<u2").tobytes() for a in (sl, tl) if a is not None)
    if flags is not None:
        blob += np.asarray(flags, np.uint8).tobytes()
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    open(fin, "wb").write(blob)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw = open(fout, "rb").read()
    k = len(st)
    assert len(raw) == n * (6 * k + 32) + (0 if flags is not None else n_slices * 73)
    params = [np.frombuffer(raw[c * n * 6: (c + 1) * n * 6], ro.SAO_CTB_DTYPE).reshape(rows, cols) for c in range(k)]
    records = np.frombuffer(raw[k * n * 6: k * n * 6 + n * 32], D.DECISION_DTYPE).reshape(rows, cols)
    if flags is not None:
        return params, records
    tail = raw[k * n * 6 + n * 32:]
    return params, records, np.frombuffer(tail[:n_slices], np.uint8), np.frombuffer(tail[n_slices:], R.SLICE_RECORD_DTYPE)


def same(got, res, tag):
    params, dec = got[:2]
    for c, p in enumerate(params):
        assert p.tobytes() == res["params"][c].tobytes(), (tag, "params", c, np.argwhere(p != res["params"][c])[:4].tolist())
    assert dec.tobytes() == res["decision"].tobytes(), (tag, [f for f in D.DECISION_DTYPE.names if not np.array_equal(dec[f], res["decision"][f])],
                                                        np.argwhere(dec["merge"] != res["decision"]["merge"])[:4].tolist())
    if len(got) == 4:
        assert got[2].tolist() == res["flags"], (tag, got[2].tolist(), res["flags"])
        want = R.records(res)
        assert got[3].tobytes() == want.tobytes(), (tag, [f for f in R.SLICE_RECORD_DTYPE.names if not np.array_equal(got[3][f], want[f])])


def layouts_of(cols, rows, choosing):
    for lay in ("none",) + V.LAYOUTS:
        if not (choosing and lay == "ctb_slices" and cols * rows + 1 > V.MAX_SLICES):
            yield lay


@pytest.mark.parametrize("chroma", [False, True])
@pytest.mark.parametrize("name", list(V.CONFIGS))
def test_procedure_chooses_as_the_reference(sim, name, chroma):
    for cols, rows in D.GRIDS:
        for lay in layouts_of(cols, rows, True):
            dec, idx, sl, tl, n = V.case(name, chroma, cols, rows, lay)
            same(run_sim(sim, dec, idx, sl, tl, n, name), V.chosen(name, chroma, cols, rows, lay), (name, chroma, cols, rows, lay))
    dec, idx, sl, tl, n = V.case(name, chroma, 5, 7, "slices", short=True)
    same(run_sim(sim, dec, idx, sl, tl, n, name), V.chosen(name, chroma, 5, 7, "slices", short=True), (name, chroma, "short"))


@pytest.mark.parametrize("chroma", [False, True])
@pytest.mark.parametrize("name", list(V.CONFIGS))
def test_procedure_under_given_flags_reproduces_the_reference(sim, name, chroma):
    for cols, rows in D.GRIDS:
        for lay in layouts_of(cols, rows, False):
            for short in (False, True) if (cols, rows) == (5, 7) else (False,):
                dec, idx, sl, tl, n = V.case(name, chroma, cols, rows, lay, short)
                flags = V.given_flags(n, cols)
                same(run_sim(sim, dec, idx, sl, tl, n, name, flags), dec.decide(idx, sl, tl, [int(f) for f in flags], n), (name, chroma, cols, rows, lay, short))
    dec, idx, sl, tl, n = V.case(name, chroma, 61, 34, "both")
    same(run_sim(sim, dec, idx, sl, tl, n, name, np.full(n, 3, np.uint8)), dec.decide(idx, sl, tl), (name, chroma, "all 3"))
