"""SAO statistics of a semi-planar chroma plane without a GPU: the entry exists everywhere it must and refuses bad operands with the
documented codes in the documented order; the vectors of tests/sao_stats_sp_ref.py satisfy their census; and csrc/sao_stats_sp.h with
csrc/sao_stats.h, compiled into a stand-alone program (plain and under the address and undefined-behaviour sanitizers), reproduces the
reference's integers for both components, through the wide loads and sample by sample, on every shape the GPU tests use."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import sao_stats_ref as S
import sao_stats_sp_ref as P

CSRC = os.path.join(ROOT, "gpu_video_codec_amd", "csrc")
SIM_SRC = os.path.join(ROOT, "tests", "sao_stats_sp_sim", "sao_stats_sp_sim.cpp")
SIM_DEPTHS = ("8b", "8b_in_16", "10b", "16b")


@pytest.fixture(scope="module")
def L():
    from gpu_video_codec_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


@pytest.fixture(scope="module", autouse=True)
def entry(L):
    """every test of this file is about hevcdbk_sao_stats_device_sp -- its codes, its vectors, its lanes: without the entry none passes"""
    from gpu_video_codec_amd import _lib
    assert "hevcdbk_sao_stats_device_sp" in _lib.EXPORTS and hasattr(L, "hevcdbk_sao_stats_device_sp")


# ---- the entry and its codes --------------------------------------------------------------------------------------------------

def test_entry_is_exported_declared_and_bound(L):
    from gpu_video_codec_amd import _lib, deblock
    import inspect
    hdr = open(os.path.join(ROOT, "include", "hevc_deblock.h")).read()
    sym = "hevcdbk_sao_stats_device_sp"
    assert re.search(r"\b%s\s*\(" % sym, hdr)
    assert sym in _lib.EXPORTS and hasattr(L, sym)
    assert getattr(L, sym).argtypes is not None and len(getattr(L, sym).argtypes) == 15
    prm = inspect.signature(deblock.Context.sao_stats_device).parameters
    assert "semi_planar" in prm and "out_cr_ptr" in prm
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert re.search(r"\bT %s\b" % sym, out)


def _pairs(w=64, h=64, depth=8, sb=1, pitch=None, n=1, chroma=1):
    from gpu_video_codec_amd import _lib
    p = _lib.DevicePlanes()
    p.src, p.dst = 0x10000, 0
    p.pitch = 2 * w * sb if pitch is None else pitch
    p.frame_stride = p.pitch * h
    p.n_frames, p.plane_w, p.plane_h, p.bit_depth, p.sample_bytes, p.is_chroma = n, w, h, depth, sb, chroma
    return p


ORG, CB, CR, KEEP, NOX = 0x200000, 0x300000, 0x400000, 0x500000, 0x600000


@pytest.fixture(scope="module")
def call(L):
    """the entry on a context that no device stands behind (a zeroed block of memory: never looked into before every operand passed)"""
    ctx = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)

    def stats(p, org=ORG, org_pitch=None, org_frame_stride=None, lg=4, keep=None, keep_stride=0, borders=None, cb=CB, cr=CR, stride=4, frame_stride=0,
              ctx=ctx):
        return L.hevcdbk_sao_stats_device_sp(ctx, None if p is None else C.byref(p), org, (p.pitch if p is not None else 128) if org_pitch is None else org_pitch,
                                             (p.frame_stride if p is not None else 0) if org_frame_stride is None else org_frame_stride, lg, keep,
                                             keep_stride, 0, None if borders is None else C.byref(borders), cb, cr, stride, frame_stride, None)
    return stats


def test_documented_codes_without_a_device(call):
    from gpu_video_codec_amd import _lib
    ARG, DIM, UNS = _lib.ERR_ARG, _lib.ERR_DIMENSIONS, _lib.ERR_UNSUPPORTED
    assert call(_pairs(), ctx=None) == ARG and call(None) == ARG
    assert call(_pairs(), org=None) == ARG
    assert call(_pairs(), cb=None) == ARG and call(_pairs(), cr=None) == ARG
    p = _pairs()
    p.src = 0
    assert call(p) == ARG
    for depth, sb in ((7, 1), (17, 2), (10, 1), (8, 3), (8, 0)):
        assert call(_pairs(depth=depth, sb=sb)) == ARG, (depth, sb)
    assert call(_pairs(chroma=0)) == ARG
    for w, h in ((62, 64), (64, 66), (4, 64), (64, 0), (64, 4)):      # not multiples of 4, or below 8
        assert call(_pairs(w, h), stride=8) == DIM, (w, h)
    for lg in (0, 2, 6, 7):                                            # the range of hevcdbk_sao_filter_device_sp
        assert call(_pairs(), lg=lg, stride=8) == ARG, lg
    assert call(_pairs(pitch=127)) == ARG and call(_pairs(pitch=64)) == ARG       # a plane's pitch is not a pair plane's
    assert call(_pairs(), org_pitch=127) == ARG
    assert call(_pairs(64, 64, 10, 2, pitch=254)) == ARG
    assert call(_pairs(n=65536), frame_stride=16) == ARG
    assert call(_pairs(), keep=KEEP, keep_stride=7) == ARG
    assert call(_pairs(), borders=_lib.SaoBorders(None, 4, 0)) == ARG
    assert call(_pairs(), borders=_lib.SaoBorders(NOX, 3, 0)) == ARG
    assert call(_pairs(), stride=3) == ARG                           # four CTB columns
    assert call(_pairs(72, 40), stride=4) == ARG                     # five, by ceiling
    assert call(_pairs(), cb=CB + 2) == ARG and call(_pairs(), cr=CR + 1) == ARG
    assert call(_pairs(n=2), frame_stride=15) == ARG                 # the second frame's grid would overlap the first
    # the two outputs: the same array, Cr inside Cb's extent from either side, and -- with three frames -- inside the gap of a frame stride
    assert call(_pairs(), cr=CB) == ARG
    assert call(_pairs(), cr=CB + 15 * 384) == ARG and call(_pairs(), cb=CR + 15 * 384) == ARG
    assert call(_pairs(n=3), frame_stride=100, cr=CB + 216 * 384 - 4) == ARG
    assert call(_pairs(64, 64, 10, 2, pitch=257)) == UNS             # a sample at an odd address
    assert call(_pairs(64, 64, 10, 2), org=ORG + 1) == UNS
    assert call(_pairs(64, 64, 10, 2), org_frame_stride=64 * 256 + 1) == UNS
    for code in (ARG, DIM, UNS):
        assert _lib.lib().hevcdbk_strerror(code)


def test_codes_come_in_the_documented_order(call):
    """two faults in one call: the earlier check speaks.  NULL -> depth / is_chroma -> dimensions -> ctb_log2 -> pitch -> keep -> borders ->
    stride -> output alignment -> frame stride -> overlap -> misaligned sample"""
    from gpu_video_codec_amd import _lib
    ARG, DIM, UNS = _lib.ERR_ARG, _lib.ERR_DIMENSIONS, _lib.ERR_UNSUPPORTED
    assert call(_pairs(62, 64, depth=7)) == ARG                       # depth before dimensions
    assert call(_pairs(62, 64, chroma=0)) == ARG                      # is_chroma before dimensions
    assert call(_pairs(62, 64), lg=7) == DIM                          # dimensions before ctb_log2
    assert call(_pairs(62, 64), cr=CB) == DIM                         # ... and before the overlap
    assert call(_pairs(62, 64, 10, 2, pitch=249)) == DIM              # ... and before the misaligned sample
    assert call(_pairs(64, 64, 10, 2, pitch=257), lg=6) == ARG        # ctb_log2 before the misaligned sample
    assert call(_pairs(64, 64, 10, 2, pitch=257), stride=3) == ARG    # stride before the misaligned sample
    assert call(_pairs(64, 64, 10, 2, pitch=257), cr=CB) == ARG       # overlap before the misaligned sample
    assert call(_pairs(64, 64, 10, 2, pitch=255)) == ARG              # a pitch too small AND odd: too small


def test_valid_operands_without_a_device(call):
    """valid operands, shared and per-frame, with and without the small operands: past every check the context is bound -- a context
    that no device stands behind answers HEVCDBK_ERR_HIP, never a CPU path.  As tests/test_abi_cpu.py: only where there is no device"""
    from gpu_video_codec_amd import _lib, deblock
    if deblock.device_count() > 0:
        pytest.skip("a GPU is present")
    HIP = _lib.ERR_HIP
    assert call(_pairs()) == HIP
    assert call(_pairs(72, 40, 10, 2, n=3), lg=3, stride=9, frame_stride=45, org_frame_stride=0, keep=KEEP, keep_stride=9,
                borders=_lib.SaoBorders(NOX, 9, 0)) == HIP
    assert call(_pairs(8, 8), lg=5, stride=1) == HIP
    assert call(_pairs(64, 64, 10, 2, pitch=258)) == HIP               # an odd number of pairs per row: sample by sample, not refused
    assert call(_pairs(n=3), frame_stride=100, cr=CB + 216 * 384) == HIP   # Cr's array right behind Cb's extent


def test_python_layer_raises(L):
    from gpu_video_codec_amd import deblock
    c = deblock.Context.__new__(deblock.Context)
    c.handle = None
    p = _pairs()
    with pytest.raises(ValueError, match="4:2:0"):
        c.sao_stats_device(p, ORG, 4, chroma_format="422", out_ptr=CB, out_stride=4, semi_planar=True, out_cr_ptr=CR)
    with pytest.raises(ValueError, match="4:2:0"):
        c.sao_stats_device(p, ORG, 4, chroma_format="444", out_ptr=CB, out_stride=4, semi_planar=True, out_cr_ptr=CR)
    with pytest.raises(ValueError, match="out_cr_ptr"):
        c.sao_stats_device(p, ORG, 4, out_ptr=CB, out_stride=4, semi_planar=True)
    with pytest.raises(ValueError, match="square"):
        c.sao_stats_device(p, ORG, 4, ctb_log2_h=5, out_ptr=CB, out_stride=4, semi_planar=True, out_cr_ptr=CR)
    with pytest.raises(ValueError, match="semi_planar"):
        c.sao_stats_device(p, ORG, 4, out_ptr=CB, out_stride=4, out_cr_ptr=CR)


# ---- the vectors ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("vec", P.VECTORS, ids=lambda v: "%dx%d_%s_%s_%d" % v)
def test_census(vec):
    """conditions on the vectors, from the reference alone: in every CTB of every frame, at every CTB size, Cb's entry differs from
    Cr's, every edge class has a non-empty category in both components, and at least two bands are hit per component"""
    w, h, depth, kind, frames = vec
    rec, org = P.content(w, h, depth, kind, frames)
    assert rec.shape == (frames, h, w, 2) and rec.dtype.itemsize == P.DEPTHS[depth][1]
    for f in range(frames):
        for lg in P.CTBS:
            assert not P.census_fails(rec[f], org[f], P.DEPTHS[depth][0], lg), (vec, f, lg)
    if kind == "full" and w * h >= 72 * 40:                           # the range is walked to both ends
        max_v = (1 << P.DEPTHS[depth][0]) - 1
        for c in (0, 1):
            assert rec[..., c].min() == 0 and rec[..., c].max() == max_v


def test_the_small_operands_bite():
    """the keep map and the border bytes change the statistics of both components"""
    w, h = P.PLANES[0]
    for lg in P.CTBS:
        free, kept, nox = (P.reference(w, h, "10b", "planes", lg, k, n)[0] for (k, n) in ((False, False), (True, False), (False, True)))
        for c in (0, 1):
            assert (kept[c]["bo_count"] != free[c]["bo_count"]).any()
            assert (nox[c]["eo_count"] != free[c]["eo_count"]).any() and np.array_equal(nox[c]["bo_count"], free[c]["bo_count"])


# ---- csrc/sao_stats_sp.h on the CPU ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=["plain", "sanitized"])
def sim(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("sao_stats_sp_sim_" + request.param)
    exe = str(d / "sao_stats_sp_sim")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas"] + flags + ["-I", CSRC, "-o", exe, SIM_SRC])
    return exe, str(d)


def sim_stats(sim, rec, org, bd, lg, *, keeps=None, noxs=None, wide, pad=0):
    """rec (n, h, w, 2); org the same or (1, h, w, 2) = shared; keeps, noxs per frame or None.  pad: samples a row has beyond its 2 w.
    Returns (n, 2, rows, cols)"""
    exe, d = sim
    n, h, w, _ = rec.shape
    sb = rec.itemsize
    pitch = 2 * w + pad

    def pitched(a):
        out = np.full((a.shape[0], h, pitch), 0x5A, a.dtype)
        out[:, :, : 2 * w] = a.reshape(a.shape[0], h, 2 * w)
        return out.tobytes()

    blob = np.array([w, h, sb, bd, lg, keeps is not None, noxs is not None, pitch, int(wide), n, int(org.shape[0] == 1 and n > 1)], "<i4").tobytes()
    blob += pitched(rec) + pitched(org) + (b"" if keeps is None else np.ascontiguousarray(keeps).tobytes()) + \
        (b"" if noxs is None else np.ascontiguousarray(noxs).tobytes())
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    open(fin, "wb").write(blob)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return np.fromfile(fout, S.STATS_DTYPE).reshape((n, 2) + S.grid(w, h, lg, lg))


def same(got, want, tag):
    for c, name in enumerate(("Cb", "Cr")):
        assert got[c].tobytes() == want[c].tobytes(), (tag, name, [f for f in S.STATS_DTYPE.names if not np.array_equal(got[c][f], want[c][f])])


@pytest.mark.parametrize("lg", P.CTBS)
@pytest.mark.parametrize("depth", SIM_DEPTHS)
def test_lanes_reproduce_the_reference(sim, depth, lg):
    """every plane, both kinds of content, with and without a keep map and random border bytes; the wide loads on rows of 2 w samples
    (a multiple of 8) and on a padded aligned pitch, sample by sample on the same rows and on a pitch of 2 w + 10"""
    bd = P.DEPTHS[depth][0]
    for (w, h) in P.PLANES:
        for kind in P.KINDS:
            rec, org = P.content(w, h, depth, kind)
            for small in (False, True):
                k, b = (P.keep_map(w, h), P.border_bytes(w, h, lg)) if small else (None, None)
                want = P.reference(w, h, depth, kind, lg, small, small)[0]
                for wide, pad in ((True, 0), (False, 0), (False, 10)) + (((True, 8),) if small else ()):
                    same(sim_stats(sim, rec, org, bd, lg, keeps=k, noxs=b, wide=wide, pad=pad)[0], want, (w, h, depth, kind, lg, small, wide, pad))


@pytest.mark.parametrize("lg", P.CTBS)
def test_every_block_kept_writes_zeros(sim, lg):
    """every plane at every depth: nothing is counted, and every int32 of both grids is written, as zero"""
    for (w, h) in P.PLANES:
        for depth in SIM_DEPTHS:
            rec, org = P.content(w, h, depth, "full")
            for wide in (True, False):
                got = sim_stats(sim, rec, org, P.DEPTHS[depth][0], lg, keeps=np.ones((1, -(-h // 8), -(-w // 8)), np.uint8), noxs=P.border_bytes(w, h, lg),
                                wide=wide)
                assert got.shape[2:] == S.grid(w, h, lg, lg) and not got.tobytes().strip(b"\0"), (w, h, depth, wide)


@pytest.mark.parametrize("shared", [False, True])
def test_frames(sim, shared):
    """three frames of 72x40 with per-frame small operands; org per frame or one for all"""
    w, h, lg = 72, 40, 4
    rec, org = P.content(w, h, "10b", "planes", 3)
    keeps, noxs = P.keep_map(w, h, 3), P.border_bytes(w, h, lg, 3)
    o = org[1:2] if shared else org
    for wide in (True, False):
        got = sim_stats(sim, rec, o, 10, lg, keeps=keeps, noxs=noxs, wide=wide)
        for f in range(3):
            same(got[f], P.stats_pairs(rec[f], o[0 if shared else f], lg, 10, keep=keeps[f], nox=noxs[f]), (shared, wide, f))
        assert got[0].tobytes() != got[1].tobytes() and got[1].tobytes() != got[2].tobytes()
