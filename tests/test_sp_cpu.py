"""Semi-planar chroma (one plane of interleaved Cb / Cr pairs, the _sp entry) without a GPU: the library has the entry and
answers with the documented codes where it can answer without a device; the kernels' block procedure -- deblock_sp.h's split and
merge around the planar chroma procedures -- gives on the CPU, over whole interleaved planes of the GPU vectors' shapes, the bytes of
tests/sp_ref.py; and every GPU vector exercises what it is there for."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sp_ref as S

NEW = ["hevcdbk_h265_filter_device_sp"]


@pytest.fixture(scope="module")
def L():
    from gpu_video_codec_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


# ---- the library ------------------------------------------------------------------------------------------------------------------

def test_new_symbols_are_exported(L):
    from gpu_video_codec_amd import _lib
    for s in NEW:
        assert s in _lib.EXPORTS and hasattr(L, s), s


def test_python_keyword_exists():
    import inspect
    from gpu_video_codec_amd import deblock
    p = inspect.signature(deblock.Context.filter_device_h265).parameters
    assert "semi_planar" in p and p["semi_planar"].default is False and p["semi_planar"].kind is inspect.Parameter.KEYWORD_ONLY
    p = inspect.signature(deblock.DeviceBatch.__init__).parameters
    assert p["semi_planar"].default is False and p["semi_planar"].kind is inspect.Parameter.KEYWORD_ONLY


def _plane(w, h, chroma=True, depth=8, pitch=None):
    from gpu_video_codec_amd import _lib
    p = _lib.DevicePlanes()
    sb = 1 if depth == 8 else 2
    p.src, p.dst = 0x1000, 0x400000
    p.pitch = 2 * w * sb if pitch is None else pitch
    p.frame_stride, p.n_frames, p.plane_w, p.plane_h = p.pitch * h, 1, w, h
    p.bit_depth, p.sample_bytes, p.is_chroma = depth, sb, int(chroma)
    p.vert_bs = p.hor_bs = 0x1000
    return p


def test_documented_codes_without_a_device(L):
    """a context that no device stands behind (a zeroed block of memory: never looked into): every operand is checked before the
    device is asked for anything"""
    from gpu_video_codec_amd import _lib
    ctx = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    hp = _lib.H265Params(0, 0, -6, 6)
    DIM, ARG, UNS = _lib.ERR_DIMENSIONS, _lib.ERR_ARG, _lib.ERR_UNSUPPORTED

    def filt(p, ctx_=ctx, variant=0, so=None, prm=hp):
        return L.hevcdbk_h265_filter_device_sp(ctx_, C.byref(p), 30, C.byref(prm), variant, so, None)

    # sizes per component: multiples of 4, at least 8
    for (w, h) in [(4, 16), (16, 4), (10, 16), (16, 10), (12, 6), (0, 16), (964, 542)]:
        assert filt(_plane(w, h)) == DIM, (w, h)
    g = _plane(960, 540)
    assert filt(g, ctx_=None) == ARG
    # a luma plane is no pair plane
    assert filt(_plane(960, 544, chroma=False)) == ARG
    # a row holds 2 * plane_w samples
    for depth in (8, 10):
        sb = 1 if depth == 8 else 2
        assert filt(_plane(960, 540, depth=depth, pitch=2 * 960 * sb - 4 * sb)) == ARG
        assert filt(_plane(960, 540, depth=depth, pitch=960 * sb)) == ARG
    # the arguments of the entries they are like
    assert filt(g, variant=77) == ARG and filt(g, variant=_lib.KERNEL_PACKED | 0x300) == ARG
    assert filt(g, prm=_lib.H265Params(0, 0, 13, 0)) == ARG and filt(g, prm=_lib.H265Params(0, 0, 0, -13)) == ARG
    assert filt(g, so=C.byref(_lib.SliceOffsets(None, 120, 0, 4))) == ARG
    assert filt(g, so=C.byref(_lib.SliceOffsets(0x1000, 119, 0, 4))) == ARG   # 1920 luma columns = 120 CTBs of 16
    # alignment: one 4-sample word for every kernel ...
    odd = _plane(960, 540, pitch=2 * 960 + 2)
    assert filt(odd) == UNS
    # ... half a block's row for the packed kernels; deeper than 12 bit, wider than a workgroup: the 32-bit kernel only
    assert filt(_plane(960, 540, pitch=2 * 960 + 4), variant=_lib.KERNEL_PACKED) == UNS
    assert filt(_plane(960, 540, depth=10, pitch=4 * 960 + 8), variant=_lib.KERNEL_PACKED) == UNS
    assert filt(_plane(72, 24, depth=14), variant=_lib.KERNEL_PACKED) == UNS
    assert filt(_plane(8192, 16), variant=_lib.KERNEL_PACKED) == UNS
    assert filt(g, variant=_lib.KERNEL_PACKED | _lib.MAP_LINEAR) == UNS         # the row map only


def test_planar_entries_do_not_change(L):
    """with semi_planar left out nothing moves: the planar _g4 entry still wants c_idx and takes plane_w samples per row"""
    from gpu_video_codec_amd import _lib
    ctx = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    hp = _lib.H265Params(0, 0, 0, 0)
    g = _plane(960, 540, pitch=960)
    assert L.hevcdbk_h265_filter_device_g4(ctx, C.byref(g), 0, 1, 30, C.byref(hp), 0, None, None) == _lib.ERR_ARG
    assert L.hevcdbk_h265_filter_device_sp(ctx, C.byref(g), 30, C.byref(hp), 0, None, None) == _lib.ERR_ARG


# ---- the kernels' block procedure on the CPU -------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    from conftest import ROOT
    out = str(tmp_path_factory.mktemp("sp_sim") / "libsp_sim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", out,
                           os.path.join(ROOT, "tests", "sp_sim", "sp_sim.cpp")])
    lib = C.CDLL(out)
    lib.sp_sim_filter_plane.restype = C.c_int
    lib.sp_sim_split_merge.restype = None
    return lib


@pytest.mark.parametrize("sb", [1, 2])
def test_split_and_merge(sim, sb):
    """a row of pairs -> the register layouts of the planar procedures (8-bit: L | R of four bytes each; 16-bit: W[0..3]) and back"""
    dt = np.uint8 if sb == 1 else np.uint16
    rng = np.random.default_rng(sb)
    for _ in range(8):
        row = rng.integers(0, 256 if sb == 1 else 65536, 16).astype(dt)
        c0, c1, back = np.zeros(8, dt), np.zeros(8, dt), np.zeros(16, dt)
        sim.sp_sim_split_merge(row.ctypes.data_as(C.c_void_p), sb, c0.ctypes.data_as(C.c_void_p), c1.ctypes.data_as(C.c_void_p),
                               back.ctypes.data_as(C.c_void_p))
        assert np.array_equal(c0, row[0::2]) and np.array_equal(c1, row[1::2]) and np.array_equal(back, row)


@pytest.fixture(scope="module")
def dbk_cases():
    """the GPU vectors and their expectations, computed once"""
    out = {}
    for spec in S.DBK:
        c = S.dbk_case(spec)
        out[spec[0]] = (c, {(q, sl): S.dbk_expected(c, 0, q, sl) for q in (False, True) for sl in (False, True)})
    return out


@pytest.mark.parametrize("spec", S.DBK, ids=lambda s: s[0])
def test_kernel_block_procedure_on_pair_planes(sim, dbk_cases, spec):
    """one QP and a map, the call's own offset and per-slice pairs; the 32-bit form and, up to 12 bit, the packed form"""
    c, wants = dbk_cases[spec[0]]
    vb, hb = c["bs"][0]
    m = c["qp_map"]
    pr = np.ascontiguousarray(c["pairs"], np.int8)
    for (q, sl), want in wants.items():
        for form in ((0, 1) if c["depth"] <= 12 else (0,)):
            out = np.ascontiguousarray(c["planes"][0]).copy()
            rc = sim.sp_sim_filter_plane(out.ctypes.data_as(C.c_void_p), c["w"], c["h"], C.c_long(out.strides[0]), out.itemsize, c["depth"],
                                         vb.ctypes.data_as(C.c_void_p), hb.ctypes.data_as(C.c_void_p), c["qp"],
                                         m.ctypes.data_as(C.c_void_p) if q else None, m.shape[1], S.UNIT_LOG2, S.CB_OFF, S.CR_OFF,
                                         0 if sl else S.TC_DIV2, pr.ctypes.data_as(C.c_void_p) if sl else None, pr.shape[1],
                                         S.SL_CTB_LOG2, form)
            assert rc == 0
            assert np.array_equal(out, want), (spec[0], q, sl, form, int((out != want).sum()))


def test_the_packed_form_stops_at_12_bit(sim):
    z = np.zeros((8, 8, 2), np.uint16)
    b = np.zeros(64, np.uint8)
    assert sim.sp_sim_filter_plane(z.ctypes.data_as(C.c_void_p), 8, 8, C.c_long(32), 2, 14, b.ctypes.data_as(C.c_void_p),
                                   b.ctypes.data_as(C.c_void_p), 30, None, 0, 3, 0, 0, 0, None, 0, 4, 1) == 3


# ---- the vectors are not vacuous -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spec", S.DBK, ids=lambda s: s[0])
def test_deblocking_vectors_bite_in_both_components(dbk_cases, spec):
    """both components change; the expectation with the two QP offsets exchanged differs in BOTH; on g4 shapes the new last edge
    moves samples of both; the frames' operands differ"""
    c, wants = dbk_cases[spec[0]]
    for (q, sl), want in wants.items():
        cen = S.dbk_census(c, 0, q, sl, want)
        assert S.dbk_census_ok(c, cen), (spec[0], q, sl, cen)
    cen = S.dbk_census(c, 1, True, True)
    assert S.dbk_census_ok(c, cen), (spec[0], "frame 1", cen)
    assert not np.array_equal(c["bs"][0][0], c["bs"][1][0]) and not np.array_equal(c["bs"][0][1], c["bs"][1][1])
    assert not np.array_equal(c["planes"][0], c["planes"][1])
    assert not np.array_equal(wants[(False, False)], wants[(True, False)]) and not np.array_equal(wants[(False, False)], wants[(False, True)])


def test_exchanging_the_offsets_bites_on_small_planes():
    """QP 37 with offsets -6 / +6, random bS and blocky planes: exchanging the offsets changes both components"""
    for (w, h, depth) in [(12, 12, 8), (16, 16, 8), (24, 20, 10), (72, 24, 8), (520, 12, 8)]:
        c = S.dbk_case(("census%dx%d" % (w, h), w, h, depth), frames=1)
        cen = S.dbk_census(c, 0, False, False)
        assert all(x["swap"] > 0 and x["changed"] > 0 for x in cen), (w, h, cen)
