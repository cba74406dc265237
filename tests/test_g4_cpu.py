"""Planes sized in multiples of 4, not 8 (the _g4 entries), without a GPU: the two statements the GPU expectations rest on agree byte
for byte, every vector exercises what it is there for, and the library has the entries and answers with the documented codes where it
can answer without a device."""
import ctypes as C
import os

import numpy as np
import pytest

import g4_ref as G
import rext_oracle as rx
import slice_offsets_ref as R

NEW = ["hevcdbk_h265_derive_bs_device_g4", "hevcdbk_h265_filter_device_g4", "hevcdbk_sao_filter_device_g4",
       "hevcdbk_h265_deblock_sao_device_g4", "hevcdbk_h265_deblock_sao_device_planes_g4"]


@pytest.fixture(scope="module")
def L():
    from gpu_video_codec_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


# ---- the two statements ------------------------------------------------------------------------------------------------------------

SIX = [(20, 28, 8), (28, 20, 8), (36, 36, 10), (64, 44, 8), (44, 64, 10), (12, 12, 8)]


@pytest.mark.parametrize("w,h,depth", SIX, ids=lambda v: str(v))
def test_rext_oracle_on_the_g4_plane_equals_the_c_oracle_by_pad_and_crop(w, h, depth):
    """random bS with KEEP flags, a QP map or one QP, offsets (+1, -1), c_qp_offset 2, two pad contents"""
    changed_at_new_edge = 0
    for k in range(2):
        rng = np.random.default_rng(w * 1000 + h * 10 + k)
        pl = G.blocky_plane(w, h, depth, rng)
        vb, hb = G.random_bs(w, h, rng)
        qmap = G.random_qp_map(w, h, 1, 3, rng) if k == 0 else None
        for tc in (1, -1):
            kw = dict(qp=37, qp_map=qmap, unit_log2=3, bit_depth=depth, c_qp_offset=2, tc_offset_div2=tc)
            one = G.deblock_direct(pl, vb, hb, 1, **kw)
            for seed in (1, 2):
                two = G.deblock_padcrop(pl, vb, hb, seed=seed, **kw)
                assert np.array_equal(one, two), (w, h, depth, k, tc, seed, int((one != two).sum()))
            changed_at_new_edge += sum(G.new_edge_changes(pl, one))
            assert (one != pl).any()
    assert changed_at_new_edge > 0


def test_per_slice_composition_by_pad_and_crop_equals_the_composition_on_the_g4_plane(monkeypatch):
    """4:2:0: tests/slice_offsets_ref.py composes runs of the C oracle, which takes the padded plane only; the same composition of runs
    of rext_oracle on the g4 plane itself gives the same bytes"""
    for (w, h, depth) in SIX:
        rng = np.random.default_rng(w * 77 + h)
        pl = G.blocky_plane(w, h, depth, rng)
        vb, hb = G.random_bs(w, h, rng)
        qmap = G.random_qp_map(w, h, 1, 3, rng)
        rows, cols = -(-2 * h >> 4), -(-2 * w >> 4)
        sidx = R.slices_raster(rows, cols, 2)
        pairs = R.ctb_pairs(sidx, R.table_for(int(sidx.max()) + 1))
        kw = dict(qp=35, qp_map=qmap, unit_log2=3, bit_depth=depth, c_qp_offset=-1)
        padded = G.deblock_sl(pl, vb, hb, 1, pairs, 4, **kw)

        def rx_run(plane, v, hh, pair, c_idx, cf, k):
            return rx.filter_chroma_plane(plane, v, hh, cf, qp=k["qp"], qp_map=k["qp_map"], unit_log2=k["unit_log2"],
                                          bit_depth=k["bit_depth"], c_qp_offset=k["c_qp_offset"], tc_offset_div2=int(pair[1]))
        with monkeypatch.context() as m:
            m.setattr(R, "_run", rx_run)
            direct = R.expected(pl, vb, hb, pairs, 4, c_idx=1, chroma_format=1, **kw)
        assert np.array_equal(padded, direct), (w, h, depth)
        uniform = G.deblock_direct(pl, vb, hb, 1, tc_offset_div2=0, **kw)
        assert not np.array_equal(padded, uniform) or min(w, h) < 16, (w, h)


def test_padding_is_not_sao():
    """why the entries exist: SAO of the plane padded to a multiple of 8 differs from SAO of the plane in its last row / column"""
    for spec in G.SMALL:
        c = G.sao_case(spec)
        differing = 0
        for pl, p in zip(c["planes"], c["params"]):
            want = G.sao_direct(pl, p, c["lw"], c["lh"], bit_depth=c["depth"])
            pad = G.padded_sao(pl, p, c["lw"], c["lh"], bit_depth=c["depth"])
            d = want != pad
            differing += int(d.sum())
            inner = d[: c["h"] - 1 if c["h"] % 8 else c["h"], : c["w"] - 1 if c["w"] % 8 else c["w"]]
            assert not inner.any(), "padding may only differ in the last row / column of the direction that was padded"
        assert differing > 0, spec[0]


# ---- the vectors are not vacuous -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spec", G.CASES, ids=lambda s: s[0])
def test_deblocking_vectors_exercise_the_new_edge(spec):
    c = G.dbk_case(spec)
    assert G.is_g4(c["w"], c["h"])
    for sl in (False, True):
        want = G.dbk_expected(c, 0, sl)
        cols, rows = G.new_edge_changes(c["planes"][0], want)
        assert cols + rows > 0, (spec[0], sl)
    assert not np.array_equal(G.dbk_expected(c, 0, False), G.dbk_expected(c, 0, True))


@pytest.mark.parametrize("spec", G.CASES, ids=lambda s: s[0])
def test_sao_vectors_hold_what_tells_the_picture_edge_from_padding(spec):
    c = G.sao_case(spec)
    cen = G.sao_census(c["planes"], c["params"], c["lw"], c["lh"], c["depth"])
    assert G.census_ok(cen, c["w"], c["h"]), (spec[0], cen)
    rows, cols = G.ctb_grid(c["w"], c["h"], c["lw"], c["lh"])
    assert c["params"][0].shape == (rows, cols) and c["keep"][0].shape == ((c["h"] + 7) // 8, (c["w"] + 7) // 8)


@pytest.mark.parametrize("spec", G.DEEP, ids=lambda s: s[0])
def test_deep_sao_vectors_are_full_range_and_clip_at_max_v(spec):
    """14 and 16 bit, 12 x 12 and 28 x 20: g4 planes above the packed procedures' 12 bit, on content that holds 0 and max_v; in every
    case an offset lands above max_v and is clipped there, a keep map and borders (the layouts of the GPU test) change the output"""
    import h265_vectors as hv
    assert spec[3] in (14, 16) and spec[1:3] in ((12, 12), (28, 20)) and G.is_g4(*spec[1:3])
    c = G.sao_case(spec, content="full")
    max_v = (1 << c["depth"]) - 1
    cen = G.sao_census(c["planes"], c["params"], c["lw"], c["lh"], c["depth"])
    assert G.census_ok(cen, c["w"], c["h"]), (spec[0], cen)
    assert all(p.min() == 0 and p.max() == max_v and p.dtype == np.uint16 for p in c["planes"])
    tags = set().union(*(hv.sao_census(p, q, c["lw"], c["depth"]) for p, q in zip(c["planes"], c["params"])))
    assert "clip_hi" in tags and "clip_lo" in tags, spec[0]
    cuts = 0
    for f in range(len(c["planes"])):
        free = G.sao_direct(c["planes"][f], c["params"][f], c["lw"], c["lh"], bit_depth=c["depth"])
        kept = G.sao_direct(c["planes"][f], c["params"][f], c["lw"], c["lh"], bit_depth=c["depth"], keep=c["keep"][f])
        cut = G.sao_direct(c["planes"][f], c["params"][f], c["lw"], c["lh"], bit_depth=c["depth"], layout=G.sao_layout(c, f))
        assert (free != kept).any(), (spec[0], f)
        cuts += int((free != cut).any())
    assert cuts >= 2, (spec[0], cuts)   # the borders: in two frames at the least (2 x 2 CTBs: a layout may forbid nothing that is looked at)


# ---- the library ------------------------------------------------------------------------------------------------------------------

def test_new_symbols_are_exported(L):
    from gpu_video_codec_amd import _lib
    for s in NEW:
        assert s in _lib.EXPORTS and hasattr(L, s), s


def test_python_keyword_exists():
    import inspect
    from gpu_video_codec_amd import deblock
    for name in ("filter_device_h265", "sao_device", "deblock_sao_h265_device", "deblock_sao_device_planes", "derive_bs_h265"):
        p = inspect.signature(getattr(deblock.Context, name)).parameters
        assert "g4" in p and p["g4"].default is False and p["g4"].kind is inspect.Parameter.KEYWORD_ONLY, name
    b = deblock.DeviceBatch.__new__(deblock.DeviceBatch)
    b.w, b.h = 960, 540
    assert b.keep_shape == (68, 120) and b.ctb_shape(5) == (17, 30) and b.ctb_shape(4, 5) == (17, 60)
    b.w, b.h = 1920, 1088
    assert b.keep_shape == (136, 240)


def _plane(w, h, chroma=True, depth=8):
    from gpu_video_codec_amd import _lib
    p = _lib.DevicePlanes()
    sb = 1 if depth == 8 else 2
    p.src, p.dst = 0x1000, 0x400000
    p.pitch, p.frame_stride, p.n_frames, p.plane_w, p.plane_h = w * sb, w * h * sb, 1, w, h
    p.bit_depth, p.sample_bytes, p.is_chroma = depth, sb, int(chroma)
    p.vert_bs = p.hor_bs = 0x1000
    return p


def test_documented_codes_without_a_device(L):
    """a context that no device stands behind (a zeroed block of memory: never looked into): sizes and arguments are refused with
    the documented codes before the device is asked for anything"""
    from gpu_video_codec_amd import _lib
    ctx = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    hp = _lib.H265Params(0, 0, 0, 0)
    DIM, ARG = _lib.ERR_DIMENSIONS, _lib.ERR_ARG

    def filt(p, c_idx, cf=1, ctx_=ctx, variant=0, so=None):
        return L.hevcdbk_h265_filter_device_g4(ctx_, C.byref(p), c_idx, cf, 30, C.byref(hp), variant, so, None)

    def sao(p, ctx_=ctx, lw=4, lh=4, stride=None, keep=None, keep_stride=0):
        cols = -(-p.plane_w >> lw) if stride is None else stride
        return L.hevcdbk_sao_filter_device_g4(ctx_, C.byref(p), 0x1000, cols, 0, lw, lh, keep, keep_stride, 0, None, None)

    def both(p, c_idx, cf=1, ctx_=ctx, fused=0):
        cols = -(-p.plane_w >> 4)
        return L.hevcdbk_h265_deblock_sao_device_g4(ctx_, C.byref(p), c_idx, cf, 30, C.byref(hp), 0x1000, cols, 0, 4, 4, None, 0, 0, fused,
                                                    None, None, None)

    # a luma plane stays a multiple of 8; sizes that are no multiple of 4, or below 8
    assert filt(_plane(960, 540, False), 0) == DIM and both(_plane(960, 540, False), 0) == DIM
    for (w, h) in [(4, 16), (16, 4), (10, 16), (16, 10), (12, 6), (0, 16), (964, 542)]:
        assert filt(_plane(w, h), 1) == DIM, (w, h)
        assert sao(_plane(w, h)) == DIM, (w, h)
        assert both(_plane(w, h), 1) == DIM, (w, h)
    # argument errors as in the entries they extend, on a g4 plane
    g = _plane(960, 540)
    assert filt(g, 1, ctx_=None) == ARG and sao(g, ctx_=None) == ARG and both(g, 1, ctx_=None) == ARG
    assert filt(g, 0) == ARG                                   # c_idx 0 on a chroma plane
    assert filt(g, 1, cf=0) == ARG and filt(g, 1, cf=4) == ARG  # 4:0:0 has no chroma plane
    assert filt(g, 1, variant=77) == ARG
    assert filt(g, 1, so=C.byref(_lib.SliceOffsets(None, 120, 0, 4))) == ARG
    assert filt(g, 1, so=C.byref(_lib.SliceOffsets(0x1000, 119, 0, 4))) == ARG   # 1920 luma columns = 120 CTBs of 16
    assert both(g, 1, fused=9) == ARG
    assert sao(g, stride=59) == ARG                            # ceil(960 / 16) = 60 CTB columns
    assert sao(_plane(964, 540), stride=60) == ARG             # ceil(964 / 16) = 61
    assert sao(_plane(964, 540), keep=0x1000, keep_stride=120) == ARG   # ceil(964 / 8) = 121 bytes per row of the keep map
    assert sao(g, lw=4, lh=6) == ARG
    tight = _plane(964, 540)
    tight.pitch = 960
    assert filt(tight, 1) == ARG and sao(tight) == ARG
    # the planes entry: planes[0] is the luma plane, a multiple of 8, and the chroma planes are planes[0] / (SubWidthC, SubHeightC)
    sp = (_lib.SaoPlaneCf * 3)()
    for i in range(3):
        sp[i].params, sp[i].params_stride, sp[i].ctb_log2_w, sp[i].ctb_log2_h = 0x1000, 200, 5 if i else 6, 5 if i else 6

    def planes(sizes, cf=1, n=3, ctx_=ctx):
        arr = (_lib.DevicePlanes * 3)(*[_plane(w, h, i > 0) for i, (w, h) in enumerate(sizes)])
        return L.hevcdbk_h265_deblock_sao_device_planes_g4(ctx_, arr, n, cf, 30, C.byref(hp), sp, 0, None, None, None)

    assert planes([(1920, 1080), (960, 540), (960, 540)], ctx_=None) == ARG
    assert planes([(1918, 1080), (959, 540), (959, 540)]) == DIM          # not a multiple of 4
    assert planes([(1920, 1084), (960, 540), (960, 540)]) == DIM          # a g4 luma plane
    assert planes([(1920, 1080), (960, 544), (960, 540)]) == ARG          # Cb is not planes[0] / 2
    assert planes([(1920, 1080), (960, 540), (964, 540)]) == ARG
    assert planes([(1928, 24), (964, 12), (964, 12)], cf=2) == ARG        # 4:2:2: the chroma planes keep the height
    # bS derivation: the luma picture stays a multiple of 8, the chroma planes need 8 samples
    un = _lib.H265Units(0x1000, 0x1000, 0x1000, 0x1000, 0x1000)

    def bs(w, h, cf=1, chroma=True, ctx_=ctx):
        return L.hevcdbk_h265_derive_bs_device_g4(ctx_, C.byref(un), w, h, cf, 0x1000, 0x1000, 0x1000 if chroma else None,
                                                  0x1000 if chroma else None, None)
    assert bs(1920, 1080, ctx_=None) == ARG
    assert bs(1924, 1080) == DIM and bs(1920, 1084) == DIM and bs(0, 8) == DIM
    assert bs(8, 16) == DIM and bs(16, 8) == DIM              # 4:2:0 chroma of 4 samples
    assert bs(1920, 1080, cf=0) == ARG                        # 4:0:0 with chroma arrays
    assert bs(1920, 1080, cf=5) == ARG


def test_existing_entries_still_refuse_g4_planes(L):
    """nothing moves for the entries there were: a g4 plane is HEVCDBK_ERR_DIMENSIONS everywhere but in the _g4 entries"""
    from gpu_video_codec_amd import _lib
    ctx = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    hp = _lib.H265Params(0, 0, 0, 0)
    g = _plane(960, 540)
    D = _lib.ERR_DIMENSIONS
    assert L.hevc_deblocking_filter_h265_device(ctx, C.byref(g), 1, 30, C.byref(hp), 0, None) == D
    assert L.hevcdbk_h265_filter_device_cf(ctx, C.byref(g), 1, 1, 30, C.byref(hp), 0, None) == D
    assert L.hevcdbk_h265_filter_device_sl(ctx, C.byref(g), 1, 1, 30, C.byref(hp), 0, None, None) == D
    assert L.hevc_sao_filter_device(ctx, C.byref(g), 0x1000, 60, 0, 4, None, 0, 0, None) == D
    assert L.hevcdbk_sao_filter_device_nox(ctx, C.byref(g), 0x1000, 60, 0, 4, 4, None, 0, 0, None, None) == D
    assert L.hevcdbk_h265_deblock_sao_device_sl(ctx, C.byref(g), 1, 1, 30, C.byref(hp), 0x1000, 60, 0, 4, 4, None, 0, 0, 0, None, None,
                                                None) == D
    un = _lib.H265Units(0x1000, 0x1000, 0x1000, 0x1000, 0x1000)
    assert L.hevcdbk_h265_derive_bs_device(ctx, C.byref(un), 1920, 1080, 0x1000, 0x1000, 0x1000, 0x1000, None) == D


# ---- the kernels' per-block procedure on the CPU ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    import subprocess
    from conftest import ROOT
    out = str(tmp_path_factory.mktemp("g4_sim") / "libg4_sim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", out,
                           os.path.join(ROOT, "tests", "g4_sim", "g4_sim.cpp")])
    L = C.CDLL(out)
    L.g4_sim_filter_plane.restype = C.c_int
    return L


@pytest.mark.parametrize("spec", G.SMALL + G.WIDE[:1] + G.TILES8 + G.TILES16 + G.P1080[1:3] + G.FORMATS, ids=lambda s: s[0])
def test_kernel_block_procedure_on_g4_planes(sim, spec):
    """offset blocks with `8 bx < plane_w` / `8 by < plane_h` for "this half is inside" and "this edge is not the picture boundary"
    (deblock_h265.h load_block_bs_h265_g4), the 32-bit form and the packed kernels' per-lane form, with and without per-slice offsets:
    the bytes of the picture-order statements"""
    c = G.dbk_case(spec)
    vb, hb = c["bs"][0]
    m = c["qp_map"]
    for sl in (False, True):
        want = G.dbk_expected(c, 0, sl)
        pr = np.ascontiguousarray(c["pairs"], np.int8)
        for packed in (0, 1):
            out = np.ascontiguousarray(c["planes"][0]).copy()
            rc = sim.g4_sim_filter_plane(out.ctypes.data_as(C.c_void_p), c["w"], c["h"], C.c_long(out.strides[0]), out.itemsize, c["depth"],
                                         c["cf"], vb.ctypes.data_as(C.c_void_p), hb.ctypes.data_as(C.c_void_p), c["qp"],
                                         None if m is None else m.ctypes.data_as(C.c_void_p), 0 if m is None else m.shape[1], G.UNIT_LOG2,
                                         G.CQP, 0 if sl else G.TC_DIV2, pr.ctypes.data_as(C.c_void_p) if sl else None, pr.shape[1],
                                         G.SL_CTB_LOG2, packed)
            assert rc == 0
            assert np.array_equal(out, want), (spec[0], sl, packed, int((out != want).sum()))
