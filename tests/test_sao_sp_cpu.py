"""SAO and deblocking + SAO of a semi-planar chroma plane (the _sp SAO entries) without a GPU: the library has the entries and answers
with the documented codes where it can answer without a device; the kernels' block procedures -- sao_sp.h: deblock_sp.h's split and
merge around the packed procedures of sao_packed.h, and the per-sample procedure with a component stride of 2 -- give on the CPU,
over whole interleaved planes of the GPU vectors' shapes, the bytes of tests/sao_sp_ref.py, whatever surrounds the plane; and every
GPU vector exercises what it is there for."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import sao_borders_ref as B
import sao_sp_ref as P

NEW = ["hevcdbk_sao_filter_device_sp", "hevcdbk_h265_deblock_sao_device_sp"]


@pytest.fixture(scope="module")
def L():
    from gpu_video_codec_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def cases():
    """the GPU vectors, made once"""
    return {spec[0]: P.case(spec) for spec in P.VECTORS}


# ---- the library ------------------------------------------------------------------------------------------------------------------

def test_new_symbols_are_exported_and_declared(L):
    from conftest import ROOT
    from gpu_video_codec_amd import _lib
    header = open(os.path.join(ROOT, "include", "hevc_deblock.h")).read()
    for s in NEW:
        assert s in _lib.EXPORTS and hasattr(L, s), s
        assert re.search(r"HEVCDBK_API int %s\(" % s, header), s


def test_python_keywords_exist():
    from gpu_video_codec_amd import deblock
    for fn in (deblock.Context.sao_device, deblock.Context.deblock_sao_h265_device):
        p = inspect.signature(fn).parameters
        assert p["semi_planar"].default is False and p["semi_planar"].kind is inspect.Parameter.KEYWORD_ONLY
        assert p["params_cr_ptr"].default is None and p["params_cr_ptr"].kind is inspect.Parameter.KEYWORD_ONLY


def test_python_misuse_raises():
    """before the library is asked for anything: no context is needed"""
    from gpu_video_codec_amd import deblock
    ctx = object.__new__(deblock.Context)
    with pytest.raises(ValueError):
        ctx.sao_device(None, 1, 1, 4, semi_planar=True)
    with pytest.raises(ValueError):
        ctx.sao_device(None, 1, 1, 4, semi_planar=True, params_cr_ptr=1, chroma_format="422")
    with pytest.raises(ValueError):
        ctx.deblock_sao_h265_device(None, 30, 1, 1, 4, semi_planar=True)
    with pytest.raises(ValueError):
        ctx.deblock_sao_h265_device(None, 30, 1, 1, 4, semi_planar=True, params_cr_ptr=1, chroma_format="444")


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
    PB, PR = 0x2000, 0x3000

    def sao(p, ctx_=ctx, pcb=PB, pcr=PR, stride=64, lg=4, keep=None, keep_stride=0, borders=None):
        return L.hevcdbk_sao_filter_device_sp(ctx_, C.byref(p), pcb, pcr, stride, 0, lg, keep, keep_stride, 0, borders, None)

    def chain(p, ctx_=ctx, pcb=PB, pcr=PR, stride=64, lg=4, fused=_lib.FUSED_AUTO, borders=None, so=None):
        return L.hevcdbk_h265_deblock_sao_device_sp(ctx_, C.byref(p), 30, C.byref(hp), pcb, pcr, stride, 0, lg, None, 0, 0, fused, borders,
                                                    so, None)

    for call in (sao, chain):
        # sizes per component: multiples of 4, at least 8
        for (w, h) in [(4, 16), (16, 4), (10, 16), (16, 10), (12, 6), (0, 16), (964, 542)]:
            assert call(_plane(w, h)) == DIM, (w, h)
        g = _plane(960, 540)
        assert call(g, ctx_=None) == ARG
        # a luma plane is no pair plane
        assert call(_plane(960, 544, chroma=False)) == ARG
        # a pitch that holds one component only
        for depth in (8, 10):
            sb = 1 if depth == 8 else 2
            assert call(_plane(960, 540, depth=depth, pitch=960 * sb)) == ARG
            assert call(_plane(960, 540, depth=depth, pitch=2 * 960 * sb - 4 * sb)) == ARG
        # both parameter arrays
        assert call(g, pcr=None) == ARG and call(g, pcb=None) == ARG
        # square CTBs of 8, 16, 32
        assert call(g, lg=2) == ARG and call(g, lg=6) == ARG
        # the parameter stride: 960 / 16 = 60 CTBs per row
        assert call(g, stride=59) == ARG
        # borders on the CTB grid
        assert call(g, borders=C.byref(_lib.SaoBorders(0x5000, 59, 0))) == ARG
        assert call(g, borders=C.byref(_lib.SaoBorders(None, 60, 0))) == ARG
        # src == dst: as the planar SAO entry answers it
        same = _plane(960, 540)
        same.dst = same.src
        assert call(same) == ARG
        # alignment: one 4-sample word, as for every plane
        assert call(_plane(960, 540, pitch=2 * 960 + 2)) == UNS
    g = _plane(960, 540)
    # the keep map: ceil(960 / 8) bytes per row
    assert sao(g, keep=0x6000, keep_stride=119) == ARG
    # the chain: fused
    assert chain(g, fused=_lib.FUSED_ON) == UNS
    assert chain(g, fused=7) == ARG and chain(g, fused=-1) == ARG
    assert chain(g, so=C.byref(_lib.SliceOffsets(None, 120, 0, 4))) == ARG


# ---- the kernels' block procedures on the CPU -------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    from conftest import ROOT
    out = str(tmp_path_factory.mktemp("sao_sp_sim") / "libsao_sp_sim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", out,
                           os.path.join(ROOT, "tests", "sao_sp_sim", "sao_sp_sim.cpp")])
    lib = C.CDLL(out)
    lib.sao_sp_sim_plane.restype = C.c_int
    return lib


PAD_ROWS, PAD_BYTES = 3, 32


def run_sim(sim, c, f, keep, layout, form, poison, nox=None):
    """the plane inside a larger array of `poison`: rows above and below, bytes behind every row; nox: boundary bytes of the
    caller's own (rows x stride) in place of a layout's"""
    h, w, sb = c["h"], c["w"], c["sb"]
    row = 2 * w * sb
    pitch = row + PAD_BYTES
    src = np.full((h + 2 * PAD_ROWS, pitch), poison, np.uint8)
    src[PAD_ROWS: PAD_ROWS + h, :row] = np.ascontiguousarray(c["planes"][f]).view(np.uint8).reshape(h, row)
    dst = np.full_like(src, 0x5A)
    pcb, pcr = np.ascontiguousarray(c["pcb"][f]), np.ascontiguousarray(c["pcr"][f])
    k = np.ascontiguousarray(c["keep"][f]) if keep else None
    if nox is None and layout is not None:
        nox = B.expected_nox(layout)
    nox = None if nox is None else np.ascontiguousarray(nox, np.uint8)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = sim.sao_sp_sim_plane(C.c_void_p(src.ctypes.data + PAD_ROWS * pitch), C.c_void_p(dst.ctypes.data + PAD_ROWS * pitch), w, h, C.c_long(pitch),
                              sb, c["depth"], vp(pcb), vp(pcr), pcb.shape[1], c["lg"], vp(k), 0 if k is None else k.shape[1], vp(nox),
                              0 if nox is None else nox.shape[1], form)
    assert rc == 0
    out = np.ascontiguousarray(dst[PAD_ROWS: PAD_ROWS + h, :row]).view(np.uint8 if sb == 1 else np.uint16).reshape(h, w, 2)
    rest = dst.copy()
    rest[PAD_ROWS: PAD_ROWS + h, :row] = 0x5A
    assert (rest == 0x5A).all(), "bytes outside the plane were written"
    return out


@pytest.mark.parametrize("spec", P.VECTORS, ids=lambda s: s[0])
def test_kernel_block_procedures_on_pair_planes(sim, cases, spec):
    """every frame x {no keep map, keep map} x {no borders, the layout}; the per-sample form and, up to 12 bit, the packed form"""
    c = cases[spec[0]]
    for f in range(P.FRAMES):
        for keep in (False, True):
            for layout in (None, c["layout"]):
                want = P.expected(c, f, keep=keep, layout=layout)
                for form in ((0, 1) if c["depth"] <= 12 else (0,)):
                    got = run_sim(sim, c, f, keep, layout, form, 0xEE)
                    assert np.array_equal(got, want), (spec[0], f, keep, layout is not None, form, int((got != want).sum()),
                                                       np.argwhere(got != want)[:4].tolist())


@pytest.mark.parametrize("spec", P.VECTORS, ids=lambda s: s[0])
def test_what_surrounds_the_plane_does_not_matter(sim, cases, spec):
    c = cases[spec[0]]
    for form in ((0, 1) if c["depth"] <= 12 else (0,)):
        a = run_sim(sim, c, 1, True, c["layout"], form, 0x00)
        b = run_sim(sim, c, 1, True, c["layout"], form, 0xFF)
        assert np.array_equal(a, b), (spec[0], form)


def test_the_packed_form_stops_at_12_bit(sim):
    z = np.zeros((8, 8, 2), np.uint16)
    p = np.zeros(1, P.rx_dtype())
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert sim.sao_sp_sim_plane(vp(z), vp(z.copy()), 8, 8, C.c_long(32), 2, 14, vp(p), vp(p), 1, 3, None, 0, None, 0, 1) == 3


# ---- the vectors are not vacuous -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spec", P.VECTORS, ids=lambda s: s[0])
def test_vectors_bite_in_both_components(cases, spec):
    """per component every edge class and the band offset change samples; exchanging the two parameter arrays changes BOTH components;
    a kept block would have changed; the layout changes samples; on g4 shapes g4_ref.census_ok per component; more than half of the
    CTBs agree in type and class, some differ in type, some in class"""
    c = cases[spec[0]]
    cen = P.census(c)
    assert P.census_ok(c, cen), (spec[0], cen)
