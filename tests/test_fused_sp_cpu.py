"""Deblocking + SAO of a semi-planar picture in one kernel (hevcdbk_h265_deblock_sao_device_sp_fused, hevcdbk_h265_deblock_sao_device_nv12)
without a GPU: the library has the entries and answers with the documented codes where it can answer without a device; the per-lane
procedures of the pair body (csrc/deblock_sao_sp_fused.h), driven tile by tile on the CPU through a host array that stands for the LDS
tile (tests/fused_sp_sim, a stand-alone program), give the bytes of tests/sao_sp_ref.py whatever the array and the memory around the
plane held before; the shapes bite where a tile's halo matters; the Python entries refuse what they document.

There is no new filter logic here: the expectation is sp_ref.dbk_expected followed by sao_sp_ref.sao -- sao_sp_ref.chain_expected, which
fixes the QP map, with the choice "one QP or the map" passed on."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import sao_borders_ref as B
import sao_sp_ref as P
import sp_ref as S

NEW = ["hevcdbk_h265_deblock_sao_device_sp_fused", "hevcdbk_h265_deblock_sao_device_nv12"]
SHAPES = ["16x16", "12x12", "136x136", "140x132", "264x136_10", "140x132_12"]
TILE_W, TILE_H = {1: 96, 2: 64}, 128   # pairs per tile row (8-bit samples, 16-bit containers), rows: spf::Geo of deblock_sao_sp_fused.h


@pytest.fixture(scope="module")
def L():
    from gpu_video_codec_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def chains():
    return {name: P.chain_case(P.spec_of(name)) for name in SHAPES}


def chain_expected(c, f, qmap, sl, layout):
    """sao_sp_ref.chain_expected with one QP (qmap False) or the map"""
    dbk = S.dbk_expected(c, f, qmap, sl)
    return dbk, P.sao(dbk, c["pcb"][f], c["pcr"][f], c["lg"], c["depth"], keep=c["keep"][f], layout=layout)


# ---- the library ------------------------------------------------------------------------------------------------------------------

def test_new_symbols_are_exported_and_declared(L):
    import re
    from conftest import ROOT
    from gpu_video_codec_amd import _lib
    header = open(os.path.join(ROOT, "include", "hevc_deblock.h")).read()
    for s in NEW:
        assert s in _lib.EXPORTS and hasattr(L, s), s
        assert re.search(r"HEVCDBK_API int %s\(" % s, header), s


def _plane(w, h, chroma=True, depth=8, pitch=None, frames=1):
    from gpu_video_codec_amd import _lib
    p = _lib.DevicePlanes()
    sb = 1 if depth == 8 else 2
    p.src, p.dst = 0x1000, 0x4000000
    p.pitch = (2 if chroma else 1) * w * sb if pitch is None else pitch
    p.frame_stride, p.n_frames, p.plane_w, p.plane_h = p.pitch * h, frames, w, h
    p.bit_depth, p.sample_bytes, p.is_chroma = depth, sb, int(chroma)
    p.vert_bs = p.hor_bs = 0x1000
    return p


def test_documented_codes_without_a_device(L):
    """a context that no device stands behind (a zeroed block of memory: never looked into): every operand is checked before the
    device is asked for anything, so every call here is one that is refused"""
    from gpu_video_codec_amd import _lib
    ctx = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    hp = _lib.H265Params(0, 0, -6, 6)
    DIM, ARG, UNS = _lib.ERR_DIMENSIONS, _lib.ERR_ARG, _lib.ERR_UNSUPPORTED
    PB, PR = 0x2000, 0x3000

    def chain(p, ctx_=ctx, pcb=PB, pcr=PR, stride=64, lg=4, keep=None, keep_stride=0, fused=_lib.FUSED_AUTO, borders=None, so=None, prm=hp):
        return L.hevcdbk_h265_deblock_sao_device_sp_fused(ctx_, C.byref(p), 30, C.byref(prm), pcb, pcr, stride, 0, lg, keep, keep_stride, 0,
                                                          fused, borders, so, None)

    # ---- _sp_fused: every mistake of the _sp chain entry, with that entry's code ----
    for (w, h) in [(4, 16), (16, 4), (10, 16), (16, 10), (12, 6), (0, 16), (964, 542)]:
        assert chain(_plane(w, h)) == DIM, (w, h)
    g = _plane(960, 540)
    assert chain(g, ctx_=None) == ARG
    assert chain(_plane(960, 544, chroma=False)) == ARG                       # a luma plane is no pair plane
    for depth in (8, 10):                                                     # a pitch that holds one component only
        sb = 1 if depth == 8 else 2
        assert chain(_plane(960, 540, depth=depth, pitch=960 * sb)) == ARG
        assert chain(_plane(960, 540, depth=depth, pitch=2 * 960 * sb - 4 * sb)) == ARG
    assert chain(g, pcr=None) == ARG and chain(g, pcb=None) == ARG            # both parameter arrays
    assert chain(g, lg=2) == ARG and chain(g, lg=6) == ARG                    # square CTBs of 8, 16, 32
    assert chain(g, stride=59) == ARG                                         # 960 / 16 = 60 CTBs per row
    assert chain(g, keep=0x6000, keep_stride=119) == ARG                      # ceil(960 / 8) bytes per row
    assert chain(g, borders=C.byref(_lib.SaoBorders(0x5000, 59, 0))) == ARG   # borders on the CTB grid
    assert chain(g, borders=C.byref(_lib.SaoBorders(None, 60, 0))) == ARG
    same = _plane(960, 540)
    same.dst = same.src
    assert chain(same) == ARG                                                 # src == dst
    assert chain(_plane(960, 540, pitch=2 * 960 + 2)) == UNS                  # one 4-sample word, as for every plane
    assert chain(g, prm=_lib.H265Params(7, 0, 0, 0)) == ARG and chain(g, prm=_lib.H265Params(0, 0, 13, 0)) == ARG
    assert chain(g, so=C.byref(_lib.SliceOffsets(None, 120, 0, 4))) == ARG    # slice_offsets: no array, a short stride, a CTB size
    assert chain(g, so=C.byref(_lib.SliceOffsets(0x7000, 29, 0, 6))) == ARG
    assert chain(g, so=C.byref(_lib.SliceOffsets(0x7000, 120, 0, 3))) == ARG
    assert chain(g, fused=7) == ARG and chain(g, fused=-1) == ARG
    # FUSED_ON where the kernel's guards refuse the plane: before the device is asked for anything
    assert chain(_plane(960, 540, pitch=2 * 960 + 8), fused=_lib.FUSED_ON) == UNS
    assert chain(_plane(960, 540, depth=14), fused=_lib.FUSED_ON) == UNS

    # ---- _nv12 ----
    def nv12(luma, pairs, ctx_=ctx, lg=5, lgc=4, fused=_lib.FUSED_AUTO, borders=None, so=None, sl_null=False, sp_null=False, stride=64):
        sl = _lib.SaoPlaneCf(PB, stride, 0, lg, lg, None, 0, 0)
        sp = _lib.SaoPlaneSp(PB, PR, stride, 0, lgc, None, 0, 0)
        return L.hevcdbk_h265_deblock_sao_device_nv12(ctx_, C.byref(luma) if luma is not None else None, C.byref(pairs) if pairs is not None else None,
                                                      30, C.byref(hp), None if sl_null else C.byref(sl), None if sp_null else C.byref(sp), fused,
                                                      borders, so, None)

    Y, UV = _plane(1920, 1088, chroma=False), _plane(960, 544)
    assert nv12(Y, UV, ctx_=None) == ARG and nv12(None, UV) == ARG and nv12(Y, None) == ARG
    assert nv12(Y, UV, sl_null=True) == ARG and nv12(Y, UV, sp_null=True) == ARG
    assert nv12(Y, UV, fused=7) == ARG and nv12(Y, UV, fused=-1) == ARG
    assert nv12(_plane(1920, 1088), UV) == ARG and nv12(Y, _plane(960, 544, chroma=False)) == ARG     # which plane is which
    assert nv12(_plane(1920, 1084, chroma=False), _plane(960, 542)) == DIM                              # luma in multiples of 8
    assert nv12(Y, _plane(960, 546)) == DIM                                                             # pairs in multiples of 4
    for (w, h) in [(952, 544), (960, 540), (1920, 1088), (968, 544)]:                                   # a pair plane that is not luma / 2
        assert nv12(Y, _plane(w, h)) == ARG, (w, h)
    for lg, lgc in [(5, 5), (5, 3), (6, 4), (4, 4), (4, 5)]:                                            # chroma CTBs are half the luma CTBs
        assert nv12(Y, UV, lg=lg, lgc=lgc) == ARG, (lg, lgc)
    assert nv12(_plane(1920, 1088, chroma=False, depth=10), UV) == ARG                                  # one depth
    assert nv12(Y, _plane(960, 544, depth=10)) == ARG
    assert nv12(_plane(1920, 1088, chroma=False, frames=2), UV) == ARG                                  # one frame count
    assert nv12(Y, UV, stride=29) == ARG                                                                # 1920 / 32 = 60 CTBs per row
    assert nv12(Y, UV, borders=C.byref(_lib.SaoBorders(0x5000, 59, 0))) == ARG
    assert nv12(Y, UV, so=C.byref(_lib.SliceOffsets(None, 120, 0, 4))) == ARG
    assert nv12(Y, _plane(960, 544, pitch=2 * 960 + 2)) == UNS                                          # alignment, as for every plane
    # FUSED_ON with a plane that cannot be fused: the pair plane's pitch, then both planes at 14 bit
    assert nv12(Y, _plane(960, 544, pitch=2 * 960 + 8), fused=_lib.FUSED_ON) == UNS
    assert nv12(_plane(1920, 1088, chroma=False, depth=14), _plane(960, 544, depth=14), fused=_lib.FUSED_ON) == UNS


# ---- the Python entries -------------------------------------------------------------------------------------------------------------

def test_python_argument_errors():
    """before the library is asked for anything: no context is needed"""
    import inspect
    from gpu_video_codec_amd import deblock
    p = inspect.signature(deblock.Context.deblock_sao_h265_device).parameters
    assert p["one_kernel"].default is False and p["one_kernel"].kind is inspect.Parameter.KEYWORD_ONLY
    ctx = object.__new__(deblock.Context)
    with pytest.raises(ValueError):
        ctx.deblock_sao_h265_device(None, 30, 1, 1, 4, one_kernel=True)
    with pytest.raises(ValueError):
        ctx.deblock_sao_h265_device(None, 30, 1, 1, 4, one_kernel=True, g4=True)
    with pytest.raises(ValueError):
        ctx.deblock_sao_h265_device(None, 30, 1, 1, 4, semi_planar=True, one_kernel=True)   # params_cr_ptr is still needed
    good_l, good_p = {"params": 1, "params_stride": 1, "ctb_log2": 5}, {"params_cb": 1, "params_cr": 2, "params_stride": 1, "ctb_log2": 4}
    with pytest.raises(ValueError):
        ctx.deblock_sao_nv12(None, None, 30, good_l, good_p, h265=None)
    with pytest.raises(ValueError):
        ctx.deblock_sao_nv12(None, None, 30, good_l, {"params_cb": 1, "params_stride": 1, "ctb_log2": 4}, h265={})
    with pytest.raises(ValueError):
        ctx.deblock_sao_nv12(None, None, 30, (1, 1, 5), good_p, h265={})
    with pytest.raises(TypeError):
        ctx.deblock_sao_nv12(None, None, 30, good_l, good_p)   # h265 is a required keyword


# ---- the pair body on the CPU ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    from conftest import ROOT
    out = str(tmp_path_factory.mktemp("fused_sp_sim")) + os.sep
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "fused_sp_sim"), "OUT=" + out, "all"])
    return out


PAD_ROWS, PAD_BYTES = 3, 32


def run_sim(sim, c, f, qmap, sl, layout, lds_poison, poison, nox=None):
    """frame f of chain case c through the program: the plane inside a larger array of `poison` (rows above and below, bytes behind
    every row), the "LDS" array filled with `lds_poison`; the QP offsets and the tC offset are sp_ref's unless c has its own ("cb", "cr",
    "tc_div2"); nox: boundary bytes of the caller's own (rows x stride) in place of a layout's"""
    h, w, sb = c["h"], c["w"], c["sb"]
    row = 2 * w * sb
    pitch = row + PAD_BYTES
    src = np.full((h + 2 * PAD_ROWS, pitch), poison, np.uint8)
    src[PAD_ROWS: PAD_ROWS + h, :row] = np.ascontiguousarray(c["planes"][f]).view(np.uint8).reshape(h, row)
    vb, hb = c["bs"][f]
    qm = np.ascontiguousarray(c["qp_map"], np.uint8)
    pr = np.ascontiguousarray(c["pairs"], np.int8)
    pcb, pcr = np.ascontiguousarray(c["pcb"][f]), np.ascontiguousarray(c["pcr"][f])
    keep = np.ascontiguousarray(c["keep"][f], np.uint8)
    if nox is None and layout is not None:
        nox = B.expected_nox(layout)
    nox = None if nox is None else np.ascontiguousarray(nox, np.uint8)
    head = [w, h, pitch, sb, c["depth"], c["qp"], int(qmap), qm.shape[-1], S.UNIT_LOG2, c.get("cb", S.CB_OFF), c.get("cr", S.CR_OFF),
            0 if sl else 2 * c.get("tc_div2", S.TC_DIV2), 0,
            int(sl), pr.shape[1], S.SL_CTB_LOG2, pcb.shape[1], c["lg"], keep.shape[1], 0 if nox is None else nox.shape[1], PAD_ROWS,
            lds_poison, 0, 0]
    blobs = [src, np.ascontiguousarray(vb, np.uint8), np.ascontiguousarray(hb, np.uint8), qm, pr, pcb, pcr, keep, nox]
    keepdir = os.environ.get("FUSED_SP_SIM_KEEP")
    tag = "%s_f%d_q%d_s%d_l%d_%02x_%02x" % (c["name"].replace("/", "_"), f, qmap, sl, nox is not None, lds_poison, poison)
    job, out = os.path.join(keepdir or sim, tag + ".job"), os.path.join(sim, tag + ".out")
    with open(job, "wb") as fh:
        fh.write(struct.pack("<24q", *head))
        for b in blobs:
            raw = b"" if b is None else b.tobytes()
            fh.write(struct.pack("<q", len(raw)))
            fh.write(raw)
    r = subprocess.run([os.path.join(sim, "fused_sp_sim"), job, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (tag, r.returncode, r.stderr[-2000:])
    dst = np.fromfile(out, np.uint8).reshape(src.shape)
    os.remove(out)
    if not keepdir:
        os.remove(job)
    got = np.ascontiguousarray(dst[PAD_ROWS: PAD_ROWS + h, :row]).view(np.uint8 if sb == 1 else np.uint16).reshape(h, w, 2)
    rest = dst.copy()
    rest[PAD_ROWS: PAD_ROWS + h, :row] = 0x5A
    assert (rest == 0x5A).all(), "bytes outside the plane were written"
    return got


@pytest.mark.parametrize("name", SHAPES)
def test_pair_body_tile_by_tile(sim, chains, name):
    """two frames x {one QP, the map} x {the call's own pair, per-slice pairs} x {no borders, the layout}, the keep map always"""
    c = chains[name]
    for f in range(2):
        for qmap in (False, True):
            for sl in (False, True):
                for layout in (None, c["layout"]):
                    want = chain_expected(c, f, qmap, sl, layout)[1]
                    got = run_sim(sim, c, f, qmap, sl, layout, 0xC3, 0xEE)
                    assert np.array_equal(got, want), (name, f, qmap, sl, layout is not None, int((got != want).sum()),
                                                       np.argwhere(got != want)[:4].tolist())


@pytest.mark.parametrize("name", SHAPES)
def test_what_the_tile_and_the_surroundings_held_does_not_matter(sim, chains, name):
    c = chains[name]
    a = run_sim(sim, c, 1, True, True, c["layout"], 0x00, 0x00)
    b = run_sim(sim, c, 1, True, True, c["layout"], 0xFF, 0xFF)
    assert np.array_equal(a, b), name
    assert np.array_equal(a, chain_expected(c, 1, True, True, c["layout"])[1]), name


def test_the_program_refuses_what_the_kernels_refuse(sim, tmp_path):
    job = tmp_path / "deep.job"
    job.write_bytes(struct.pack("<24q", 8, 8, 32, 2, 14, *([0] * 19)) + struct.pack("<q", 0) * 9)
    assert subprocess.run([os.path.join(sim, "fused_sp_sim"), str(job), str(tmp_path / "o")]).returncode == 3


# ---- the shapes are not vacuous ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SHAPES)
def test_shapes_bite_in_both_stages_and_at_the_tile_boundaries(chains, name):
    """per component: deblocking changes samples and SAO changes the deblocked samples; where the plane has more than one tile in a
    direction, the expectation differs from SAO of the UN-deblocked plane in samples within one sample of a tile boundary in that
    direction -- what a tile without its halo of deblocked samples would get wrong; the SAO vector's own census holds"""
    c = chains[name]
    tw, th = TILE_W[c["sb"]], TILE_H
    cols = [x for b in range(tw, c["w"], tw) for x in (b - 1, b)]
    rows = [y for b in range(th, c["h"], th) for y in (b - 1, b)]
    if name in ("136x136", "140x132", "264x136_10"):   # at least two tiles in a direction, the last one cut
        assert cols and rows and c["w"] % tw and c["h"] % th, (name, cols, rows)
    at_cols, at_rows = [0, 0], [0, 0]
    for f in range(2):
        for qmap in (False, True):
            for sl in (False, True):
                dbk, want = chain_expected(c, f, qmap, sl, c["layout"])
                raw = P.sao(c["planes"][f], c["pcb"][f], c["pcr"][f], c["lg"], c["depth"], keep=c["keep"][f], layout=c["layout"])
                for k in range(2):
                    assert (dbk[..., k] != c["planes"][f][..., k]).any() and (want[..., k] != dbk[..., k]).any(), (name, f, qmap, sl, k)
                    d = want[..., k] != raw[..., k]
                    at_cols[k] += int(d[:, cols].sum())
                    at_rows[k] += int(d[rows, :].sum())
    for k in range(2):
        assert (at_cols[k] > 0 or not cols) and (at_rows[k] > 0 or not rows), (name, k, at_cols, at_rows)
    v = P.case(P.spec_of(name))
    assert P.census_ok(v, P.census(v)), name
