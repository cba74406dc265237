"""Deblocking + SAO of a semi-planar picture in ONE kernel on the GPU: the plane of interleaved Cb / Cr pairs through
hevcdbk_h265_deblock_sao_device_sp_fused, the Y plane with it in one launch through hevcdbk_h265_deblock_sao_device_nv12.  The pair
plane's bytes are those of tests/sao_sp_ref.py (sp_ref.dbk_expected, then sao_sp_ref.sao: chain_expected with the choice of one QP or
the map passed on), the Y plane's those of the statement tests/test_gpu_g4.py uses for a luma plane; test_fused_sp_cpu.py asserts that
the shapes bite at the tile boundaries.  Every destination is pre-filled, has row padding, a gap between frames and guard rows, all of
which must come back untouched.  The kernels that ran are read from a stream capture.  PARITY UNPINNED, like the rest of the spec-exact
mode."""
import ctypes as C

import numpy as np
import pytest

import g4_ref as G
import sao_sp_ref as P
import slice_offsets_ref as R
import sp_ref as S
from test_gpu_g4 import Plane as LumaPlane, borders_operand
from test_gpu_sao_sp import GENERIC as SAO_GENERIC, PIECE, Operands, pad_of, sao_name
from test_gpu_sp import PACKED_NAMES as DBK_PACKED, PairPlane, captured, check, hp_of, sl_operand

pytestmark = pytest.mark.gpu

FUSED = {1: "dbk_sao_fused_h265_sp_kernel", 2: "dbk_sao_fused16_h265_sp_kernel"}
MULTI = "dbk_sao_fused_multi_h265_sp_kernel"
DBK_GENERIC = "dbk_h265_sp_kernel"
SHAPES = ["16x16", "12x12", "136x136", "140x132", "264x136_10", "140x132_12"]


@pytest.fixture(scope="module")
def ctx():
    from gpu_video_codec_amd import deblock
    c = deblock.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def lib():
    from gpu_video_codec_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def chains():
    """the chain cases, made once and left unchanged"""
    return {name: P.chain_case(P.spec_of(name)) for name in SHAPES + ["72x24_14"]}


_wants = {}


def expected(c, f, qmap, sl, borders):
    """(deblocked, final) of frame f, computed once per combination"""
    key = (c["name"], f, qmap, sl, borders)
    if key not in _wants:
        dbk = S.dbk_expected(c, f, qmap, sl)
        _wants[key] = (dbk, P.sao(dbk, c["pcb"][f], c["pcr"][f], c["lg"], c["depth"], keep=c["keep"][f], layout=c["layout"] if borders else None))
    return _wants[key]


def two_launches(c):
    return [DBK_PACKED[c["sb"]] if c["depth"] <= 12 else DBK_GENERIC, sao_name(c)]


def fused_call(L, ctx, ops, p, c, hp, fused, borders, so, st=None):
    return L.hevcdbk_h265_deblock_sao_device_sp_fused(ctx.handle, C.byref(p), c["qp"], C.byref(hp), ops.pcb.ptr, ops.pcr.ptr, ops.cols,
                                                      ops.rows * ops.cols, ops.lg, ops.keep.ptr, ops.kc, ops.kr * ops.kc, fused,
                                                      C.byref(ops.borders) if borders else None, so, st)


# ---- the pair plane ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SHAPES)
def test_sp_fused(ctx, lib, chains, name):
    """two frames with per-frame operands; {one QP, the map} x {slice_offsets} x {borders}; AUTO and ON: exactly one kernel, the
    fused one; OFF: the two _sp kernels; the same bytes every time"""
    L = lib.lib()
    c = chains[name]
    hp = hp_of(lib)
    so, dso = sl_operand(ctx, lib, c["pairs"])
    ops = Operands(ctx, lib, c, frames=range(2))
    for qmap in (False, True):
        for sl in (False, True):
            for borders in (False, True):
                pairs = [expected(c, f, qmap, sl, borders) for f in range(2)]
                for f in range(2):   # both stages do something
                    assert (pairs[f][0] != c["planes"][f]).any() and (pairs[f][1] != pairs[f][0]).any()
                for fused, kernels in ((lib.FUSED_AUTO, [FUSED[c["sb"]]]), (lib.FUSED_ON, [FUSED[c["sb"]]]), (lib.FUSED_OFF, two_launches(c))):
                    pl = PairPlane(ctx, c, qmap=qmap, pad=pad_of(c))
                    call = lambda st: fused_call(L, ctx, ops, pl.p, c, hp, fused, borders, C.byref(so) if sl else None, st)
                    rc, k = captured(call)
                    assert rc == 0 and k == kernels, (rc, k, fused)
                    assert call(None) == 0
                    ctx.synchronize()
                    check(pl, [p[1] for p in pairs], (name, qmap, sl, borders, fused))
                    pl.free()
    ops.free()
    dso.free()


def test_sp_fused_falls_back(ctx, lib, chains):
    """samples deeper than 12 bit, and a plane whose pitch the fused kernel's guard refuses: AUTO runs the two launches and the bytes
    are right, ON is refused with nothing enqueued"""
    L = lib.lib()
    hp = hp_of(lib)
    for name, rest, kernels in (("72x24_14", 0, [DBK_GENERIC, SAO_GENERIC]), ("140x132", 8, [DBK_PACKED[1], SAO_GENERIC])):
        c = chains[name]
        ops = Operands(ctx, lib, c, frames=range(2))
        pl = PairPlane(ctx, c, qmap=True, pad=pad_of(c, rest))
        assert pl.p.pitch % PIECE[c["sb"]] == rest
        call = lambda st, fused: fused_call(L, ctx, ops, pl.p, c, hp, fused, True, None, st)
        assert captured(lambda st: call(st, lib.FUSED_AUTO)) == (0, kernels), name
        assert captured(lambda st: call(st, lib.FUSED_ON)) == (lib.ERR_UNSUPPORTED, []), name
        assert call(None, lib.FUSED_AUTO) == 0
        ctx.synchronize()
        check(pl, [expected(c, f, True, False, True)[1] for f in range(2)], ("fallback", name))
        pl.free()
        ops.free()


def test_dispatch_guards_of_the_fused_kernels(ctx, lib, chains):
    """each guard of dbk_deblock_sao_sp_supports that a call can reach, on both sides, by kernel name (the frame count and the tile
    counts cannot be reached: the entry refuses more than 65535 frames or rows as arguments)"""
    L = lib.lib()
    hp = hp_of(lib)
    for name in ("140x132", "140x132_12"):
        c = chains[name]
        sb, piece = c["sb"], PIECE[c["sb"]]
        ops = Operands(ctx, lib, c, frames=range(2))
        probe = lambda pl: captured(lambda st: fused_call(L, ctx, ops, pl.p, c, hp, lib.FUSED_AUTO, True, None, st))
        refused = lambda pl: captured(lambda st: fused_call(L, ctx, ops, pl.p, c, hp, lib.FUSED_ON, True, None, st)) == (lib.ERR_UNSUPPORTED, [])
        for rest, fused in ((0, True), (piece // 2, False)):
            pl = PairPlane(ctx, c, qmap=True, pad=pad_of(c, rest))
            assert pl.p.pitch % piece == rest
            rc, k = probe(pl)
            assert rc == 0 and (k == [FUSED[sb]]) == fused and (len(k) == 2) != fused, ("pitch", name, rest, k)
            assert refused(pl) != fused
            pl.free()
        for field in ("src", "dst", "frame_stride"):
            pl = PairPlane(ctx, c, qmap=True, pad=pad_of(c))
            setattr(pl.p, field, getattr(pl.p, field) + piece // 2)
            rc, k = probe(pl)
            assert rc == 0 and len(k) == 2 and FUSED[sb] not in k, (field, name, k)
            assert refused(pl)
            pl.free()
        ops.free()
    # depth: 12 bit is fused (above), 14 bit is not (test_sp_fused_falls_back)
    # pitch * plane_h < 2^31: captured only, never run -- no such plane is allocated
    c = chains["16x16"]
    ops = Operands(ctx, lib, c, frames=range(1))
    pl = PairPlane(ctx, c, frames=[c["planes"][0]], qmap=True, pad=pad_of(c))
    for pitch, fused in (((1 << 27) - 16, True), (1 << 27, False)):
        pl.p.pitch, pl.p.frame_stride, pl.p.n_frames = pitch, pitch * 16, 1
        rc, k = captured(lambda st: fused_call(L, ctx, ops, pl.p, c, hp, lib.FUSED_AUTO, False, None, st))
        assert rc == 0 and (k == [FUSED[1]]) == fused, (pitch, k)
    pl.free()
    ops.free()


@pytest.mark.parametrize("name", ["140x132", "264x136_10"])
def test_sp_fused_equals_the_two_launch_entry(ctx, lib, chains, name):
    """no reference: hevcdbk_h265_deblock_sao_device_sp on the same operands, GPU against GPU"""
    L = lib.lib()
    c = chains[name]
    hp = hp_of(lib)
    so, dso = sl_operand(ctx, lib, c["pairs"])
    ops = Operands(ctx, lib, c, frames=range(2))
    a, b = PairPlane(ctx, c, qmap=True, pad=pad_of(c)), PairPlane(ctx, c, qmap=True, pad=pad_of(c))
    assert fused_call(L, ctx, ops, a.p, c, hp, lib.FUSED_ON, True, C.byref(so)) == 0
    assert ops.chain(L, ctx, b.p, c["qp"], hp, lib.FUSED_AUTO, True, C.byref(so)) == 0
    ctx.synchronize()
    two, clean = b.read()
    assert clean and (two[0] != c["planes"][0]).any()
    check(a, two, ("GPU against GPU", name))
    for x in (a, b, ops, dso):
        x.free()


def test_a_batch_equals_single_frame_calls(ctx, lib, chains):
    L = lib.lib()
    c = chains["140x132"]
    hp = hp_of(lib)
    ops = Operands(ctx, lib, c, frames=range(2))
    pl = PairPlane(ctx, c, qmap=True, pad=pad_of(c))
    assert fused_call(L, ctx, ops, pl.p, c, hp, lib.FUSED_ON, True, None) == 0
    ctx.synchronize()
    batch, clean = pl.read()
    assert clean and not np.array_equal(batch[0], batch[1])
    for f in range(2):
        o1 = Operands(ctx, lib, c, frames=[f])
        one = PairPlane(ctx, dict(c, bs=[c["bs"][f]]), frames=[c["planes"][f]], qmap=True, pad=pad_of(c))
        assert fused_call(L, ctx, o1, one.p, c, hp, lib.FUSED_ON, True, None) == 0
        ctx.synchronize()
        check(one, [batch[f]], ("batch", f))
        one.free()
        o1.free()
    pl.free()
    ops.free()


# ---- the whole picture -------------------------------------------------------------------------------------------------------------

def luma_of(c, seed):
    """a luma plane for the pair plane of chain case c: twice the size, the same QP map, slices and layout (one CTB grid), its own
    samples, bS, SAO parameters (CTBs twice as large) and keep map"""
    rng = np.random.default_rng(seed)
    w, h, depth, n = 2 * c["w"], 2 * c["h"], c["depth"], len(c["planes"])
    lg = c["lg"] + 1
    return {"w": w, "h": h, "depth": depth, "sb": c["sb"], "lw": lg, "lh": lg, "planes": [G.blocky_plane(w, h, depth, rng) for _ in range(n)],
            "bs": [G.random_bs(w, h, rng, p2=0.4) for _ in range(n)], "params": G.border_params(w, h, lg, lg, depth, n, rng),
            "keep": [G.keep_map(w, h, rng) for _ in range(n)]}


def luma_expected(y, c, qmap, extra):
    """the statement of test_gpu_g4.picture_expected for plane 0: (SAO parameters fitted to the deblocked frames, final frames)"""
    from oracle import h265
    mid = []
    for f in range(len(y["planes"])):
        vb, hb = y["bs"][f]
        m = c["qp_map"] if qmap else None
        if extra:
            mid.append(R.expected(y["planes"][f], vb, hb, c["pairs"], S.SL_CTB_LOG2, c_idx=0, qp=c["qp"], qp_map=m, unit_log2=S.UNIT_LOG2, bit_depth=y["depth"]))
        else:
            mid.append(h265.filter_plane(y["planes"][f], c["qp"], vb, hb, c_idx=0, bit_depth=y["depth"], qp_map=m, unit_log2=S.UNIT_LOG2,
                                         tc_offset_div2=S.TC_DIV2, beta_offset_div2=0))
        assert (mid[f] != y["planes"][f]).any()
    params = [p.copy() for p in y["params"]]
    G.fit_bands(mid, params, y["lw"], y["lh"], y["depth"])
    fin = [G.sao_direct(mid[f], params[f], y["lw"], y["lh"], bit_depth=y["depth"], keep=y["keep"][f], layout=c["layout"] if extra else None)
           for f in range(len(mid))]
    return params, fin


class Picture:
    """both planes of a semi-planar picture in HBM with their operands"""

    def __init__(self, ctx, lib, c, y, params, qmap, pitch_rest=0):
        from test_gpu_sao_borders import up
        self.lib, self.c = lib, c
        self.luma = LumaPlane(ctx, dict(y, qp_map=c["qp_map"] if qmap else None), chroma=False)
        self.pairs = PairPlane(ctx, c, qmap=qmap, pad=pad_of(c, pitch_rest))
        self.ops = Operands(ctx, lib, c, frames=range(2))
        rows, cols = params[0].shape
        kr, kc = y["keep"][0].shape
        self.dp, self.dk = up(ctx, np.stack(params)), up(ctx, np.stack(y["keep"]))
        self.sl = lib.SaoPlaneCf(self.dp.ptr, cols, rows * cols, y["lw"], y["lh"], self.dk.ptr, kc, kr * kc)
        o = self.ops
        self.sp = lib.SaoPlaneSp(o.pcb.ptr, o.pcr.ptr, o.cols, o.rows * o.cols, o.lg, o.keep.ptr, o.kc, o.kr * o.kc)
        self.so, self.dso = sl_operand(ctx, lib, c["pairs"])
        self.bo, self.dbo = borders_operand(ctx, lib, [c["layout"]])

    def nv12(self, ctx, hp, fused, extra, st=None):
        return self.lib.lib().hevcdbk_h265_deblock_sao_device_nv12(ctx.handle, C.byref(self.luma.p), C.byref(self.pairs.p), self.c["qp"], C.byref(hp),
                                                                   C.byref(self.sl), C.byref(self.sp), fused, C.byref(self.bo) if extra else None,
                                                                   C.byref(self.so) if extra else None, st)

    def planes_g4(self, ctx, hp, fused, extra, st=None):
        """the luma plane alone through the existing entry"""
        return self.lib.lib().hevcdbk_h265_deblock_sao_device_planes_g4(ctx.handle, C.byref(self.luma.p), 1, 1, self.c["qp"], C.byref(hp),
                                                                        C.byref(self.sl), fused, C.byref(self.bo) if extra else None,
                                                                        C.byref(self.so) if extra else None, st)

    def free(self):
        for x in (self.luma, self.pairs, self.ops, self.dp, self.dk, self.dso, self.dbo):
            x.free()


@pytest.mark.parametrize("name", ["136x136", "140x132_12", "140x132"])
def test_nv12(ctx, lib, chains, name):
    """Y 272x272 with pairs 136x136 (8 bit, luma CTBs of 64), Y 280x264 with pairs 140x132 at 12 and at 8 bit (luma CTBs of 32); with
    and without borders / slice_offsets, one QP and the map.  AUTO and ON: exactly one kernel, the frame kernel; OFF: the kernels
    the per-plane entries run.  Y = the _planes_g4 entry's result (GPU against GPU) = the reference statement; pairs = the expectation"""
    c = chains[name]
    y = luma_of(c, 7 + len(name))
    hp = hp_of(lib)
    for qmap in (False, True):
        for extra in (False, True):
            params, want_y = luma_expected(y, c, qmap, extra)
            want_c = [expected(c, f, qmap, extra, extra)[1] for f in range(2)]
            ref = Picture(ctx, lib, c, y, params, qmap)   # the luma plane alone through the existing entry
            assert ref.planes_g4(ctx, hp, lib.FUSED_AUTO, extra) == 0
            ctx.synchronize()
            g4_y, clean = ref.luma.dst.read()
            assert clean
            per_plane = captured(lambda st: ref.planes_g4(ctx, hp, lib.FUSED_OFF, extra, st))[1] + two_launches(c)
            ref.free()
            for fused in (lib.FUSED_AUTO, lib.FUSED_ON, lib.FUSED_OFF):
                pic = Picture(ctx, lib, c, y, params, qmap)
                rc, k = captured(lambda st: pic.nv12(ctx, hp, fused, extra, st))
                assert rc == 0 and k == ([MULTI] if fused != lib.FUSED_OFF else per_plane), (rc, k, fused)
                assert pic.nv12(ctx, hp, fused, extra) == 0
                ctx.synchronize()
                what = (name, qmap, extra, fused)
                check(pic.luma.dst, want_y, what + ("Y, the reference",))
                check(pic.luma.dst, g4_y, what + ("Y, the _planes_g4 entry",))
                check(pic.pairs, want_c, what + ("CbCr",))
                pic.free()


def test_nv12_plane_by_plane(ctx, lib, chains):
    """a pair plane the fused kernel refuses (its pitch): AUTO runs Y in its one-kernel form and the pairs in two launches; ON is
    refused with nothing enqueued.  Both planes at 14 bit: ON refused, AUTO plane by plane with the right pair bytes"""
    hp = hp_of(lib)
    c = chains["140x132"]
    y = luma_of(c, 11)
    params, want_y = luma_expected(y, c, True, True)
    pic = Picture(ctx, lib, c, y, params, True, pitch_rest=8)
    luma_alone = captured(lambda st: pic.planes_g4(ctx, hp, lib.FUSED_AUTO, True, st))[1]
    assert len(luma_alone) == 1
    assert captured(lambda st: pic.nv12(ctx, hp, lib.FUSED_AUTO, True, st)) == (0, luma_alone + [DBK_PACKED[1], SAO_GENERIC])
    assert captured(lambda st: pic.nv12(ctx, hp, lib.FUSED_ON, True, st)) == (lib.ERR_UNSUPPORTED, [])
    assert pic.nv12(ctx, hp, lib.FUSED_AUTO, True) == 0
    ctx.synchronize()
    check(pic.luma.dst, want_y, "Y beside a pair plane in two launches")
    check(pic.pairs, [expected(c, f, True, True, True)[1] for f in range(2)], "pairs in two launches beside Y")
    pic.free()
    c = chains["72x24_14"]
    y = luma_of(c, 12)
    pic = Picture(ctx, lib, c, y, y["params"], True)
    assert captured(lambda st: pic.nv12(ctx, hp, lib.FUSED_ON, False, st)) == (lib.ERR_UNSUPPORTED, [])
    rc, k = captured(lambda st: pic.nv12(ctx, hp, lib.FUSED_AUTO, False, st))
    assert rc == 0 and k[-2:] == [DBK_GENERIC, SAO_GENERIC] and MULTI not in k, (rc, k)
    assert pic.nv12(ctx, hp, lib.FUSED_AUTO, False) == 0
    ctx.synchronize()
    check(pic.pairs, [expected(c, f, True, False, False)[1] for f in range(2)], "14 bit")
    pic.free()


def test_two_streams(ctx, lib, chains):
    """an _nv12 picture and an _sp_fused plane on two caller streams, then the fallback route of both, alternating three times: the
    fused route touches no scratch plane, the fallback route fences it"""
    from kernel_capture import _hip
    hip = _hip()
    L = lib.lib()
    hp = hp_of(lib)
    c = chains["136x136"]
    y = luma_of(c, 13)
    params, want_y = luma_expected(y, c, True, False)
    want_c = [expected(c, f, True, False, True)[1] for f in range(2)]
    want_c0 = [expected(c, f, True, False, False)[1] for f in range(2)]
    streams = [C.c_void_p(), C.c_void_p()]
    for s in streams:
        assert hip.hipStreamCreate(C.byref(s)) == 0
    try:
        for fused in (lib.FUSED_AUTO, lib.FUSED_OFF):
            pic = Picture(ctx, lib, c, y, params, True)
            pl = PairPlane(ctx, c, qmap=True, pad=pad_of(c))
            for _ in range(3):
                assert pic.nv12(ctx, hp, fused, False, streams[0].value) == 0
                assert fused_call(L, ctx, pic.ops, pl.p, c, hp, fused, True, None, streams[1].value) == 0
            for s in streams:
                assert hip.hipStreamSynchronize(s) == 0
            check(pic.luma.dst, want_y, ("stream 0, Y", fused))
            check(pic.pairs, want_c0, ("stream 0, CbCr", fused))
            check(pl, want_c, ("stream 1", fused))
            pl.free()
            pic.free()
    finally:
        for s in streams:
            hip.hipStreamDestroy(s)


def test_python_entries(ctx, lib, chains):
    """Context.deblock_sao_h265_device(semi_planar=True, one_kernel=True) and Context.deblock_sao_nv12 on DeviceBatches"""
    from gpu_video_codec_amd import deblock
    from test_gpu_sao_borders import up
    c = chains["136x136"]   # a tight pitch of 272 bytes: a DeviceBatch's rows are whole row pieces
    y = luma_of(c, 14)
    params, want_y = luma_expected(y, c, False, False)
    ops = Operands(ctx, lib, c, frames=range(2))
    held = [up(ctx, np.stack([b[0] for b in c["bs"]])), up(ctx, np.stack([b[1] for b in c["bs"]])), up(ctx, np.stack([b[0] for b in y["bs"]])),
            up(ctx, np.stack([b[1] for b in y["bs"]])), up(ctx, np.stack(params)), up(ctx, np.stack(y["keep"]))]
    h265 = dict(tc_offset_div2=S.TC_DIV2, cb_qp_offset=S.CB_OFF, cr_qp_offset=S.CR_OFF)

    def pair_batch():
        b = deblock.DeviceBatch(ctx, c["w"], c["h"], 2, bit_depth=c["depth"], semi_planar=True)
        b.upload_all(np.stack(c["planes"]))
        p = b.planes()
        p.vert_bs, p.hor_bs, p.vert_bs_stride, p.hor_bs_stride = held[0].ptr, held[1].ptr, c["bs"][0][0].size, c["bs"][0][1].size
        return b, p

    b, p = pair_batch()
    ctx.deblock_sao_h265_device(p, c["qp"], ops.pcb.ptr, ops.cols, ops.lg, params_frame_stride=ops.rows * ops.cols, keep_ptr=ops.keep.ptr,
                                keep_stride=ops.kc, keep_frame_stride=ops.kr * ops.kc, fused=lib.FUSED_ON, borders=ops.borders, semi_planar=True,
                                params_cr_ptr=ops.pcr.ptr, one_kernel=True, **h265)
    ctx.synchronize()
    for f in range(2):
        assert np.array_equal(b.download_frame(f), expected(c, f, False, False, True)[1]), f
    b.free()

    b, p = pair_batch()
    yb = deblock.DeviceBatch(ctx, y["w"], y["h"], 2, bit_depth=y["depth"])
    yb.upload_all(np.stack(y["planes"]))
    yp = yb.planes()
    yp.vert_bs, yp.hor_bs, yp.vert_bs_stride, yp.hor_bs_stride = held[2].ptr, held[3].ptr, y["bs"][0][0].size, y["bs"][0][1].size
    rows, cols = params[0].shape
    kr, kc = y["keep"][0].shape
    ctx.deblock_sao_nv12(yp, p, c["qp"],
                         dict(params=held[4].ptr, params_stride=cols, params_frame_stride=rows * cols, ctb_log2=y["lw"], keep=held[5].ptr,
                              keep_stride=kc, keep_frame_stride=kr * kc),
                         dict(params_cb=ops.pcb.ptr, params_cr=ops.pcr.ptr, params_stride=ops.cols, params_frame_stride=ops.rows * ops.cols,
                              ctb_log2=ops.lg, keep=ops.keep.ptr, keep_stride=ops.kc, keep_frame_stride=ops.kr * ops.kc),
                         h265=h265, fused=lib.FUSED_ON)
    ctx.synchronize()
    for f in range(2):
        assert np.array_equal(yb.download_frame(f), want_y[f]), ("Y", f)
        assert np.array_equal(b.download_frame(f), expected(c, f, False, False, False)[1]), ("CbCr", f)
    for x in [b, yb, ops] + held:
        x.free()
