"""SAO and deblocking + SAO of a semi-planar chroma plane -- one plane of interleaved Cb / Cr pairs, both components in one launch,
each with its own CTB parameters -- on the GPU through the _sp SAO entries of the C ABI, bit-exact against tests/sao_sp_ref.py (the
planar statements applied per component; test_sao_sp_cpu.py asserts that every vector bites in both components).  Every destination is
pre-filled, has row padding, a gap between frames and guard rows before and after, all of which must come back untouched.  The kernel
that ran is read from a stream capture.  PARITY UNPINNED, like the rest of the spec-exact mode."""
import ctypes as C

import numpy as np
import pytest

import sao_borders_ref as B
import sao_sp_ref as P
import sp_ref as S
from test_gpu_sao_borders import up
from test_gpu_sp import PACKED_NAMES as DBK_PACKED, PairPlane, captured, check, hp_of, row_pad, sl_operand

pytestmark = pytest.mark.gpu

PACKED = {1: "sao8_sp_kernel", 2: "sao16_sp_kernel"}
GENERIC = "sao_sp_kernel"
PIECE = {1: 16, 2: 32}   # a lane's row piece in bytes: what the packed kernels want pitch, frame stride and addresses aligned to


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
def cases():
    return {spec[0]: P.case(spec) for spec in P.VECTORS}


def sao_name(c):
    return PACKED[c["sb"]] if c["depth"] <= 12 else GENERIC


def pad_of(c, rest=0):
    return row_pad(c["w"], c["sb"], PIECE[c["sb"]], rest)


class Operands:
    """both components' parameters, the keep maps (per frame, tight strides) and the boundary bytes of ONE layout for every frame;
    nox: bytes of the caller's own instead, (frames, rows, stride), one array per frame"""

    def __init__(self, ctx, lib, c, frames=None, nox=None):
        frames = range(len(c["pcb"])) if frames is None else frames
        self.rows, self.cols = c["pcb"][0].shape
        self.kr, self.kc = c["keep"][0].shape
        self.pcb, self.pcr = up(ctx, np.stack([c["pcb"][f] for f in frames])), up(ctx, np.stack([c["pcr"][f] for f in frames]))
        self.keep = up(ctx, np.stack([c["keep"][f] for f in frames]))
        per_frame = nox is not None
        nox = np.ascontiguousarray(np.stack([nox[f] for f in frames]) if per_frame else B.expected_nox(c["layout"]), np.uint8)
        self.nox = up(ctx, nox)
        self.borders = lib.SaoBorders(self.nox.ptr, nox.shape[-1], nox.shape[1] * nox.shape[2] if per_frame else 0)
        self.lg = c["lg"]

    def sao(self, L, ctx, p, keep, borders, stream=None, pcb=None, pcr=None):
        return L.hevcdbk_sao_filter_device_sp(ctx.handle, C.byref(p), pcb or self.pcb.ptr, pcr or self.pcr.ptr, self.cols, self.rows * self.cols,
                                              self.lg, self.keep.ptr if keep else None, self.kc, self.kr * self.kc if keep else 0,
                                              C.byref(self.borders) if borders else None, stream)

    def chain(self, L, ctx, p, qp, hp, fused, borders, so, stream=None):
        return L.hevcdbk_h265_deblock_sao_device_sp(ctx.handle, C.byref(p), qp, C.byref(hp), self.pcb.ptr, self.pcr.ptr, self.cols,
                                                    self.rows * self.cols, self.lg, self.keep.ptr, self.kc, self.kr * self.kc, fused,
                                                    C.byref(self.borders) if borders else None, so, stream)

    def free(self):
        for x in (self.pcb, self.pcr, self.keep, self.nox):
            x.free()


# ---- SAO --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spec", P.VECTORS, ids=lambda s: s[0])
def test_sao_device(ctx, lib, cases, spec):
    """five frames with per-frame parameters of both components in one call; {no keep map, keep map} x {no borders, the layout}"""
    L = lib.lib()
    c = cases[spec[0]]
    ops = Operands(ctx, lib, c)
    for keep in (False, True):
        for borders in (False, True):
            want = [P.expected(c, f, keep=keep, layout=c["layout"] if borders else None) for f in range(P.FRAMES)]
            pl = PairPlane(ctx, c, bs=False, pad=pad_of(c))
            rc, k = captured(lambda st: ops.sao(L, ctx, pl.p, keep, borders, st))
            assert rc == 0 and k == [sao_name(c)], (rc, k)
            assert ops.sao(L, ctx, pl.p, keep, borders) == 0
            ctx.synchronize()
            check(pl, want, (spec[0], keep, borders))
            pl.free()
    ops.free()


def test_dispatch_guards_of_the_packed_kernels(ctx, lib, cases):
    """each guard on both sides, by kernel name; the per-sample kernel's bytes on a plane the packed kernels refuse"""
    L = lib.lib()
    for name in ("140x132", "140x132_12"):
        c = cases[name]
        sb, piece = c["sb"], PIECE[c["sb"]]
        ops = Operands(ctx, lib, c)
        probe = lambda pl: captured(lambda st: ops.sao(L, ctx, pl.p, True, True, st))
        for rest, packed in ((0, True), (piece // 2, False)):
            pl = PairPlane(ctx, c, bs=False, pad=pad_of(c, rest))
            assert pl.p.pitch % piece == rest
            assert probe(pl) == (0, [PACKED[sb] if packed else GENERIC]), ("pitch", name, rest)
            if not packed:   # the bytes of the kernel that took the plane
                assert ops.sao(L, ctx, pl.p, True, True) == 0
                ctx.synchronize()
                check(pl, [P.expected(c, f, keep=True, layout=c["layout"]) for f in range(P.FRAMES)], ("per-sample kernel", name))
            pl.free()
        for field in ("src", "dst", "frame_stride"):
            pl = PairPlane(ctx, c, bs=False, pad=pad_of(c))
            setattr(pl.p, field, getattr(pl.p, field) + piece // 2)
            assert probe(pl) == (0, [GENERIC]), (field, name)
            pl.free()
        ops.free()
    # depth: 12 bit is packed, 14 bit is not (max_v / band_shift)
    assert sao_name(cases["140x132_12"]) == PACKED[2] and sao_name(cases["72x24_14"]) == GENERIC   # asserted by name in test_sao_device
    # pitch * plane_h < 2^31: captured only, never run -- no such plane is allocated
    c = cases["16x16"]
    ops = Operands(ctx, lib, c)
    pl = PairPlane(ctx, c, bs=False, pad=pad_of(c))
    for pitch, packed in (((1 << 27) - 16, True), (1 << 27, False)):
        pl.p.pitch, pl.p.frame_stride, pl.p.n_frames = pitch, pitch * 16, 1
        got = captured(lambda st: ops.sao(L, ctx, pl.p, False, False, st))
        assert got == (0, [PACKED[1] if packed else GENERIC]), (pitch, got)
    pl.free()
    ops.free()


@pytest.mark.parametrize("name", ["140x132", "264x136_10"])
def test_sao_equals_the_planar_entry_on_the_split_planes(ctx, lib, cases, name):
    """no reference: per component, hevcdbk_sao_filter_device_g4 on the split plane with that component's parameters"""
    L = lib.lib()
    c = cases[name]
    ops = Operands(ctx, lib, c)
    pl = PairPlane(ctx, c, bs=False, pad=pad_of(c))
    assert ops.sao(L, ctx, pl.p, True, True) == 0
    ctx.synchronize()
    got, clean = pl.read()
    assert clean
    for k, prm in enumerate((ops.pcb, ops.pcr)):
        pk = PairPlane(ctx, c, bs=False, planar=k)
        assert L.hevcdbk_sao_filter_device_g4(ctx.handle, C.byref(pk.p), prm.ptr, ops.cols, ops.rows * ops.cols, ops.lg, ops.lg, ops.keep.ptr,
                                              ops.kc, ops.kr * ops.kc, C.byref(ops.borders), None) == 0
        ctx.synchronize()
        planar, clean = pk.read()
        assert clean
        for f in range(P.FRAMES):
            assert np.array_equal(got[f][..., k], planar[f]), (name, k, f)
            assert (planar[f] != c["planes"][f][..., k]).any()
        pk.free()
    pl.free()
    ops.free()


def test_a_batch_equals_single_frame_calls(ctx, lib, cases):
    L = lib.lib()
    c = cases["140x132"]
    ops = Operands(ctx, lib, c)
    pl = PairPlane(ctx, c, bs=False, pad=pad_of(c))
    assert ops.sao(L, ctx, pl.p, True, True) == 0
    ctx.synchronize()
    batch, clean = pl.read()
    assert clean and not np.array_equal(batch[0], batch[1])
    for f in (0, 3):
        o1 = Operands(ctx, lib, c, frames=[f])
        one = PairPlane(ctx, c, frames=[c["planes"][f]], bs=False, pad=pad_of(c))
        assert o1.sao(L, ctx, one.p, True, True) == 0
        ctx.synchronize()
        check(one, [batch[f]], ("SAO", f))
        one.free()
        o1.free()
    pl.free()
    ops.free()


# ---- the chain ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def chains():
    return {name: P.chain_case(P.spec_of(name)) for name in P.CHAIN}


@pytest.mark.parametrize("name", P.CHAIN)
def test_deblock_sao_device(ctx, lib, chains, name):
    """one QP and a map, the keep map; with and without slice_offsets and borders; exactly one _sp deblocking kernel and one _sp SAO
    kernel; FUSED_OFF the same, FUSED_ON refused with nothing enqueued"""
    L = lib.lib()
    c = chains[name]
    hp = hp_of(lib)
    so, dso = sl_operand(ctx, lib, c["pairs"])
    ops = Operands(ctx, lib, c, frames=range(2))
    for sl in (False, True):
        for borders in (False, True):
            pairs = [P.chain_expected(c, f, sl, c["layout"] if borders else None) for f in range(2)]
            for f in range(2):   # both stages do something
                assert (pairs[f][0] != c["planes"][f]).any() and (pairs[f][1] != pairs[f][0]).any()
            for fused in (lib.FUSED_AUTO, lib.FUSED_OFF):
                pl = PairPlane(ctx, c, qmap=True, pad=pad_of(c))
                call = lambda st: ops.chain(L, ctx, pl.p, c["qp"], hp, fused, borders, C.byref(so) if sl else None, st)
                rc, k = captured(call)
                assert rc == 0 and k == [DBK_PACKED[c["sb"]], sao_name(c)], (rc, k)
                assert call(None) == 0
                ctx.synchronize()
                check(pl, [p[1] for p in pairs], (name, sl, borders, fused))
                pl.free()
    pl = PairPlane(ctx, c, qmap=True, pad=pad_of(c))
    got = captured(lambda st: ops.chain(L, ctx, pl.p, c["qp"], hp, lib.FUSED_ON, False, None, st))
    assert got == (lib.ERR_UNSUPPORTED, []), got
    pl.free()
    ops.free()
    dso.free()


def test_two_chains_on_two_streams_share_the_scratch(ctx, lib, chains):
    """the deblocked plane goes through ONE scratch buffer of the context: two calls on two streams, then both results"""
    from kernel_capture import _hip
    hip = _hip()
    L = lib.lib()
    c = chains["136x136"]
    hp = hp_of(lib)
    ops = Operands(ctx, lib, c, frames=range(2))
    want = [P.chain_expected(c, f, False, c["layout"])[1] for f in range(2)]
    streams = [C.c_void_p(), C.c_void_p()]
    for s in streams:
        assert hip.hipStreamCreate(C.byref(s)) == 0
    try:
        pls = [PairPlane(ctx, c, qmap=True, pad=pad_of(c)) for _ in streams]
        for _ in range(3):
            for s, pl in zip(streams, pls):
                assert ops.chain(L, ctx, pl.p, c["qp"], hp, lib.FUSED_AUTO, True, None, s.value) == 0
        for s in streams:
            assert hip.hipStreamSynchronize(s) == 0
        for i, pl in enumerate(pls):
            check(pl, want, ("stream", i))
            pl.free()
    finally:
        for s in streams:
            hip.hipStreamDestroy(s)
    ops.free()


def test_python_entries(ctx, lib, cases):
    """Context.sao_device(semi_planar=True) on a DeviceBatch(semi_planar=True)"""
    from gpu_video_codec_amd import deblock
    c = cases["140x132"]
    ops = Operands(ctx, lib, c)
    b = deblock.DeviceBatch(ctx, c["w"], c["h"], P.FRAMES, bit_depth=c["depth"], semi_planar=True)
    b.upload_all(np.stack(c["planes"]))
    ctx.sao_device(b.planes(), ops.pcb.ptr, ops.cols, ops.lg, params_frame_stride=ops.rows * ops.cols, keep_ptr=ops.keep.ptr, keep_stride=ops.kc,
                   keep_frame_stride=ops.kr * ops.kc, borders=ops.borders, semi_planar=True, params_cr_ptr=ops.pcr.ptr)
    ctx.synchronize()
    for f in range(P.FRAMES):
        assert np.array_equal(b.download_frame(f), P.expected(c, f, keep=True, layout=c["layout"])), f
    b.free()
    ops.free()
