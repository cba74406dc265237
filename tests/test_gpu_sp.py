"""Semi-planar chroma -- one plane of interleaved Cb / Cr pairs, both components in one launch -- on the GPU through the _sp entry
of the C ABI, bit-exact against tests/sp_ref.py (the planar statements applied per component; test_sp_cpu.py asserts that every vector
bites in both components).  Every destination is pre-filled, has row padding, a gap between frames and guard rows before and after,
all of which must come back untouched.  The kernel that ran is read from a stream capture.  PARITY UNPINNED, like the rest of the
spec-exact mode."""
import ctypes as C

import numpy as np
import pytest

import sp_ref as S
from test_gpu_sao_borders import Surface, dev_planes, up

pytestmark = pytest.mark.gpu

PACKED_NAMES = {1: "dbk_packed_h265_sp_kernel", 2: "dbk_packed16_h265_sp_kernel"}


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


def names(k):
    from kernel_capture import parse_kernel
    return [parse_kernel(x[0])[0] for x in k]


def captured(call):
    from kernel_capture import kernels_enqueued
    rc, k = kernels_enqueued(call)
    return rc, names(k)


def row_pad(w, sb, mod=16, rest=0):
    """bytes of row padding such that the pitch of a row of 2 * w samples is `rest` modulo `mod`"""
    return 16 + (rest - (2 * w * sb + 16)) % mod


class PairPlane:
    """frames of interleaved pairs in HBM with their operands: src / dst surfaces (rows of 2 * w samples), per-frame bS at a tight
    stride, the QP map; planar=k: the planar surface of component k of the same frames instead"""

    def __init__(self, ctx, c, frames=None, in_place=False, pad=None, bs=True, qmap=False, planar=None):
        frames = c["planes"] if frames is None else frames
        self.n, self.h, self.w, self.sb = len(frames), c["h"], c["w"], c["sb"]
        self.planar = planar
        if planar is None:
            rows, rw = [np.ascontiguousarray(p).reshape(self.h, 2 * self.w) for p in frames], 2 * self.w
        else:
            rows, rw = [np.ascontiguousarray(p[..., planar]) for p in frames], self.w
        pad = (row_pad(self.w, self.sb) if planar is None else 16 + (-(self.w * self.sb)) % 16) if pad is None else pad
        self.src = Surface(ctx, self.n, self.h, rw, self.sb, pad, rows)
        self.dst = self.src if in_place else Surface(ctx, self.n, self.h, rw, self.sb, pad)
        self.bufs = []
        dv = dh = dm = None
        if bs:
            sel = range(self.n) if len(c["bs"]) >= self.n else [0] * self.n
            dv, dh = up(ctx, np.stack([c["bs"][f][0] for f in sel])), up(ctx, np.stack([c["bs"][f][1] for f in sel]))
            self.bufs += [dv, dh]
        if qmap:
            dm = up(ctx, c["qp_map"])
            self.bufs.append(dm)
        self.p = dev_planes(self.src, self.dst, c["depth"], True, dv, dh, dm, c["qp_map"].shape[1] if qmap else 0, S.UNIT_LOG2)
        self.p.plane_w = self.w
        if bs:
            self.p.vert_bs_stride, self.p.hor_bs_stride = c["bs"][0][0].size, c["bs"][0][1].size

    def read(self):
        got, clean = self.dst.read()
        return [g.reshape(self.h, self.w, 2) if self.planar is None else g for g in got], clean

    def free(self):
        for x in {self.src, self.dst} | set(self.bufs):
            x.free()


def check(pl, want, what):
    got, clean = pl.read()
    assert clean, ("bytes outside the frames were written", what)
    for f, w in enumerate(want):
        assert np.array_equal(got[f], w), (what, f, int((got[f] != w).sum()), np.argwhere(got[f] != w)[:4].tolist())


def hp_of(lib):
    return lib.H265Params(S.TC_DIV2, 0, S.CB_OFF, S.CR_OFF)


def sl_operand(ctx, lib, pairs):
    d = up(ctx, pairs)
    return lib.SliceOffsets(d.ptr, pairs.shape[1], 0, S.SL_CTB_LOG2), d


# ---- deblocking ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spec", S.DBK, ids=lambda s: s[0])
def test_filter_device(ctx, lib, spec):
    """two frames with per-frame bS; {GENERIC, PACKED, AUTO} x {one QP, a map per 8 x 8} x {with, without slice_offsets} x {out of
    place, in place}: every combination"""
    L = lib.lib()
    c = S.dbk_case(spec)
    so, dso = sl_operand(ctx, lib, c["pairs"])
    hp = hp_of(lib)
    packs = c["depth"] <= 12
    for qmap in (False, True):
        for sl in (False, True):
            want = [S.dbk_expected(c, f, qmap, sl) for f in range(2)]
            assert S.dbk_census_ok(c, S.dbk_census(c, 0, qmap, sl, want[0])), "the vector does not bite"
            for variant in (lib.KERNEL_GENERIC, lib.KERNEL_PACKED, lib.KERNEL_AUTO):
                for in_place in (False, True):
                    pl = PairPlane(ctx, c, in_place=in_place, qmap=qmap)
                    call = lambda st: L.hevcdbk_h265_filter_device_sp(ctx.handle, C.byref(pl.p), c["qp"], C.byref(hp), variant,
                                                                     C.byref(so) if sl else None, st)
                    rc, k = captured(call)
                    if variant == lib.KERNEL_PACKED and not packs:
                        assert rc == lib.ERR_UNSUPPORTED and k == [], (rc, k)
                    else:
                        assert rc == 0 and k == ["dbk_h265_sp_kernel" if variant == lib.KERNEL_GENERIC or not packs else PACKED_NAMES[c["sb"]]], (rc, k)
                        assert call(None) == 0
                        ctx.synchronize()
                        check(pl, want, (spec[0], qmap, sl, variant, in_place))
                    pl.free()
    dso.free()


def test_dispatch_guards_of_the_packed_kernels(ctx, lib):
    """each alignment / width / depth guard, on both sides, by kernel name; the 32-bit kernel's bytes on a plane the packed kernels
    refuse"""
    L = lib.lib()
    hp = hp_of(lib)
    GEN = "dbk_h265_sp_kernel"

    def probe(c, pl):
        out = []
        for variant in (lib.KERNEL_AUTO, lib.KERNEL_PACKED):
            out.append(captured(lambda st: L.hevcdbk_h265_filter_device_sp(ctx.handle, C.byref(pl.p), c["qp"], C.byref(hp), variant, None, st)))
        return out

    def expect(c, pl, packed, what):
        auto, forced = probe(c, pl)
        if packed:
            assert auto == (0, [PACKED_NAMES[c["sb"]]]) and forced == auto, (what, auto, forced)
        else:
            assert auto == (0, [GEN]) and forced == (lib.ERR_UNSUPPORTED, []), (what, auto, forced)

    # pitch: half a block's row -- 8 bytes (8 bit), 16 bytes (16 bit); one 4-sample word is what every kernel needs
    for spec, mod in ((S.DBK[0], 8), (S.DBK[5], 16)):
        c = S.dbk_case(spec)
        for rest, packed in ((0, True), (mod // 2, False)):
            pl = PairPlane(ctx, c, pad=row_pad(c["w"], c["sb"], mod, rest))
            assert pl.p.pitch % mod == rest
            expect(c, pl, packed, ("pitch", spec[0], rest))
            if not packed:   # the bytes of the kernel that took the plane
                assert L.hevcdbk_h265_filter_device_sp(ctx.handle, C.byref(pl.p), c["qp"], C.byref(hp), lib.KERNEL_AUTO, None, None) == 0
                ctx.synchronize()
                check(pl, [S.dbk_expected(c, f, False, False) for f in range(2)], ("32-bit kernel", spec[0]))
            pl.free()
        # the plane addresses and the frame stride
        for field in ("src", "dst", "frame_stride"):
            pl = PairPlane(ctx, c)
            setattr(pl.p, field, getattr(pl.p, field) + mod // 2)
            expect(c, pl, False, (field, spec[0]))
            pl.free()
    # depth: 12 bit is packed, 14 bit is not
    for depth, packed in ((12, True), (14, False)):
        c = S.dbk_case(("d%d" % depth, 16, 16, depth))
        pl = PairPlane(ctx, c)
        expect(c, pl, packed, ("depth", depth))
        pl.free()
    # width: 1024 blocks per row are one workgroup, 1025 are not
    for w, packed in ((8188, True), (8192, False)):
        c = S.dbk_case(("w%d" % w, w, 8, 8), frames=1)
        pl = PairPlane(ctx, c)
        expect(c, pl, packed, ("width", w))
        pl.free()
    # the row map only
    c = S.dbk_case(S.DBK[0])
    pl = PairPlane(ctx, c)
    for m, rc in ((lib.MAP_ROWS, 0), (lib.MAP_LINEAR, lib.ERR_UNSUPPORTED)):
        got = captured(lambda st: L.hevcdbk_h265_filter_device_sp(ctx.handle, C.byref(pl.p), c["qp"], C.byref(hp), lib.KERNEL_PACKED | m, None, st))
        assert got[0] == rc and len(got[1]) == (1 if rc == 0 else 0), (m, got)
    pl.free()


# ---- metamorphic: no oracle -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spec", [S.DBK[4], S.DBK[5]], ids=lambda s: s[0])
def test_deblocking_equals_the_planar_entry_on_the_split_planes(ctx, lib, spec):
    L = lib.lib()
    c = S.dbk_case(spec)
    so, dso = sl_operand(ctx, lib, c["pairs"])
    hp = hp_of(lib)
    pl = PairPlane(ctx, c, qmap=True)
    assert L.hevcdbk_h265_filter_device_sp(ctx.handle, C.byref(pl.p), c["qp"], C.byref(hp), lib.KERNEL_AUTO, C.byref(so), None) == 0
    ctx.synchronize()
    got, clean = pl.read()
    assert clean
    for k in range(2):
        pk = PairPlane(ctx, c, qmap=True, planar=k)
        assert L.hevcdbk_h265_filter_device_g4(ctx.handle, C.byref(pk.p), 1 + k, 1, c["qp"], C.byref(hp), lib.KERNEL_AUTO, C.byref(so), None) == 0
        ctx.synchronize()
        planar, clean = pk.read()
        assert clean
        for f in range(2):
            assert np.array_equal(got[f][..., k], planar[f]), (spec[0], k, f)
            assert (planar[f] != c["planes"][f][..., k]).any()
        pk.free()
    pl.free()
    dso.free()


def test_a_batch_equals_single_frame_calls(ctx, lib):
    """per-frame bS at a tight stride: frame f of the batch = a call on frame f alone with frame f's arrays"""
    L = lib.lib()
    hp = hp_of(lib)
    c = S.dbk_case(S.DBK[4])
    pl = PairPlane(ctx, c)
    assert L.hevcdbk_h265_filter_device_sp(ctx.handle, C.byref(pl.p), c["qp"], C.byref(hp), lib.KERNEL_AUTO, None, None) == 0
    ctx.synchronize()
    batch, clean = pl.read()
    assert clean and not np.array_equal(batch[0], batch[1])
    for f in range(2):
        one = PairPlane(ctx, dict(c, bs=[c["bs"][f]]), frames=[c["planes"][f]])
        assert L.hevcdbk_h265_filter_device_sp(ctx.handle, C.byref(one.p), c["qp"], C.byref(hp), lib.KERNEL_AUTO, None, None) == 0
        ctx.synchronize()
        check(one, [batch[f]], ("deblocking", f))
        one.free()
    pl.free()
