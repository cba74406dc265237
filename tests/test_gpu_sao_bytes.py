"""The boundary-byte operand of SAO (hevcdbk_sao_borders.nox) as the C ABI defines it -- one ARBITRARY byte per CTB, never
reconciled with the neighbour's -- on the GPU through every entry that takes it, bit-exact against the by-byte statement
tests/sao_borders_ref.py: sao_plane_by_bytes, on the vectors of tests/sao_bytes_vectors.py: every (byte value, edge class) pair on
an interior CTB, rim CTBs whose bits point outside the picture, a byte array wider than the CTB columns with poison beyond,
per-frame bytes in the batches.  test_sao_bytes_cpu.py shows on the reference alone that every bit a class looks at changes every
interior CTB's output, so a kernel that mishandled one (byte, class) pair fails here.  Every destination is pre-filled, has row
padding, a gap between frames and guard rows, all of which must come back untouched.  PARITY UNPINNED, like the rest of the
spec-exact mode."""
import ctypes as C

import numpy as np
import pytest

import g4_ref as G
import rext_oracle as rx
import sao_borders_ref as R
import sao_bytes_vectors as V
from test_gpu_sao_borders import Surface, dev_planes, up

pytestmark = pytest.mark.gpu

CF = {"420": 1, "422": 2, "444": 3}
HP = dict(tc_offset_div2=1, beta_offset_div2=-1, cb_qp_offset=3, cr_qp_offset=-2)
QP = 36


@pytest.fixture(scope="module")
def h265():
    from oracle import h265 as h
    return h


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


def row_pad(w, sb, aligned=True):
    """bytes of row padding: a pitch that is a multiple of 8 (the packed 8-bit SAO kernel's condition), or one that is not"""
    p = 16 + (-(w * sb) % 8)
    return p if aligned else p + 4 * sb


class Operands:
    """a vector's planes and operands in HBM: source and pre-filled destination surfaces, parameters (params: others on the same
    grid, refitted to deblocked planes), keep map, bS arrays and QP map where given, the vector's bytes (borders) and a byte array
    of the same shape that forbids nothing (zero_borders)"""

    def __init__(self, ctx, lib, c, *, aligned=True, chroma=False, bs=None, qp_map=None, params=None):
        self.c, self.n = c, len(c["planes"])
        pad = row_pad(c["w"], c["sb"], aligned)
        self.src = Surface(ctx, self.n, c["h"], c["w"], c["sb"], pad, c["planes"])
        self.dst = Surface(ctx, self.n, c["h"], c["w"], c["sb"], pad)
        self.bufs = [self.src, self.dst]
        rows, cols = c["rows"], c["cols"]
        dp = up(ctx, np.stack(c["params"] if params is None else params))
        self.bufs.append(dp)
        dk = None
        if c["keeps"] is not None:
            dk = up(ctx, np.stack(c["keeps"]))
            self.bufs.append(dk)
        kr, kc = c["h"] // 8, c["w"] // 8
        # the arguments between `planes` and `borders` of the single-plane SAO entries
        self.sao_args = (dp.ptr, cols, rows * cols, c["lw"], c["lh"], dk.ptr if dk else None, kc if dk else 0, kr * kc if dk else 0)
        self.sao_plane = lib.SaoPlaneCf(dp.ptr, cols, rows * cols, c["lw"], c["lh"], dk.ptr if dk else None, kc if dk else 0, kr * kc if dk else 0)
        dv = dh = dm = None
        if bs is not None:
            dv, dh = up(ctx, bs[0]), up(ctx, bs[1])
            self.bufs += [dv, dh]
        if qp_map is not None:
            dm = up(ctx, qp_map)
            self.bufs.append(dm)
        self.p = dev_planes(self.src, self.dst, c["depth"], chroma, dv, dh, dm, 0 if qp_map is None else qp_map.shape[1], 3)
        nox = c["nox"]
        dn, dz = up(ctx, nox), up(ctx, np.zeros_like(nox))
        self.bufs += [dn, dz]
        fs = nox.shape[1] * nox.shape[2] if self.n > 1 else 0      # per-frame bytes in every batch
        self.borders, self.zero_borders = lib.SaoBorders(dn.ptr, nox.shape[2], fs), lib.SaoBorders(dz.ptr, nox.shape[2], fs)

    def check(self, want, what):
        got, clean = self.dst.read()
        assert clean, ("bytes outside the frames were written", what)
        for f in range(self.n):
            assert np.array_equal(got[f], want[f]), (what, f, int((got[f] != want[f]).sum()), np.argwhere(got[f] != want[f])[:4].tolist())

    def free(self):
        for x in self.bufs:
            x.free()


def run_and_check(ctx, ops, call, want, free, what, null_too):
    """call(borders or None, stream): with the vector's bytes against `want`; with no operand and with bytes of zero (null_too) against
    `free`, the border-less oracle"""
    for o in ops:
        o.dst.refill()
    assert call(C.byref(ops[0].borders), None) == 0, what
    ctx.synchronize()
    for o, w in zip(ops, want):
        o.check(w, what)
    if null_too:
        for b, tag in ((None, "no operand"), (C.byref(ops[0].zero_borders), "bytes of zero")):
            for o in ops:
                o.dst.refill()
            assert call(b, None) == 0, (what, tag)
            ctx.synchronize()
            for o, w in zip(ops, free):
                o.check(w, (what, tag))


def expected(name):
    return [V.expected(name, f) for f in range(len(V.case(name)["planes"]))]


def border_less(name):
    return [V.free(name, f) for f in range(len(V.case(name)["planes"]))]


def is_g4(c):
    return bool(c["w"] % 8 or c["h"] % 8)


# ---- 1. the SAO pass ------------------------------------------------------------------------------------------------------------------

def _cut(name):      # from the vector's description: the planes are not built at collection time
    return bool(V.CASES[name][2].get("cut_w") or V.CASES[name][2].get("cut_h"))


PITCH4 = ["every_8b_ctb8", "every_8b_ctb16", "every_8b_ctb32", "every_8b_ctb64", "every_8b_ctb8x16", "mixed_8b"]
SAO_PASS = [(n, True) for n in V.CASES if not _cut(n)] + [(n, False) for n in PITCH4]
NULL_TOO = {"every_8b_ctb16", "every_10b_ctb32", "every_8b_ctb8x16", "mixed_8b", "every_8b_g4_ctb8", "every_10b_g4_ctb16"}


@pytest.mark.parametrize("name,aligned", SAO_PASS, ids=["%s%s" % (n, "" if a else "_pitch4") for n, a in SAO_PASS])
def test_sao_pass(ctx, lib, name, aligned):
    """hevcdbk_sao_filter_device_nox: the packed 8-bit kernel (pitch a multiple of 8), the 32-bit one (another pitch), 16-bit
    containers; CTBs twice as tall as wide through the rewrite of parameters AND of arbitrary bytes"""
    from kernel_capture import kernels_enqueued
    L = lib.lib()
    c = V.case(name)
    o = Operands(ctx, lib, c, aligned=aligned)
    call = lambda b, st: L.hevcdbk_sao_filter_device_nox(ctx.handle, C.byref(o.p), *o.sao_args, b, st)
    run_and_check(ctx, [o], call, [expected(name)], [border_less(name)], (name, aligned), name in NULL_TOO and aligned)
    rc, k = kernels_enqueued(lambda st: call(C.byref(o.borders), st))
    assert rc == 0 and names(k)[-1] == ("sao8_nox_kernel" if c["sb"] == 1 and aligned else "sao_nox_kernel"), names(k)
    tall = c["lh"] != c["lw"]
    assert ("sao_nox_rows_x2_kernel" in names(k)) == tall and ("sao_rows_x2_kernel" in names(k)) == tall, names(k)
    o.free()


# ---- 2. deblocking + SAO of one plane -------------------------------------------------------------------------------------------------

def luma_operands(h265, c, mode, seed):
    """bS arrays and QP map of a luma plane: all zero / none ("bs0": deblocking changes nothing), or random with a QP map ("bs")"""
    w, h = c["w"], c["h"]
    if mode == "bs0":
        return (np.zeros(G.num_vert_bs(w, h), np.uint8), np.zeros(G.num_hor_bs(w, h), np.uint8)), None
    vb, hb = h265.derive_bs(*h265.random_units(w, h, seed=seed), w, h)
    assert vb.size == G.num_vert_bs(w, h) and hb.size == G.num_hor_bs(w, h)
    return (vb, hb), np.random.default_rng(seed).integers(22, 50, (h // 8, w // 8)).astype(np.uint8)


def after_deblocking(c, mids):
    """expected SAO results of the deblocked planes: parameters refitted to them (g4_ref.fit_bands), then the by-byte statement;
    (parameters, expected, border-less)"""
    params = [p.copy() for p in c["params"]]
    G.fit_bands(mids, params, c["lw"], c["lh"], c["depth"])
    want = [R.sao_plane_by_bytes(mids[f], params[f], c["lw"], c["lh"], c["nox"][f], bit_depth=c["depth"], keep=V.keep_of(c, f))
            for f in range(len(mids))]
    free = [rx.sao_plane(mids[f], params[f], c["lw"], c["lh"], bit_depth=c["depth"], keep=V.keep_of(c, f)) for f in range(len(mids))]
    return params, want, free


@pytest.mark.parametrize("mode", ["bs0", "bs"])
@pytest.mark.parametrize("name", ["every_8b_ctb16", "every_8b_ctb32", "every_8b_ctb64", "every_10b_ctb16", "every_10b_ctb32", "every_10b_ctb64"])
def test_deblock_sao_plane(ctx, lib, h265, name, mode):
    """hevcdbk_h265_deblock_sao_device_nox, the fused kernel and the two launches; 32-sample CTBs take the 2-row lanes"""
    L = lib.lib()
    c = V.case(name)
    bs, qmap = luma_operands(h265, c, mode, 5 + c["lw"])
    if mode == "bs0":
        params, want, free = None, expected(name), border_less(name)
    else:
        mids = [h265.filter_plane(p, QP, bs[0], bs[1], bit_depth=c["depth"], qp_map=qmap, unit_log2=3, tc_offset_div2=1, beta_offset_div2=-1)
                for p in c["planes"]]
        assert any((m != p).any() for m, p in zip(mids, c["planes"]))
        params, want, free = after_deblocking(c, mids)
    o = Operands(ctx, lib, c, bs=bs, qp_map=qmap, params=params)
    hp = lib.H265Params(**HP)
    for fused in (lib.FUSED_ON, lib.FUSED_OFF):
        call = lambda b, st: L.hevcdbk_h265_deblock_sao_device_nox(ctx.handle, C.byref(o.p), 0, 1, QP, C.byref(hp), *o.sao_args, fused, b, st)
        run_and_check(ctx, [o], call, [want], [free], (name, mode, fused), name == "every_8b_ctb32" or (name == "every_10b_ctb16" and mode == "bs0"))
    o.free()


# ---- 3. Y + Cb + Cr in one launch ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["bs0", "bs"])
@pytest.mark.parametrize("luma,fmt", [("every_8b_ctb16", "420"), ("every_8b_ctb16", "422"), ("every_8b_ctb16", "444"), ("every_10b_ctb32", "420")])
def test_deblock_sao_planes(ctx, lib, h265, luma, fmt, mode):
    """hevcdbk_h265_deblock_sao_device_planes_nox: ONE byte array serves the three planes, the chroma planes with the sub-sampled
    CTB size (4:2:2: CTBs twice as tall as wide)"""
    L = lib.lib()
    cf = CF[fmt]
    cases = [V.case(luma), V.case("%s_cb%s" % (luma, fmt)), V.case("%s_cr%s" % (luma, fmt))]
    y = cases[0]
    sx, sy = rx.SUB[cf]
    assert all(np.array_equal(c["nox"], y["nox"]) and (c["w"], c["h"]) == (y["w"] // sx, y["h"] // sy) for c in cases[1:])
    bs_y, _ = luma_operands(h265, y, mode, 9 + cf)
    bs_c = rx.chroma_bs(bs_y[0], bs_y[1], y["w"], y["h"], cf)
    ops, want, free = [], [], []
    for i, c in enumerate(cases):
        bs = bs_y if i == 0 else bs_c
        if mode == "bs0":
            params, w_, f_ = None, expected(c["name"]), border_less(c["name"])
        else:
            if i == 0:
                mids = [h265.filter_plane(p, QP, bs[0], bs[1], bit_depth=c["depth"], tc_offset_div2=1, beta_offset_div2=-1) for p in c["planes"]]
            else:
                mids = [rx.filter_chroma_plane(p, bs[0], bs[1], cf, qp=QP, bit_depth=c["depth"], tc_offset_div2=1, c_qp_offset=3 if i == 1 else -2)
                        for p in c["planes"]]
            params, w_, f_ = after_deblocking(c, mids)
        ops.append(Operands(ctx, lib, c, chroma=i > 0, bs=bs, params=params))
        want.append(w_)
        free.append(f_)
    arr = (lib.DevicePlanes * 3)(*[o.p for o in ops])
    sp = (lib.SaoPlaneCf * 3)(*[o.sao_plane for o in ops])
    hp = lib.H265Params(**HP)
    for fused in (lib.FUSED_ON, lib.FUSED_OFF):
        call = lambda b, st: L.hevcdbk_h265_deblock_sao_device_planes_nox(ctx.handle, arr, 3, cf, QP, C.byref(hp), sp, fused, b, st)
        run_and_check(ctx, ops, call, want, free, (luma, fmt, mode, fused), fmt in ("420", "422") and mode == "bs0" and fused == lib.FUSED_ON)
    for o in ops:
        o.free()


# ---- 4. planes whose last CTB column / row is cut to a multiple of 4 ---------------------------------------------------------------------

G4 = [("every_8b_g4_ctb8", 1), ("every_10b_g4_ctb16", 1), ("every_8b_g4_ctb8x16", 2)]


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("name,cf", G4)
def test_sao_pass_g4(ctx, lib, name, cf, aligned):
    """hevcdbk_sao_filter_device_g4: arbitrary bytes, those of the cut CTBs pointing outside"""
    from kernel_capture import kernels_enqueued
    L = lib.lib()
    c = V.case(name)
    assert is_g4(c)
    o = Operands(ctx, lib, c, aligned=aligned)
    call = lambda b, st: L.hevcdbk_sao_filter_device_g4(ctx.handle, C.byref(o.p), *o.sao_args, b, st)
    run_and_check(ctx, [o], call, [expected(name)], [border_less(name)], (name, aligned), name in NULL_TOO)
    rc, k = kernels_enqueued(lambda st: call(C.byref(o.borders), st))
    assert rc == 0 and names(k)[-1] == ("sao8_g4_kernel" if c["sb"] == 1 and aligned else "sao_g4_kernel"), names(k)
    o.free()


@pytest.mark.parametrize("mode", ["bs0", "bs"])
@pytest.mark.parametrize("name,cf", G4)
def test_deblock_sao_plane_g4(ctx, lib, name, cf, mode):
    """hevcdbk_h265_deblock_sao_device_g4 on a chroma plane of a 4:2:0 / 4:2:2 picture"""
    L = lib.lib()
    c = V.case(name)
    w, h = c["w"], c["h"]
    if mode == "bs0":
        bs = (np.zeros(G.num_vert_bs(w, h), np.uint8), np.zeros(G.num_hor_bs(w, h), np.uint8))
        params, want, free = None, expected(name), border_less(name)
    else:
        bs = G.random_bs(w, h, np.random.default_rng(31 + cf + c["depth"]))
        mids = [G.deblock_direct(p, bs[0], bs[1], cf, qp=G.QP, bit_depth=c["depth"], c_qp_offset=G.CQP, tc_offset_div2=G.TC_DIV2) for p in c["planes"]]
        assert any((m != p).any() for m, p in zip(mids, c["planes"]))
        params, want, free = after_deblocking(c, mids)
    o = Operands(ctx, lib, c, chroma=True, bs=bs, params=params)
    hp = lib.H265Params(G.TC_DIV2, 0, G.CQP, G.CQP)
    for fused in (lib.FUSED_ON, lib.FUSED_OFF):
        call = lambda b, st: L.hevcdbk_h265_deblock_sao_device_g4(ctx.handle, C.byref(o.p), 1, cf, G.QP, C.byref(hp), *o.sao_args, fused, b, None, st)
        run_and_check(ctx, [o], call, [want], [free], (name, mode, fused), name in NULL_TOO and mode == "bs0")
    o.free()
