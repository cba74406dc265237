"""The semi-planar kernels on the GPU at the decision edges, over the full sample range and over every boundary byte: the vectors of
tests/sp_edge_vectors.py through the four _sp entries of the C ABI, bit-exact against the existing statements applied per component
(sp_ref.deblock, rext_oracle.sao_plane / sao_borders_ref.sao_plane_by_bytes, the chain of the two).  tests/test_sp_edges_cpu.py asserts
what each vector reaches -- tC = 0 and tC' at the clipped Q = 53, the knees of Table 8-10, both sides of the delta clip and of Clip1 in
both components, SAO clips, band wraps, offsets of -128 / 127, 0 next to max_v across every wave, strip and tile border, every (byte,
class) pair -- and that the per-lane procedures are right on them; what is left to go wrong here is the device side: the operand fetch
for two components, the v_perm split and merge, the de-interleaved LDS tile and its halo, the merged stores, the luma body beside
the pair body.  Every destination is pre-filled, has row padding, a gap between frames and guard rows, all of which must come back
untouched.  The kernel that ran is read from a stream capture, for every call.  PARITY UNPINNED, like the rest of the spec-exact mode."""
import ctypes as C

import numpy as np
import pytest

import g4_ref as G
import h265_vectors as hv
import sao_borders_ref as B
import slice_offsets_ref as R
import sp_edge_vectors as E
import sp_ref as S
from test_gpu_fused_sp import FUSED, MULTI, Picture, fused_call, two_launches
from test_gpu_sao_sp import GENERIC as SAO_GENERIC, PIECE, Operands, pad_of, sao_name
from test_gpu_sp import PACKED_NAMES as DBK_PACKED, PairPlane, captured, check, sl_operand

pytestmark = pytest.mark.gpu

OPS = [o[0] for o in E.OPERANDS]
FUSED_OPS = ["q51", "allqp", "slices"]   # one QP, the all-QP map, per-slice pairs


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


def hp_of(lib, c):
    return lib.H265Params(c["tc_div2"], 0, c["cb"], c["cr"])


def slices_of(ctx, lib, c):
    """(the slice_offsets operand or None, its buffer or None)"""
    if c["pairs"] is None:
        return None, None
    return sl_operand(ctx, lib, c["pairs"])


def ByteOperands(ctx, lib, c, frames=None):
    """test_gpu_sao_sp.Operands with the vector's ARBITRARY boundary bytes, per frame, in place of a layout's"""
    return Operands(ctx, lib, c, frames=frames, nox=c["nox"])


# ---- deblocking --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("spec", S.DBK, ids=lambda s: s[0])
def test_filter_device(ctx, lib, spec, op):
    """the three frames (vertical, horizontal, both ways) in one batch; the 32-bit kernel and the packed kernel, out of place and in
    place"""
    L = lib.lib()
    c = E.dbk_case(spec, op)
    hp = hp_of(lib, c)
    so, dso = slices_of(ctx, lib, c)
    want = [E.dbk_expected(c, f) for f in range(3)]
    packs = c["depth"] <= 12
    for variant in (lib.KERNEL_GENERIC, lib.KERNEL_PACKED):
        for in_place in (False, True):
            pl = PairPlane(ctx, c, in_place=in_place, qmap=c["qp_map"] is not None)
            call = lambda st: L.hevcdbk_h265_filter_device_sp(ctx.handle, C.byref(pl.p), c["qp"], C.byref(hp), variant,
                                                             C.byref(so) if so else None, st)
            rc, k = captured(call)
            if variant == lib.KERNEL_PACKED and not packs:
                assert rc == lib.ERR_UNSUPPORTED and k == [], (rc, k)
            else:
                assert rc == 0 and k == ["dbk_h265_sp_kernel" if variant == lib.KERNEL_GENERIC else DBK_PACKED[c["sb"]]], (rc, k)
                assert call(None) == 0
                ctx.synchronize()
                check(pl, want, (c["name"], variant, in_place))
            pl.free()
    if dso:
        dso.free()


# ---- SAO ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spec", E.SAO, ids=lambda s: s[0])
def test_sao_device_full_range(ctx, lib, spec):
    """{no keep map, keep map} x {no borders, arbitrary bytes}: the packed kernel up to 12 bit, the per-sample kernel at 14 bit and on
    a pitch that the packed kernels' guard refuses"""
    L = lib.lib()
    c = E.sao_case(spec)
    n = len(c["planes"])
    ops = ByteOperands(ctx, lib, c)
    for rest in ((0, PIECE[c["sb"]] // 2) if c["depth"] <= 12 else (0,)):
        kernel = sao_name(c) if rest == 0 else SAO_GENERIC
        for keep in (False, True):
            for borders in (False, True):
                want = [E.sao_expected(c, f, keep, borders) for f in range(n)]
                pl = PairPlane(ctx, c, bs=False, pad=pad_of(c, rest))
                assert pl.p.pitch % PIECE[c["sb"]] == rest
                rc, k = captured(lambda st: ops.sao(L, ctx, pl.p, keep, borders, st))
                assert rc == 0 and k == [kernel], (rc, k)
                assert ops.sao(L, ctx, pl.p, keep, borders) == 0
                ctx.synchronize()
                check(pl, want, (spec[0], rest, keep, borders))
                pl.free()
    ops.free()


@pytest.mark.parametrize("name", list(E.BYTES))
def test_sao_device_every_byte(ctx, lib, name):
    """every (byte 0..255, class) pair on an interior CTB of each component, one byte array for both"""
    L = lib.lib()
    c = E.bytes_case(name)
    ops = ByteOperands(ctx, lib, c)
    want = [E.bytes_expected(name, f) for f in range(len(c["planes"]))]
    for rest in (0, PIECE[c["sb"]] // 2):
        pl = PairPlane(ctx, c, bs=False, pad=pad_of(c, rest))
        rc, k = captured(lambda st: ops.sao(L, ctx, pl.p, False, True, st))
        assert rc == 0 and k == [sao_name(c) if rest == 0 else SAO_GENERIC], (rc, k)
        assert ops.sao(L, ctx, pl.p, False, True) == 0
        ctx.synchronize()
        check(pl, want, (name, rest))
        pl.free()
    ops.free()


# ---- deblocking + SAO in one kernel ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("op", FUSED_OPS)
@pytest.mark.parametrize("name", E.FUSED)
def test_sp_fused(ctx, lib, name, op):
    """the deblocking vectors under full-range SAO content over every third 16 x 16 block, tile borders in both directions; with and
    without the arbitrary bytes; FUSED_ON: exactly the fused kernel; FUSED_OFF: the two _sp kernels on the same bytes"""
    L = lib.lib()
    c = E.chain_case(name, op)
    hp = hp_of(lib, c)
    so, dso = slices_of(ctx, lib, c)
    ops = ByteOperands(ctx, lib, c, frames=range(E.SAO_FRAMES))
    for borders in (False, True):
        want = [E.chain_expected(c, f, borders)[1] for f in range(E.SAO_FRAMES)]
        for fused, kernels in ((lib.FUSED_ON, [FUSED[c["sb"]]]), (lib.FUSED_OFF, two_launches(c))):
            pl = PairPlane(ctx, c, qmap=c["qp_map"] is not None, pad=pad_of(c))
            call = lambda st: fused_call(L, ctx, ops, pl.p, c, hp, fused, borders, C.byref(so) if so else None, st)
            rc, k = captured(call)
            assert rc == 0 and k == kernels, (rc, k, fused)
            assert call(None) == 0
            ctx.synchronize()
            check(pl, want, (name, op, borders, fused))
            pl.free()
    ops.free()
    if dso:
        dso.free()


@pytest.mark.parametrize("name", list(E.BYTES))
def test_sp_fused_every_byte(ctx, lib, name):
    """bS all 0: deblocking is the identity and the SAO stage of the fused kernel sees every byte"""
    L = lib.lib()
    c = dict(E.bytes_case(name), qp=30, cb=-3, cr=4, tc_div2=0, qp_map=None, pairs=None)
    c["bs"] = E.bytes_bs(c)
    hp = hp_of(lib, c)
    ops = ByteOperands(ctx, lib, c)
    want = [E.bytes_expected(name, f) for f in range(len(c["planes"]))]
    for fused, kernels in ((lib.FUSED_ON, [FUSED[c["sb"]]]), (lib.FUSED_OFF, two_launches(c))):
        pl = PairPlane(ctx, c, pad=pad_of(c))
        rc, k = captured(lambda st: fused_call(L, ctx, ops, pl.p, c, hp, fused, True, None, st))
        assert rc == 0 and k == kernels, (rc, k, fused)
        assert fused_call(L, ctx, ops, pl.p, c, hp, fused, True, None) == 0
        ctx.synchronize()
        check(pl, want, (name, fused))
        pl.free()
    ops.free()


# ---- the whole picture ---------------------------------------------------------------------------------------------------------------

_pictures = {}


def picture_case(name, op):
    """(pair case, luma case, luma parameters, expected Y frames, expected pair frames): Y = h265_vectors.luma_edge_plane 528x272, its
    vertical and horizontal twins as the two frames, under full-range SAO parameters; the pairs = chain_case 264x136.  With per-slice
    pairs ("slices") the picture also has a slice / tile layout for SAO, as test_gpu_fused_sp.test_nv12 runs it"""
    if (name, op) in _pictures:
        return _pictures[(name, op)]
    from oracle import h265
    c = dict(E.chain_case(name, op))
    extra = c["pairs"] is not None
    c["params"] = c["pcb"]
    c["layout"] = G.sao_layout(c)
    rng = np.random.default_rng(G.seed_of("nv12" + name + op))
    w, h, depth, lg = 2 * c["w"], 2 * c["h"], c["depth"], c["lg"] + 1
    fr = [hv.luma_edge_plane(depth, c["qp"], c["tc_div2"], 0, rng, w=w, h=h, direction=d) for d in ("v", "h")]
    sao = [hv.sao_full_range(depth, lg, rng, w=w, h=h) for _ in range(2)]
    y = {"w": w, "h": h, "depth": depth, "sb": c["sb"], "lw": lg, "lh": lg, "planes": [x[0] for x in fr], "bs": [(x[1], x[2]) for x in fr],
         "keep": [x[2] for x in sao]}
    params = [x[1] for x in sao]
    want_y = []
    for f in range(2):
        vb, hb = y["bs"][f]
        if extra:
            mid = R.expected(y["planes"][f], vb, hb, c["pairs"], E.SL_CTB_LOG2, c_idx=0, qp=c["qp"], unit_log2=E.UNIT_LOG2, bit_depth=depth)
        else:
            mid = h265.filter_plane(y["planes"][f], c["qp"], vb, hb, c_idx=0, bit_depth=depth, unit_log2=E.UNIT_LOG2,
                                    tc_offset_div2=c["tc_div2"], beta_offset_div2=0)
        assert (mid != y["planes"][f]).any()
        want_y.append(G.sao_direct(mid, params[f], lg, lg, bit_depth=depth, keep=y["keep"][f], layout=c["layout"] if extra else None))
        assert (want_y[f] != mid).any()
    nox = B.expected_nox(c["layout"])
    want_c = []
    for f in range(2):
        dbk = E.chain_expected(c, f, False)[0]
        want_c.append(E.sao(dbk, c["pcb"][f], c["pcr"][f], c["lg"], depth, keep=c["keep"][f], nox=nox if extra else None))
    if not extra:   # Picture uploads the pairs; without per-slice pairs they are handed to no call
        c["pairs"] = np.zeros((-(-2 * c["h"] >> E.SL_CTB_LOG2), -(-2 * c["w"] >> E.SL_CTB_LOG2), 2), np.int8)
    _pictures[(name, op)] = (c, y, params, want_y, want_c)
    return _pictures[(name, op)]


@pytest.mark.parametrize("op", ["q37", "slices"])
@pytest.mark.parametrize("name", ["264x136", "264x136_10"])
def test_nv12(ctx, lib, name, op):
    """the only place where the luma body, compiled with the pair body's registers, meets decision-edge content: FUSED_ON runs exactly
    the frame kernel; FUSED_OFF exactly the per-plane entries' kernels, on the same bytes"""
    c, y, params, want_y, want_c = picture_case(name, op)
    extra = op == "slices"
    hp = hp_of(lib, c)
    ref = Picture(ctx, lib, c, y, params, False)   # what the per-plane entries run: Y through _planes_g4, then the two _sp kernels
    per_plane = captured(lambda st: ref.planes_g4(ctx, hp, lib.FUSED_OFF, extra, st))[1] + two_launches(c)
    ref.free()
    for fused in (lib.FUSED_ON, lib.FUSED_OFF):
        pic = Picture(ctx, lib, c, y, params, False)
        rc, k = captured(lambda st: pic.nv12(ctx, hp, fused, extra, st))
        assert rc == 0 and k == ([MULTI] if fused == lib.FUSED_ON else per_plane), (rc, k, fused)
        assert pic.nv12(ctx, hp, fused, extra) == 0
        ctx.synchronize()
        check(pic.luma.dst, want_y, (name, op, fused, "Y"))
        check(pic.pairs, want_c, (name, op, fused, "CbCr"))
        pic.free()
