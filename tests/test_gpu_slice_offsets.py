"""Per-slice deblocking offsets (H.265 8.7.2.5.3 / 8.7.2.5.5) on the GPU through the C ABI: the producer
hevcdbk_h265_slice_offsets_device and the three _sl entries, bit-exact against the composition of tests/slice_offsets_ref.py.
Every destination is pre-filled, has row padding, a gap between frames and guard rows before and after, all of which must come back
untouched.  PARITY UNPINNED, like the rest of the spec-exact mode.  test_slice_offsets_cpu.py shows that every vector differs in
every 32 x 32 cell from the zero-offset picture, from every single pair applied uniformly and from the P-side selection, so a
library that took the operand and ignored or misread it fails here.  The kernel family that ran is read from a stream capture."""
import ctypes as C

import numpy as np
import pytest

import rext_oracle as rx
import sao_borders_ref as B
import slice_offsets_ref as R
import slice_offsets_vectors as V
from test_gpu_sao_borders import FILL, Surface, dev_planes, up

pytestmark = pytest.mark.gpu

POISON = 6   # (+6, +6) wherever the operand has bytes that belong to no CTB of the frame


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


def operand(ctx, pairs, layout="tight"):
    """(SliceOffsets, buffer) of per-frame pair arrays: 'shared' = the first frame's for all, 'tight', or 'padded' = a row stride
    of 3 CTBs more and two rows of gap between the frames, poison in all of it"""
    from gpu_video_codec_amd import _lib
    rows, cols = pairs[0].shape[:2]
    if layout == "shared":
        host = pairs[0].copy()
        so = (cols, 0)
    elif layout == "tight":
        host = np.stack(pairs)
        so = (cols, rows * cols * 2)
    else:
        host = np.full((len(pairs), rows + 2, cols + 3, 2), POISON, np.int8)
        for f, p in enumerate(pairs):
            host[f, :rows, :cols] = p
        so = (cols + 3, (rows + 2) * (cols + 3) * 2)
    d = up(ctx, host)
    return _lib.SliceOffsets(d.ptr, so[0], so[1], V.CTB_LOG2), d


def surfaces(ctx, c, in_place=False):
    n = len(c["planes"])
    src = Surface(ctx, n, c["ph"], c["pw"], c["sb"], 16, c["planes"])
    dst = src if in_place else Surface(ctx, n, c["ph"], c["pw"], c["sb"], 16)
    return src, dst


def plane_of(ctx, c, src, dst):
    dv, dh = up(ctx, c["vb"]), up(ctx, c["hb"])
    dm = up(ctx, c["qp_map"]) if c["qp_map"] is not None else None
    p = dev_planes(src, dst, c["depth"], c["c_idx"] != 0, dv, dh, dm, 0 if dm is None else c["qp_map"].shape[1], 3)
    return p, [dv, dh] + ([dm] if dm else [])


def hp_of(lib, c, tc=0, beta=0):
    return lib.H265Params(tc, beta, V.CQP[1], V.CQP[2])


def names(k):
    from kernel_capture import parse_kernel
    return [parse_kernel(x[0])[0] for x in k]


# ---- the producer -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows,cols", [(1, 1), (1, 7), (5, 1), (3, 4), (12, 16), (34, 60), (68, 120)])
def test_producer(ctx, lib, rows, cols):
    rng = np.random.default_rng(rows * 131 + cols)
    L = lib.lib()
    for run in (1, 3, 5, cols, rows * cols):
        sidx = R.slices_raster(rows, cols, run)
        n = int(sidx.max()) + 1
        table = rng.integers(-6, 7, (n, 2)).astype(np.int8)
        for n_used in sorted({n, max(n // 2, 1), 0}):
            want = R.ctb_pairs(sidx, table[:n_used])
            if n_used:
                assert np.array_equal(ctx.derive_slice_offsets(sidx, table[:n_used]), want), (rows, cols, run, n_used)
            # guarded: row strides beyond the CTB columns on both sides, the bytes beyond untouched
            ins, outs = cols + 3, cols + 5
            ds = up(ctx, np.pad(sidx, ((0, 0), (0, ins - cols)), constant_values=0))
            dt = up(ctx, table if n else np.zeros((1, 2), np.int8))
            out = up(ctx, np.full((rows + 2, outs, 2), FILL, np.uint8))
            assert L.hevcdbk_h265_slice_offsets_device(ctx.handle, ds.ptr, ins, dt.ptr, n_used, cols, rows, out.ptr + outs * 2, outs, None) == 0
            ctx.synchronize()
            got = out.download((rows + 2) * outs * 2).reshape(rows + 2, outs, 2)
            assert np.array_equal(got[1:-1, :cols].view(np.int8), want), (rows, cols, run, n_used)
            assert (got[0] == FILL).all() and (got[-1] == FILL).all() and (got[:, cols:] == FILL).all()
            for x in (ds, dt, out):
                x.free()


# ---- deblocking only: every family against the reference ----------------------------------------------------------------------

def _filter_call(L, ctx, p, c, hp, variant, so, st=None):
    return L.hevcdbk_h265_filter_device_sl(ctx.handle, C.byref(p), c["c_idx"], c["cf"], c["qp"], C.byref(hp), variant,
                                           None if so is None else C.byref(so), st)


@pytest.mark.parametrize("spec", V.CASES, ids=lambda s: s[0])
def test_filter_device(ctx, lib, spec):
    from kernel_capture import kernels_enqueued
    L = lib.lib()
    c = V.case(spec)
    want = V.expected(c)
    so, dso = operand(ctx, c["pairs"])
    hp = hp_of(lib, c)
    for in_place in (False, True):
        for variant in (lib.KERNEL_GENERIC, lib.KERNEL_PACKED, lib.KERNEL_AUTO):
            src, dst = surfaces(ctx, c, in_place)
            p, bufs = plane_of(ctx, c, src, dst)
            rc_plain, k_plain = kernels_enqueued(lambda st: _filter_call(L, ctx, p, c, hp, variant, None, st))
            rc, k = kernels_enqueued(lambda st: _filter_call(L, ctx, p, c, hp, variant, so, st))
            # the operand refuses nothing the entry takes without it (12-bit luma has no packed kernel either way)
            assert rc == rc_plain, (spec[0], variant, rc, rc_plain)
            if rc == 0:
                assert len(k) == 1 and names(k)[0].endswith("_sl_kernel"), names(k)
                packed = names(k_plain)[0].startswith("dbk_packed")
                assert names(k)[0].startswith("dbk_packed") == packed, (names(k), names(k_plain))
                if variant == lib.KERNEL_GENERIC:
                    assert names(k)[0] == "dbk_h265_sl_kernel"
                assert _filter_call(L, ctx, p, c, hp, variant, so) == 0
                ctx.synchronize()
                got, clean = dst.read()
                assert clean, "bytes outside the frame were written"
                assert np.array_equal(got[0], want), (spec[0], in_place, variant, int((got[0] != want).sum()))
            else:
                assert rc == lib.ERR_UNSUPPORTED and variant == lib.KERNEL_PACKED
            for x in {src, dst} | set(bufs):
                x.free()
    dso.free()


@pytest.mark.parametrize("low", [True, False], ids=["qp0_3_minus6", "qp48_51_plus6"])
@pytest.mark.parametrize("depth", [8, 10])
def test_clips(ctx, lib, low, depth):
    """both ends of Clip3(0, 51, .) and Clip3(0, 53, .): test_slice_offsets_cpu.py asserts that the vectors reach them"""
    L = lib.lib()
    c = V.clip_case(low, depth)
    want = V.expected(c)
    so, dso = operand(ctx, c["pairs"])
    hp = hp_of(lib, c)
    for variant in (lib.KERNEL_GENERIC, lib.KERNEL_PACKED):
        src, dst = surfaces(ctx, c)
        p, bufs = plane_of(ctx, c, src, dst)
        assert _filter_call(L, ctx, p, c, hp, variant, so) == 0
        ctx.synchronize()
        got, clean = dst.read()
        assert clean and np.array_equal(got[0], want), (low, depth, variant, int((got[0] != want).sum()))
        for x in [src, dst] + bufs:
            x.free()
    dso.free()


def test_null_operand_and_ignored_params_offsets(ctx, lib):
    """slice_offsets == NULL enqueues exactly the _cf entry's kernel, grid and block and gives its bytes; with the operand the two
    offsets of params change no byte"""
    from kernel_capture import kernels_enqueued
    L = lib.lib()
    for spec in (V.CASES[0], V.CASES[1], V.CASES[3], V.CASES[9], V.CASES[22]):
        c = V.case(spec)
        so, dso = operand(ctx, c["pairs"])
        hp = hp_of(lib, c, tc=2, beta=-3)
        src, dst = surfaces(ctx, c)
        p, bufs = plane_of(ctx, c, src, dst)
        for variant in (lib.KERNEL_AUTO, lib.KERNEL_GENERIC, lib.KERNEL_PACKED):
            cf_call = lambda st: L.hevcdbk_h265_filter_device_cf(ctx.handle, C.byref(p), c["c_idx"], c["cf"], c["qp"], C.byref(hp), variant, st)
            rc0, k0 = kernels_enqueued(cf_call)
            rc1, k1 = kernels_enqueued(lambda st: _filter_call(L, ctx, p, c, hp, variant, None, st))
            assert rc0 == 0 and rc1 == 0 and k0 == k1, (spec[0], variant)
            assert cf_call(None) == 0
            ctx.synchronize()
            base = dst.read()[0][0]
            dst.refill()
            assert _filter_call(L, ctx, p, c, hp, variant, None) == 0
            ctx.synchronize()
            got, clean = dst.read()
            assert clean and np.array_equal(got[0], base)
            assert np.array_equal(base, V.expected(c, pairs=V.uniform((-3, 2))))
            for (tc, beta) in ((2, -3), (-6, 6), (0, 0)):
                dst.refill()
                assert _filter_call(L, ctx, p, c, hp_of(lib, c, tc, beta), variant, so) == 0
                ctx.synchronize()
                got, clean = dst.read()
                assert clean and np.array_equal(got[0], V.expected(c)), (spec[0], variant, tc, beta)
        for x in [src, dst, dso] + bufs:
            x.free()


@pytest.mark.parametrize("n", [2, 3, 5])
@pytest.mark.parametrize("layout", ["shared", "tight", "padded"])
def test_batch(ctx, lib, n, layout):
    """the operand of a batch shared, tight and padded (poison in the gap): the batch equals n single-frame calls"""
    L = lib.lib()
    for spec in (V.CASES[1], V.CASES[9], V.CASES[3]):
        c = V.case(spec, frames=n)
        so, dso = operand(ctx, c["pairs"], layout)
        hp = hp_of(lib, c)
        for variant in (lib.KERNEL_GENERIC, lib.KERNEL_PACKED):
            src, dst = surfaces(ctx, c)
            p, bufs = plane_of(ctx, c, src, dst)
            assert _filter_call(L, ctx, p, c, hp, variant, so) == 0
            ctx.synchronize()
            got, clean = dst.read()
            assert clean
            for f in range(n):
                want = V.expected(c, f, pairs=c["pairs"][0 if layout == "shared" else f])
                assert np.array_equal(got[f], want), (spec[0], n, layout, variant, f, int((got[f] != want).sum()))
                # and n single-frame calls
                one = dict(c, planes=[c["planes"][f]])
                s1, d1 = surfaces(ctx, one)
                p1, b1 = plane_of(ctx, one, s1, d1)
                so1, dso1 = operand(ctx, [c["pairs"][0 if layout == "shared" else f]])
                assert _filter_call(L, ctx, p1, one, hp, variant, so1) == 0
                ctx.synchronize()
                assert np.array_equal(d1.read()[0][0], got[f])
                for x in [s1, d1, dso1] + b1:
                    x.free()
            for x in [src, dst] + bufs:
                x.free()
        dso.free()


def test_batch_far(ctx, lib):
    """the frames' pair arrays further apart than 31 bits reach (tests/batch_vectors.py FAR_STRIDE, made even: pairs are 16-bit
    words): f * frame_stride in 64 bits"""
    import batch_vectors as bv
    L = lib.lib()
    stride = bv.FAR_STRIDE + 1
    for spec in (V.CASES[1], V.CASES[9], V.CASES[2]):
        c = V.case(spec, frames=2)
        far = ctx.alloc(stride + c["pairs"][1].nbytes)
        for f in range(2):
            far.upload(c["pairs"][f].view(np.uint8).ravel(), f * stride)
        so = lib.SliceOffsets(far.ptr, V.COLS, stride, V.CTB_LOG2)
        hp = hp_of(lib, c)
        for variant in (lib.KERNEL_GENERIC, lib.KERNEL_PACKED):
            src, dst = surfaces(ctx, c)
            p, bufs = plane_of(ctx, c, src, dst)
            assert _filter_call(L, ctx, p, c, hp, variant, so) == 0
            ctx.synchronize()
            got, clean = dst.read()
            assert clean
            for f in range(2):
                assert np.array_equal(got[f], V.expected(c, f)), (spec[0], variant, f)
            for x in [src, dst] + bufs:
                x.free()
        far.free()


# ---- deblocking + SAO ---------------------------------------------------------------------------------------------------------

FUSED_NAMES = {0: "auto", 1: "off", 2: "on"}


def _sao_operands(ctx, lib, c, rng, lay):
    """SAO parameters (edge offset everywhere, so that slice / tile borders bite) of the plane's CTB grid under the border layout
    lay (None: no borders), and the expected SAO of a deblocked plane"""
    sx, sy = (1, 1) if c["c_idx"] == 0 else rx.SUB[c["cf"]]
    lw, lh = V.CTB_LOG2 - (sx - 1), V.CTB_LOG2 - (sy - 1)
    n = len(c["planes"])
    prm = [B.edge_params(V.ROWS, V.COLS, rng, c["depth"]) for _ in range(n)]
    dp = up(ctx, np.stack(prm))
    sp = lib.SaoPlaneCf()
    sp.params, sp.params_stride, sp.params_frame_stride, sp.ctb_log2_w, sp.ctb_log2_h = dp.ptr, V.COLS, V.ROWS * V.COLS, lw, lh

    def sao(d, f):
        if lay is None:
            return rx.sao_plane(d, prm[f], lw, lh, bit_depth=c["depth"])
        return B.sao_plane(d, prm[f], lw, lh, lay, bit_depth=c["depth"])
    return sp, dp, sao


def _borders(ctx, lib, lay):
    if lay is None:
        return None, None
    nox = B.expected_nox(lay)
    d = up(ctx, nox)
    return lib.SaoBorders(d.ptr, nox.shape[1], 0), d


@pytest.mark.parametrize("with_borders", [False, True], ids=["noborders", "borders"])
@pytest.mark.parametrize("spec", V.CASES, ids=lambda s: s[0])
def test_deblock_sao_single_plane(ctx, lib, spec, with_borders):
    from kernel_capture import kernels_enqueued
    L = lib.lib()
    c = V.case(spec, frames=2)
    rng = np.random.default_rng(len(spec[0]) + 17 * with_borders)
    so, dso = operand(ctx, c["pairs"])
    hp = hp_of(lib, c)
    lay = B._layout_of("mixed", V.ROWS, V.COLS, rng) if with_borders else None
    sp, dp, sao = _sao_operands(ctx, lib, c, rng, lay)
    b, db = _borders(ctx, lib, lay)
    src, dst = surfaces(ctx, c)
    p, bufs = plane_of(ctx, c, src, dst)
    want = [sao(V.expected(c, f), f) for f in range(2)]

    def call(fused, st=None, operand_=so):
        return L.hevcdbk_h265_deblock_sao_device_sl(ctx.handle, C.byref(p), c["c_idx"], c["cf"], c["qp"], C.byref(hp), sp.params, sp.params_stride,
                                                    sp.params_frame_stride, sp.ctb_log2_w, sp.ctb_log2_h, None, 0, 0, fused,
                                                    None if b is None else C.byref(b), None if operand_ is None else C.byref(operand_), st)
    for fused in (lib.FUSED_AUTO, lib.FUSED_ON, lib.FUSED_OFF):
        dst.refill()
        assert call(fused) == 0, (spec[0], FUSED_NAMES[fused])   # also the first use of the context's scratch, outside a capture
        ctx.synchronize()
        got, clean = dst.read()
        assert clean, "bytes outside the frames were written"
        for f in range(2):
            assert np.array_equal(got[f], want[f]), (spec[0], FUSED_NAMES[fused], f, int((got[f] != want[f]).sum()))
        rc, k = kernels_enqueued(lambda st: call(fused, st))
        rc0, k0 = kernels_enqueued(lambda st: call(fused, st, None))
        assert rc == 0 and rc0 == 0
        main = [x for x in names(k) if "rows_x2" not in x]
        main0 = [x for x in names(k0) if "rows_x2" not in x]
        assert len(main) == len(main0), (main, main0)   # fused where the entry without the operand is fused
        assert main[0].endswith("_sl_kernel"), main
        if fused == lib.FUSED_ON:
            assert len(main) == 1 and "fused" in main[0], main
        if fused == lib.FUSED_OFF:
            assert len(main) == 2 and "fused" not in main[0], main
        # NULL operand: exactly the _nox entry's kernels, grids and blocks, and its bytes
        nox_call = lambda st: L.hevcdbk_h265_deblock_sao_device_nox(ctx.handle, C.byref(p), c["c_idx"], c["cf"], c["qp"], C.byref(hp), sp.params,
                                                                    sp.params_stride, sp.params_frame_stride, sp.ctb_log2_w, sp.ctb_log2_h, None, 0,
                                                                    0, fused, None if b is None else C.byref(b), st)
        rc1, k1 = kernels_enqueued(nox_call)
        assert rc1 == 0 and k0 == k1, (spec[0], FUSED_NAMES[fused])
        dst.refill()
        assert nox_call(None) == 0
        ctx.synchronize()
        base = dst.read()[0]
        dst.refill()
        assert call(fused, None, None) == 0
        ctx.synchronize()
        got, clean = dst.read()
        assert clean and all(np.array_equal(got[f], base[f]) for f in range(2)), (spec[0], FUSED_NAMES[fused])
    for x in [src, dst, dso, dp] + bufs + ([db] if db else []):
        x.free()


def _picture(ctx, lib, cf, depth, use_map, n, rng, with_borders, layout="tight"):
    tag = "map" if use_map else "qp"
    specs = [s for s in V.CASES if s[3] == depth and s[4] == use_map and ((s[2] == 0) or (s[1] == cf and s[2] in (1, 2)))]
    specs = sorted(specs, key=lambda s: s[2])
    assert [s[2] for s in specs] == [0, 1, 2], (cf, depth, tag)
    pic = dict(cases=[V.case(s, frames=n) for s in specs], planes=[], sao=[], dst=[], free=[], want=[])
    # ONE operand and one border layout for the picture: the luma case's
    pairs = pic["cases"][0]["pairs"]
    if layout == "shared":
        pairs = [pairs[0]] * n
    lay = B._layout_of("mixed", V.ROWS, V.COLS, rng) if with_borders else None
    for c in pic["cases"]:
        c["pairs"] = pairs
        src, dst = surfaces(ctx, c)
        p, bufs = plane_of(ctx, c, src, dst)
        sp, dp, sao = _sao_operands(ctx, lib, c, rng, lay)
        pic["planes"].append(p)
        pic["sao"].append(sp)
        pic["dst"].append(dst)
        pic["free"] += [src, dst, dp] + bufs
        pic["want"] += [sao(V.expected(c, f), f) for f in range(n)]
    pic["so"], dso = operand(ctx, pairs, layout)
    pic["b"], db = _borders(ctx, lib, lay)
    pic["free"] += [dso] + ([db] if db else [])
    return pic


@pytest.mark.parametrize("with_borders", [False, True], ids=["noborders", "borders"])
@pytest.mark.parametrize("use_map", [False, True], ids=["qp", "map"])
@pytest.mark.parametrize("depth", [8, 10, 12])
@pytest.mark.parametrize("cf", [1, 2, 3], ids=["420", "422", "444"])
def test_deblock_sao_planes(ctx, lib, cf, depth, use_map, with_borders):
    """Y + Cb + Cr in one call, ONE operand for the picture"""
    from kernel_capture import kernels_enqueued, parse_kernel
    L = lib.lib()
    n = 2
    rng = np.random.default_rng(cf * 100 + depth + 7 * use_map + 3 * with_borders)
    pic = _picture(ctx, lib, cf, depth, use_map, n, rng, with_borders)
    arr = (lib.DevicePlanes * 3)(*pic["planes"])
    sp = (lib.SaoPlaneCf * 3)(*pic["sao"])
    hp = lib.H265Params(0, 0, V.CQP[1], V.CQP[2])
    b = pic["b"]

    def call(fused, st=None, so=pic["so"]):
        return L.hevcdbk_h265_deblock_sao_device_planes_sl(ctx.handle, arr, 3, cf, 32, C.byref(hp), sp, fused, None if b is None else C.byref(b),
                                                           None if so is None else C.byref(so), st)
    for fused in (lib.FUSED_AUTO, lib.FUSED_ON, lib.FUSED_OFF):
        for d in pic["dst"]:
            d.refill()
        assert call(fused) == 0, (cf, depth, use_map, FUSED_NAMES[fused])
        ctx.synchronize()
        for i, dst in enumerate(pic["dst"]):
            got, clean = dst.read()
            assert clean
            for f in range(n):
                want = pic["want"][i * n + f]
                assert np.array_equal(got[f], want), (cf, depth, use_map, FUSED_NAMES[fused], i, f, int((got[f] != want).sum()))
        rc, k = kernels_enqueued(lambda st: call(fused, st))
        rc0, k0 = kernels_enqueued(lambda st: call(fused, st, None))
        assert rc == 0 and rc0 == 0
        main = [x for x in names(k) if "rows_x2" not in x]
        main0 = [x for x in names(k0) if "rows_x2" not in x]
        assert len(main) == len(main0), (main, main0)   # one launch where the entry without the operand makes one
        assert all(x.endswith("_sl_kernel") for x in main if "sao_kernel" not in x and not x.startswith("sao")), main
        if fused != lib.FUSED_OFF:
            # ONE launch of the multi-plane kernel of this container, depth (12 bit: the WIDE luma form) and chroma format
            multi = [parse_kernel(x[0]) for x in k if "rows_x2" not in parse_kernel(x[0])[0]]
            assert multi == [("dbk_sao_fused_multi_h265_sl_kernel", (1 if depth == 8 else 2, int(depth == 12), cf))], multi
    # NULL operand: exactly the _nox entry's kernels, and its bytes
    rc0, k0 = kernels_enqueued(lambda st: call(lib.FUSED_AUTO, st, None))
    rc1, k1 = kernels_enqueued(lambda st: L.hevcdbk_h265_deblock_sao_device_planes_nox(ctx.handle, arr, 3, cf, 32, C.byref(hp), sp, lib.FUSED_AUTO,
                                                                                       None if b is None else C.byref(b), st))
    assert rc0 == 0 and rc1 == 0 and k0 == k1
    for d in pic["dst"]:
        d.refill()
    assert L.hevcdbk_h265_deblock_sao_device_planes_nox(ctx.handle, arr, 3, cf, 32, C.byref(hp), sp, lib.FUSED_AUTO, None if b is None else C.byref(b),
                                                        None) == 0
    ctx.synchronize()
    base = [d.read()[0] for d in pic["dst"]]
    for d in pic["dst"]:
        d.refill()
    assert call(lib.FUSED_AUTO, None, None) == 0
    ctx.synchronize()
    for i, d in enumerate(pic["dst"]):
        got, clean = d.read()
        assert clean and all(np.array_equal(got[f], base[i][f]) for f in range(n)), (cf, depth, use_map, i)
    for x in pic["free"]:
        x.free()


@pytest.mark.parametrize("layout", ["shared", "padded"])
def test_fused_batch_layouts_and_ignored_params_offsets(ctx, lib, layout):
    """the fused kernels, single plane and Y + Cb + Cr in one launch, with the operand of a 3-frame batch shared and padded (poison in
    the gap) and params' two offsets set: they change no byte"""
    L = lib.lib()
    n = 3
    for spec in (V.CASES[1], V.CASES[2], V.CASES[9]):
        c = V.case(spec, frames=n)
        pairs = [c["pairs"][0]] * n if layout == "shared" else c["pairs"]
        so, dso = operand(ctx, pairs, layout)
        rng = np.random.default_rng(len(spec[0]))
        sp, dp, sao = _sao_operands(ctx, lib, c, rng, None)
        src, dst = surfaces(ctx, c)
        p, bufs = plane_of(ctx, c, src, dst)
        for (tc, beta) in ((2, -3), (-6, 6)):
            hp = hp_of(lib, c, tc, beta)
            dst.refill()
            assert L.hevcdbk_h265_deblock_sao_device_sl(ctx.handle, C.byref(p), c["c_idx"], c["cf"], c["qp"], C.byref(hp), sp.params, sp.params_stride,
                                                        sp.params_frame_stride, sp.ctb_log2_w, sp.ctb_log2_h, None, 0, 0, lib.FUSED_ON, None,
                                                        C.byref(so), None) == 0
            ctx.synchronize()
            got, clean = dst.read()
            assert clean
            for f in range(n):
                want = sao(V.expected(c, f, pairs=pairs[f]), f)
                assert np.array_equal(got[f], want), (spec[0], layout, tc, beta, f, int((got[f] != want).sum()))
        for x in [src, dst, dso, dp] + bufs:
            x.free()
    for (cf, depth, use_map) in ((1, 8, True), (3, 10, False)):
        rng = np.random.default_rng(cf + depth)
        pic = _picture(ctx, lib, cf, depth, use_map, n, rng, True, layout)
        arr = (lib.DevicePlanes * 3)(*pic["planes"])
        sp3 = (lib.SaoPlaneCf * 3)(*pic["sao"])
        hp = lib.H265Params(-5, 4, V.CQP[1], V.CQP[2])
        assert L.hevcdbk_h265_deblock_sao_device_planes_sl(ctx.handle, arr, 3, cf, 32, C.byref(hp), sp3, lib.FUSED_ON, C.byref(pic["b"]),
                                                           C.byref(pic["so"]), None) == 0
        ctx.synchronize()
        for i, dst in enumerate(pic["dst"]):
            got, clean = dst.read()
            assert clean
            for f in range(n):
                assert np.array_equal(got[f], pic["want"][i * n + f]), (cf, depth, layout, i, f)
        for x in pic["free"]:
            x.free()


def test_python_wrapper(ctx, lib):
    c = V.case(V.CASES[1])
    so, dso = operand(ctx, c["pairs"])
    src, dst = surfaces(ctx, c)
    p, bufs = plane_of(ctx, c, src, dst)
    ctx.filter_device_h265(p, c["qp"], chroma_format="420", slice_offsets=so, tc_offset_div2=3)
    ctx.synchronize()
    assert np.array_equal(dst.read()[0][0], V.expected(c))
    rng = np.random.default_rng(3)
    sp, dp, sao = _sao_operands(ctx, lib, c, rng, None)
    dst.refill()
    ctx.deblock_sao_h265_device(p, c["qp"], sp.params, sp.params_stride, sp.ctb_log2_w, params_frame_stride=sp.params_frame_stride, slice_offsets=so)
    ctx.synchronize()
    assert np.array_equal(dst.read()[0][0], sao(V.expected(c), 0))
    dst.refill()
    ctx.deblock_sao_device_planes([p], c["qp"], [{"params": sp.params, "params_stride": sp.params_stride, "ctb_log2": sp.ctb_log2_w,
                                                  "params_frame_stride": sp.params_frame_stride}], h265={}, slice_offsets=so)
    ctx.synchronize()
    assert np.array_equal(dst.read()[0][0], sao(V.expected(c), 0))
    with pytest.raises(ValueError):
        ctx.deblock_sao_device_planes([p], c["qp"], [(sp.params, sp.params_stride, sp.ctb_log2_w)], slice_offsets=so)
    for x in [src, dst, dso, dp] + bufs:
        x.free()
