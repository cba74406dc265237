"""bS derivation on the GPU (dbk_h265_bs_kernel, the chroma gathers, the `units` route of the host-frame operators and the
decoder's chain on device memory) against tests/bs_vectors.py, byte for byte.

The reference is the set-shaped restatement of 8.7.2.4 of bs_vectors.py, not oracle/h265_oracle.c (whose decision tree the
kernel shares); tests/test_bs_rules_cpu.py proves the vectors reach every leaf of the rule on both sides of every threshold.
Every test is one bounded pass.  PARITY UNPINNED, like the rest of the spec-exact mode.
"""
import ctypes as C

import numpy as np
import pytest

import bs_vectors as bv
import rext_oracle as rx

pytestmark = pytest.mark.gpu

GUARD = 256        # bytes in front of and behind every output array
FILL = 0xA5
FORMATS = (("400", 0), ("420", 1), ("422", 2), ("444", 3))


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
def hip():
    L = C.CDLL("libamdhip64.so")
    L.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    L.hipStreamSynchronize.argtypes = [C.c_void_p]
    L.hipStreamDestroy.argtypes = [C.c_void_p]
    L.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    L.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    L.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    L.hipStreamWaitEvent.argtypes = [C.c_void_p, C.c_void_p, C.c_uint]
    L.hipEventDestroy.argtypes = [C.c_void_p]
    return L


class Pic:
    """a picture's units with the reference's answer for every chroma format"""

    def __init__(self, name, units, w, h):
        self.name, self.units, self.w, self.h = name, units, w, h
        self.arrs = [np.ascontiguousarray(a, dt) for a, dt in zip(units, bv.UNIT_DTYPES)]
        self.luma = bv.derive_bs(units, w, h)
        self._chroma = {}

    def chroma(self, cf):
        if cf not in self._chroma:
            self._chroma[cf] = bv.chroma_bs(self.luma[0], self.luma[1], self.w, self.h, cf)
        return self._chroma[cf]

    def upload(self, ctx):
        bufs = [ctx.alloc(a.nbytes) for a in self.arrs]
        for b, a in zip(bufs, self.arrs):
            b.upload(a)
        return bufs


def chroma_accepted(cf, w, h):
    """include/hevc_deblock.h: 4:2:0 chroma outputs need W and H in multiples of 16, 4:2:2 W in multiples of 16"""
    return cf == 3 or (cf == 2 and w % 16 == 0) or (cf == 1 and w % 16 == 0 and h % 16 == 0)


def guarded(ctx, n):
    b = ctx.alloc(n + 2 * GUARD)
    b.upload(np.full(n + 2 * GUARD, FILL, np.uint8))   # a blocking copy: done before anything is launched
    return b


def derive_on_device(ctx, dev_units, w, h, cf, chroma, *, stream=None, sync=None, plain_entry=False):
    """hevcdbk_h265_derive_bs_device[_cf] into 0xA5-filled outputs with guard bytes on both sides; returns (rc, arrays) after
    checking that the guards came back untouched"""
    from gpu_video_codec_amd import _lib
    L = _lib.lib()
    sx, sy = bv.SUB.get(cf, (1, 1))
    sizes = [(w // 8 + 1) * (h // 4), (h // 8 + 1) * (w // 4)]
    if chroma:
        cw, ch = w // sx, h // sy
        sizes += [(cw // 8 + 1) * (ch // 4), (ch // 8 + 1) * (cw // 4)]
    outs = [guarded(ctx, n) for n in sizes]
    ptrs = [o.ptr + GUARD for o in outs] + [None] * (4 - len(outs))
    un = _lib.H265Units(*[b.ptr for b in dev_units])
    try:
        if plain_entry:
            assert cf == 1
            rc = L.hevcdbk_h265_derive_bs_device(ctx.handle, C.byref(un), w, h, *ptrs, stream)
        else:
            rc = L.hevcdbk_h265_derive_bs_device_cf(ctx.handle, C.byref(un), w, h, cf, *ptrs, stream)
        if sync is None:
            ctx.synchronize()
        else:
            sync()
        res = []
        for o, n in zip(outs, sizes):
            a = o.download()
            assert (a[:GUARD] == FILL).all() and (a[GUARD + n:] == FILL).all(), "guard bytes overwritten"
            res.append(a[GUARD:GUARD + n].copy())
    finally:
        for o in outs:
            o.free()
    return rc, res


def check(res, pic, cf, chroma, tag):
    w, h = pic.w, pic.h
    want = list(pic.luma) + (list(pic.chroma(cf)) if chroma else [])
    assert len(res) == len(want)
    for g, wnt, nm in zip(res, want, ("vert", "hor", "chroma vert", "chroma hor")):
        bad = np.flatnonzero(g != wnt)
        assert not bad.size, (tag, nm, bad.size, bad[:8].tolist(), g[bad[:8]].tolist(), wnt[bad[:8]].tolist())
    # picture-boundary entries are written, as zero, over the 0xA5 the buffers held
    v, hh = res[0].reshape(h // 4, w // 8 + 1), res[1].reshape(h // 8 + 1, w // 4)
    assert not v[:, 0].any() and not v[:, -1].any() and not hh[0].any() and not hh[-1].any(), tag


def all_formats(ctx, pic, dev_units, **kw):
    n = 0
    for fmt, cf in FORMATS:
        for chroma in ((False,) if cf == 0 else (False, True)):
            if chroma and not chroma_accepted(cf, pic.w, pic.h):
                continue
            rc, res = derive_on_device(ctx, dev_units, pic.w, pic.h, cf, chroma, plain_entry=(cf == 1 and chroma), **kw)
            assert rc == 0, (pic.name, fmt, chroma, rc)
            check(res, pic, cf, chroma, (pic.name, fmt, chroma))
            n += 1
    return n


@pytest.fixture(scope="module")
def rule_pictures():
    pics = []
    for name, made in (("product", bv.rule_product()), ("extreme", bv.extreme_cases())):
        for d, (units, w, h) in zip(("vert", "hor"), made):
            pics.append(Pic(name + "_" + d, units, w, h))
    for (w, h, seed, ctb) in ((64, 64, 11, 4), (272, 144, 12, 5), (1920, 1088, 13, 6)):
        pics.append(Pic("coded_%dx%d" % (w, h), bv.coded_picture(w, h, seed, ctb), w, h))
    return pics


def test_rules_every_format_on_the_context_stream(ctx, rule_pictures):
    """derive_bs for 4:0:0 / 4:2:0 / 4:2:2 / 4:4:4, chroma outputs on and off, on the rule product, the extremes and coded
    pictures; outputs pre-filled with 0xA5 between guard bytes"""
    for pic in rule_pictures:
        dev = pic.upload(ctx)
        try:
            assert all_formats(ctx, pic, dev) == 7
        finally:
            for b in dev:
                b.free()
    # the binding a caller uses gives the same arrays
    pic = rule_pictures[0]
    for fmt, cf in FORMATS:
        res = ctx.derive_bs_h265(pic.units, pic.w, pic.h, chroma_format=fmt)
        check(res, pic, cf, cf != 0, ("binding", fmt))


def test_rules_every_format_on_a_callers_stream(ctx, hip, rule_pictures):
    """the same on a second stream created here: the units are uploaded asynchronously on the context's stream and the
    caller's stream is ordered behind that upload by an event"""
    from gpu_video_codec_amd import _lib
    s2, ev = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(s2), 1) == 0    # hipStreamNonBlocking
    assert hip.hipEventCreate(C.byref(ev)) == 0
    compute = C.c_void_p(_lib.lib().hevcdbk_compute_stream(ctx.handle))
    bufs = []
    try:
        for pic in rule_pictures:
            dev = [ctx.alloc(a.nbytes) for a in pic.arrs]
            bufs += dev
            for b, a in zip(dev, pic.arrs):
                assert hip.hipMemcpyAsync(b.ptr, a.ctypes.data, a.nbytes, 1, compute) == 0   # hipMemcpyHostToDevice
            assert hip.hipEventRecord(ev, compute) == 0
            assert hip.hipStreamWaitEvent(s2, ev, 0) == 0
            assert all_formats(ctx, pic, dev, stream=s2, sync=lambda: hip.hipStreamSynchronize(s2)) == 7
    finally:
        hip.hipStreamSynchronize(s2)
        ctx.synchronize()
        hip.hipEventDestroy(ev)
        hip.hipStreamDestroy(s2)
        for b in bufs:
            b.free()


def _sizes_with_entry_counts():
    """pictures whose entry counts sit at the workgroup size's multiples.  nv = (W/8+1) * (H/4) and nh = (H/8+1) * (W/4) are
    always even (H/4 and W/4 are), so 256k - 1 and 256k + 1 cannot occur: the nearest counts, 256k - 2 and 256k + 2, take
    their place next to 256k itself.  For k = 1, 2, 3: the first size found with nv at each target, with nh at it, and with the
    larger of the two (which sizes the grid) at it."""
    out = []
    for k in (1, 2, 3):
        for t in (256 * k - 2, 256 * k, 256 * k + 2):
            found = {}
            for w8 in range(1, 401):
                for h8 in range(1, 401):
                    nv, nh = (w8 + 1) * 2 * h8, (h8 + 1) * 2 * w8
                    if nv == t:
                        found.setdefault("nv", (8 * w8, 8 * h8))
                    if nh == t:
                        found.setdefault("nh", (8 * w8, 8 * h8))
                    if max(nv, nh) == t:                   # what sizes the grid
                        found.setdefault("grid", (8 * w8, 8 * h8))
            assert {"nv", "nh"} <= set(found), (k, t)      # (254 is no picture's larger count: 127 is prime)
            out += sorted(set(found.values()))
    return out


def test_launch_geometry(ctx):
    """the grid is sized by max(nv, nh) and blockIdx.y picks the direction: pictures without an interior edge, with nv and nh
    orders of magnitude apart, with entry counts next to the workgroup size's multiples, and an 8K picture; chroma outputs
    wherever the entry accepts the size"""
    sizes = [(8, 8), (16, 8), (8, 16), (16, 16), (16, 4096), (8192, 16), (4096, 8), (8, 4096)] + _sizes_with_entry_counts()
    for i, (w, h) in enumerate(sizes):
        pic = Pic("geometry_%dx%d" % (w, h), bv.coded_picture(w, h, 100 + i, 4 + i % 3), w, h)
        dev = pic.upload(ctx)
        try:
            assert all_formats(ctx, pic, dev) >= 4
        finally:
            for b in dev:
                b.free()
    w, h = 8192, 4320
    pic = Pic("coded_8k", bv.coded_picture(w, h, 21, 6), w, h)
    assert (pic.luma[0] & 3 == 1).any() and (pic.luma[0] & 3 == 2).any() and (pic.luma[1] & 12).any()
    dev = pic.upload(ctx)
    try:
        assert all_formats(ctx, pic, dev) == 7
    finally:
        for b in dev:
            b.free()


def test_refusals_on_the_other_side_of_the_size_limits(ctx):
    """chroma outputs: 4:2:0 needs W and H in multiples of 16, 4:2:2 W in multiples of 16 -- accepted at the limit (the tests
    above), refused just beyond it with the documented code and with nothing written; luma alone takes every multiple of 8"""
    from gpu_video_codec_amd import _lib
    for (w, h, cf, code) in ((24, 16, 1, _lib.ERR_DIMENSIONS), (16, 24, 1, _lib.ERR_DIMENSIONS), (24, 24, 1, _lib.ERR_DIMENSIONS),
                             (24, 16, 2, _lib.ERR_ARG), (40, 8, 2, _lib.ERR_ARG), (16, 16, 0, _lib.ERR_ARG),
                             (12, 16, 3, _lib.ERR_DIMENSIONS), (16, 12, 3, _lib.ERR_DIMENSIONS), (0, 16, 3, _lib.ERR_DIMENSIONS)):
        W, H = (w // 8 + 2) * 8, (h // 8 + 2) * 8      # unit and output arrays large enough whatever the entry reads
        pic = Pic("refused", bv.coded_picture(W, H, 7, 4), W, H)
        dev = pic.upload(ctx)
        try:
            rc, res = derive_on_device(ctx, dev, w, h, cf, True)
            assert rc == code, (w, h, cf, rc)
            assert all((a == FILL).all() for a in res), (w, h, cf)
            if w % 8 == 0 and h % 8 == 0 and w and h:      # the same size without chroma outputs is fine
                small = Pic("accepted", bv.coded_picture(w, h, 8, 4), w, h)
                d2 = small.upload(ctx)
                rc, res = derive_on_device(ctx, d2, w, h, cf, False)
                for b in d2:
                    b.free()
                assert rc == 0
                check(res, small, cf, False, ("accepted", w, h, cf))
        finally:
            for b in dev:
                b.free()
    # 4:2:2 takes a height that is a multiple of 8 only, 4:4:4 every multiple of 8
    for (w, h, cf) in ((32, 24, 2), (16, 8, 2), (24, 24, 3), (8, 8, 3)):
        pic = Pic("limit", bv.coded_picture(w, h, 9, 4), w, h)
        dev = pic.upload(ctx)
        rc, res = derive_on_device(ctx, dev, w, h, cf, True)
        for b in dev:
            b.free()
        assert rc == 0
        check(res, pic, cf, True, ("limit", w, h, cf))


def blocky(rng, w, h, bd):
    top = (1 << bd) - 1
    base = rng.integers(top // 4, 3 * top // 4, (h // 8 + 1, w // 8 + 1))
    p = np.kron(base, np.ones((8, 8), np.int64))[:h, :w] + rng.integers(-2, 3, (h, w)) * (1 << (bd - 8))
    return np.clip(p, 0, top).astype(np.uint8 if bd == 8 else np.uint16)


def expected_frame(h265, planes, units, cf, qp, bd, qmap, prm):
    """oracle deblocking fed with the NEW reference's bS"""
    y = planes[0]
    h, w = y.shape
    vb, hb = bv.derive_bs(units, w, h)
    out = [h265.filter_plane(y, qp, vb, hb, bit_depth=bd, qp_map=qmap, unit_log2=3, tc_offset_div2=prm["tc_offset_div2"],
                             beta_offset_div2=prm["beta_offset_div2"])]
    if len(planes) == 3:
        cvb, chb = bv.chroma_bs(vb, hb, w, h, cf)
        for c_idx, key in ((1, "cb_qp_offset"), (2, "cr_qp_offset")):
            if cf == 1:
                out.append(h265.filter_plane(planes[c_idx], qp, cvb, chb, c_idx=c_idx, bit_depth=bd, qp_map=qmap, unit_log2=3,
                                             tc_offset_div2=prm["tc_offset_div2"], beta_offset_div2=prm["beta_offset_div2"],
                                             c_qp_offset=prm[key]))
            else:
                out.append(rx.filter_chroma_plane(planes[c_idx], cvb, chb, cf, qp=qp, qp_map=qmap, unit_log2=3, bit_depth=bd,
                                                  tc_offset_div2=prm["tc_offset_div2"], c_qp_offset=prm[key]))
    return out, (vb, hb)


def test_units_route_of_the_host_frame_operator(h265, oracle):
    """filter_frame_h265(units=...) for 4:2:0, 4:2:2, 4:4:4 and luma only, 8 and 10 bit, one QP and a QP map: five uploads into
    one device buffer at computed offsets, reused and grown across calls.  Three calls on ONE context per combination -- a
    large picture, a different unit set of the same size, a smaller picture -- so a stale or mis-offset buffer shows; then a
    default-bS filter_frame of the first size, which must still equal the pinned reference-mode oracle."""
    from gpu_video_codec_amd import deblock
    rng = np.random.default_rng(41)
    prm = dict(tc_offset_div2=1, beta_offset_div2=-2, cb_qp_offset=3, cr_qp_offset=-4)
    big, small = (640, 368), (208, 112)
    with deblock.Context(0) as c:
        for combo, (fmt, cf) in enumerate(FORMATS + (("420", -1),)):      # -1: a 4:2:0 call without chroma planes
            luma_only = cf <= 0
            cf = abs(cf)
            for bd in (8, 10):
                for use_map in (False, True):
                    calls = [(big, 50 + combo), (big, 60 + combo), (small, 70 + combo)]
                    first = None
                    for k, ((w, h), seed) in enumerate(calls):
                        sx, sy = bv.SUB.get(cf, (1, 1))
                        planes = [blocky(rng, w, h, bd)]
                        if not luma_only:
                            planes += [blocky(rng, w // sx, h // sy, bd), blocky(rng, w // sx, h // sy, bd)]
                        units = bv.coded_picture(w, h, seed + 7 * bd + use_map, 4 + k % 3)
                        qp = 30 + 3 * k
                        qmap = rng.integers(22, 50, (h // 8, w // 8)).astype(np.uint8) if use_map else None
                        want, bs = expected_frame(h265, planes, units, cf, qp, bd, qmap, prm)
                        assert (bs[0] & 3 == 1).any() and (bs[0] & 3 == 2).any() and (bs[1] & 3 == 1).any()
                        got = [p.copy() for p in planes]
                        c.filter_frame_h265(*got, qp=qp, bit_depth=bd, units=units, qp_map=qmap, unit_log2=3, chroma_format=fmt, **prm)
                        for g, wnt, nm in zip(got, want, "YUV"):
                            assert np.array_equal(g, wnt), (fmt, luma_only, bd, use_map, k, nm)
                        assert not np.array_equal(got[0], planes[0])
                        if k == 0:
                            first = planes
                    # the reference-exact operator on the same context afterwards: default bS, 4:2:0 geometry of the first size
                    w, h = big
                    y = first[0].copy()
                    if luma_only:
                        c.filter_frame(y, qp=33, bit_depth=bd)
                    else:
                        u, v = blocky(rng, w // 2, h // 2, bd), blocky(rng, w // 2, h // 2, bd)
                        gu, gv = u.copy(), v.copy()
                        c.filter_frame(y, gu, gv, qp=33, bit_depth=bd)
                        assert np.array_equal(gu, oracle.filter_plane(u, 33, is_chroma=True, bit_depth=bd))
                        assert np.array_equal(gv, oracle.filter_plane(v, 33, is_chroma=True, bit_depth=bd))
                    assert np.array_equal(y, oracle.filter_plane(first[0], 33, bit_depth=bd)), (fmt, bd, use_map, "default bS")


@pytest.mark.parametrize("fmt,cf", [("420", 1), ("444", 3)])
def test_decoders_chain_on_device_memory(ctx, h265, fmt, cf):
    """units -> derive_bs_h265 -> deblocking + SAO in one fused launch, everything in device memory, against the new
    reference's bS -> oracle deblocking -> oracle SAO"""
    from gpu_video_codec_amd import _lib, deblock
    rng = np.random.default_rng(90 + cf)
    sx, sy = bv.SUB[cf]
    prm_h = dict(tc_offset_div2=-1, beta_offset_div2=2, cb_qp_offset=-3, cr_qp_offset=5)
    for (w, h, bd, ctb, seed) in ((416, 240, 8, 6, 1), (272, 144, 10, 5, 2), (1920, 1088, 8, 6, 3)):
        units = bv.coded_picture(w, h, 200 + seed + cf, ctb)
        pic = Pic("chain", units, w, h)
        dev_units = pic.upload(ctx)
        cw, ch = w // sx, h // sy
        sizes = [(w // 8 + 1) * (h // 4), (h // 8 + 1) * (w // 4), (cw // 8 + 1) * (ch // 4), (ch // 8 + 1) * (cw // 4)]
        outs = [guarded(ctx, n) for n in sizes]
        un = _lib.H265Units(*[b.ptr for b in dev_units])
        assert _lib.lib().hevcdbk_h265_derive_bs_device_cf(ctx.handle, C.byref(un), w, h, cf, *[o.ptr + GUARD for o in outs], None) == 0
        qp = 36
        batches, planes, sao, want, keep = [], [], [], [], []
        cvb, chb = pic.chroma(cf)
        for i in range(3):
            pw, ph = (w, h) if i == 0 else (cw, ch)
            lw, lh = (ctb, ctb) if i == 0 else (ctb - (sx - 1), ctb - (sy - 1))
            fr = blocky(rng, pw, ph, bd)
            b = deblock.DeviceBatch(ctx, pw, ph, 1, bit_depth=bd, is_chroma=i > 0, per_frame_bs=False)
            b.upload_all(fr[None])
            p = b.planes()
            p.vert_bs, p.hor_bs = (outs[0].ptr + GUARD, outs[1].ptr + GUARD) if i == 0 else (outs[2].ptr + GUARD, outs[3].ptr + GUARD)
            p.vert_bs_stride = p.hor_bs_stride = 0
            sp = rx.random_sao_params(pw, ph, lw, lh, rng, bd)
            dp = ctx.alloc(sp.nbytes)
            dp.upload(np.ascontiguousarray(sp).view(np.uint8))
            keep.append(dp)
            batches.append(b)
            planes.append(p)
            sao.append({"params": dp.ptr, "params_stride": sp.shape[1], "ctb_log2": lw})
            if i == 0:
                d = h265.filter_plane(fr, qp, pic.luma[0], pic.luma[1], bit_depth=bd, tc_offset_div2=-1, beta_offset_div2=2)
            else:
                d = rx.filter_chroma_plane(fr, cvb, chb, cf, qp=qp, bit_depth=bd, tc_offset_div2=-1,
                                           c_qp_offset=prm_h["cb_qp_offset"] if i == 1 else prm_h["cr_qp_offset"])
            assert not np.array_equal(d, fr)
            want.append(rx.sao_plane(d, sp, lw, lh, bit_depth=bd))
        try:
            ctx.deblock_sao_device_planes(planes, qp, sao, h265=prm_h, fused=_lib.FUSED_ON, chroma_format=fmt)
            ctx.synchronize()
            for i, b in enumerate(batches):
                assert np.array_equal(b.download_frame(0), want[i]), (fmt, w, h, bd, "YUV"[i])
            # the bS arrays the chain read are the reference's, and their guards are intact
            for o, n, wnt in zip(outs, sizes, list(pic.luma) + [cvb, chb]):
                a = o.download()
                assert (a[:GUARD] == FILL).all() and (a[GUARD + n:] == FILL).all() and np.array_equal(a[GUARD:GUARD + n], wnt)
        finally:
            for x in batches + keep + outs + dev_units:
                x.free()
