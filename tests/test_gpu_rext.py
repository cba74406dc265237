"""Chroma formats 4:0:0 / 4:2:2 / 4:4:4 of the spec-exact mode and SAO on the GPU, through the C ABI (the _cf entries),
against tests/rext_oracle.py (chroma) and oracle/h265.py (luma).  PARITY UNPINNED, like the rest of the spec-exact mode."""
import numpy as np
import pytest

import rext_oracle as rx

pytestmark = pytest.mark.gpu

FMT = {"422": 2, "444": 3}


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


def blocky(rng, w, h, bd):
    top = (1 << bd) - 1
    base = rng.integers(top // 4, 3 * top // 4, (h // 8 + 1, w // 8 + 1))
    p = np.kron(base, np.ones((8, 8), np.int64))[:h, :w] + rng.integers(-2, 3, (h, w)) * (1 << (bd - 8))
    p[: h // 4, : w // 4] = rng.integers(0, top + 1, (h // 4, w // 4))
    return np.clip(p, 0, top).astype(np.uint8 if bd == 8 else np.uint16)


def rand_bs(rng, w, h):
    nv, nh = (w // 8 + 1) * (h // 4), (h // 8 + 1) * (w // 4)
    mk = lambda n: (rng.integers(0, 3, n) | (rng.integers(0, 10, n) == 0) * rx.KEEP_P | (rng.integers(0, 10, n) == 0) * rx.KEEP_Q)
    return mk(nv).astype(np.uint8), mk(nh).astype(np.uint8)


class Plane:
    """n frames of one plane in HBM (src -> dst) with shared spec-exact bS arrays and an optional QP map"""

    def __init__(self, ctx, frames, bd, chroma, vb, hb, qp_map=None, unit_log2=3, in_place=False):
        from gpu_video_codec_amd import deblock
        n, h, w = frames.shape
        self.b = deblock.DeviceBatch(ctx, w, h, n, bit_depth=bd, is_chroma=chroma, per_frame_bs=False, in_place=in_place)
        self.b.upload_all(frames)
        self.bufs = [ctx.alloc(max(vb.size, 1)), ctx.alloc(max(hb.size, 1))]
        self.bufs[0].upload(vb)
        self.bufs[1].upload(hb)
        if qp_map is not None:
            self.b.set_qp_map(qp_map, unit_log2)

    def planes(self):
        p = self.b.planes()
        p.vert_bs, p.hor_bs, p.vert_bs_stride, p.hor_bs_stride = self.bufs[0].ptr, self.bufs[1].ptr, 0, 0
        return p

    def out(self, f):
        return self.b.download_frame(f)

    def free(self):
        for x in self.bufs:
            x.free()
        if self.b.qp_map is not None:
            self.b.qp_map.free()
        self.b.free()


def upload_params(ctx, prm):
    a = np.ascontiguousarray(prm)
    d = ctx.alloc(a.nbytes)
    d.upload(a.view(np.uint8))
    return d


def test_derive_bs_formats(ctx, h265):
    for cf_name, cf in (("400", 0), ("420", 1), ("422", 2), ("444", 3)):
        for (w, h) in [(64, 32), (96, 80), (208, 64)]:  # 4:2:0 entry: multiples of 16
            units = h265.random_units(w, h, seed=w + cf)
            vb, hb = h265.derive_bs(*units, w, h)
            res = ctx.derive_bs_h265(units, w, h, chroma_format=cf_name)
            assert np.array_equal(res[0], vb) and np.array_equal(res[1], hb)
            if cf == 0:
                assert len(res) == 2
            else:
                cv, ch = rx.chroma_bs(vb, hb, w, h, cf)
                assert np.array_equal(res[2], cv) and np.array_equal(res[3], ch), (cf_name, w, h)


@pytest.mark.parametrize("fmt", ["422", "444"])
def test_device_filter_generic_and_packed(ctx, fmt):
    from gpu_video_codec_amd import _lib, deblock
    cf = FMT[fmt]
    sx, sy = rx.SUB[cf]
    rng = np.random.default_rng(30 + cf)
    for (w, h) in [(64, 48), (208, 72), (1040, 136)]:
        cw, ch = w // sx, h // sy
        for bd in (8, 10, 12):
            frames = np.stack([blocky(rng, cw, ch, bd) for _ in range(2)])
            vb, hb = rand_bs(rng, cw, ch)
            for qp, tco, cb, cr in ((27, 0, 0, 0), (33, 2, 5, -3), (44, -3, 12, -12), (51, 6, 0, 0)):
                for c_idx in (1, 2):
                    coff = cb if c_idx == 1 else cr
                    want = [rx.filter_chroma_plane(frames[f], vb, hb, cf, qp=qp, bit_depth=bd, tc_offset_div2=tco, c_qp_offset=coff)
                            for f in range(2)]
                    for variant in (_lib.KERNEL_GENERIC, _lib.KERNEL_PACKED, _lib.KERNEL_AUTO):
                        pl = Plane(ctx, frames, bd, True, vb, hb)
                        ctx.filter_device_h265(pl.planes(), qp, c_idx=c_idx, tc_offset_div2=tco, cb_qp_offset=cb, cr_qp_offset=cr,
                                               variant=variant, chroma_format=fmt)
                        ctx.synchronize()
                        for f in range(2):
                            assert np.array_equal(pl.out(f), want[f]), (fmt, w, h, bd, qp, c_idx, variant)
                        pl.free()
            # QP map: values that put qPi on both sides of 30; the 32-bit kernel and the format's packed kernels
            for u in (3, 4, 6):
                m = rng.integers(22, 52, (-(-h >> u), -(-w >> u))).astype(np.uint8)
                want = [rx.filter_chroma_plane(frames[f], vb, hb, cf, qp_map=m, unit_log2=u, bit_depth=bd, c_qp_offset=4, tc_offset_div2=1)
                        for f in range(2)]
                for variant in (_lib.KERNEL_GENERIC, _lib.KERNEL_PACKED, _lib.KERNEL_AUTO):
                    pl = Plane(ctx, frames, bd, True, vb, hb, qp_map=m, unit_log2=u)
                    ctx.filter_device_h265(pl.planes(), 0, c_idx=1, cb_qp_offset=4, tc_offset_div2=1, variant=variant, chroma_format=fmt)
                    ctx.synchronize()
                    for f in range(2):
                        assert np.array_equal(pl.out(f), want[f]), (fmt, w, h, bd, u, variant)
                    pl.free()


@pytest.mark.parametrize("fmt", ["420", "422", "444"])
def test_sao_ctb_sizes(ctx, fmt):
    cf = {"420": 1, "422": 2, "444": 3}[fmt]
    sx, sy = rx.SUB[cf]
    rng = np.random.default_rng(40 + cf)
    for (w, h) in [(128, 64), (336, 208)]:
        cw, ch = w // sx, h // sy
        for ctb_y in (4, 5, 6):
            lw, lh = ctb_y - (sx - 1), ctb_y - (sy - 1)
            for bd in (8, 10):
                n = 2
                frames = np.stack([blocky(rng, cw, ch, bd) for _ in range(n)])
                prm = np.stack([rx.random_sao_params(cw, ch, lw, lh, rng, bd) for _ in range(n)])
                keep = (rng.integers(0, 6, (n, ch // 8, cw // 8)) == 0).astype(np.uint8)
                dp, dk = upload_params(ctx, prm), ctx.alloc(keep.nbytes)
                dk.upload(keep)
                pl = Plane(ctx, frames, bd, True, np.zeros(1, np.uint8), np.zeros(1, np.uint8))
                ctx.sao_device(pl.planes(), dp.ptr, prm.shape[2], lw, params_frame_stride=prm.shape[1] * prm.shape[2], keep_ptr=dk.ptr,
                               keep_stride=cw // 8, keep_frame_stride=keep[0].size, chroma_format=fmt)
                ctx.synchronize()
                for f in range(n):
                    want = rx.sao_plane(frames[f], prm[f], lw, lh, bit_depth=bd, keep=keep[f])
                    assert np.array_equal(pl.out(f), want), (fmt, w, h, ctb_y, bd, f)
                pl.free()
                dp.free()
                dk.free()


def _batch(ctx, h265, rng, fmt, w, h, n, bd, qp_map=None, unit_log2=3, ctb_y=6):
    """Y, Cb, Cr of n frames in format fmt with their operands and the expected deblocking + SAO output"""
    cf = FMT.get(fmt, 1)
    sx, sy = rx.SUB[cf]
    cw, ch = w // sx, h // sy
    prm_h = dict(tc_offset_div2=1, beta_offset_div2=-1, cb_qp_offset=3, cr_qp_offset=-2)
    units = h265.random_units(w, h, seed=w + h + cf)
    vb, hb = h265.derive_bs(*units, w, h)
    cvb, chb = rx.chroma_bs(vb, hb, w, h, cf)
    qp = 37
    planes, sao, want, keepalive = [], [], [], []
    for i in range(3):
        pw, ph = (w, h) if i == 0 else (cw, ch)
        lw, lh = (ctb_y, ctb_y) if i == 0 else (ctb_y - (sx - 1), ctb_y - (sy - 1))
        frames = np.stack([blocky(rng, pw, ph, bd) for _ in range(n)])
        prm = np.stack([rx.random_sao_params(pw, ph, lw, lh, rng, bd) for _ in range(n)])
        b_v, b_h = (vb, hb) if i == 0 else (cvb, chb)
        pl = Plane(ctx, frames, bd, i > 0, b_v, b_h, qp_map=qp_map, unit_log2=unit_log2)
        dp = upload_params(ctx, prm)
        keepalive += [pl, dp]
        planes.append(pl)
        sao.append({"params": dp.ptr, "params_stride": prm.shape[2], "ctb_log2": lw, "params_frame_stride": prm.shape[1] * prm.shape[2]})
        for f in range(n):
            if i == 0:
                d = h265.filter_plane(frames[f], qp, vb, hb, bit_depth=bd, qp_map=qp_map, unit_log2=unit_log2,
                                      tc_offset_div2=1, beta_offset_div2=-1)
            else:
                d = rx.filter_chroma_plane(frames[f], cvb, chb, cf, qp=qp, qp_map=qp_map, unit_log2=unit_log2, bit_depth=bd,
                                           tc_offset_div2=1, c_qp_offset=3 if i == 1 else -2)
            want.append(rx.sao_plane(d, prm[f], lw, lh, bit_depth=bd))
    return planes, sao, want, keepalive, qp, prm_h


def _check(planes, want, n, tag):
    for i in range(3):
        for f in range(n):
            assert np.array_equal(planes[i].out(f), want[i * n + f]), (tag, i, f)


@pytest.mark.parametrize("fmt", ["422", "444"])
def test_deblock_sao_planes_fused_modes(ctx, h265, fmt):
    from gpu_video_codec_amd import _lib, deblock
    rng = np.random.default_rng(50 + FMT[fmt])
    for (w, h, bd, ctb_y) in [(192, 128, 8, 6), (400, 136, 8, 5), (272, 120, 10, 4), (320, 64, 12, 6)]:
        n = 2
        planes, sao, want, keep, qp, prm_h = _batch(ctx, h265, rng, fmt, w, h, n, bd, ctb_y=ctb_y)
        for fused in (_lib.FUSED_ON, _lib.FUSED_AUTO, _lib.FUSED_OFF):
            for pl in planes:
                pl.b.dst.upload(np.zeros(pl.b.frame_bytes * n, np.uint8))
            ctx.deblock_sao_device_planes([p.planes() for p in planes], qp, sao, h265=prm_h, fused=fused, chroma_format=fmt)
            ctx.synchronize()
            _check(planes, want, n, (fmt, w, h, bd, ctb_y, fused))
        # one plane at a time, through hevcdbk_h265_deblock_sao_device_cf
        for i, pl in enumerate(planes):
            pl.b.dst.upload(np.zeros(pl.b.frame_bytes * n, np.uint8))
            ctx.deblock_sao_h265_device(pl.planes(), qp, sao[i]["params"], sao[i]["params_stride"], sao[i]["ctb_log2"], c_idx=i,
                                        params_frame_stride=sao[i]["params_frame_stride"], chroma_format=fmt, fused=_lib.FUSED_ON, **prm_h)
        ctx.synchronize()
        _check(planes, want, n, (fmt, w, h, "single"))
        for x in keep:
            x.free()
    # a QP map (qPi on both sides of 30): the format's fused kernels, and the two launches, at 8, 10 and 12 bit
    for bd, u in ((8, 3), (10, 4), (12, 6)):
        planes, sao, want, keep, qp, prm_h = _batch(ctx, h265, rng, fmt, 256, 128, 2, bd,
                                                    qp_map=rng.integers(20, 52, (-(-128 >> u), -(-256 >> u))).astype(np.uint8), unit_log2=u)
        for fused in (_lib.FUSED_ON, _lib.FUSED_AUTO, _lib.FUSED_OFF):
            for pl in planes:
                pl.b.dst.upload(np.zeros(pl.b.frame_bytes * 2, np.uint8))
            ctx.deblock_sao_device_planes([p.planes() for p in planes], qp, sao, h265=prm_h, fused=fused, chroma_format=fmt)
            ctx.synchronize()
            _check(planes, want, 2, (fmt, "map", bd, fused))
        for i, pl in enumerate(planes):
            pl.b.dst.upload(np.zeros(pl.b.frame_bytes * 2, np.uint8))
            ctx.deblock_sao_h265_device(pl.planes(), qp, sao[i]["params"], sao[i]["params_stride"], sao[i]["ctb_log2"], c_idx=i,
                                        params_frame_stride=sao[i]["params_frame_stride"], chroma_format=fmt, fused=_lib.FUSED_ON, **prm_h)
        ctx.synchronize()
        _check(planes, want, 2, (fmt, "map", bd, "single"))
        for x in keep:
            x.free()


def test_host_frame_operator(ctx, h265):
    rng = np.random.default_rng(60)
    for fmt in ("400", "422", "444"):
        cf = {"400": 0, "422": 2, "444": 3}[fmt]
        for (w, h, bd) in [(16, 8, 8), (48, 24, 10), (272, 88, 8), (336, 40, 12)]:
            y = blocky(rng, w, h, bd)
            units = h265.random_units(w, h, seed=w * 3 + cf)
            vb, hb = h265.derive_bs(*units, w, h)
            m = rng.integers(20, 52, (-(-h >> 3), -(-w >> 3))).astype(np.uint8)
            for use_units, qmap in ((True, None), (False, m)):
                wy = h265.filter_plane(y, 40, vb, hb, bit_depth=bd, qp_map=qmap, unit_log2=3, tc_offset_div2=-1)
                kw = dict(qp=40, bit_depth=bd, qp_map=qmap, unit_log2=3, tc_offset_div2=-1, cb_qp_offset=2, cr_qp_offset=-5,
                          chroma_format=fmt)
                kw.update(dict(units=units) if use_units else dict(vert_bs4=vb, hor_bs4=hb))
                gy = y.copy()
                if cf == 0:
                    ctx.filter_frame_h265(gy, **kw)
                    assert np.array_equal(gy, wy), (fmt, w, h)
                    continue
                sx, sy = rx.SUB[cf]
                u, v = blocky(rng, w // sx, h // sy, bd), blocky(rng, w // sx, h // sy, bd)
                cvb, chb = rx.chroma_bs(vb, hb, w, h, cf)
                wu = rx.filter_chroma_plane(u, cvb, chb, cf, qp=40, qp_map=qmap, unit_log2=3, bit_depth=bd, tc_offset_div2=-1, c_qp_offset=2)
                wv = rx.filter_chroma_plane(v, cvb, chb, cf, qp=40, qp_map=qmap, unit_log2=3, bit_depth=bd, tc_offset_div2=-1, c_qp_offset=-5)
                gu, gv = u.copy(), v.copy()
                ctx.filter_frame_h265(gy, gu, gv, **kw)
                assert np.array_equal(gy, wy) and np.array_equal(gu, wu) and np.array_equal(gv, wv), (fmt, w, h, bd, use_units)


def test_4k_422_10bit_batch(ctx, h265):
    """one 3840x2160 4:2:2 10-bit batch of several frames, one QP, deblocking + SAO in one call: every byte against the oracles"""
    from gpu_video_codec_amd import _lib
    rng = np.random.default_rng(70)
    n = 3
    planes, sao, want, keep, qp, prm_h = _batch(ctx, h265, rng, "422", 3840, 2160, n, 10, ctb_y=6)
    ctx.deblock_sao_device_planes([p.planes() for p in planes], qp, sao, h265=prm_h, fused=_lib.FUSED_ON, chroma_format="422")
    ctx.synchronize()
    _check(planes, want, n, "4k422")
    for x in keep:
        x.free()


def test_420_cf_entries_equal_existing_entries(ctx, h265):
    """every _cf entry with format 4:2:0 gives the bytes of the existing entry on the same operands"""
    from gpu_video_codec_amd import _lib
    import ctypes as C
    L = _lib.lib()
    rng = np.random.default_rng(80)
    w, h, bd, n = 272, 144, 10, 2
    # bS derivation
    units = h265.random_units(w, h, seed=5)
    a = ctx.derive_bs_h265(units, w, h)
    arrs = [np.ascontiguousarray(x, dt) for x, dt in zip(units, (np.uint16, np.int16, np.int16, np.int32, np.int32))]
    bufs = [ctx.alloc(x.nbytes) for x in arrs]
    for b_, x in zip(bufs, arrs):
        b_.upload(x)
    outs = [ctx.alloc(len(x)) for x in a]
    un = _lib.H265Units(*[b_.ptr for b_ in bufs])
    assert L.hevcdbk_h265_derive_bs_device_cf(ctx.handle, C.byref(un), w, h, 1, outs[0].ptr, outs[1].ptr, outs[2].ptr, outs[3].ptr, None) == 0
    ctx.synchronize()
    for o, x in zip(outs, a):
        assert np.array_equal(o.download(len(x)), x)
    for b_ in bufs + outs:
        b_.free()
    # device filter, SAO, deblocking + SAO
    c = np.stack([blocky(rng, w // 2, h // 2, bd) for _ in range(n)])
    vb, hb = rand_bs(rng, w // 2, h // 2)
    prm = np.stack([rx.random_sao_params(w // 2, h // 2, 5, 5, rng, bd) for _ in range(n)])
    dp = upload_params(ctx, prm)
    p1, p2 = Plane(ctx, c, bd, True, vb, hb), Plane(ctx, c, bd, True, vb, hb)
    hp = _lib.H265Params(1, 0, 4, -3)
    for variant in (_lib.KERNEL_GENERIC, _lib.KERNEL_PACKED):
        assert L.hevc_deblocking_filter_h265_device(ctx.handle, C.byref(p1.planes()), 2, 41, C.byref(hp), variant, None) == 0
        assert L.hevcdbk_h265_filter_device_cf(ctx.handle, C.byref(p2.planes()), 2, 1, 41, C.byref(hp), variant, None) == 0
        ctx.synchronize()
        for f in range(n):
            assert np.array_equal(p1.out(f), p2.out(f))
    fs = prm.shape[1] * prm.shape[2]
    assert L.hevc_sao_filter_device(ctx.handle, C.byref(p1.planes()), dp.ptr, prm.shape[2], fs, 5, None, 0, 0, None) == 0
    assert L.hevcdbk_sao_filter_device_cf(ctx.handle, C.byref(p2.planes()), dp.ptr, prm.shape[2], fs, 5, 5, None, 0, 0, None) == 0
    ctx.synchronize()
    for f in range(n):
        assert np.array_equal(p1.out(f), p2.out(f))
    for fused in (_lib.FUSED_ON, _lib.FUSED_OFF):
        assert L.hevc_deblock_sao_h265_device(ctx.handle, C.byref(p1.planes()), 1, 41, C.byref(hp), dp.ptr, prm.shape[2], fs, 5, None, 0,
                                              0, fused, None) == 0
        assert L.hevcdbk_h265_deblock_sao_device_cf(ctx.handle, C.byref(p2.planes()), 1, 1, 41, C.byref(hp), dp.ptr, prm.shape[2], fs, 5, 5,
                                                 None, 0, 0, fused, None) == 0
        ctx.synchronize()
        for f in range(n):
            assert np.array_equal(p1.out(f), p2.out(f))
    p1.free()
    p2.free()
    dp.free()
    # the planes form and the host-frame operator
    r1, r2 = np.random.default_rng(81), np.random.default_rng(81)
    A = _batch(ctx, h265, r1, "420", 256, 128, 2, 8)
    B = _batch(ctx, h265, r2, "420", 256, 128, 2, 8)
    ctx.deblock_sao_device_planes([p.planes() for p in A[0]], A[4], A[1], h265=A[5])
    sp = (_lib.SaoPlaneCf * 3)()
    for i, d in enumerate(B[1]):
        sp[i].params, sp[i].params_stride, sp[i].ctb_log2_w, sp[i].ctb_log2_h = d["params"], d["params_stride"], d["ctb_log2"], d["ctb_log2"]
        sp[i].params_frame_stride = d["params_frame_stride"]
    arr = (_lib.DevicePlanes * 3)(*[p.planes() for p in B[0]])
    hp = _lib.H265Params(1, -1, 3, -2)
    assert L.hevcdbk_h265_deblock_sao_device_planes_cf(ctx.handle, arr, 3, 1, B[4], C.byref(hp), sp, _lib.FUSED_AUTO, None) == 0
    ctx.synchronize()
    for i in range(3):
        for f in range(2):
            assert np.array_equal(A[0][i].out(f), B[0][i].out(f))
    for x in A[3] + B[3]:
        x.free()
    y, u, v = blocky(rng, w, h, 8), blocky(rng, w // 2, h // 2, 8), blocky(rng, w // 2, h // 2, 8)
    units = h265.random_units(w, h, seed=9)
    g1 = [y.copy(), u.copy(), v.copy()]
    g2 = [y.copy(), u.copy(), v.copy()]
    ctx.filter_frame_h265(*g1, qp=38, units=units, cb_qp_offset=2)
    fr = _lib.Frame()
    fr.height, fr.width, fr.bit_depth, fr.sample_bytes = h, w, 8, 1
    for i, p in enumerate(g2):
        fr.plane[i], fr.pitch[i] = p.ctypes.data, p.strides[0]
    un = _lib.H265Units()
    keep_arrs = []
    for nm, x, dt in zip(("flags", "mv0", "mv1", "ref0", "ref1"), units, (np.uint16, np.int16, np.int16, np.int32, np.int32)):
        aa = np.ascontiguousarray(x, dt)
        keep_arrs.append(aa)
        setattr(un, nm, aa.ctypes.data)
    q = _lib.Qp()
    q.qp, q.ctu_log2 = 38, 3
    assert L.hevcdbk_h265_filter_frame_cf(ctx.handle, C.byref(fr), 1, C.byref(un), None, C.byref(q), C.byref(_lib.H265Params(0, 0, 2, 0)),
                                            None) == 0
    for a_, b_ in zip(g1, g2):
        assert np.array_equal(a_, b_)


def test_argument_errors(ctx, h265):
    from gpu_video_codec_amd import _lib
    import ctypes as C
    L = _lib.lib()
    rng = np.random.default_rng(90)
    c = np.stack([blocky(rng, 32, 32, 8)])
    vb, hb = rand_bs(rng, 32, 32)
    pl = Plane(ctx, c, 8, True, vb, hb)
    hp = _lib.H265Params(0, 0, 0, 0)
    ARG = _lib.ERR_ARG
    for cf in (-1, 4):
        assert L.hevcdbk_h265_filter_device_cf(ctx.handle, C.byref(pl.planes()), 1, cf, 30, C.byref(hp), 0, None) == ARG
    assert L.hevcdbk_h265_filter_device_cf(ctx.handle, C.byref(pl.planes()), 1, 0, 30, C.byref(hp), 0, None) == ARG  # 4:0:0 chroma
    prm = rx.random_sao_params(32, 32, 4, 5, rng)
    dp = upload_params(ctx, prm)
    assert L.hevcdbk_sao_filter_device_cf(ctx.handle, C.byref(pl.planes()), dp.ptr, 1, 0, 4, 5, None, 0, 0, None) == ARG  # stride < 2 columns
    assert L.hevcdbk_sao_filter_device_cf(ctx.handle, C.byref(pl.planes()), dp.ptr, 2, 0, 4, 6, None, 0, 0, None) == ARG  # not w or 2w tall
    assert L.hevcdbk_sao_filter_device_cf(ctx.handle, C.byref(pl.planes()), dp.ptr, 2, 0, 5, 4, None, 0, 0, None) == ARG  # wider than tall
    # a frame whose 4:2:2 chroma plane is not a multiple of 8 wide (W = 24), and chroma planes with 4:0:0
    y, u, v = blocky(rng, 24, 16, 8), blocky(rng, 12, 16, 8), blocky(rng, 12, 16, 8)
    fr = _lib.Frame()
    fr.height, fr.width, fr.bit_depth, fr.sample_bytes = 16, 24, 8, 1
    for i, p in enumerate((y, u, v)):
        fr.plane[i], fr.pitch[i] = p.ctypes.data, p.strides[0]
    lv, lh = np.zeros(h265.num_vert_bs(24, 16), np.uint8), np.zeros(h265.num_hor_bs(24, 16), np.uint8)
    bs = _lib.Bs()
    bs.vert, bs.n_vert, bs.hor, bs.n_hor = lv.ctypes.data, lv.size, lh.ctypes.data, lh.size
    q = _lib.Qp()
    q.qp = 30
    assert L.hevcdbk_h265_filter_frame_cf(ctx.handle, C.byref(fr), 2, None, C.byref(bs), C.byref(q), C.byref(hp), None) == ARG
    assert L.hevcdbk_h265_filter_frame_cf(ctx.handle, C.byref(fr), 0, None, C.byref(bs), C.byref(q), C.byref(hp), None) == ARG
    assert L.hevcdbk_h265_filter_frame_cf(ctx.handle, C.byref(fr), 5, None, C.byref(bs), C.byref(q), C.byref(hp), None) == ARG
    # chroma planes of the wrong geometry for the format in the planes call
    A = _batch(ctx, h265, rng, "444", 64, 32, 1, 8)
    sp = (_lib.SaoPlaneCf * 3)()
    for i, d in enumerate(A[1]):
        sp[i].params, sp[i].params_stride, sp[i].ctb_log2_w, sp[i].ctb_log2_h = d["params"], d["params_stride"], d["ctb_log2"], d["ctb_log2"]
    arr = (_lib.DevicePlanes * 3)(*[p.planes() for p in A[0]])
    assert L.hevcdbk_h265_deblock_sao_device_planes_cf(ctx.handle, arr, 3, 2, 30, C.byref(hp), sp, 0, None) == ARG  # 4:4:4 planes as 4:2:2
    assert L.hevcdbk_h265_deblock_sao_device_planes_cf(ctx.handle, arr, 3, 0, 30, C.byref(hp), sp, 0, None) == ARG  # chroma with 4:0:0
    for x in A[3]:
        x.free()
    pl.free()
    dp.free()


def _kernels_enqueued(call):
    """number of kernels call(stream) puts on a fresh stream (tests/kernel_capture.py: captured, never launched)"""
    from kernel_capture import kernel_count
    return kernel_count(call)


@pytest.mark.parametrize("fmt,use_map", [("420", False), ("420", True), ("444", False), ("444", True)])
def test_fused_on_is_one_launch(ctx, h265, fmt, use_map):
    """FUSED_ON of Y + Cb + Cr through hevcdbk_h265_deblock_sao_device_planes_cf enqueues ONE kernel, with one QP and with a QP
    map (a regression to one fused launch per plane would enqueue three); the bytes are the oracle's"""
    from gpu_video_codec_amd import _lib
    import ctypes as C
    L = _lib.lib()
    rng = np.random.default_rng(95)
    cf = {"420": 1, "444": 3}[fmt]
    w, h = 256, 128
    qmap = rng.integers(20, 52, (h // 8, w // 8)).astype(np.uint8) if use_map else None
    planes, sao, want, keep, qp, prm_h = _batch(ctx, h265, rng, fmt, w, h, 2, 8, qp_map=qmap, unit_log2=3)
    sp = (_lib.SaoPlaneCf * 3)()
    for i, d in enumerate(sao):
        sp[i].params, sp[i].params_stride, sp[i].ctb_log2_w, sp[i].ctb_log2_h = d["params"], d["params_stride"], d["ctb_log2"], d["ctb_log2"]
        sp[i].params_frame_stride = d["params_frame_stride"]
    arr = (_lib.DevicePlanes * 3)(*[p.planes() for p in planes])
    hp = _lib.H265Params(prm_h["tc_offset_div2"], prm_h["beta_offset_div2"], prm_h["cb_qp_offset"], prm_h["cr_qp_offset"])
    call = lambda stream: L.hevcdbk_h265_deblock_sao_device_planes_cf(ctx.handle, arr, 3, cf, qp, C.byref(hp), sp, _lib.FUSED_ON, stream)
    assert call(None) == 0  # first use of the context's resources outside the capture
    ctx.synchronize()
    rc, kernels = _kernels_enqueued(call)
    assert rc == 0 and kernels == 1, (rc, kernels)
    _check(planes, want, 2, (fmt, use_map))
    for x in keep:
        x.free()


def _scratch_422_on_two_streams():
    """the body of test_422_parameter_scratch_on_two_caller_streams, run in a process of its own"""
    import ctypes as C
    from gpu_video_codec_amd import _lib, deblock
    L = _lib.lib()
    hip = C.CDLL("libamdhip64.so")
    hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    # a context of its own: grow_device never shrinks, so on a context that an earlier 4:2:2 call has used the scratch may
    # already hold the large plane's grid.  Here the first small call allocates exactly what it needs (4 x 8 x 2 entries), the
    # other small one less, and the large plane (16 x 32 x 2 entries) finds it too small
    ctx = deblock.Context(0)
    streams, cases = [], []
    try:
        for _ in range(2):
            s = C.c_void_p()
            assert hip.hipStreamCreateWithFlags(C.byref(s), 1) == 0   # hipStreamNonBlocking
            streams.append(s)
        rng = np.random.default_rng(422)
        cf, lw, lh, bd, n, qp = 2, 4, 5, 8, 2, 35
        hp = _lib.H265Params(1, -1, 3, -2)
        # (plane, parameters on the device, parameters, expected frames, deblocked first)
        for (w, h, dbk) in ((64, 128, False), (32, 64, True), (256, 512, False)):   # the third is the large one
            frames = np.stack([blocky(rng, w, h, bd) for _ in range(n)])
            prm = np.stack([rx.random_sao_params(w, h, lw, lh, rng, bd) for _ in range(n)])
            vb, hb = rand_bs(rng, w, h)
            pl = Plane(ctx, frames, bd, True, vb, hb)
            dp = upload_params(ctx, prm)
            want = []
            for f in range(n):
                d = rx.filter_chroma_plane(frames[f], vb, hb, cf, qp=qp, bit_depth=bd, tc_offset_div2=1, c_qp_offset=3) if dbk else frames[f]
                want.append(rx.sao_plane(d, prm[f], lw, lh, bit_depth=bd))
            cases.append((pl, dp, prm, want, dbk))
        entries = [2 * (-(-pl.b.w >> lw)) * (-(-pl.b.h >> lw)) for pl, _d, _p, _w, _k in cases]   # of the doubled grid, both frames
        assert entries[1] < entries[0] < entries[2], entries
        ctx.synchronize()   # the uploads are done; from here on nothing synchronises with the host until the end

        def call(k, stream):
            pl, dp, prm, _want, dbk = cases[k]
            planes = pl.planes()
            stride, frame_stride = prm.shape[2], prm.shape[1] * prm.shape[2]
            if dbk:
                rc = L.hevcdbk_h265_deblock_sao_device_cf(ctx.handle, C.byref(planes), 1, cf, qp, C.byref(hp), dp.ptr, stride, frame_stride, lw, lh,
                                                          None, 0, 0, _lib.FUSED_AUTO, stream)
            else:
                rc = L.hevcdbk_sao_filter_device_cf(ctx.handle, C.byref(planes), dp.ptr, stride, frame_stride, lw, lh, None, 0, 0, stream)
            assert rc == 0, (k, rc, L.hevcdbk_last_error(ctx.handle))
        for rnd in range(6):
            call(0, streams[0])      # the first of them is the scratch's first use
            call(1, streams[1])
        call(2, streams[0])          # the scratch grows: the library waits for the event of the last small call first
        for rnd in range(2):
            call(1, streams[1])
            call(0, streams[0])
            call(2, streams[1])      # ... and the large one on the other stream, fenced against its own previous use
        for s in streams:
            assert hip.hipStreamSynchronize(s) == 0
        for k, (pl, dp, prm, want, dbk) in enumerate(cases):
            for f in range(n):
                assert np.array_equal(pl.out(f), want[f]), (k, f)
    finally:
        for s in streams:
            hip.hipStreamSynchronize(s)
            hip.hipStreamDestroy(s)
        for pl, dp, _p, _w, _d in cases:
            pl.free()
            dp.free()
        ctx.close()


def test_422_parameter_scratch_on_two_caller_streams():
    """the SAO parameters of a 4:2:2 chroma plane are rewritten for square CTBs into ONE scratch buffer per context (dev_sao) while
    the caller may hand in any stream; its reuse is fenced by an event (sao_ev) and it is only re-allocated after that event has
    completed.  On a context of its own -- so that the scratch is as small as the first call made it -- two non-blocking streams,
    hevcdbk_sao_filter_device_cf on one plane and hevcdbk_h265_deblock_sao_device_cf on another (CTBs of 16 x 32 samples, a parameter
    grid of its own each) alternately with NO host synchronisation between them, then a plane large enough for the scratch to grow,
    on the other stream, and the small ones again; every output against tests/rext_oracle.py.  The stream phase runs in a child
    process under a time limit of its own: calls queued without a host synchronisation are what would hang if a fence were wrong.
    A card is too fast for this to prove the fence (tests/device_stream_sim does that on the CPU); it ties the sessions there to
    operands the card accepts."""
    import os
    import subprocess
    import sys
    tests = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_rext as t; t._scratch_422_on_two_streams(); print('SCRATCH-OK')" % (os.path.dirname(tests), tests)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "SCRATCH-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
