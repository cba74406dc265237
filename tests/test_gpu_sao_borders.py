"""SAO and deblocking + SAO that stop at slice and tile boundaries (H.265 8.7.3.2), on the GPU through the C ABI: the producer
hevcdbk_h265_sao_borders_device and the three _nox entries, bit-exact against the per-sample statement of tests/sao_borders_ref.py.
Every destination is pre-filled, has row padding, a gap between frames and guard rows before and after, all of which must come back
untouched.  PARITY UNPINNED, like the rest of the spec-exact mode.  test_sao_borders_cpu.py shows that every vector with a
forbidden border differs from the border-less result, so a library that took the operand and ignored it fails here."""
import ctypes as C

import numpy as np
import pytest

import bs_vectors as bv
import rext_oracle as rx
import sao_borders_ref as R

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 4      # rows before the first and after the last frame
GAP = 2        # rows between frames


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


def up(ctx, a):
    a = np.ascontiguousarray(a)
    d = ctx.alloc(max(a.nbytes, 1))
    if a.nbytes:
        d.upload(a.view(np.uint8).ravel())
    return d


class Surface:
    """n frames of h x w samples in HBM: pitch = row + pad bytes, GAP rows between frames, GUARD rows around, all FILL"""

    def __init__(self, ctx, n, h, w, sb, pad, frames=None):
        self.n, self.h, self.w, self.sb = n, h, w, sb
        self.pitch = w * sb + pad
        self.fs = self.pitch * (h + GAP)
        self.total = self.pitch * 2 * GUARD + self.fs * n
        host = np.full(self.total, FILL, np.uint8)
        if frames is not None:
            v = self._view(host)
            for f in range(n):
                v[f][:] = np.ascontiguousarray(frames[f]).view(np.uint8).reshape(h, w * sb)
        self.buf = ctx.alloc(self.total)
        self.buf.upload(host)
        self.ptr = self.buf.ptr + self.pitch * GUARD

    def _view(self, host):
        base = self.pitch * GUARD
        return [host[base + f * self.fs: base + f * self.fs + self.pitch * self.h].reshape(self.h, self.pitch)[:, : self.w * self.sb]
                for f in range(self.n)]

    def refill(self):
        self.buf.upload(np.full(self.total, FILL, np.uint8))

    def read(self):
        """(frames, True when every byte outside the frames still is FILL)"""
        host = self.buf.download(self.total)
        dt = np.uint8 if self.sb == 1 else np.uint16
        frames = [np.ascontiguousarray(v).view(dt).reshape(self.h, self.w) for v in self._view(host)]
        rest = host.copy()
        for v in self._view(rest):
            v[:] = FILL
        return frames, bool((rest == FILL).all())

    def free(self):
        self.buf.free()


def dev_planes(src, dst, depth, chroma=False, vb=None, hb=None, qp_map=None, map_stride=0, ctu_log2=3):
    from gpu_video_codec_amd import _lib
    p = _lib.DevicePlanes()
    p.src, p.dst, p.pitch, p.frame_stride, p.n_frames = src.ptr, dst.ptr, src.pitch, src.fs, src.n
    p.plane_w, p.plane_h, p.bit_depth, p.sample_bytes, p.is_chroma = src.w, src.h, depth, src.sb, int(chroma)
    if vb is not None:
        p.vert_bs, p.hor_bs = vb.ptr, hb.ptr
    if qp_map is not None:
        p.qp_map, p.qp_map_stride, p.ctu_log2 = qp_map.ptr, map_stride, ctu_log2
    return p


def borders_of(ctx, layouts, shared):
    """(SaoBorders, device buffer) of the expected bytes of one layout, or of one per frame"""
    from gpu_video_codec_amd import _lib
    nox = np.stack([R.expected_nox(l) for l in layouts])
    d = up(ctx, nox)
    return _lib.SaoBorders(d.ptr, nox.shape[2], 0 if shared else nox.shape[1] * nox.shape[2]), d


# ---- the producer -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows,cols", [(1, 1), (1, 7), (5, 1), (2, 2), (3, 4), (9, 13), (17, 30), (34, 60), (68, 120)])
def test_producer_bytes(ctx, rows, cols):
    rng = np.random.default_rng(rows * 131 + cols)
    lays = [R.one_slice(rows, cols), R.every_ctb(rows, cols)]
    for kind in ("tiles", "slices", "mixed", "random", "random"):
        lays.append(R._layout_of(kind, rows, cols, rng))
    for lay in lays:
        s, a, t = R.per_ctb(lay)
        got = ctx.derive_sao_borders(s, a, t, tiles_across=lay["tiles_across"])
        assert np.array_equal(got, R.expected_nox(lay)), (rows, cols)
        # tile_idx NULL = one tile
        flat = dict(lay, tile_idx=np.zeros((rows, cols), np.int64))
        got = ctx.derive_sao_borders(s, a, None, tiles_across=False)
        assert np.array_equal(got, R.expected_nox(flat)), (rows, cols, "no tiles")


def test_producer_strides_and_layout_of_coded_pictures(ctx):
    """input and output row strides larger than the CTB columns (the bytes beyond stay untouched), on the layouts of
    bs_vectors.coded_picture"""
    from gpu_video_codec_amd import _lib
    L = _lib.lib()
    for (w, h, seed, lg) in [(416, 240, 3, 6), (256, 192, 5, 4), (192, 128, 8, 5)]:
        lay = R.coded_picture_layout(w, h, seed, lg)
        s, a, t = R.per_ctb(lay)
        rows, cols = s.shape
        ins, outs = cols + 3, cols + 5
        pad = lambda x: np.pad(x, ((0, 0), (0, ins - cols)), constant_values=7)
        ds, da, dt = up(ctx, pad(s)), up(ctx, pad(a)), up(ctx, pad(t))
        out = up(ctx, np.full((rows, outs), FILL, np.uint8))
        assert L.hevcdbk_h265_sao_borders_device(ctx.handle, ds.ptr, da.ptr, dt.ptr, int(lay["tiles_across"]), cols, rows, ins, out.ptr, outs, None) == 0
        ctx.synchronize()
        got = out.download(rows * outs).reshape(rows, outs)
        assert np.array_equal(got[:, :cols], R.expected_nox(lay)) and (got[:, cols:] == FILL).all(), (w, h, seed)
        for x in (ds, da, dt, out):
            x.free()


# ---- the SAO pass -------------------------------------------------------------------------------------------------------------

def _sao_call(ctx, c, src, dst, dp, dk, borders, entry):
    from gpu_video_codec_amd import _lib
    L = _lib.lib()
    rows, cols = c["params"][0].shape
    p = dev_planes(src, dst, c["depth"])
    args = [ctx.handle, C.byref(p), dp.ptr, cols, rows * cols, c["lw"], c["lh"], dk.ptr if dk else None, c["w"] // 8,
            (c["h"] // 8) * (c["w"] // 8) if dk else 0]
    if entry == "cf":
        return L.hevcdbk_sao_filter_device_cf(*args, None)
    return L.hevcdbk_sao_filter_device_nox(*args, None if borders is None else C.byref(borders), None)


@pytest.mark.parametrize("spec", R.SAO_CASES, ids=[s[0] for s in R.SAO_CASES])
def test_sao_pass(ctx, spec):
    c = R.sao_case(spec)
    n, sb = len(c["planes"]), c["sb"]
    pad = 4 if c["name"] == "8b_unaligned_pitch" else 16
    src, dst = Surface(ctx, n, c["h"], c["w"], sb, pad, c["planes"]), Surface(ctx, n, c["h"], c["w"], sb, pad)
    dp = up(ctx, np.stack(c["params"]))
    dk = up(ctx, np.stack(c["keeps"])) if c["keeps"] is not None else None
    b, db = borders_of(ctx, c["layouts"], c["shared"])
    assert _sao_call(ctx, c, src, dst, dp, dk, b, "nox") == 0
    ctx.synchronize()
    got, clean = dst.read()
    assert clean, "bytes outside the frames were written"
    for f in range(n):
        want = R.case_expected(c, f)
        assert np.array_equal(got[f], want), (c["name"], f, int((got[f] != want).sum()))
    # no operand, and an operand that forbids nothing: the _cf entry's bytes
    dst.refill()
    assert _sao_call(ctx, c, src, dst, dp, dk, None, "cf") == 0
    ctx.synchronize()
    base, _ = dst.read()
    for f in range(n):
        assert np.array_equal(base[f], rx.sao_plane(c["planes"][f], c["params"][f], c["lw"], c["lh"], bit_depth=c["depth"],
                                                    keep=None if c["keeps"] is None else c["keeps"][f]))
    zb, dz = borders_of(ctx, [R.one_slice(*c["params"][0].shape)], True)
    for bb in (None, zb):
        dst.refill()
        assert _sao_call(ctx, c, src, dst, dp, dk, bb, "nox") == 0
        ctx.synchronize()
        got, clean = dst.read()
        assert clean and all(np.array_equal(got[f], base[f]) for f in range(n)), (c["name"], bb is None)
    for x in (src, dst, dp, db, dz) + ((dk,) if dk else ()):
        x.free()


# ---- deblocking + SAO ---------------------------------------------------------------------------------------------------------

HP = dict(tc_offset_div2=1, beta_offset_div2=-1, cb_qp_offset=3, cr_qp_offset=-2)
CF = {"400": 0, "420": 1, "422": 2, "444": 3}


def _picture(ctx, h265, rng, fmt, w, h, n, depth, ctb_y, kind, qp_map=None, unit_log2=3):
    """the planes of n frames in format fmt: surfaces, operands, and the expected deblocking + SAO result under one layout"""
    from gpu_video_codec_amd import _lib
    cf = CF[fmt]
    sx, sy = rx.SUB.get(cf, (1, 1))
    sb = 1 if depth == 8 else 2
    qp = 36
    units = h265.random_units(w, h, seed=int(rng.integers(1, 1 << 20)))
    vb, hb = h265.derive_bs(*units, w, h)
    rows, cols = -(-h >> ctb_y), -(-w >> ctb_y)
    lay = R._layout_of(kind, rows, cols, rng)
    dmap = up(ctx, qp_map) if qp_map is not None else None
    out = {"planes": [], "sao": [], "want": [], "free": [dmap] if dmap else [], "dst": [], "qp": qp, "layout": lay, "cf": cf}
    for i in range(1 if cf == 0 else 3):
        pw, ph = (w, h) if i == 0 else (w // sx, h // sy)
        lw, lh = (ctb_y, ctb_y) if i == 0 else (ctb_y - (sx - 1), ctb_y - (sy - 1))
        frames = [rng.integers(0, 1 << depth, (ph, pw)).astype(np.uint8 if sb == 1 else np.uint16) for _ in range(n)]
        for fr in frames:   # blocky in part, so that the deblocking filter decides both ways
            fr[: ph // 2] = (fr[: ph // 2] >> 4) + (1 << (depth - 2))
        prm = [R.edge_params(rows, cols, rng, depth) for _ in range(n)]
        b_v, b_h = (vb, hb) if i == 0 else rx.chroma_bs(vb, hb, w, h, cf)
        src, dst = Surface(ctx, n, ph, pw, sb, 16, frames), Surface(ctx, n, ph, pw, sb, 16)
        dv, dh, dp = up(ctx, b_v), up(ctx, b_h), up(ctx, np.stack(prm))
        out["free"] += [src, dst, dv, dh, dp]
        out["dst"].append(dst)
        out["planes"].append(dev_planes(src, dst, depth, i > 0, dv, dh, dmap, 0 if qp_map is None else qp_map.shape[1], unit_log2))
        sp = _lib.SaoPlaneCf()
        sp.params, sp.params_stride, sp.params_frame_stride, sp.ctb_log2_w, sp.ctb_log2_h = dp.ptr, cols, rows * cols, lw, lh
        out["sao"].append(sp)
        for f in range(n):
            if i == 0:
                d = h265.filter_plane(frames[f], qp, b_v, b_h, bit_depth=depth, qp_map=qp_map, unit_log2=unit_log2, tc_offset_div2=1,
                                      beta_offset_div2=-1)
            else:
                d = rx.filter_chroma_plane(frames[f], b_v, b_h, cf, qp=qp, qp_map=qp_map, unit_log2=unit_log2, bit_depth=depth,
                                           tc_offset_div2=1, c_qp_offset=3 if i == 1 else -2)
            want = R.sao_plane(d, prm[f], lw, lh, lay, bit_depth=depth)
            free = rx.sao_plane(d, prm[f], lw, lh, bit_depth=depth)
            out["want"].append((i, f, want, free))
    b, db = borders_of(ctx, [lay], True)
    out["borders"] = b
    out["free"].append(db)
    return out


def _check_picture(pic, tag, which=2):
    """which = 2: against the result under the layout, 3: against the border-less result"""
    differs = 0
    for dst in pic["dst"]:
        assert dst.read()[1], (tag, "bytes outside the frames were written")
    for (i, f, want, free) in pic["want"]:
        got = pic["dst"][i].read()[0][f]
        ref = want if which == 2 else free
        assert np.array_equal(got, ref), (tag, i, f, int((got != ref).sum()))
        differs += int((want != free).sum())
    return differs


def _release(pic):
    for x in pic["free"]:
        x.free()


@pytest.mark.parametrize("depth,use_map,w,h,ctb_y,kind", [(8, False, 384, 256, 6, "mixed"), (8, True, 256, 192, 6, "tiles"),
                                                          (10, False, 256, 256, 6, "every"), (10, True, 320, 192, 5, "mixed"),
                                                          (8, False, 192, 160, 4, "random"), (8, False, 3840, 2160, 6, "tiles"),
                                                          (10, False, 3840, 2160, 6, "mixed")])
def test_fused_single_plane(ctx, h265, depth, use_map, w, h, ctb_y, kind):
    from gpu_video_codec_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(depth * 1000 + w + ctb_y)
    n = 1 if w > 2000 else 2
    qmap = rng.integers(22, 50, (h // 8, w // 8)).astype(np.uint8) if use_map else None
    pic = _picture(ctx, h265, rng, "400", w, h, n, depth, ctb_y, kind, qp_map=qmap)
    hp = _lib.H265Params(**HP)
    sp = pic["sao"][0]
    for fused in (_lib.FUSED_ON, _lib.FUSED_OFF):
        pic["dst"][0].refill()
        rc = L.hevcdbk_h265_deblock_sao_device_nox(ctx.handle, C.byref(pic["planes"][0]), 0, 0, pic["qp"], C.byref(hp), sp.params,
                                                   sp.params_stride, sp.params_frame_stride, sp.ctb_log2_w, sp.ctb_log2_h, None, 0, 0,
                                                   fused, C.byref(pic["borders"]), None)
        assert rc == 0
        ctx.synchronize()
        assert _check_picture(pic, (depth, use_map, w, fused)) > 0
    _release(pic)


@pytest.mark.parametrize("fmt", ["420", "422", "444", "400"])
@pytest.mark.parametrize("depth", [8, 10])
def test_fused_planes(ctx, h265, fmt, depth):
    from gpu_video_codec_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(depth * 7 + CF[fmt])
    for (w, h, ctb_y, kind, use_map) in [(384, 256, 6, "mixed", False), (256, 128, 5, "tiles", True), (192, 192, 4, "every", False)]:
        qmap = rng.integers(22, 50, (h // 8, w // 8)).astype(np.uint8) if use_map else None
        pic = _picture(ctx, h265, rng, fmt, w, h, 2, depth, ctb_y, kind, qp_map=qmap)
        hp = _lib.H265Params(**HP)
        npl = len(pic["planes"])
        arr = (_lib.DevicePlanes * npl)(*pic["planes"])
        sp = (_lib.SaoPlaneCf * npl)(*pic["sao"])
        for fused in (_lib.FUSED_ON, _lib.FUSED_OFF, _lib.FUSED_AUTO):
            for d in pic["dst"]:
                d.refill()
            rc = L.hevcdbk_h265_deblock_sao_device_planes_nox(ctx.handle, arr, npl, pic["cf"], pic["qp"], C.byref(hp), sp, fused,
                                                              C.byref(pic["borders"]), None)
            assert rc == 0, (fmt, depth, w, fused)
            ctx.synchronize()
            assert _check_picture(pic, (fmt, depth, w, fused)) > 0
        # no operand: the _cf entry's bytes, which are the border-less result
        for d in pic["dst"]:
            d.refill()
        assert L.hevcdbk_h265_deblock_sao_device_planes_nox(ctx.handle, arr, npl, pic["cf"], pic["qp"], C.byref(hp), sp, _lib.FUSED_AUTO, None, None) == 0
        ctx.synchronize()
        _check_picture(pic, (fmt, depth, w, "null"), which=3)
        _release(pic)


def test_python_wrapper(ctx, h265):
    from gpu_video_codec_amd import _lib
    rng = np.random.default_rng(77)
    pic = _picture(ctx, h265, rng, "420", 256, 128, 2, 8, 6, "mixed")
    sao = [{"params": s.params, "params_stride": s.params_stride, "ctb_log2": s.ctb_log2_w, "params_frame_stride": s.params_frame_stride}
           for s in pic["sao"]]
    ctx.deblock_sao_device_planes(pic["planes"], pic["qp"], sao, h265=HP, borders=pic["borders"])
    ctx.synchronize()
    assert _check_picture(pic, "wrapper planes") > 0
    with pytest.raises(ValueError):
        ctx.deblock_sao_device_planes(pic["planes"], pic["qp"], sao, borders=pic["borders"])
    pic["dst"][0].refill()
    ctx.deblock_sao_h265_device(pic["planes"][0], pic["qp"], sao[0]["params"], sao[0]["params_stride"], 6, params_frame_stride=sao[0]["params_frame_stride"],
                                borders=pic["borders"], **HP)
    ctx.synchronize()
    got = pic["dst"][0].read()[0]
    for (i, f, want, _free) in pic["want"]:
        if i == 0:
            assert np.array_equal(got[f], want)
    _release(pic)


# ---- the chain of a decoder: units -> bS -> borders -> deblocking + SAO ----------------------------------------------------------

@pytest.mark.parametrize("w,h,seed,ctb_log2", [(416, 240, 3, 6), (256, 192, 5, 4), (384, 256, 11, 5), (192, 128, 8, 5)])
def test_chain_on_coded_pictures(ctx, h265, w, h, seed, ctb_log2):
    from gpu_video_codec_amd import _lib
    L = _lib.lib()
    units = bv.coded_picture(w, h, seed, ctb_log2)
    lay = R.coded_picture_layout(w, h, seed, ctb_log2)
    vb, hb = ctx.derive_bs_h265(units, w, h, chroma=False)[:2]
    assert np.array_equal(vb, bv.derive_bs(units, w, h)[0])
    s, a, t = R.per_ctb(lay)
    nox = ctx.derive_sao_borders(s, a, t, tiles_across=lay["tiles_across"])
    rng = np.random.default_rng(seed)
    rows, cols = s.shape
    frame = rng.integers(0, 256, (h, w)).astype(np.uint8)
    frame[:, : w // 2] = (frame[:, : w // 2] >> 4) + 96
    prm = R.edge_params(rows, cols, rng)
    src, dst = Surface(ctx, 1, h, w, 1, 16, [frame]), Surface(ctx, 1, h, w, 1, 16)
    dv, dh, dp, dn = up(ctx, vb), up(ctx, hb), up(ctx, prm), up(ctx, nox)
    p = dev_planes(src, dst, 8, False, dv, dh)
    b = _lib.SaoBorders(dn.ptr, cols, 0)
    hp = _lib.H265Params(0, 0, 0, 0)
    d = h265.filter_plane(frame, 30, vb, hb, bit_depth=8)
    want = R.sao_plane(d, prm, ctb_log2, ctb_log2, lay)
    for fused in (_lib.FUSED_ON, _lib.FUSED_OFF):
        dst.refill()
        assert L.hevcdbk_h265_deblock_sao_device_nox(ctx.handle, C.byref(p), 0, 1, 30, C.byref(hp), dp.ptr, cols, 0, ctb_log2, ctb_log2, None,
                                                     0, 0, fused, C.byref(b), None) == 0
        ctx.synchronize()
        got, clean = dst.read()
        assert clean and np.array_equal(got[0], want), (w, h, seed, fused, int((got[0] != want).sum()))
    for x in (src, dst, dv, dh, dp, dn):
        x.free()


# ---- what is enqueued ---------------------------------------------------------------------------------------------------------

def test_null_enqueues_the_cf_kernels_and_an_operand_the_nox_twins(ctx, h265):
    from gpu_video_codec_amd import _lib
    from kernel_capture import kernels_enqueued, parse_kernel
    L = _lib.lib()
    rng = np.random.default_rng(5)
    hp = _lib.H265Params(**HP)
    for fmt, depth in (("420", 8), ("444", 10)):
        pic = _picture(ctx, h265, rng, fmt, 256, 128, 2, depth, 6, "mixed")
        arr = (_lib.DevicePlanes * 3)(*pic["planes"])
        sp = (_lib.SaoPlaneCf * 3)(*pic["sao"])
        s0 = pic["sao"][0]
        calls = {
            "planes": (lambda st, b: L.hevcdbk_h265_deblock_sao_device_planes_nox(ctx.handle, arr, 3, pic["cf"], pic["qp"], C.byref(hp), sp, _lib.FUSED_AUTO, b, st),
                       lambda st: L.hevcdbk_h265_deblock_sao_device_planes_cf(ctx.handle, arr, 3, pic["cf"], pic["qp"], C.byref(hp), sp, _lib.FUSED_AUTO, st)),
            "plane": (lambda st, b: L.hevcdbk_h265_deblock_sao_device_nox(ctx.handle, C.byref(pic["planes"][0]), 0, pic["cf"], pic["qp"], C.byref(hp), s0.params, s0.params_stride,
                                                                          s0.params_frame_stride, 6, 6, None, 0, 0, _lib.FUSED_AUTO, b, st),
                      lambda st: L.hevcdbk_h265_deblock_sao_device_cf(ctx.handle, C.byref(pic["planes"][0]), 0, pic["cf"], pic["qp"], C.byref(hp), s0.params, s0.params_stride,
                                                                      s0.params_frame_stride, 6, 6, None, 0, 0, _lib.FUSED_AUTO, st)),
            "sao": (lambda st, b: L.hevcdbk_sao_filter_device_nox(ctx.handle, C.byref(pic["planes"][0]), s0.params, s0.params_stride, s0.params_frame_stride, 6, 6, None, 0, 0, b, st),
                    lambda st: L.hevcdbk_sao_filter_device_cf(ctx.handle, C.byref(pic["planes"][0]), s0.params, s0.params_stride, s0.params_frame_stride, 6, 6, None, 0, 0, st)),
        }
        for tag, (nox, cf_entry) in calls.items():
            assert cf_entry(None) == 0 and nox(None, C.byref(pic["borders"])) == 0   # first use of the context's scratch outside a capture
            ctx.synchronize()
            rc0, k_cf = kernels_enqueued(cf_entry)
            rc1, k_null = kernels_enqueued(lambda st: nox(st, None))
            rc2, k_nox = kernels_enqueued(lambda st: nox(st, C.byref(pic["borders"])))
            assert rc0 == 0 and rc1 == 0 and rc2 == 0
            assert k_null == k_cf, (fmt, tag)
            assert not any("nox" in parse_kernel(k[0])[0] for k in k_cf), (fmt, tag)
            sao_like = [k for k in k_nox if "sao" in parse_kernel(k[0])[0] and "rows_x2" not in parse_kernel(k[0])[0]]
            assert sao_like and all(parse_kernel(k[0])[0].endswith("nox_kernel") for k in sao_like), (fmt, tag, [k[0] for k in k_nox])
            # the same grids and blocks as the kernels they stand in for
            plain = [k for k in k_cf if "sao" in parse_kernel(k[0])[0] and "rows_x2" not in parse_kernel(k[0])[0]]
            assert [k[1:] for k in sao_like] == [k[1:] for k in plain], (fmt, tag)
        _release(pic)


def test_argument_errors(ctx, h265):
    from gpu_video_codec_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(9)
    pic = _picture(ctx, h265, rng, "420", 256, 128, 1, 8, 6, "mixed")
    hp = _lib.H265Params(**HP)
    s0 = pic["sao"][0]
    arr = (_lib.DevicePlanes * 3)(*pic["planes"])
    sp = (_lib.SaoPlaneCf * 3)(*pic["sao"])
    good = pic["borders"]
    for bad in (_lib.SaoBorders(None, good.stride, 0), _lib.SaoBorders(good.nox, 3, 0)):   # NULL bytes; stride below the 4 CTB columns
        assert L.hevcdbk_sao_filter_device_nox(ctx.handle, C.byref(pic["planes"][0]), s0.params, s0.params_stride, 0, 6, 6, None, 0, 0,
                                               C.byref(bad), None) == _lib.ERR_ARG
        assert L.hevcdbk_h265_deblock_sao_device_nox(ctx.handle, C.byref(pic["planes"][0]), 0, 1, 30, C.byref(hp), s0.params, s0.params_stride, 0,
                                                     6, 6, None, 0, 0, _lib.FUSED_AUTO, C.byref(bad), None) == _lib.ERR_ARG
        assert L.hevcdbk_h265_deblock_sao_device_planes_nox(ctx.handle, arr, 3, 1, 30, C.byref(hp), sp, _lib.FUSED_AUTO, C.byref(bad), None) == _lib.ERR_ARG
    # 4:0:0 with chroma
    assert L.hevcdbk_h265_deblock_sao_device_planes_nox(ctx.handle, arr, 3, 0, 30, C.byref(hp), sp, _lib.FUSED_AUTO, C.byref(good), None) == _lib.ERR_ARG
    assert L.hevcdbk_h265_deblock_sao_device_nox(ctx.handle, C.byref(pic["planes"][1]), 1, 0, 30, C.byref(hp), s0.params, s0.params_stride, 0, 5, 5,
                                                 None, 0, 0, _lib.FUSED_AUTO, C.byref(good), None) == _lib.ERR_ARG
    # the producer
    d = up(ctx, np.zeros(64, np.uint16))
    assert L.hevcdbk_h265_sao_borders_device(ctx.handle, None, d.ptr, None, 1, 4, 4, 4, d.ptr, 4, None) == _lib.ERR_ARG
    assert L.hevcdbk_h265_sao_borders_device(ctx.handle, d.ptr, d.ptr, None, 1, 4, 4, 3, d.ptr, 4, None) == _lib.ERR_ARG
    assert L.hevcdbk_h265_sao_borders_device(ctx.handle, d.ptr, d.ptr, None, 1, 4, 4, 4, d.ptr, 3, None) == _lib.ERR_ARG
    assert L.hevcdbk_h265_sao_borders_device(ctx.handle, d.ptr, d.ptr, None, 1, 0, 4, 4, d.ptr, 4, None) == _lib.ERR_ARG
    d.free()
    _release(pic)
