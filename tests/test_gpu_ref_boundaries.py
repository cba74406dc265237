"""Reference-exact deblocking on the GPU at its decision edges (run with -m gpu on an MI355X).

The vectors of tests/ref_vectors.py -- segments solved onto every threshold of cpu.h's filter, its clips, the range extremes,
the picture border, chroma on the +-tc clips -- go through every reference-mode device path and must equal the C oracle bit
for bit: filter_device with each kernel and block map, 8-bit planes and 16-bit containers at 8..12 bit, the QP-map kernels,
the one-launch Y+U+V form, deblocking + SAO fused and in two launches, the host-frame operator (direct and strip pipeline,
pageable and registered memory), the sequence operator and the file operator on the pinned boundary frames.
"""
import functools
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, sha256
import ref_vectors as rv

pytestmark = pytest.mark.gpu

W, H = 520, 72   # 66 x 10 offset blocks: more than one 512-lane workgroup, so MAP_LINEAR really runs row-major
QPS = (18, 30, 41, 51)


@pytest.fixture(scope="module")
def ctx():
    from gpu_video_codec_amd import deblock
    c = deblock.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def h265():
    from oracle import h265 as h
    return h


def _variants():
    from gpu_video_codec_amd import _lib
    return [(v, m) for v in (_lib.KERNEL_AUTO, _lib.KERNEL_GENERIC, _lib.KERNEL_PACKED) for m in (_lib.MAP_ROWS, _lib.MAP_LINEAR)]


def run_batch(ctx, frames, qp, bss, *, variant, bit_depth=8, sample_bytes=None, is_chroma=False, in_place=False, pitch=None,
              qp_map=None, ctu_log2=6, tc_table=None, beta_table=None):
    """frames (n, h, w) through hevc_deblocking_filter_device in one launch; returns (n, h, w)"""
    from gpu_video_codec_amd import deblock
    a = np.asarray(frames)
    n, h, w = a.shape
    sb = sample_bytes or (1 if bit_depth == 8 else 2)
    b = deblock.DeviceBatch(ctx, w, h, n, bit_depth=bit_depth, sample_bytes=sb, is_chroma=is_chroma, in_place=in_place,
                            pitch=pitch)
    try:
        b.upload_all(a, fill=0x5A)
        for f in range(n):
            b.set_bs(f, *bss[f])
        if qp_map is not None:
            b.set_qp_map(qp_map, ctu_log2)
        ctx.filter_device(b.planes(), qp, variant=variant, tc_table=tc_table, beta_table=beta_table)
        ctx.synchronize()
        out = np.stack([b.download_frame(f) for f in range(n)])
        if not in_place:
            assert np.array_equal(np.stack([b.download_frame(f, "src") for f in range(n)]), a.astype(b.dtype))
        return out
    finally:
        b.free()


def _luma_frames(bd, rng, qp, **kw):
    out = [rv.luma_plane(bd, rng, w=W, h=H, wave=wave, qp=qp, **kw) for wave in rv.WAVES]
    return np.stack([p for p, _, _ in out]), [(vb, hb) for _, vb, hb in out]


CONTAINERS = ((8, 1), (8, 2), (9, 2), (10, 2), (11, 2), (12, 2))


@functools.lru_cache(maxsize=None)
def _luma_cases(bd):
    """(qp, tables, frames, bS) of every scalar-QP luma case at bit depth bd (8-bit data serves both containers)"""
    rng = np.random.default_rng(100 * bd)
    cases = [(qp, {}) for qp in QPS] + [(40, dict(tc_table=t, beta_table=b)) for _, t, b in rv.custom_tables()]
    return [(qp, tab) + _luma_frames(bd, rng, qp, **tab) for qp, tab in cases]


@pytest.mark.parametrize("bd,sb", CONTAINERS)
def test_filter_device_luma(ctx, oracle, bd, sb):
    """luma waves (vertical-only, horizontal-only, mixed bS) solved for each QP, three frames per launch, every kernel and
    block map, in place and out of place; custom tables that decouple beta and tc"""
    from gpu_video_codec_amd import _lib
    for k, (qp, tab, frames, bss) in enumerate(_luma_cases(bd)):
        want = [oracle.filter_plane(frames[f], qp, bit_depth=bd, sample_bytes=sb, vert_bs=bss[f][0], hor_bs=bss[f][1], **tab)
                for f in range(len(frames))]
        fits = rv.packed_tc_fits((1 << bd) - 1, int(rv.tables_of(tab.get("tc_table"))[0][qp]) << (bd - 8))
        for i, (v, m) in enumerate(_variants()):
            if v == _lib.KERNEL_PACKED and not fits:
                continue
            got = run_batch(ctx, frames, qp, bss, variant=v | m, bit_depth=bd, sample_bytes=sb, in_place=(i + k) % 2 == 1, **tab)
            for f in range(len(frames)):
                assert np.array_equal(got[f], want[f]), (bd, sb, qp, k, v, m, f, np.argwhere(got[f] != want[f])[:4])


def test_pitched_rows(ctx, oracle):
    """8-bit rows with a pitch that is no multiple of 8 (w + 4 bytes) through every kernel; 16-bit containers whose pitch is no
    multiple of 8 bytes are refused by the device entry (HEVCDBK_ERR_UNSUPPORTED), with rows of w + 4 samples they run"""
    from gpu_video_codec_amd import _lib, deblock
    rng = np.random.default_rng(7)
    frames, bss = _luma_frames(8, rng, 37)
    want = [oracle.filter_plane(frames[f], 37, vert_bs=bss[f][0], hor_bs=bss[f][1]) for f in range(3)]
    for v, m in _variants():
        got = run_batch(ctx, frames, 37, bss, variant=v | m, pitch=W + 4)
        assert all(np.array_equal(got[f], want[f]) for f in range(3)), (v, m)
    f10, b10 = _luma_frames(10, rng, 37)
    want = [oracle.filter_plane(f10[f], 37, bit_depth=10, vert_bs=b10[f][0], hor_bs=b10[f][1]) for f in range(3)]
    for v, m in _variants():
        got = run_batch(ctx, f10, 37, b10, variant=v | m, bit_depth=10, pitch=2 * (W + 4))
        assert all(np.array_equal(got[f], want[f]) for f in range(3)), (v, m)
        with pytest.raises(deblock.DeblockError) as e:
            run_batch(ctx, f10, 37, b10, variant=v | m, bit_depth=10, pitch=2 * W + 4)
        assert e.value.code == _lib.ERR_UNSUPPORTED


@pytest.mark.parametrize("bd", (8, 10, 12))
def test_filter_device_chroma(ctx, oracle, bd):
    """chroma planes on the +-tc clips of dp and dq, the rounding cases and Clip2, under vertical, horizontal (with the shifted
    hor2 read at bx = w/8) and default bS"""
    rng = np.random.default_rng(200 + bd)
    for qp in QPS:
        out = [rv.chroma_plane(bd, rng, w=264, h=40, wave=wave, qp=qp) for wave in ("v", "h", "default")]
        frames, bss = np.stack([p for p, _, _ in out]), [(vb, hb) for _, vb, hb in out]
        want = [oracle.filter_plane(frames[f], qp, is_chroma=True, bit_depth=bd, vert_bs=bss[f][0], hor_bs=bss[f][1])
                for f in range(3)]
        for i, (v, m) in enumerate(_variants()):
            got = run_batch(ctx, frames, qp, bss, variant=v | m, bit_depth=bd, is_chroma=True, in_place=i % 2 == 1)
            for f in range(3):
                assert np.array_equal(got[f], want[f]), (bd, qp, v, m, f)


@pytest.mark.parametrize("bd,sb", ((8, 1), (10, 2), (12, 2)))
def test_qp_map_kernels(ctx, oracle, bd, sb):
    """QP maps holding every QP, units of 8 .. 256 luma samples: many distinct operand rows per launch (the packed kernels'
    LDS table), segments solved with their own map-derived (beta, tc) across unit borders; chroma with the map too"""
    from gpu_video_codec_amd import _lib
    rng = np.random.default_rng(300 + bd)
    for lg in range(3, 9):
        m = rv.all_qp_map(W, H, lg, rng)
        frames, bss = _luma_frames(bd, rng, 0, qp_map=m, ctu_log2=lg)
        want = [oracle.filter_plane(frames[f], 0, bit_depth=bd, vert_bs=bss[f][0], hor_bs=bss[f][1], qp_map=m, ctu_log2=lg)
                for f in range(3)]
        for i, (v, mp) in enumerate(_variants()):
            got = run_batch(ctx, frames, 0, bss, variant=v | mp, bit_depth=bd, sample_bytes=sb, qp_map=m, ctu_log2=lg,
                            in_place=i % 2 == 0)
            for f in range(3):
                assert np.array_equal(got[f], want[f]), (bd, lg, v, mp, f, np.argwhere(got[f] != want[f])[:4])
        cw, chh = W // 2 // 8 * 8, H // 2 // 8 * 8
        out = [rv.chroma_plane(bd, rng, w=cw, h=chh, wave=wave, qp_map=m, ctu_log2=lg) for wave in ("v", "h")]
        cf, cb = np.stack([p for p, _, _ in out]), [(vb, hb) for _, vb, hb in out]
        want = [oracle.filter_plane(cf[f], 0, is_chroma=True, bit_depth=bd, vert_bs=cb[f][0], hor_bs=cb[f][1], qp_map=m,
                                    ctu_log2=lg) for f in range(2)]
        for v in (_lib.KERNEL_AUTO, _lib.KERNEL_GENERIC, _lib.KERNEL_PACKED):
            got = run_batch(ctx, cf, 0, cb, variant=v, bit_depth=bd, is_chroma=True, qp_map=m, ctu_log2=lg)
            assert all(np.array_equal(got[f], want[f]) for f in range(2)), (bd, lg, v)


@pytest.mark.parametrize("bd", (8, 9, 10, 11, 12))
def test_operand_range_edge(ctx, oracle, bd):
    """the largest tc table packed_luma_tc_fits admits (255 up to 10 bit, 128 at 11 / 12) and, where it is a legal table, that
    table plus one: AUTO and GENERIC equal the oracle; a forced PACKED runs and equals it inside the range and is refused with
    HEVCDBK_ERR_UNSUPPORTED beyond it; with a QP map the largest entry of the table decides"""
    from gpu_video_codec_amd import _lib, deblock
    rng = np.random.default_rng(400 + bd)
    edge = rv.fits_edge(bd)
    for e in (edge, edge + 1):
        if e > 255:
            continue
        tct, bt = np.full(52, e, np.int64), np.full(52, 255, np.int64)
        frames, bss = _luma_frames(bd, rng, 40, tc_table=tct, beta_table=bt)
        want = [oracle.filter_plane(frames[f], 40, bit_depth=bd, vert_bs=bss[f][0], hor_bs=bss[f][1], tc_table=tct,
                                    beta_table=bt) for f in range(3)]
        for v in (_lib.KERNEL_AUTO, _lib.KERNEL_GENERIC):
            got = run_batch(ctx, frames, 40, bss, variant=v, bit_depth=bd, tc_table=tct, beta_table=bt)
            assert all(np.array_equal(got[f], want[f]) for f in range(3)), (bd, e, v)
        if e == edge:
            got = run_batch(ctx, frames, 40, bss, variant=_lib.KERNEL_PACKED, bit_depth=bd, tc_table=tct, beta_table=bt)
            assert all(np.array_equal(got[f], want[f]) for f in range(3)), (bd, e, "packed")
        else:
            with pytest.raises(deblock.DeblockError) as ex:
                run_batch(ctx, frames, 40, bss, variant=_lib.KERNEL_PACKED, bit_depth=bd, tc_table=tct, beta_table=bt)
            assert ex.value.code == _lib.ERR_UNSUPPORTED
        tcm = np.full(52, 4, np.int64)
        tcm[51] = e
        m = rv.all_qp_map(W, H, 4, rng, lo=20, hi=40)
        fm, bm = _luma_frames(bd, rng, 0, qp_map=m, ctu_log2=4, tc_table=tcm, beta_table=bt)
        want = [oracle.filter_plane(fm[f], 0, bit_depth=bd, vert_bs=bm[f][0], hor_bs=bm[f][1], qp_map=m, ctu_log2=4,
                                    tc_table=tcm, beta_table=bt) for f in range(3)]
        got = run_batch(ctx, fm, 0, bm, variant=_lib.KERNEL_AUTO, bit_depth=bd, qp_map=m, ctu_log2=4, tc_table=tcm, beta_table=bt)
        assert all(np.array_equal(got[f], want[f]) for f in range(3)), (bd, e, "map")


def _yuv_batches(ctx, bd, rng, qp, n=2, w=W + 8, h=H + 8):
    """n frames of Y (luma waves with bS override) + U, V (chroma under the default pattern) as three DeviceBatches"""
    from gpu_video_codec_amd import deblock
    ys, bss = [], []
    for f in range(n):
        y, vb, hb = rv.luma_plane(bd, rng, w=w, h=h, wave=rv.WAVES[f % 3], qp=qp)
        ys.append(y)
        bss.append((vb, hb))
    us = [rv.chroma_plane(bd, rng, w=w // 2, h=h // 2, wave="default", qp=qp)[0] for _ in range(n)]
    vs = [rv.chroma_plane(bd, rng, w=w // 2, h=h // 2, wave="default", qp=qp)[0] for _ in range(n)]
    batches = []
    for k, planes in enumerate((ys, us, vs)):
        b = deblock.DeviceBatch(ctx, planes[0].shape[1], planes[0].shape[0], n, bit_depth=bd, is_chroma=k > 0)
        b.upload_all(np.stack(planes))
        if k == 0:
            for f in range(n):
                b.set_bs(f, *bss[f])
        batches.append(b)
    return (ys, us, vs), bss, batches


def _deblock_want(oracle, planes, bss, qp, bd):
    ys, us, vs = planes
    return [[oracle.filter_plane(ys[f], qp, bit_depth=bd, vert_bs=bss[f][0], hor_bs=bss[f][1]) for f in range(len(ys))],
            [oracle.filter_plane(u, qp, is_chroma=True, bit_depth=bd) for u in us],
            [oracle.filter_plane(v, qp, is_chroma=True, bit_depth=bd) for v in vs]]


@pytest.mark.parametrize("bd", (8, 10, 12))
def test_filter_device_planes(ctx, oracle, bd):
    """Y + U + V of a batch in one call (one fused launch where the operands allow), AUTO and PACKED"""
    from gpu_video_codec_amd import _lib
    rng = np.random.default_rng(500 + bd)
    for qp in (24, 37, 51):
        planes, bss, batches = _yuv_batches(ctx, bd, rng, qp)
        want = _deblock_want(oracle, planes, bss, qp, bd)
        try:
            for v in (_lib.KERNEL_AUTO, _lib.KERNEL_PACKED):
                for b in batches:
                    b.dst.upload(np.zeros(b.frame_bytes * b.n, np.uint8))
                ctx.filter_device_planes([b.planes() for b in batches], qp, variant=v)
                ctx.synchronize()
                for k, b in enumerate(batches):
                    for f in range(b.n):
                        assert np.array_equal(b.download_frame(f), want[k][f]), (bd, qp, v, k, f)
        finally:
            for b in batches:
                b.free()


@pytest.mark.parametrize("bd", (8, 10, 12))
def test_deblock_sao(ctx, oracle, h265, bd):
    """deblock_sao_device per plane and deblock_sao_device_planes, fused ON and OFF, on planes sized so that solved segments sit
    on the fused tile borders (192 x 128 at 8 bit, 128 x 128 in 16-bit containers): with SAO type 0 everywhere the output is
    the deblocking alone; with random SAO parameters it is the deblocking oracle followed by the SAO oracle"""
    from gpu_video_codec_amd import _lib
    rng = np.random.default_rng(600 + bd)
    ctb_log2 = 5
    w, h = (400, 272) if bd == 8 else (272, 272)   # tile borders at x = 192, 384 / 128, 256 and y = 128, 256
    for sao_kind in ("off", "random"):
        qp = 37 if sao_kind == "off" else 45
        planes, bss, batches = _yuv_batches(ctx, bd, rng, qp, w=w, h=h)
        deb = _deblock_want(oracle, planes, bss, qp, bd)
        held, sao, want = [], [], []
        for k, b in enumerate(batches):
            prm = np.stack([h265.random_sao_params(b.w, b.h, ctb_log2, seed=int(rng.integers(1 << 30)), bit_depth=bd)
                            for _ in range(b.n)])
            if sao_kind == "off":
                prm["type"] = 0
            dp = ctx.alloc(prm.nbytes)
            dp.upload(prm.view(np.uint8).ravel())
            held.append(dp)
            sao.append({"params": dp.ptr, "params_stride": prm.shape[2], "ctb_log2": ctb_log2,
                        "params_frame_stride": prm.shape[1] * prm.shape[2]})
            want.append([deb[k][f] if sao_kind == "off" else h265.sao_plane(deb[k][f], prm[f], ctb_log2, bit_depth=bd)
                         for f in range(b.n)])
        try:
            for fused in (_lib.FUSED_ON, _lib.FUSED_OFF):
                for k, b in enumerate(batches):   # plane by plane
                    b.dst.upload(np.zeros(b.frame_bytes * b.n, np.uint8))
                    s = sao[k]
                    ctx.deblock_sao_device(b.planes(), qp, s["params"], s["params_stride"], ctb_log2, fused=fused,
                                           params_frame_stride=s["params_frame_stride"])
                    ctx.synchronize()
                    for f in range(b.n):
                        assert np.array_equal(b.download_frame(f), want[k][f]), (bd, sao_kind, fused, k, f, "plane")
                for b in batches:
                    b.dst.upload(np.zeros(b.frame_bytes * b.n, np.uint8))
                ctx.deblock_sao_device_planes([b.planes() for b in batches], qp, sao, fused=fused)
                ctx.synchronize()
                for k, b in enumerate(batches):
                    for f in range(b.n):
                        assert np.array_equal(b.download_frame(f), want[k][f]), (bd, sao_kind, fused, k, f, "planes")
        finally:
            for x in held:
                x.free()
            for b in batches:
                b.free()


def _tile_bs(vb, hb, w, h, ry, rx):
    """the bS arrays of a (ry h) x (rx w) plane tiled from a w x h one"""
    v = vb.reshape(h // 8, w // 8 + 1)
    v = np.hstack([np.tile(v[:, :-1], (ry, rx)), np.tile(v[:, -1:], (ry, 1))])
    hh = hb.reshape(h // 8 + 1, w // 8)
    hh = np.vstack([np.tile(hh[:-1], (ry, rx)), np.tile(hh[-1:], (1, rx))])
    return v.ravel(), hh.ravel()


def test_filter_frame(ctx, oracle):
    """the host-frame operator on 8-bit 4:2:0 boundary frames: one under 2 MiB (direct page-locked path) and one over 2 MiB
    tiled from the vectors (crew and strip pipeline), from pageable memory and from registered memory"""
    rng = np.random.default_rng(700)
    y, u, v, vb, hb = rv.boundary_frame(528, 48, 37, "mixed", rng)
    ry, rx = 24, 4   # 2112 x 1152 luma: 3.6 MiB
    big = (np.tile(y, (ry, rx)), np.tile(u, (ry, rx)), np.tile(v, (ry, rx))) + _tile_bs(vb, hb, 528, 48, ry, rx)
    for (yy, uu, vv, vbs, hbs) in ((y, u, v, vb, hb), big):
        want = oracle.filter_yuv420(oracle.join_yuv420(yy, uu, vv), yy.shape[1], yy.shape[0], 37, vbs, hbs)
        planes = [yy.copy(), uu.copy(), vv.copy()]
        ctx.filter_frame(*planes, qp=37, vert_bs=vbs, hor_bs=hbs)
        assert oracle.join_yuv420(*planes) == want, ("pageable", yy.shape)
        # registered: the three planes inside one page-locked buffer
        buf = np.empty(yy.size + uu.size + vv.size, np.uint8)
        ctx.host_register(buf)
        try:
            ry_, ru = buf[: yy.size].reshape(yy.shape), buf[yy.size: yy.size + uu.size].reshape(uu.shape)
            rvv = buf[yy.size + uu.size:].reshape(vv.shape)
            ry_[:], ru[:], rvv[:] = yy, uu, vv
            ctx.filter_frame(ry_, ru, rvv, qp=37, vert_bs=vbs, hor_bs=hbs)
            assert buf.tobytes() == want, ("registered", yy.shape)
        finally:
            ctx.host_unregister(buf)


def test_filter_sequence(ctx, oracle):
    """the streaming operator on a sequence of boundary frames sharing one luma bS (groups of small frames, and 16-bit
    containers at 10 bit)"""
    rng = np.random.default_rng(800)
    for bd in (8, 10):
        frames, want = [], []
        vb = hb = None
        for i in range(5):
            y, vb0, hb0 = rv.luma_plane(bd, rng, w=112, h=48, wave=rv.WAVES[i % 3], qp=42)
            if vb is None:
                vb, hb = vb0, hb0
            u = rv.chroma_plane(bd, rng, w=56, h=24, wave="default", qp=42)[0]
            v = rv.chroma_plane(bd, rng, w=56, h=24, wave="default", qp=42)[0]
            frames.append((y.copy(), u.copy(), v.copy()))
            want.append((oracle.filter_plane(y, 42, bit_depth=bd, vert_bs=vb, hor_bs=hb),
                         oracle.filter_plane(u, 42, is_chroma=True, bit_depth=bd),
                         oracle.filter_plane(v, 42, is_chroma=True, bit_depth=bd)))
        ctx.filter_sequence(frames, qp=42, bit_depth=bd, vert_bs=vb, hor_bs=hb)
        for i, (got, w_) in enumerate(zip(frames, want)):
            for k in range(3):
                assert np.array_equal(got[k], w_[k]), (bd, i, k)


def test_filter_yuv_file_on_pinned_frames(ctx, oracle, tmp_path):
    """the file operator on the boundary frames of tests/golden/ref_boundaries.json: each one-frame file with its luma bS
    reproduces the reference's recorded output hash; the frames of one size as one multi-frame file (default bS) equal the
    oracle frame by frame"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(GOLDEN, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    with open(os.path.join(GOLDEN, "ref_boundaries.json")) as fh:
        rec = json.load(fh)["cases"]
    by_size = {}
    for (w, h, qp, wave, buf, vb, hb), want in zip(mg.boundary_cases(), rec):
        assert sha256(buf) == want["input_sha256"]
        src, dst = tmp_path / "in.yuv", tmp_path / "out.yuv"
        src.write_bytes(buf)
        n, _ = ctx.filter_yuv_file(str(src), str(dst), w, h, qp, vert_bs=vb, hor_bs=hb)
        assert n == 1 and sha256(dst.read_bytes()) == want["sha256"], (w, h, qp, wave)
        by_size.setdefault((w, h), []).append(buf)
    for (w, h), bufs in by_size.items():
        src, dst = tmp_path / "multi.yuv", tmp_path / "multi_out.yuv"
        src.write_bytes(b"".join(bufs))
        n, _ = ctx.filter_yuv_file(str(src), str(dst), w, h, 45)
        assert n == len(bufs)
        got = dst.read_bytes()
        fb = 3 * w * h // 2
        for i, b in enumerate(bufs):
            assert got[i * fb:(i + 1) * fb] == oracle.filter_yuv420(b, w, h, 45), (w, h, i)
