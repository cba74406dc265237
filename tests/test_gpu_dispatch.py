"""Kernel selection on both sides of every dispatch guard (tests/dispatch_cases.py), on the GPU.

Each case runs through its public device entry with KERNEL_AUTO / FUSED_AUTO (or the forced form it names) and asserts three
things: the bytes equal the oracle (the windowed oracle for giant planes), nothing outside the planes was written (row padding,
frame padding, sentinels before a misaligned base and after the last frame), and the kernels enqueued are the ones the
restatement predicts -- read from a stream capture on a throwaway context (tests/kernel_capture.py: captured, never launched).
Operand sets the entry refuses return the documented error and enqueue nothing."""
import ctypes as C
import zlib

import numpy as np
import pytest

import dispatch_cases as dc
from kernel_capture import kernels_enqueued, parse_kernel

pytestmark = pytest.mark.gpu

QP = 37
GUARD = 256          # sentinel bytes before and after every plane buffer
SENT, DST_FILL, SRC_PAD = 0xA5, 0x5A, 0x33
CASES = {c.name: c for c in dc.cases() if c.gpu}
SMALL = [n for n, c in CASES.items() if not c.giant]
GIANT = [n for n, c in CASES.items() if c.giant]


def _device_used():
    """bytes of device memory in use (hipMemGetInfo), for the peak a giant case reports"""
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return total.value - free.value


def _lib():
    from gpu_video_codec_amd import _lib
    return _lib


class Buf:
    """nbytes at an offset from an aligned base, GUARD sentinel bytes on both sides"""

    def __init__(self, ctx, nbytes, off, fill):
        self.ctx, self.n, self.off = ctx, nbytes, off
        self.raw = ctx.alloc(nbytes + off + 2 * GUARD)
        L = _lib().lib()
        assert L.hevcdbk_memset_d(ctx.handle, self.raw.ptr, SENT, self.raw.nbytes) == 0
        assert L.hevcdbk_memset_d(ctx.handle, self.ptr, fill, nbytes) == 0

    @property
    def ptr(self):
        return self.raw.ptr + GUARD + self.off

    def upload(self, arr, at=0):
        self.raw.upload(np.ascontiguousarray(arr).view(np.uint8).ravel(), GUARD + self.off + at)

    def download(self, nbytes, at=0):
        return self.raw.download(nbytes, GUARD + self.off + at)

    def sentinels_intact(self):
        head = self.raw.download(GUARD + self.off, 0)
        tail = self.raw.download(GUARD, GUARD + self.off + self.n)
        return bool(np.all(head == SENT) and np.all(tail == SENT))

    def free(self):
        self.raw.free()


def _planes_struct(p, src, dst, vb, hb):
    dp = _lib().DevicePlanes()
    dp.src, dp.dst, dp.pitch, dp.frame_stride, dp.n_frames = src.ptr, dst.ptr, p.P, p.fs, p.n
    dp.plane_w, dp.plane_h, dp.bit_depth, dp.sample_bytes, dp.is_chroma = p.w, p.h, p.bd, p.sb, int(p.chroma)
    dp.vert_bs, dp.hor_bs, dp.vert_bs_stride, dp.hor_bs_stride = vb.ptr, hb.ptr, 0, 0
    return dp


def _ctb_h(case, i, p):
    """log2 of the CTB height of plane i (4:2:2 chroma: twice the width)"""
    lw = case.ctb_log2 - (1 if (case.entry == "dbk_sao_h265_planes_cf" and i > 0 and case.cf == 2) else 0)
    return lw, lw + (1 if (p.chroma and case.cf == 2) else 0)


class Operands:
    """device operands of a case: per plane src / dst / bS / SAO parameters"""

    def __init__(self, ctx, case):
        self.ctx, self.case, self.bufs, self.dp, self.sao, self.params, self.io, self.maps = ctx, case, [], [], [], [], [], []
        h265 = "h265" in case.entry
        for i, p in enumerate(case.planes):
            src = Buf(ctx, p.nbytes(), p.src_off, SRC_PAD)
            dst = Buf(ctx, p.nbytes(), p.dst_off, DST_FILL)
            vb_h, hb_h = dc.bs_arrays(h265, p.w, p.h)
            vb, hb = ctx.alloc(vb_h.size), ctx.alloc(hb_h.size)
            vb.upload(vb_h)
            hb.upload(hb_h)
            self.bufs += [src, dst, vb, hb]
            self.io.append((src, dst))
            self.dp.append(_planes_struct(p, src, dst, vb, hb))
            m = None
            if p.qpmap:  # one map for every frame, units of 1 << qpmap luma samples
                m = np.random.default_rng(11 + i).integers(15, 52, (-(-p.h >> p.qpmap), -(-p.w >> p.qpmap))).astype(np.uint8)
                dm = ctx.alloc(m.size)
                dm.upload(m)
                self.bufs.append(dm)
                self.dp[-1].qp_map, self.dp[-1].qp_map_stride, self.dp[-1].ctu_log2, self.dp[-1].qp_map_frame_stride = \
                    dm.ptr, m.shape[1], p.qpmap, 0
            self.maps.append(m)
            lw, lh = _ctb_h(case, i, p)
            cols, rows = -(-p.w >> lw), -(-p.h >> lh)
            stride = cols + case.params_pad
            nf = p.n if case.params_per_frame else 1
            pfs = rows * stride + case.params_pad if case.params_per_frame else 0
            prm = np.zeros(max(pfs, rows * stride) * nf, dc_sao_dtype())
            per = []
            for f in range(nf):
                q = dc.sao_params_for(cols << lw, rows << lw, lw, seed=7 + 13 * f + i, bd=p.bd)  # rows x cols entries
                for r in range(rows):
                    prm[f * pfs + r * stride:f * pfs + r * stride + cols] = q[r]
                per.append(q)
            d = ctx.alloc(prm.nbytes)
            d.upload(prm.view(np.uint8))
            self.bufs.append(d)
            self.sao.append((d.ptr, stride, pfs, lw, lh))
            self.params.append(per)

    def free(self):
        for b in self.bufs:
            b.free()


def dc_sao_dtype():
    return np.dtype(_lib().SAO_CTB_DTYPE)


def entry_call(case, ops):
    """call(ctx_handle, stream) -> rc for the case's public entry"""
    L, lib = _lib().lib(), _lib()
    e, p0 = case.entry, case.planes[0]
    dp = ops.dp
    prm = lib.H265Params(0, 0, 0, 0)
    c_idx = 1 if p0.chroma else 0
    s0 = ops.sao[0]
    if e == "filter":
        return lambda h, s: L.hevc_deblocking_filter_device(h, C.byref(dp[0]), QP, None, case.variant, s)
    if e == "filter_h265":
        if case.cf != 1:
            return lambda h, s: L.hevcdbk_h265_filter_device_cf(h, C.byref(dp[0]), c_idx, case.cf, QP, C.byref(prm), case.variant, s)
        return lambda h, s: L.hevc_deblocking_filter_h265_device(h, C.byref(dp[0]), c_idx, QP, C.byref(prm), case.variant, s)
    if e == "filter_planes":
        arr = (lib.DevicePlanes * len(dp))(*dp)
        return lambda h, s: L.hevc_deblocking_filter_device_planes(h, arr, len(dp), QP, None, case.variant, s)
    if e == "sao":
        if case.cf != 1:
            return lambda h, s: L.hevcdbk_sao_filter_device_cf(h, C.byref(dp[0]), s0[0], s0[1], s0[2], s0[3], s0[4], None, 0, 0, s)
        return lambda h, s: L.hevc_sao_filter_device(h, C.byref(dp[0]), s0[0], s0[1], s0[2], s0[3], None, 0, 0, s)
    if e == "dbk_sao":
        return lambda h, s: L.hevc_deblock_sao_device(h, C.byref(dp[0]), QP, None, s0[0], s0[1], s0[2], s0[3], None, 0, 0, case.fused, s)
    if e == "dbk_sao_h265":
        if case.cf != 1:
            return lambda h, s: L.hevcdbk_h265_deblock_sao_device_cf(h, C.byref(dp[0]), c_idx, case.cf, QP, C.byref(prm), s0[0], s0[1],
                                                                    s0[2], s0[3], s0[4], None, 0, 0, case.fused, s)
        return lambda h, s: L.hevc_deblock_sao_h265_device(h, C.byref(dp[0]), c_idx, QP, C.byref(prm), s0[0], s0[1], s0[2], s0[3],
                                                          None, 0, 0, case.fused, s)
    arr = (lib.DevicePlanes * len(dp))(*dp)
    if e in ("dbk_sao_planes", "dbk_sao_h265_planes"):
        sp = (lib.SaoPlane * len(dp))()
        for i, (ptr, stride, pfs, lw, lh) in enumerate(ops.sao):
            sp[i].params, sp[i].params_stride, sp[i].params_frame_stride, sp[i].ctb_log2 = ptr, stride, pfs, lw
        if e == "dbk_sao_h265_planes":
            return lambda h, s: L.hevc_deblock_sao_h265_device_planes(h, arr, len(dp), QP, C.byref(prm), sp, case.fused, s)
        return lambda h, s: L.hevc_deblock_sao_device_planes(h, arr, len(dp), QP, None, sp, case.fused, s)
    if e == "dbk_sao_h265_planes_cf":
        sp = (lib.SaoPlaneCf * len(dp))()
        for i, (ptr, stride, pfs, lw, lh) in enumerate(ops.sao):
            sp[i].params, sp[i].params_stride, sp[i].params_frame_stride, sp[i].ctb_log2_w, sp[i].ctb_log2_h = ptr, stride, pfs, lw, lh
        return lambda h, s: L.hevcdbk_h265_deblock_sao_device_planes_cf(h, arr, len(dp), case.cf, QP, C.byref(prm), sp, case.fused, s)
    raise ValueError(e)


def check_identity(case, call):
    """the kernels a captured call enqueues (on a throwaway context) are the predicted ones; refused operands enqueue nothing"""
    from gpu_video_codec_amd import deblock
    want = dc.predict(case)
    cap = deblock.Context(0)
    try:
        rc, got = kernels_enqueued(lambda s: call(cap.handle, s))
    finally:
        cap.close()
    if isinstance(want, int):
        assert rc == want and got == [], (case.name, rc, got)
        return
    assert rc == 0, (case.name, rc)
    assert len(got) == len(want), (case.name, got, want)
    for (name, grid, block, lds), w in zip(got, want):
        # grid / block / LDS alone cannot tell sao8_kernel from sao_kernel<u8> or template arguments apart: the name is required
        assert name is not None, (case.name, "hipKernelNameRefByPtr returned NULL", grid, block, w)
        assert parse_kernel(name) == (w.kernel, w.args), (case.name, name, w)
        assert (grid, block, lds) == (w.grid, w.block, w.lds), (case.name, name, grid, block, lds, w)


# ---- expected output --------------------------------------------------------------------------------------------------------

def plane_op(case, i, p, params, qp_map=None):
    """op(a, y0, x0) of plane i: the entry's filters in order (SAO parameters of one frame), for a W x H plane"""
    import rext_oracle as rx
    e, h265 = case.entry, "h265" in case.entry
    ops = []
    if e.startswith("filter") or e.startswith("dbk_sao"):
        if not h265:
            ops.append(dc.op_filter_ref(QP, p.bd, p.chroma, W=p.w, H=p.h, qp_map=qp_map, ctu_log2=p.qpmap or 6))
        elif p.chroma and case.cf != 1:
            def f(a, y0, x0, p=p):
                vb, hb = dc.bs_arrays(True, a.shape[1], a.shape[0], y0, x0, p.w, p.h)
                return rx.filter_chroma_plane(a, vb, hb, case.cf, qp=QP, bit_depth=p.bd).astype(a.dtype)
            ops.append(f)
        else:
            ops.append(dc.op_filter_h265(QP, p.bd, c_idx=(i if e.startswith("dbk_sao_h265_planes") else int(p.chroma)), W=p.w, H=p.h))
    if "sao" in e:
        lw, lh = _ctb_h(case, i, p)
        sq = np.repeat(params, 2, axis=0) if lh != lw else params  # a tall CTB = two square ones with its parameters
        ops.append(dc.op_sao(sq, lw, p.bd))
    return dc.op_chain(*ops)


def frame_content(p, seed):
    """frame index -> content: a few distinct frames (the last one its own), so that 65535 frames need few oracle runs"""
    k = min(p.n, 3)
    rng = np.random.default_rng(seed)
    top = p.max_v
    pats = []
    for _ in range(k + (p.n > k)):
        base = rng.integers(top // 4, 3 * top // 4 + 1, (p.h // 8 + 1, p.w // 8 + 1))
        a = np.kron(base, np.ones((8, 8), np.int64))[:p.h, :p.w] + rng.integers(-3, 4, (p.h, p.w)) * (1 << (p.bd - 8))
        a[:min(8, p.h), :min(8, p.w)] = rng.integers(0, top + 1, (min(8, p.h), min(8, p.w)))
        pats.append(np.clip(a, 0, top).astype(np.uint8 if p.sb == 1 else np.uint16))
    idx = np.arange(p.n) % k
    if p.n > k:
        idx[-1] = k
    return pats, idx


def _layout(p, frames_bytes, fill):
    """host image of a plane buffer: rows at pitch, frames at frame_stride, padding = fill"""
    buf = np.full(p.nbytes(), fill, np.uint8)
    rowb = p.w * p.sb
    for f in range(p.n):
        v = buf[f * p.fs:f * p.fs + p.P * p.h].reshape(p.h, p.P)
        v[:, :rowb] = frames_bytes(f)
    return buf


def run_small(ctx, case):
    ops = Operands(ctx, case)
    try:
        call = entry_call(case, ops)
        contents, src_images = [], []
        for i, p in enumerate(case.planes):
            pats, idx = frame_content(p, seed=zlib.crc32(case.name.encode()) + i)
            contents.append((pats, idx))
            raw = [x.view(np.uint8).reshape(p.h, p.w * p.sb) for x in pats]
            src_images.append(_layout(p, lambda f: raw[idx[f]], SRC_PAD))
            ops.io[i][0].upload(src_images[-1])
        check_identity(case, call)
        rc = call(ctx.handle, None)
        ctx.synchronize()
        want = dc.predict(case)
        if isinstance(want, int):
            assert rc == want, (case.name, rc)
        else:
            assert rc == 0, (case.name, rc)
        for i, p in enumerate(case.planes):
            pats, idx = contents[i]
            dst = ops.io[i][1]
            got = dst.download(p.nbytes())
            if isinstance(want, int):
                exp = np.full(p.nbytes(), DST_FILL, np.uint8)
            else:
                memo = {}

                def out(f):
                    key = (idx[f], f if case.params_per_frame else 0)
                    if key not in memo:
                        prm = ops.params[i][key[1]]
                        r = plane_op(case, i, p, prm, ops.maps[i])(pats[idx[f]], 0, 0)
                        memo[key] = np.ascontiguousarray(r).view(np.uint8).reshape(p.h, p.w * p.sb)
                    return memo[key]
                exp = _layout(p, out, DST_FILL)
            if not np.array_equal(got, exp):
                bad = np.nonzero(got != exp)[0]
                f, r = bad[0] // p.fs, bad[0] % p.fs
                pytest.fail("%s plane %d: %d bytes differ, first at frame %d row %d byte %d (got %d want %d)" % (
                    case.name, i, bad.size, f, r // p.P, r % p.P, got[bad[0]], exp[bad[0]]))
            assert dst.sentinels_intact(), (case.name, i)
            src = ops.io[i][0]
            assert np.array_equal(src.download(p.nbytes()), src_images[i]) and src.sentinels_intact(), (case.name, i, "src written")
    finally:
        ops.free()


@pytest.fixture
def ctx():
    from gpu_video_codec_amd import deblock
    c = deblock.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", SMALL)
def test_dispatch_small(ctx, name):
    run_small(ctx, CASES[name])


# ---- giant planes: flat content, random windows ----------------------------------------------------------------------------

def test_giant_case_list():
    assert {n.split("_2g")[0] for n in GIANT if "_2g_" in n} >= {"filter", "filter_h265", "sao", "dbk_sao"}


@pytest.mark.parametrize("name", GIANT)
def test_dispatch_giant(ctx, name):
    case = CASES[name]
    (p,) = case.planes
    assert p.n == 1 and p.src_off == 0 and p.dst_off == 0
    base = _device_used()
    # flat content is a byte memset: 16-bit samples take a value whose two bytes are equal (0x0202 = 514 at 10 bit)
    fill = 128 if p.sb == 1 else 2
    flat = fill if p.sb == 1 else fill * 0x101
    assert flat <= p.max_v
    dt = np.uint8 if p.sb == 1 else np.uint16
    win = dc.standard_windows(p.w, p.h, p.bd, flat, p.P, seed=zlib.crc32(name.encode()) % 1000, size=(64, 256) if p.h > 128 else (p.h, 512))
    h265 = "h265" in case.entry
    src = Buf(ctx, p.nbytes(), 0, fill)
    dst = Buf(ctx, p.nbytes(), 0, DST_FILL)
    bufs = [src, dst]
    try:
        for i, (y0, y1, x0, x1) in enumerate(win.content):
            data = win.window_data(i)
            for r in range(y1 - y0):
                src.upload(data[r], (y0 + r) * p.P + x0 * p.sb)
        vb_h, hb_h = dc.bs_arrays(h265, p.w, p.h)
        vb, hb = ctx.alloc(vb_h.size), ctx.alloc(hb_h.size)
        vb.upload(vb_h)
        hb.upload(hb_h)
        bufs += [vb, hb]
        dp = _planes_struct(p, src, dst, vb, hb)
        ctb = case.ctb_log2
        cols, rows = -(-p.w >> ctb), -(-p.h >> ctb)
        prm = dc.sao_params_for(p.w, p.h, ctb, seed=5, bd=p.bd, win=win)
        d = ctx.alloc(prm.nbytes)
        d.upload(np.ascontiguousarray(prm).view(np.uint8).ravel())
        bufs.append(d)

        class O:
            pass
        ops = O()
        ops.dp, ops.sao = [dp], [(d.ptr, cols, 0, ctb, ctb)]
        call = entry_call(case, ops)
        check_identity(case, call)
        rc = call(ctx.handle, None)
        ctx.synchronize()
        print("\n%s: device memory in use during the case %.2f GiB" % (name, (_device_used() - base) / (1 << 30)))
        want = dc.predict(case)
        if isinstance(want, int):
            assert rc == want, (name, rc)
            exp_win = []
        else:
            assert rc == 0, (name, rc)
            op = plane_op(case, 0, p, prm)
            exp_win = dc.windowed(win, op, ctb if "sao" in case.entry else None)
        # the plane in chunks of rows: flat (or untouched) outside the check windows, the windowed oracle inside
        chunk = max(1, (256 << 20) // p.P)
        for y in range(0, p.h, chunk):
            n = min(chunk, p.h - y)
            got = dst.download(n * p.P, y * p.P).reshape(n, p.P)
            exp = np.full((n, p.P), DST_FILL, np.uint8)
            if not isinstance(want, int):
                smp = np.full((n, p.w), flat, dt)
                for (y0, y1, x0, x1), e in exp_win:
                    a, b = max(y0, y), min(y1, y + n)
                    if a < b:
                        smp[a - y:b - y, x0:x1] = e[a - y0:b - y0]
                exp[:, :p.w * p.sb] = smp.view(np.uint8)
            if not np.array_equal(got, exp):
                rr, cc = np.nonzero(got != exp)
                pytest.fail("%s: %d bytes differ in rows %d..%d, first at row %d col %d (got %d want %d)" % (
                    name, rr.size, y, y + n, y + rr[0], cc[0], got[rr[0], cc[0]], exp[rr[0], cc[0]]))
        assert dst.sentinels_intact() and src.sentinels_intact(), name
    finally:
        for b in bufs:
            b.free()
