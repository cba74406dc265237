"""Per-frame operands of a batch in every kernel family, on the GPU (cases and expected bytes: tests/batch_vectors.py).

Every case uploads its planes and operands (shared, tight, padded with poison in the gaps, or at a stride beyond 2 GiB), pre-fills
the destination, runs its public entry ONCE and compares every byte of every frame with the CPU expectation; row padding, the gaps
between frames, the sentinels around every buffer, the source (out of place) and every operand buffer must come back as uploaded.
The kernels enqueued are read from a stream capture (tests/kernel_capture.py) and must be of the families the dispatch restatement
predicts, so a case that fell back to another kernel cannot pass for the family it was written for.  The census of
test_batch_operands_cpu.py guarantees that an operand taken from another frame, or read at the wrong stride, changes every cell
of the frame; a mismatch here is reported with the frame whose operand would have produced the bytes seen.

The _sl, _g4, _sp and NV12 cases (Case.fam) go the same way through Run / check_output; the kernels of their capture are compared
with the literal names the case lists, and a mismatch on a plane of pairs names the frame per component.

On top, for one case per family: the batch equals n single-frame calls on the same buffers; reversing the frames and their
operands reverses the output; a shared operand and its tight replication give the same bytes."""
import collections
import ctypes as C
import dataclasses

import numpy as np
import pytest

import batch_vectors as bv
import dispatch_cases as dc
from kernel_capture import kernels_enqueued, parse_kernel

pytestmark = pytest.mark.gpu

GUARD = 256
SENT, DST_FILL, SRC_PAD = 0xA5, 0x5A, 0x33
CASES = bv.cases()
BY_NAME = {c.name: c for c in CASES}
RAN = collections.Counter()     # (family, operand, state) -> cases that ran and passed
CASES_RUN = [0]                 # test_batch_case invocations in this process
FAR_BUDGET = 6.07               # GiB: the peak test_gpu_dispatch.py needs; no case here may need more


def _lib():
    from gpu_video_codec_amd import _lib
    return _lib


def _device_used():
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return total.value - free.value


@pytest.fixture(scope="module")
def ctx():
    from gpu_video_codec_amd import deblock
    c = deblock.Context(0)
    yield c
    c.close()


class Dev:
    """a host image in device memory between GUARD sentinel bytes; the host keeps what it uploaded"""

    def __init__(self, ctx, image):
        self.image = np.ascontiguousarray(image).view(np.uint8).ravel().copy()
        self.host = np.concatenate([np.full(GUARD, SENT, np.uint8), self.image, np.full(GUARD, SENT, np.uint8)])
        self.raw = ctx.alloc(self.host.size)
        self.raw.upload(self.host)
        self.ptr = self.raw.ptr + GUARD

    def read(self):
        """(the image's bytes now, sentinels intact)"""
        got = self.raw.download(self.host.size)
        return got[GUARD:-GUARD], bool((got[:GUARD] == SENT).all() and (got[-GUARD:] == SENT).all())

    def untouched(self):
        got, ok = self.read()
        return ok and np.array_equal(got, self.image)

    def refill(self):
        self.raw.upload(self.host)

    def free(self):
        self.raw.free()


class Far:
    """n arrays at FAR_STRIDE bytes from one another; nothing else of the allocation is written"""

    def __init__(self, ctx, arrays, stride=bv.FAR_STRIDE):
        self.arrays = [np.ascontiguousarray(a).view(np.uint8).ravel().copy() for a in arrays]
        self.stride = stride
        self.raw = ctx.alloc(stride * (len(arrays) - 1) + self.arrays[0].size)
        for f, a in enumerate(self.arrays):
            self.raw.upload(a, f * stride)
        self.ptr = self.raw.ptr

    def untouched(self):
        return all(np.array_equal(self.raw.download(a.size, f * self.stride), a) for f, a in enumerate(self.arrays))

    def free(self):
        self.raw.free()


def plane_image(c, i, frames, fill):
    pw, ph, _, _ = c.geom(i)
    P, fs = c.pitch(i), c.frame_stride(i)
    buf = np.full(fs * (c.n - 1) + P * ph, fill, np.uint8)
    for f in range(c.n):
        v = buf[f * fs:f * fs + P * ph].reshape(ph, P)
        rb = c.row_samples(i) * c.sb   # a plane of pairs: (ph, pw, 2) samples, rows of 2 * pw
        v[:, :rb] = np.ascontiguousarray(frames[f], c.dtype).view(np.uint8).reshape(ph, rb)
    return buf


class Run:
    """the device side of a case: buffers, structures, and call(ctx handle, stream, frame) for its public entry"""

    def __init__(self, ctx, c, ops):
        self.ctx, self.c, self.ops, self.bufs, self.operands = ctx, c, ops, [], []
        lib = _lib()
        self.src, self.dst, self.dp, self.sao = [], [], [], []
        one_map = self._operand("map") if c.uses("map") and c.planes != "NV" else None
        self.borders = self._operand("borders") if c.uses("borders") else None
        self.sl = self._operand("sl") if c.uses("sl") else None   # (pointer, frame stride in 16-bit pairs)
        for i in range(c.n_planes):
            pw, ph, lw, lh = c.geom(i)
            s = Dev(ctx, plane_image(c, i, ops["frames"][i], SRC_PAD))
            d = s if c.in_place else Dev(ctx, np.full(s.image.size, DST_FILL, np.uint8))
            self.src.append(s)
            self.dst.append(d)
            self.bufs += [s] + ([] if c.in_place else [d])
            p = lib.DevicePlanes()
            p.src, p.dst, p.pitch, p.frame_stride, p.n_frames = s.ptr, d.ptr, c.pitch(i), c.frame_stride(i), c.n
            p.plane_w, p.plane_h, p.bit_depth, p.sample_bytes, p.is_chroma = pw, ph, c.bd, c.sb, int(c.chroma(i))
            bs = None
            if c.has_deblock():
                bs = (self._operand("bs", i, 0), self._operand("bs", i, 1))
                p.vert_bs, p.hor_bs, p.vert_bs_stride, p.hor_bs_stride = bs[0][0], bs[1][0], bs[0][1], bs[1][1]
            if c.uses("map", i):   # an NV12 call gives each plane a map of its own
                p.qp_map, p.qp_map_frame_stride = one_map if one_map is not None else self._operand("map", i)
                p.qp_map_stride, p.ctu_log2 = bv.map_of(c, ops, i)[0].shape[1], c.unit_log2
            self.dp.append(p)
            if c.has_sao():
                if c.pair(i):   # Cb and Cr: two arrays, one stride
                    cb, cr = self._operand("params", i, 0), self._operand("params", i, 1)
                    assert cb[1] == cr[1]
                    prm = ((cb[0], cr[0]), cb[1])
                else:
                    prm = self._operand("params", i)
                kp = self._operand("keep", i) if c.uses("keep", i) else (None, 0)
                self.sao.append((prm, kp, lw, lh, -(-pw // 8)))

    def _operand(self, x, i=0, which=0):
        """(device pointer, frame stride in entries) of one operand array in the case's state"""
        c = self.c
        arrs = bv.operand_arrays(c, self.ops, x, i, which)
        state = c.state(x, i)
        if state == "far" and x == "bs" and which != (0 if c.far_which == "vert" else 1):
            state = "tight"
        if state == "far" and x == "sl":
            b = Far(self.ctx, arrs[:c.n], bv.FAR_STRIDE_SL)
            stride = bv.FAR_STRIDE_SL // 2
        elif state == "far":
            b = Far(self.ctx, arrs[:c.n])
            stride = bv.FAR_STRIDE
        else:
            img, stride = bv.lay_out(arrs, state, bv.poison_entry(x, c.bd), bv.operand_dtype(x))
            b = Dev(self.ctx, img)
        self.bufs.append(b)
        self.operands.append((x, b))
        return b.ptr, stride

    def free(self):
        for b in self.bufs:
            b.free()

    def call(self, h, s, frame=None):
        """the case's entry on the whole batch, or on frame `frame` alone (pointers advanced, strides as they are)"""
        c, lib, L = self.c, _lib(), _lib().lib()
        f = frame or 0
        dps = []
        for i, p0 in enumerate(self.dp):
            p = lib.DevicePlanes.from_buffer_copy(p0)
            if frame is not None:
                p.n_frames = 1
                p.src, p.dst = p0.src + f * p0.frame_stride, p0.dst + f * p0.frame_stride
                if c.has_deblock():
                    p.vert_bs, p.hor_bs = p0.vert_bs + f * p0.vert_bs_stride, p0.hor_bs + f * p0.hor_bs_stride
                if p0.qp_map:
                    p.qp_map = p0.qp_map + f * p0.qp_map_frame_stride
            dps.append(p)
        arr = (lib.DevicePlanes * len(dps))(*dps)
        esz = bv.SAO_DT.itemsize

        def at(ptr, stride):   # a plane of pairs has two parameter arrays
            return tuple(q + f * stride * esz for q in ptr) if isinstance(ptr, tuple) else ptr + f * stride * esz
        sao = [(at(*prm), prm[1], (kp[0] + f * kp[1]) if kp[0] else None, kp[1], lw, lh, ks)
               for (prm, kp, lw, lh, ks) in self.sao]
        rows, cols = c.grid()
        bo = None
        if self.borders is not None:
            bo = C.byref(lib.SaoBorders(self.borders[0] + f * self.borders[1], cols, self.borders[1]))
        hp = lib.H265Params(*c.offs)
        c_idx = 1 if c.planes == "C" else 0
        e = c.entry
        if c.fam:
            return self.call_x(L, lib, h, s, f, arr, len(dps), sao, bo, hp, c_idx)
        if e == "filter" and not c.h265:
            return L.hevc_deblocking_filter_device(h, C.byref(arr[0]), bv.QP, None, c.variant, s)
        if e == "filter":
            if c.cf == 1:
                return L.hevc_deblocking_filter_h265_device(h, C.byref(arr[0]), c_idx, bv.QP, C.byref(hp), c.variant, s)
            return L.hevcdbk_h265_filter_device_cf(h, C.byref(arr[0]), c_idx, c.cf, bv.QP, C.byref(hp), c.variant, s)
        if e == "filter_planes":
            return L.hevc_deblocking_filter_device_planes(h, arr, len(dps), bv.QP, None, c.variant, s)
        if c.plain_entry:   # the entries without a borders argument; the square-CTB ones where the plane's CTBs are square
            assert bo is None
            if e == "sao":
                p, st, k, ks, lw, lh, kw = sao[0]
                if lw == lh:
                    return L.hevc_sao_filter_device(h, C.byref(arr[0]), p, cols, st, lw, k, kw if k else 0, ks, s)
                return L.hevcdbk_sao_filter_device_cf(h, C.byref(arr[0]), p, cols, st, lw, lh, k, kw if k else 0, ks, s)
            if e == "dbk_sao":
                p, st, k, ks, lw, lh, kw = sao[0]
                if c.cf == 1:
                    return L.hevc_deblock_sao_h265_device(h, C.byref(arr[0]), c_idx, bv.QP, C.byref(hp), p, cols, st, lw, k, kw if k else 0,
                                                          ks, c.fused, s)
                return L.hevcdbk_h265_deblock_sao_device_cf(h, C.byref(arr[0]), c_idx, c.cf, bv.QP, C.byref(hp), p, cols, st, lw, lh, k,
                                                            kw if k else 0, ks, c.fused, s)
        if e == "sao":
            p, st, k, ks, lw, lh, kw = sao[0]
            return L.hevcdbk_sao_filter_device_nox(h, C.byref(arr[0]), p, cols, st, lw, lh, k, kw if k else 0, ks, bo, s)
        if e == "dbk_sao" and not c.h265:
            p, st, k, ks, lw, lh, kw = sao[0]
            return L.hevc_deblock_sao_device(h, C.byref(arr[0]), bv.QP, None, p, cols, st, lw, k, kw if k else 0, ks, c.fused, s)
        if e == "dbk_sao":
            p, st, k, ks, lw, lh, kw = sao[0]
            return L.hevcdbk_h265_deblock_sao_device_nox(h, C.byref(arr[0]), c_idx, c.cf, bv.QP, C.byref(hp), p, cols, st, lw, lh, k,
                                                         kw if k else 0, ks, c.fused, bo, s)
        assert e == "dbk_sao_planes"
        sp = ((lib.SaoPlaneCf if c.h265 else lib.SaoPlane) * len(dps))()
        for i, (p, st, k, ks, lw, lh, kw) in enumerate(sao):
            sp[i].params, sp[i].params_stride, sp[i].params_frame_stride = p, cols, st
            sp[i].keep, sp[i].keep_stride, sp[i].keep_frame_stride = k, (kw if k else 0), ks
            if c.h265:
                sp[i].ctb_log2_w, sp[i].ctb_log2_h = lw, lh
            else:
                sp[i].ctb_log2 = lw
        if c.h265 and c.plain_entry:
            return L.hevcdbk_h265_deblock_sao_device_planes_cf(h, arr, len(dps), c.cf, bv.QP, C.byref(hp), sp, c.fused, s)
        if c.h265:
            return L.hevcdbk_h265_deblock_sao_device_planes_nox(h, arr, len(dps), c.cf, bv.QP, C.byref(hp), sp, c.fused, bo, s)
        return L.hevc_deblock_sao_device_planes(h, arr, len(dps), bv.QP, None, sp, c.fused, s)


    def call_x(self, L, lib, h, s, f, arr, n_planes, sao, bo, hp, c_idx):
        """the _sl / _g4 / _sp / NV12 entries"""
        c, e = self.c, self.c.entry
        so = None
        if self.sl is not None:
            so = C.byref(lib.SliceOffsets(self.sl[0] + f * self.sl[1] * 2, c.sl_grid()[1], self.sl[1] * 2, bv.SL_LOG2))
        cols = c.grid()[1]
        tail = e.rsplit("_", 1)[-1]
        if e in ("filter_sl", "filter_g4"):
            return getattr(L, "hevcdbk_h265_filter_device_" + tail)(h, C.byref(arr[0]), c_idx, c.cf, bv.QP, C.byref(hp), c.variant, so, s)
        if e == "filter_sp":
            return L.hevcdbk_h265_filter_device_sp(h, C.byref(arr[0]), bv.QP, C.byref(hp), c.variant, so, s)
        if e in ("dbk_sao_planes_sl", "dbk_sao_planes_g4"):
            sp = (lib.SaoPlaneCf * n_planes)()
            for i, (p, st, k, ks, lw, lh, kw) in enumerate(sao):
                sp[i].params, sp[i].params_stride, sp[i].params_frame_stride, sp[i].ctb_log2_w, sp[i].ctb_log2_h = p, cols, st, lw, lh
                sp[i].keep, sp[i].keep_stride, sp[i].keep_frame_stride = k, (kw if k else 0), ks
            return getattr(L, "hevcdbk_h265_deblock_sao_device_planes_" + tail)(h, arr, n_planes, c.cf, bv.QP, C.byref(hp), sp, c.fused, bo, so, s)
        if e == "nv12":
            p, st, k, ks, lw, lh, kw = sao[0]
            y = lib.SaoPlaneCf(p, cols, st, lw, lh, k, kw if k else 0, ks)
            (pcb, pcr), st, k, ks, lw, lh, kw = sao[1]
            pr = lib.SaoPlaneSp(pcb, pcr, cols, st, lw, k, kw if k else 0, ks)
            return L.hevcdbk_h265_deblock_sao_device_nv12(h, C.byref(arr[0]), C.byref(arr[1]), bv.QP, C.byref(hp), C.byref(y), C.byref(pr), c.fused,
                                                          bo, so, s)
        p, st, k, ks, lw, lh, kw = sao[0]
        if e == "sao_g4":
            return L.hevcdbk_sao_filter_device_g4(h, C.byref(arr[0]), p, cols, st, lw, lh, k, kw if k else 0, ks, bo, s)
        if e in ("dbk_sao_sl", "dbk_sao_g4"):
            return getattr(L, "hevcdbk_h265_deblock_sao_device_" + tail)(h, C.byref(arr[0]), c_idx, c.cf, bv.QP, C.byref(hp), p, cols, st, lw, lh, k,
                                                                         kw if k else 0, ks, c.fused, bo, so, s)
        if e == "sao_sp":
            return L.hevcdbk_sao_filter_device_sp(h, C.byref(arr[0]), p[0], p[1], cols, st, lw, k, kw if k else 0, ks, bo, s)
        fn = {"dbk_sao_sp": L.hevcdbk_h265_deblock_sao_device_sp, "dbk_sao_sp_fused": L.hevcdbk_h265_deblock_sao_device_sp_fused}[e]
        return fn(h, C.byref(arr[0]), bv.QP, C.byref(hp), p[0], p[1], cols, st, lw, k, kw if k else 0, ks, c.fused, bo, so, s)


def diagnose(c, ops, i, f, got):
    """which wrong operand would have produced the bytes seen in frame f of plane i; on a plane of pairs, per component"""
    hits = []
    comps = [("", lambda a: a)] if not c.pair(i) else [(" (Cb)", lambda a: a[..., 0]), (" (Cr)", lambda a: a[..., 1])]
    want = bv.expected(c, ops, i, f)
    for x in bv.OPERANDS:
        if c.state(x, i) not in bv.PER_FRAME:
            continue
        for g in range(c.n):
            if g != f:
                w = bv.with_frame_of(c, ops, i, f, x, g)
                hits += ["%s of frame %d%s" % (x, g, tag) for tag, v in comps if np.array_equal(v(w), v(got)) and not np.array_equal(v(want), v(got))]
        if c.state(x, i) == "padded" and f >= 1:
            kw = bv._own(c, ops, i, f)
            kw.update(bv.tight_read(c, ops, x, i, f))
            w = bv.oracle_frame(c, i, ops["frames"][i][f], **kw)
            hits += ["%s read at the tight stride%s" % (x, tag) for tag, v in comps if np.array_equal(v(w), v(got)) and not np.array_equal(v(want), v(got))]
    if c.pair(i) and c.has_sao():
        kw = bv._own(c, ops, i, f)
        kw["params"] = kw["params"][::-1]
        w = bv.oracle_frame(c, i, ops["frames"][i][f], **kw)
        hits += ["the other component's parameters%s" % tag for tag, v in comps if np.array_equal(v(w), v(got))]
    return hits or ["no single wrong operand explains the bytes"]


def check_output(c, ops, run, exp, tag):
    for i in range(c.n_planes):
        pw, ph, _, _ = c.geom(i)
        want = plane_image(c, i, [exp[i, f] for f in range(c.n)], SRC_PAD if c.in_place else DST_FILL)
        got, guards = run.dst[i].read()
        if not np.array_equal(got, want):
            P, fs = c.pitch(i), c.frame_stride(i)
            for f in range(c.n):
                g = got[f * fs:f * fs + P * ph].reshape(ph, P)
                w = want[f * fs:f * fs + P * ph].reshape(ph, P)
                if not np.array_equal(g, w):
                    rb = c.row_samples(i) * c.sb
                    inside = np.ascontiguousarray(g[:, :rb]).view(c.dtype)
                    inside = inside.reshape(ph, pw, 2) if c.pair(i) else inside
                    n_bad = int((g != w).sum())
                    pad_bad = int((g[:, rb:] != w[:, rb:]).sum())
                    pytest.fail("%s %s: plane %d frame %d of %d: %d bytes differ (%d of them row padding); states %s; %s" % (
                        c.name, tag, i, f, c.n, n_bad, pad_bad, c.st, ", ".join(diagnose(c, ops, i, f, inside))))
            pytest.fail("%s %s: plane %d: bytes between the frames were written" % (c.name, tag, i))
        assert guards, (c.name, tag, i, "sentinels around the destination")
        if not c.in_place:
            assert run.src[i].untouched(), (c.name, tag, i, "source written")
    for x, b in run.operands:
        assert b.untouched(), (c.name, tag, x, "operand buffer written")


def check_identity(c, run):
    """the kernels of a captured call (throwaway context, after one plain call that sizes its scratch) are of the predicted families"""
    from gpu_video_codec_amd import deblock
    cap = deblock.Context(0)
    try:
        if c.fam or any(bv.rewrites_422(c)) or c.uses("borders") or (c.has_sao() and c.has_deblock()):
            assert run.call(cap.handle, None) == 0
            cap.synchronize()
        rc, got = kernels_enqueued(lambda s: run.call(cap.handle, s))
    finally:
        cap.close()
    assert rc == 0, (c.name, rc)
    names = [parse_kernel(k[0]) for k in got]
    rew = (sum(n == "sao_rows_x2_kernel" for n, _ in names), sum(n == "sao_nox_rows_x2_kernel" for n, _ in names))
    assert rew == bv.rewrites_422(c), (c.name, rew, names)
    if c.name in bv.PINNED:   # the instantiation only this case reaches: its name and template arguments, not its family alone
        assert names == [bv.PINNED[c.name]], (c.name, names)
    if c.fam:   # the dispatch restatement does not know these families: the literal names the case was written for (these kernels
        # take the borders as an argument of the one kernel: there is no _nox_ twin whose name could be asserted)
        ran = [n for n, _ in names if "rows_x2" not in n]
        assert ran == list(c.kernels), (c.name, ran, c.kernels)
        for n, a in names:   # which block map the packed _sl / _g4 kernels ran: the template argument LINEAR
            if n in bv.LINEAR_ARG:
                assert a[bv.LINEAR_ARG[n]] == int(c.linear), (c.name, n, a)
        return ran
    fams = [dc.family_of(n.replace("_nox_", "_"), a) for n, a in names if "rows_x2" not in n]
    assert fams == bv.families(c), (c.name, fams, bv.families(c), names)
    if "dbk_generic_kernel" in [n for n, _ in names]:   # its launcher selects on sample width, plane kind and QP map: the arguments too
        assert names == [(l.kernel, l.args) for l in dc.predict(bv.dispatch_case(c))], (c.name, names)
    if c.uses("borders"):
        assert all("_nox_" in n for n, _ in names if "sao" in n and "rows_x2" not in n), (c.name, names)
    return fams


def run_case(ctx, c, ops, exp, tag="batch", per_frame_calls=False, identity=False):
    run = Run(ctx, c, ops)
    try:
        if per_frame_calls:
            for f in range(c.n):
                assert run.call(ctx.handle, None, frame=f) == 0, (c.name, tag, f)
        else:
            assert run.call(ctx.handle, None) == 0, (c.name, tag)
        ctx.synchronize()
        check_output(c, ops, run, exp, tag)
        if identity:
            check_identity(c, run)
    finally:
        run.free()


def expectations(c, ops):
    return {(i, f): bv.expected(c, ops, i, f) for i in range(c.n_planes) for f in range(c.n)}


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_batch_case(ctx, name):
    c = BY_NAME[name]
    ops = bv.make_operands(c, bv.seed_of(c))
    CASES_RUN[0] += 1
    far = "far" in c.st.values()
    assert not far or not c.fam or c.n == 3
    base = _device_used() if far else 0
    run = Run(ctx, c, ops)
    try:
        assert run.call(ctx.handle, None) == 0, name
        ctx.synchronize()
        if far:
            used = (_device_used() - base) / (1 << 30)
            print("\n%s: device memory in use during the case %.2f GiB" % (name, used))
            assert used <= FAR_BUDGET, (name, used)
        check_output(c, ops, run, expectations(c, ops), "batch")
        check_identity(c, run)
    finally:
        run.free()
    for key in bv.attribution(c):
        RAN[key] += 1


# ---- metamorphic checks, one case per family -------------------------------------------------------------------------------------

def _one_per_family(pred):
    seen, out = set(), []
    for c in CASES:
        if "far" in c.st.values() or not pred(c):
            continue
        key = (tuple(bv.families(c)), c.mode, c.bd > 8)
        if key not in seen:
            seen.add(key)
            out.append(c.name)
    return out


PER_FRAME_CASES = _one_per_family(lambda c: c.n > 1 and not c.in_place and any(s in bv.PER_FRAME for s in bv.all_states(c)))
SHARED_CASES = _one_per_family(lambda c: c.n > 1 and "shared" in bv.all_states(c))


@pytest.mark.parametrize("name", PER_FRAME_CASES)
def test_batch_equals_single_frame_calls(ctx, name):
    c = BY_NAME[name]
    ops = bv.make_operands(c, bv.seed_of(c))
    run_case(ctx, c, ops, expectations(c, ops), "n single-frame calls", per_frame_calls=True)


@pytest.mark.parametrize("name", PER_FRAME_CASES)
def test_reversed_frames_and_operands_reverse_the_output(ctx, name):
    c = BY_NAME[name]
    ops = bv.make_operands(c, bv.seed_of(c))
    exp = expectations(c, ops)
    rev = bv.reverse(c, ops)
    run_case(ctx, c, rev, {(i, f): exp[i, c.n - 1 - f] for (i, f) in exp}, "reversed")


@pytest.mark.parametrize("name", SHARED_CASES)
def test_shared_equals_tight_replication(ctx, name):
    c = BY_NAME[name]
    ops = bv.make_operands(c, bv.seed_of(c))
    exp = expectations(c, ops)
    for x in bv.OPERANDS:
        if "shared" in c.states(x):
            t = dataclasses.replace(c, st=bv.tightened(c.st, x), st1=bv.tightened(c.st1, x))
            run_case(ctx, t, bv.replicate(c, ops, x), exp, "%s replicated tight" % x)


# ---- the Python wrapper -------------------------------------------------------------------------------------------------------

def test_device_batch_per_frame_qp_maps(ctx):
    """DeviceBatch.set_qp_map: the 2-D form gives the DevicePlanes it always gave; (n, rows, cols) sets the frame stride, tight or
    padded, and the launch reads each frame's own map"""
    from gpu_video_codec_amd import deblock
    from oracle import oracle as o
    c = BY_NAME["map_ref_rows8_tight"] if "map_ref_rows8_tight" in BY_NAME else next(x for x in CASES if x.name.startswith("map_ref_rows8"))
    ops = bv.make_operands(c, bv.seed_of(c))
    maps = np.stack(ops["map"])
    size = maps[0].size
    for stride in (None, size + 7):
        b = deblock.DeviceBatch(ctx, c.w, c.h, c.n, per_frame_bs=False)
        b.upload_all(np.stack(ops["frames"][0]))
        b.set_qp_map(maps, c.unit_log2, **({} if stride is None else {"frame_stride": stride}))
        p = b.planes()
        assert p.qp_map_frame_stride == (size if stride is None else stride) and p.qp_map_stride == maps.shape[2] and p.ctu_log2 == c.unit_log2
        ctx.filter_device(p, bv.QP)
        ctx.synchronize()
        for f in range(c.n):
            assert np.array_equal(b.download_frame(f), o.filter_plane(ops["frames"][0][f], bv.QP, qp_map=maps[f], ctu_log2=c.unit_log2)), (stride, f)
        b.free()
    b = deblock.DeviceBatch(ctx, c.w, c.h, c.n, per_frame_bs=False)
    b.set_qp_map(maps[0], c.unit_log2)
    p = b.planes()
    assert p.qp_map_frame_stride == 0 and p.qp_map == b.qp_map.ptr and p.qp_map_stride == maps.shape[2] and b.qp_map.nbytes == size
    with pytest.raises(ValueError):
        b.set_qp_map(maps[0], c.unit_log2, frame_stride=size)
    with pytest.raises(ValueError):
        b.set_qp_map(maps[:1], c.unit_log2)
    with pytest.raises(ValueError):
        b.set_qp_map(maps, c.unit_log2, frame_stride=size - 1)
    b.free()


def test_device_batch_per_frame_qp_maps_semi_planar(ctx):
    """the sibling for DeviceBatch(..., semi_planar=True): set_qp_map with one map per frame, tight and with a gap, through
    filter_device_h265(semi_planar=True); then both planes of the picture through Context.deblock_sao_nv12, the luma maps with a
    gap and the pair plane's tight.  Every frame is the statement run with that frame's own map"""
    from gpu_video_codec_amd import deblock
    c = BY_NAME["nv12_8_n3"]
    ops = bv.make_operands(c, bv.seed_of(c))
    maps = np.stack(ops["map"][0])
    assert all((maps[f] != maps[g]).all() for f in range(c.n) for g in range(f))
    size = maps[0].size
    tc, beta, cb, cr = c.offs
    h265 = dict(tc_offset_div2=tc, beta_offset_div2=beta, cb_qp_offset=cb, cr_qp_offset=cr)

    bs_held = []

    def batch(i, stride):
        pw, ph, _, _ = c.geom(i)
        b = deblock.DeviceBatch(ctx, pw, ph, c.n, pitch=c.pitch(i), semi_planar=c.pair(i))
        b.upload_all(np.stack(ops["frames"][i]))
        b.set_qp_map(maps, c.unit_log2, **({} if stride is None else {"frame_stride": stride}))
        p = b.planes()
        if c.pair(i):
            for f in range(c.n):
                b.set_bs(f, *ops["bs"][i][f])
        else:   # a luma batch in multiples of 8 holds the reference-exact mode's arrays: the spec-exact ones in buffers of their own
            for k, field in enumerate(("vert_bs", "hor_bs")):
                a = np.stack([ops["bs"][i][f][k] for f in range(c.n)])
                bs_held.append(ctx.alloc(a.nbytes))
                bs_held[-1].upload(a)
                setattr(p, field, bs_held[-1].ptr)
                setattr(p, field + "_stride", a.shape[1])
        assert p.qp_map_frame_stride == (size if stride is None else stride) and p.qp_map_stride == maps.shape[2] and p.ctu_log2 == c.unit_log2
        return b, p

    for stride in (None, size + 7):
        b, p = batch(1, stride)
        ctx.filter_device_h265(p, bv.QP, semi_planar=True, **h265)
        ctx.synchronize()
        for f in range(c.n):
            want = bv.deblock_x(c, 1, ops["frames"][1][f], maps[f], ops["bs"][1][f], None)
            assert np.array_equal(b.download_frame(f), want), (stride, f)
            assert not np.array_equal(want, bv.deblock_x(c, 1, ops["frames"][1][f], maps[(f + 1) % c.n], ops["bs"][1][f], None))
        b.free()
    (yb, yp), (pb, pp) = batch(0, size + 7), batch(1, None)
    rows, cols = c.grid()
    held = [ctx.alloc(rows * cols * bv.SAO_DT.itemsize * c.n) for _ in range(3)]
    held[0].upload(np.stack(ops["params"][0]))
    held[1].upload(np.stack([p[0] for p in ops["params"][1]]))
    held[2].upload(np.stack([p[1] for p in ops["params"][1]]))
    ctx.deblock_sao_nv12(yp, pp, bv.QP, dict(params=held[0].ptr, params_stride=cols, params_frame_stride=rows * cols, ctb_log2=c.geom(0)[2]),
                         dict(params_cb=held[1].ptr, params_cr=held[2].ptr, params_stride=cols, params_frame_stride=rows * cols, ctb_log2=c.geom(1)[2]),
                         h265=h265)
    ctx.synchronize()
    for f in range(c.n):
        for i, b in ((0, yb), (1, pb)):
            want = bv.oracle_frame(c, i, ops["frames"][i][f], qmap=maps[f], bs=ops["bs"][i][f], params=ops["params"][i][f])
            assert np.array_equal(b.download_frame(f), want), ("nv12", i, f)
    for x in [yb, pb] + held + bs_held:
        x.free()


# ---- the 3-D forms: the frame index from the grid's z, on planes just past the guard of the renumbered grid ------------------------

@pytest.mark.parametrize("name", [g.name for g in bv.giants()])
def test_giant_3d(ctx, name):
    """flat frames with random windows, parameters / keep map / borders per frame: every byte of every frame (flat outside the check
    windows, the windowed oracle inside, the row padding as it was filled), the gap between the frames and the operand buffers; the
    capture shows the case's kernel with its template arguments on the 3-D grid (strips per row, strip rows, frames)"""
    lib, L = _lib(), _lib().lib()
    g = {x.name: x for x in bv.giants()}[name]
    p = g.plane()
    ops = bv.giant_operands(g)
    rows, cols = g.grid()
    kr, kc = g.keep_shape()
    px = g.comps * g.sb                              # bytes per sample position of a row: a pair of 8-bit samples is two
    flat_byte = g.flat & 0xFF
    assert g.flat == (flat_byte if g.sb == 1 else flat_byte * 0x0101)   # the flat value is one byte repeated: a memset makes the plane
    base = _device_used()
    src, dst = ctx.alloc(p.nbytes() + GUARD), ctx.alloc(p.nbytes() + GUARD)   # GUARD bytes behind the last row of the last frame
    bufs = [src, dst]
    try:
        assert L.hevcdbk_memset_d(ctx.handle, src.ptr, flat_byte, p.nbytes() + GUARD) == 0
        assert L.hevcdbk_memset_d(ctx.handle, dst.ptr, DST_FILL, p.nbytes() + GUARD) == 0
        for f in range(g.n):
            wins = ops["windows"][f]
            for i, (y0, y1, x0, x1) in enumerate(wins[0].content):
                data = np.stack([w.window_data(i) for w in wins], axis=-1)   # (rows, samples, components): pairs interleaved
                data = np.ascontiguousarray(data).view(np.uint8).reshape(y1 - y0, (x1 - x0) * px)
                for r in range(y1 - y0):
                    src.upload(data[r], f * p.fs + (y0 + r) * p.P + x0 * px)
        dev = {}
        for x, which in (("params", 0), ("params_cr", 1), ("keep", 0), ("borders", 0)):
            if x == "params_cr" and g.comps == 1:
                continue
            y = "params" if x == "params_cr" else x
            img, stride = bv.lay_out(bv.giant_arrays(g, ops, y, which), g.state, bv.poison_entry(y, g.bd), bv.operand_dtype(y))
            dev[x] = (Dev(ctx, img), stride)
            bufs.append(dev[x][0])
        dp = lib.DevicePlanes()
        dp.src, dp.dst, dp.pitch, dp.frame_stride, dp.n_frames = src.ptr, dst.ptr, p.P, p.fs, g.n
        dp.plane_w, dp.plane_h, dp.bit_depth, dp.sample_bytes, dp.is_chroma = g.w, g.h, g.bd, g.sb, int(g.kind == "sp")
        bo = lib.SaoBorders(dev["borders"][0].ptr, cols, dev["borders"][1])

        def call(h, s):
            if g.kind == "sp":
                assert dev["params"][1] == dev["params_cr"][1]
                return L.hevcdbk_sao_filter_device_sp(h, C.byref(dp), dev["params"][0].ptr, dev["params_cr"][0].ptr, cols, dev["params"][1], g.ctb_log2,
                                                      dev["keep"][0].ptr, kc, dev["keep"][1], C.byref(bo), s)
            entry = L.hevcdbk_sao_filter_device_g4 if g.kind == "g4" else L.hevcdbk_sao_filter_device_nox
            return entry(h, C.byref(dp), dev["params"][0].ptr, cols, dev["params"][1], g.ctb_log2, g.ctb_log2, dev["keep"][0].ptr, kc, dev["keep"][1],
                         C.byref(bo), s)
        assert call(ctx.handle, None) == 0
        ctx.synchronize()
        used = (_device_used() - base) / (1 << 30)
        print("\n%s: device memory in use during the case %.2f GiB" % (name, used))
        assert used <= FAR_BUDGET, (name, used)
        for f in range(g.n):
            exp_win = bv.giant_windows(g, ops, f)
            chunk = max(1, (256 << 20) // p.P)
            for y in range(0, g.h, chunk):
                n = min(chunk, g.h - y)
                got = dst.download(n * p.P, f * p.fs + y * p.P).reshape(n, p.P)
                exp = np.full((n, p.P), flat_byte, np.uint8)
                exp[:, g.row_bytes:] = DST_FILL      # the row padding: as the destination was filled
                for (y0, y1, x0, x1), e in exp_win:
                    a, b = max(y0, y), min(y1, y + n)
                    if a < b:
                        eb = np.ascontiguousarray(e).view(np.uint8).reshape(y1 - y0, (x1 - x0) * px)
                        exp[a - y:b - y, x0 * px:x1 * px] = eb[a - y0:b - y0]
                if not np.array_equal(got, exp):
                    rr, cc = np.nonzero(got != exp)
                    pytest.fail("%s frame %d: %d bytes differ in rows %d..%d, first at row %d byte %d (got %d want %d)" % (
                        name, f, rr.size, y, y + n, y + rr[0], cc[0], got[rr[0], cc[0]], exp[rr[0], cc[0]]))
        for f in range(g.n):    # the gap behind each frame; behind the last one the guard bytes
            gap = dst.download(p.fs - p.P * g.h if f < g.n - 1 else GUARD, f * p.fs + p.P * g.h)
            assert (gap == DST_FILL).all(), (name, "bytes between or behind the frames were written")
        for x, (b, _) in dev.items():
            assert b.untouched(), (name, x, "operand buffer written")
        from gpu_video_codec_amd import deblock
        cap = deblock.Context(0)
        try:
            rc, got = kernels_enqueued(lambda s: call(cap.handle, s))
        finally:
            cap.close()
        assert rc == 0
        names = [parse_kernel(k[0]) for k in got]
        if not g.kind:
            assert [dc.family_of(n.replace("_nox_", "_"), a) for n, a in names] == ["sao8<3d>"] == g.families(), names
        tx, tpf, _ = dc.sao_strips(p)
        assert names == [g.kernel] and got[0][1] == (tx, tpf // tx, g.n) and got[0][2] == (dc.SAO_STRIP, 1, 1), (names, got)
    finally:
        for b in bufs:
            b.free()



# ---- the report: family x operand x state ---------------------------------------------------------------------------------------

def test_report_and_no_promised_cell_is_empty():
    """runs last: every (family, operand, state) the CPU coverage test counts was run and passed here.  RAN is filled by
    test_batch_case in this process, so the emptiness assertion holds only for a run of the whole file in one process: with a
    selection of tests (-k, --lf), after a failing case or with the cases spread over workers the table is printed only"""
    promised = collections.Counter(k for c in CASES for k in bv.attribution(c))
    # the _sl / _g4 / _sp / NV12 kernels by name: each operand a kernel takes is promised shared, tight and padded (the _sl
    # deblocking kernels take sl tight: in every state it is test_gpu_slice_offsets.py's)
    for k in sorted(set(bv.K_SL.values()) | set(bv.K_G4.values()) | set(bv.K_SP.values())):
        for x in (("map", "bs", "sl") if k.startswith("dbk") else ()) + (("params", "keep", "borders") if "sao" in k else ()):
            for st in bv.THREE:
                if k in (bv.K_SL["g"], bv.K_SL[8], bv.K_SL[16]) and x == "sl" and st != "tight":
                    continue
                assert promised[k, x, st], ("no case promises", k, x, st)
    print("\nfamily                operand  state    cases passed / promised")
    for (fam, x, s), n in sorted(promised.items()):
        print("%-36s %-8s %-8s %3d / %3d" % (fam, x, s, RAN[fam, x, s], n))
    empty = [k for k in promised if RAN[k] == 0]
    if CASES_RUN[0] == len(CASES):   # every case was collected and run here
        assert not empty, empty
