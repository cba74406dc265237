"""Python binding of the C ABI (include/hevc_deblock.h) -- plumbing for tests and bench.py.

The compute path is libhevcdbk.so (hand-written HIP, gfx950).  Nothing here computes pixels.

`ReadYuvFrame` mirrors the reference's class of the same name
(hevc_deblocking_filter_cpu.h:33-132, 995-1018: ctor(file, w, h, Qp) / SetBoundaryStrenght /
DeblockingFilter / Save) so that tests read like a test of the reference would; its
DeblockingFilter() runs on the GPU through hevc_deblocking_filter().
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import (DeblockError, KERNEL_AUTO, KERNEL_GENERIC, KERNEL_PACKED)  # noqa: F401


def _chk(rc, ctx=None):
    if rc != 0:
        detail = ""
        if ctx is not None and rc == _lib.ERR_HIP:
            detail = _lib.lib().hevcdbk_last_error(ctx).decode()
        raise DeblockError(rc, detail)


def num_vert_bs(w, h):
    return int(_lib.lib().hevcdbk_num_vert_bs(w, h))


def num_hor_bs(w, h):
    return int(_lib.lib().hevcdbk_num_hor_bs(w, h))


def default_bs(w, h):
    v = np.empty(num_vert_bs(w, h), np.uint8)
    hh = np.empty(num_hor_bs(w, h), np.uint8)
    _chk(_lib.lib().hevcdbk_default_bs(w, h, v.ctypes.data, hh.ctypes.data))
    return v, hh


def default_tables():
    L = _lib.lib()
    return (np.array(L.hevcdbk_default_tc_table().contents, np.uint32),
            np.array(L.hevcdbk_default_beta_table().contents, np.uint32))


def device_count():
    return int(_lib.lib().hevcdbk_device_count())


def _tables(tc, beta):
    if tc is None and beta is None:
        return None, []
    t = _lib.Tables()
    keep = []
    for name, arr in (("tc", tc), ("beta", beta)):
        if arr is not None:
            a = np.ascontiguousarray(arr, np.uint32)
            keep.append(a)
            setattr(t, name, a.ctypes.data)
    return t, keep


def _bs(keep, **arrays):
    """an _lib.Bs of the given uint8 arrays (vert=, hor=, chroma_vert=, chroma_hor=); `keep` holds them alive for the call"""
    bs = _lib.Bs()
    for nm, arr in arrays.items():
        a = np.ascontiguousarray(arr, np.uint8)
        keep.append(a)
        setattr(bs, nm, a.ctypes.data)
        setattr(bs, "n_" + nm, a.size)
    return bs


def _frame(fr, planes, bit_depth):
    """fills the _lib.Frame `fr` from writable 2-D numpy planes (y,) or (y, u, v) with contiguous rows"""
    fr.height, fr.width = planes[0].shape
    fr.bit_depth, fr.sample_bytes = bit_depth, planes[0].dtype.itemsize
    for i, p in enumerate(planes):
        assert p.flags.writeable and p.strides[1] == p.itemsize
        fr.plane[i] = p.ctypes.data
        fr.pitch[i] = p.strides[0]
    return fr


def filter_yuv_file_multi(devices, in_name, out_name, width, height, qp, *, vert_bs=None, hor_bs=None):
    """hevcdbk_filter_yuv_file_multi: the file operator sharded frame-parallel over `devices` (one worker thread and one
    context per entry; no collective).  Returns (n_frames, wall seconds)."""
    keep = []
    bs = _bs(keep, vert=vert_bs, hor=hor_bs) if vert_bs is not None else None
    dev = (C.c_int * len(devices))(*devices)
    n, tm = C.c_uint(0), _lib.Timing()
    rc = _lib.lib().hevcdbk_filter_yuv_file_multi(dev, len(devices), os.fsencode(in_name), os.fsencode(out_name), width, height,
                                                  int(qp), None if bs is None else C.byref(bs), None, C.byref(n), C.byref(tm))
    _chk(rc)
    return n.value, tm.pipelined_s


class DeviceBuffer:
    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, int(nbytes)
        p = C.c_void_p()
        _chk(_lib.lib().hevcdbk_device_malloc(ctx.handle, self.nbytes, C.byref(p)), ctx.handle)
        self.ptr = p.value

    def upload(self, arr, offset=0):
        a = np.ascontiguousarray(arr)
        assert offset + a.nbytes <= self.nbytes
        _chk(_lib.lib().hevcdbk_memcpy_h2d(self.ctx.handle, self.ptr + offset, a.ctypes.data, a.nbytes), self.ctx.handle)

    def download(self, nbytes=None, offset=0, dtype=np.uint8):
        nbytes = self.nbytes - offset if nbytes is None else nbytes
        out = np.empty(nbytes, np.uint8)
        _chk(_lib.lib().hevcdbk_memcpy_d2h(self.ctx.handle, out.ctypes.data, self.ptr + offset, nbytes), self.ctx.handle)
        return out.view(dtype)

    def free(self):
        if self.ptr:
            _lib.lib().hevcdbk_device_free(self.ctx.handle, self.ptr)
            self.ptr = None

    @classmethod
    def adopt(cls, ctx, ptr, nbytes):
        """A DeviceBuffer around memory the library allocated (hevcdbk_device_malloc_probed); free() releases it."""
        b = cls.__new__(cls)
        b.ctx, b.nbytes, b.ptr = ctx, int(nbytes), ptr
        return b


class Context:
    """hevcdbk_context: one per HIP device; owns the compute stream and the two copy streams."""

    def __init__(self, device=0):
        h = C.c_void_p()
        _chk(_lib.lib().hevcdbk_create(device, C.byref(h)))
        self.handle = h
        self.device = device

    def close(self):
        if self.handle:
            _lib.lib().hevcdbk_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def device_info(self):
        i = _lib.DeviceInfo()
        _chk(_lib.lib().hevcdbk_get_device_info(self.handle, C.byref(i)))
        return {"name": i.name.decode(), "gcn_arch": i.gcn_arch.decode(), "compute_units": i.compute_units,
                "wavefront_size": i.wavefront_size, "total_global_mem": i.total_global_mem}

    def synchronize(self):
        _chk(_lib.lib().hevcdbk_synchronize(self.handle), self.handle)

    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    # -- hevc_deblocking_filter(frame, bS, QP, tables): host planes, in place --------------------
    def filter_frame(self, y, u=None, v=None, *, qp, bit_depth=8, vert_bs=None, hor_bs=None,
                     chroma_vert_bs=None, chroma_hor_bs=None, qp_map=None, ctu_log2=6,
                     tc_table=None, beta_table=None, check_sizes=True, want_timing=True):
        """Filters the given 2-D numpy planes IN PLACE (they must be writable, C-contiguous rows).
        Returns the reference's timing triple as a dict."""
        fr = _frame(_lib.Frame(), [y] + ([u, v] if u is not None else []), bit_depth)
        bs = None
        keep = []
        if vert_bs is not None or chroma_vert_bs is not None:
            given = {"vert": vert_bs, "hor": hor_bs, "chroma_vert": chroma_vert_bs, "chroma_hor": chroma_hor_bs}
            bs = _bs(keep, **{nm: arr for nm, arr in given.items() if arr is not None})
        q = _lib.Qp()
        q.qp, q.ctu_log2 = int(qp), ctu_log2
        if qp_map is not None:
            m = np.ascontiguousarray(qp_map, np.uint8)
            keep.append(m)
            q.map, q.map_stride = m.ctypes.data, m.shape[1]
        t, k2 = _tables(tc_table, beta_table)
        tm = _lib.Timing()
        rc = _lib.lib().hevc_deblocking_filter(self.handle, C.byref(fr), None if bs is None else C.byref(bs),
                                               C.byref(q), None if t is None else C.byref(t),
                                               C.byref(tm) if want_timing else None)
        _chk(rc, self.handle)
        return {"exec_s": tm.exec_s, "total_s": tm.total_s, "copy_s": tm.copy_s, "pipelined_s": tm.pipelined_s}

    def alloc_probed(self, planes, qp, candidates=6, *, tc_table=None, beta_table=None):
        """hevcdbk_device_malloc_probed: a destination pool for launches like `planes` (a DevicePlanes; its dst is ignored), the
        fastest of `candidates` allocations by the filter's own time on each.  Returns (DeviceBuffer, best_ms, worst_ms)."""
        t, _k = _tables(tc_table, beta_table)
        p, best, worst = C.c_void_p(), C.c_float(), C.c_float()
        _chk(_lib.lib().hevcdbk_device_malloc_probed(self.handle, C.byref(planes), int(qp), None if t is None else C.byref(t),
                                                     int(candidates), C.byref(p), C.byref(best), C.byref(worst)), self.handle)
        nbytes = planes.frame_stride * (planes.n_frames - 1) + planes.pitch * planes.plane_h
        return DeviceBuffer.adopt(self, p.value, nbytes), best.value, worst.value

    # -- host side of filter_frame on large pageable frames --------------------------------------
    def set_host_threads(self, n):
        """Threads that copy between the caller's pageable planes and the page-locked ring during a large-frame
        filter_frame call, the calling thread included (0 = the default, 4)."""
        _chk(_lib.lib().hevcdbk_set_host_threads(self.handle, int(n)), self.handle)

    def host_threads(self):
        return int(_lib.lib().hevcdbk_get_host_threads(self.handle))

    def host_register(self, arr):
        """Page-locks the numpy array's memory in place (hevcdbk_host_register): planes inside it are DMA'd where they
        lie by the host-frame operators.  Unregister before the array is freed."""
        _chk(_lib.lib().hevcdbk_host_register(self.handle, arr.ctypes.data, arr.nbytes), self.handle)

    def host_unregister(self, arr):
        _chk(_lib.lib().hevcdbk_host_unregister(self.handle, arr.ctypes.data), self.handle)

    def last_frame_trace(self):
        """Per-strip record of the last large-frame filter_frame call (hevcdbk_last_frame_trace), a list of dicts."""
        n = C.c_uint(0)
        _chk(_lib.lib().hevcdbk_last_frame_trace(self.handle, None, 0, C.byref(n)), self.handle)
        if n.value == 0:
            return []
        buf = (_lib.StripTrace * n.value)()
        _chk(_lib.lib().hevcdbk_last_frame_trace(self.handle, buf, n.value, C.byref(n)), self.handle)
        return [{f: getattr(t, f) for f, _ in _lib.StripTrace._fields_} for t in buf]

    # -- streaming operator on a sequence of host frames -----------------------------------------
    def pinned_array(self, shape, dtype=np.uint8):
        """numpy array in page-locked host memory (hevcdbk_host_malloc_pinned): planes allocated this way are
        DMA'd in place by filter_sequence / filter_frame, with no staging copy.  Free with free_pinned()."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        _chk(_lib.lib().hevcdbk_host_malloc_pinned(self.handle, n, C.byref(p)), self.handle)
        buf = (C.c_uint8 * n).from_address(p.value)
        arr = np.frombuffer(buf, dtype=dtype).reshape(shape)
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[arr.ctypes.data] = p.value
        return arr

    def free_pinned(self, arr):
        p = getattr(self, "_pinned", {}).pop(arr.ctypes.data, None)
        if p is not None:
            _chk(_lib.lib().hevcdbk_host_free_pinned(self.handle, p), self.handle)

    def filter_sequence(self, frames, *, qp, bit_depth=8, vert_bs=None, hor_bs=None):
        """frames: list of (y,) or (y, u, v) tuples of writable 2-D numpy planes of one geometry; filtered in
        place through the 3-deep H2D || kernel || D2H pipeline.  Returns the wall time of the sequence (s)."""
        arr = (_lib.Frame * len(frames))()
        for i, pl in enumerate(frames):
            _frame(arr[i], pl, bit_depth)
        keep = []
        bs = _bs(keep, vert=vert_bs, hor=hor_bs) if vert_bs is not None else None
        q = _lib.Qp()
        q.qp, q.ctu_log2 = int(qp), 6
        tm = _lib.Timing()
        rc = _lib.lib().hevc_deblocking_filter_sequence(self.handle, arr, len(frames), None if bs is None else C.byref(bs),
                                                        C.byref(q), None, C.byref(tm))
        _chk(rc, self.handle)
        return tm.pipelined_s

    def filter_yuv_file(self, in_name, out_name, width, height, qp, *, vert_bs=None, hor_bs=None,
                        tc_table=None, beta_table=None):
        """Multi-frame planar 8-bit 4:2:0 file -> file (hevcdbk_filter_yuv_file): every frame gets what the
        reference's ReadYuvFrame -> [SetBoundaryStrenght] -> DeblockingFilter -> Save gives a one-frame file
        (cpu.h:35-132, 995-1018).  Returns (n_frames, wall seconds including file I/O)."""
        keep = []
        bs = _bs(keep, vert=vert_bs, hor=hor_bs) if vert_bs is not None else None
        t, k2 = _tables(tc_table, beta_table)
        tm = _lib.Timing()
        n = C.c_uint(0)
        rc = _lib.lib().hevcdbk_filter_yuv_file(self.handle, os.fsencode(in_name), os.fsencode(out_name), width, height,
                                                int(qp), None if bs is None else C.byref(bs),
                                                None if t is None else C.byref(t), C.byref(n), C.byref(tm))
        _chk(rc, self.handle)
        return n.value, tm.pipelined_s

    # -- device-resident operator ---------------------------------------------------------------
    def filter_device(self, planes, qp, *, tc_table=None, beta_table=None, variant=KERNEL_AUTO):
        t, _k = _tables(tc_table, beta_table)
        rc = _lib.lib().hevc_deblocking_filter_device(self.handle, C.byref(planes), int(qp),
                                                      None if t is None else C.byref(t), variant, None)
        _chk(rc, self.handle)

    # -- spec-exact mode (H.265 clause 8.7.2) ------------------------------------------------------
    def filter_frame_h265(self, y, u=None, v=None, *, qp, bit_depth=8, units=None, vert_bs4=None, hor_bs4=None,
                          qp_map=None, unit_log2=3, tc_offset_div2=0, beta_offset_div2=0, cb_qp_offset=0, cr_qp_offset=0,
                          chroma_format="420"):
        """hevc_deblocking_filter_h265 on host planes, in place.  Either `units` = (flags, mv0, mv1, ref0, ref1) per 4x4
        luma unit (bS derived on the GPU, 8.7.2.4) or the 4-sample-granular luma bS arrays.  chroma_format '400' / '420' /
        '422' / '444': u, v are (H / SubHeightC) x (W / SubWidthC) planes (none for '400'; '420' = the 4:2:0 entry)."""
        cf = _lib.chroma_format_idc(chroma_format)
        fr = _frame(_lib.Frame(), [y] + ([u, v] if u is not None else []), bit_depth)
        keep, un, bs = [], None, None
        if units is not None:
            un = _lib.H265Units()
            for nm, arr, dt in zip(("flags", "mv0", "mv1", "ref0", "ref1"), units, (np.uint16, np.int16, np.int16, np.int32, np.int32)):
                a = np.ascontiguousarray(arr, dt)
                keep.append(a)
                setattr(un, nm, a.ctypes.data)
        if vert_bs4 is not None:
            bs = _bs(keep, vert=vert_bs4, hor=hor_bs4)
        q = _lib.Qp()
        q.qp, q.ctu_log2 = int(qp), unit_log2
        if qp_map is not None:
            m = np.ascontiguousarray(qp_map, np.uint8)
            keep.append(m)
            q.map, q.map_stride = m.ctypes.data, m.shape[1]
        prm = _lib.H265Params(tc_offset_div2, beta_offset_div2, cb_qp_offset, cr_qp_offset)
        tm = _lib.Timing()
        if cf == _lib.CHROMA_420:
            rc = _lib.lib().hevc_deblocking_filter_h265(self.handle, C.byref(fr), None if un is None else C.byref(un),
                                                        None if bs is None else C.byref(bs), C.byref(q), C.byref(prm), C.byref(tm))
        else:
            rc = _lib.lib().hevcdbk_h265_filter_frame_cf(self.handle, C.byref(fr), cf, None if un is None else C.byref(un),
                                                           None if bs is None else C.byref(bs), C.byref(q), C.byref(prm), C.byref(tm))
        _chk(rc, self.handle)
        return {"exec_s": tm.exec_s, "total_s": tm.total_s, "copy_s": tm.copy_s, "pipelined_s": tm.pipelined_s}

    def filter_device_h265(self, planes, qp, *, c_idx=0, tc_offset_div2=0, beta_offset_div2=0, cb_qp_offset=0, cr_qp_offset=0,
                           variant=KERNEL_AUTO, chroma_format="420", slice_offsets=None, g4=False, semi_planar=False):
        """hevc_deblocking_filter_h265_device[_cf]: a plane of a picture in chroma_format '400' / '420' / '422' / '444'.
        semi_planar=True: hevcdbk_h265_filter_device_sp -- `planes` is one plane of interleaved Cb / Cr pairs of a 4:2:0 picture
        (plane_w x plane_h per component, multiples of 4), both components in one launch: c_idx is not used, cb_qp_offset applies
        to the even samples and cr_qp_offset to the odd ones.
        slice_offsets: a _lib.SliceOffsets (per-CTB slice_beta_offset_div2 / slice_tc_offset_div2, hevcdbk_h265_filter_device_sl);
        with it tc_offset_div2 / beta_offset_div2 are not used.  g4=True: hevcdbk_h265_filter_device_g4, which also takes a chroma
        plane sized in multiples of 4 (960x540 of a 1920x1080 picture); without it such a plane is refused as ever."""
        cf = _lib.chroma_format_idc(chroma_format)
        prm = _lib.H265Params(tc_offset_div2, beta_offset_div2, cb_qp_offset, cr_qp_offset)
        if semi_planar:
            if cf != _lib.CHROMA_420:
                raise ValueError("semi_planar is 4:2:0 only")
            rc = _lib.lib().hevcdbk_h265_filter_device_sp(self.handle, C.byref(planes), int(qp), C.byref(prm), variant,
                                                          None if slice_offsets is None else C.byref(slice_offsets), None)
        elif g4:
            rc = _lib.lib().hevcdbk_h265_filter_device_g4(self.handle, C.byref(planes), c_idx, cf, int(qp), C.byref(prm), variant,
                                                          None if slice_offsets is None else C.byref(slice_offsets), None)
        elif slice_offsets is not None:
            rc = _lib.lib().hevcdbk_h265_filter_device_sl(self.handle, C.byref(planes), c_idx, cf, int(qp), C.byref(prm), variant,
                                                          C.byref(slice_offsets), None)
        elif cf == _lib.CHROMA_420:
            rc = _lib.lib().hevc_deblocking_filter_h265_device(self.handle, C.byref(planes), c_idx, int(qp), C.byref(prm), variant, None)
        else:
            rc = _lib.lib().hevcdbk_h265_filter_device_cf(self.handle, C.byref(planes), c_idx, cf, int(qp), C.byref(prm),
                                                                  variant, None)
        _chk(rc, self.handle)

    def derive_bs_h265(self, units, w, h, *, chroma=True, chroma_format="420", g4=False):
        """8.7.2.4 on the GPU from host arrays; returns (vert, hor[, chroma_vert, chroma_hor]) as host arrays; the chroma
        arrays in the geometry of chroma_format's chroma plane (none for '400').  g4=True: hevcdbk_h265_derive_bs_device_g4, whose
        chroma plane may be sized in multiples of 4 (w x h stay multiples of 8)."""
        cf = _lib.chroma_format_idc(chroma_format)
        chroma = chroma and cf != _lib.CHROMA_400
        arrs = [np.ascontiguousarray(a, dt) for a, dt in zip(units, (np.uint16, np.int16, np.int16, np.int32, np.int32))]
        bufs = [self.alloc(a.nbytes) for a in arrs]
        for b, a in zip(bufs, arrs):
            b.upload(a)
        L = _lib.lib()
        sizes = [L.hevcdbk_h265_num_vert_bs(w, h), L.hevcdbk_h265_num_hor_bs(w, h)]
        if chroma:
            sx, sy = _lib.CHROMA_SUB[cf]
            sizes += [L.hevcdbk_h265_num_vert_bs(w // sx, h // sy), L.hevcdbk_h265_num_hor_bs(w // sx, h // sy)]
        outs = [self.alloc(max(n, 1)) for n in sizes]
        un = _lib.H265Units(*[b.ptr for b in bufs])
        if g4:
            rc = L.hevcdbk_h265_derive_bs_device_g4(self.handle, C.byref(un), w, h, cf, outs[0].ptr, outs[1].ptr,
                                                    outs[2].ptr if chroma else None, outs[3].ptr if chroma else None, None)
        elif cf == _lib.CHROMA_420:
            rc = L.hevcdbk_h265_derive_bs_device(self.handle, C.byref(un), w, h, outs[0].ptr, outs[1].ptr,
                                                 outs[2].ptr if chroma else None, outs[3].ptr if chroma else None, None)
        else:
            rc = L.hevcdbk_h265_derive_bs_device_cf(self.handle, C.byref(un), w, h, cf, outs[0].ptr, outs[1].ptr,
                                                    outs[2].ptr if chroma else None, outs[3].ptr if chroma else None, None)
        _chk(rc, self.handle)
        self.synchronize()
        res = [o.download(n) for o, n in zip(outs, sizes)]
        for b in bufs + outs:
            b.free()
        return res

    def derive_sao_borders(self, slice_idx, slice_across, tile_idx=None, *, tiles_across=True):
        """hevcdbk_h265_sao_borders_device from host arrays of one entry per CTB (slice_idx: index of the CTB's slice in decoding
        order; slice_across: that slice's slice_loop_filter_across_slices_enabled_flag; tile_idx: None = one tile;
        tiles_across = loop_filter_across_tiles_enabled_flag); returns the bytes (CTB rows, CTB columns) as a host array --
        upload them and hand them on as borders=SaoBorders(ptr, stride, frame_stride)."""
        si = np.ascontiguousarray(slice_idx, np.uint16)
        sa = np.ascontiguousarray(slice_across, np.uint8)
        if si.ndim != 2 or sa.shape != si.shape:
            raise ValueError("slice_idx and slice_across must be 2-D arrays of one shape")
        arrs = [si, sa]
        if tile_idx is not None:
            arrs.append(np.ascontiguousarray(tile_idx, np.uint16))
            if arrs[2].shape != si.shape:
                raise ValueError("tile_idx must have the shape of slice_idx")
        rows, cols = si.shape
        bufs = [self.alloc(max(a.nbytes, 1)) for a in arrs]
        for b, a in zip(bufs, arrs):
            b.upload(a)
        out = self.alloc(max(rows * cols, 1))
        rc = _lib.lib().hevcdbk_h265_sao_borders_device(self.handle, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr if tile_idx is not None else None,
                                                        int(bool(tiles_across)), cols, rows, cols, out.ptr, cols, None)
        _chk(rc, self.handle)
        self.synchronize()
        res = out.download(rows * cols).reshape(rows, cols)
        for b in bufs + [out]:
            b.free()
        return res

    def derive_slice_offsets(self, slice_idx, slice_table):
        """hevcdbk_h265_slice_offsets_device from host arrays: slice_idx (CTB rows, CTB columns) = index of the CTB's slice in
        decoding order, slice_table (n_slices, 2) = (slice_beta_offset_div2, slice_tc_offset_div2) per slice; returns the pairs
        (CTB rows, CTB columns, 2) as a host int8 array -- upload them and hand them on as
        slice_offsets=SliceOffsets(ptr, stride, frame_stride, ctb_log2)."""
        si = np.ascontiguousarray(slice_idx, np.uint16)
        tb = np.ascontiguousarray(slice_table, np.int8)
        if si.ndim != 2 or tb.ndim != 2 or tb.shape[1] != 2:
            raise ValueError("slice_idx must be 2-D and slice_table (n_slices, 2)")
        rows, cols = si.shape
        bufs = [self.alloc(max(si.nbytes, 1)), self.alloc(max(tb.nbytes, 1))]
        bufs[0].upload(si)
        if tb.nbytes:
            bufs[1].upload(tb)
        out = self.alloc(max(2 * rows * cols, 1))
        rc = _lib.lib().hevcdbk_h265_slice_offsets_device(self.handle, bufs[0].ptr, cols, bufs[1].ptr, tb.shape[0], cols, rows, out.ptr,
                                                          cols, None)
        _chk(rc, self.handle)
        self.synchronize()
        res = out.download(2 * rows * cols).view(np.int8).reshape(rows, cols, 2)
        for b in bufs + [out]:
            b.free()
        return res

    def sao_device(self, planes, params_ptr, params_stride, ctb_log2, *, params_frame_stride=0, keep_ptr=None, keep_stride=0,
                   keep_frame_stride=0, chroma_format="420", ctb_log2_h=None, borders=None, g4=False, semi_planar=False,
                   params_cr_ptr=None):
        """hevc_sao_filter_device[_cf]: H.265 8.7.3 on planes in HBM, src -> dst.  ctb_log2 = log2 of this plane's CTB width;
        its height follows from chroma_format (a 4:2:2 chroma plane, planes.is_chroma: twice the width) unless ctb_log2_h says.
        borders: a _lib.SaoBorders (slice / tile boundaries not to be looked across, 8.7.3.2: hevcdbk_sao_filter_device_nox).
        g4=True: hevcdbk_sao_filter_device_g4, which also takes a plane sized in multiples of 4 (keep map and CTB grid by ceiling).
        semi_planar=True: hevcdbk_sao_filter_device_sp -- `planes` is one plane of interleaved Cb / Cr pairs of a 4:2:0 picture
        (plane_w x plane_h per component, multiples of 4); params_ptr speaks for the even samples, params_cr_ptr (needed) for the odd
        ones, with one stride and one frame stride; the keep map and borders serve both components; square CTBs of ctb_log2 3..5."""
        cf = _lib.chroma_format_idc(chroma_format)
        if semi_planar:
            if cf != _lib.CHROMA_420:
                raise ValueError("semi_planar is 4:2:0 only")
            if params_cr_ptr is None:
                raise ValueError("semi_planar needs params_cr_ptr: the parameters of the odd samples")
            _chk(_lib.lib().hevcdbk_sao_filter_device_sp(self.handle, C.byref(planes), params_ptr, params_cr_ptr, params_stride,
                                                         params_frame_stride, ctb_log2, keep_ptr, keep_stride, keep_frame_stride,
                                                         None if borders is None else C.byref(borders), None), self.handle)
            return
        if params_cr_ptr is not None:
            raise ValueError("params_cr_ptr belongs to semi_planar=True")
        lh = _ctb_log2_h(ctb_log2, ctb_log2_h, cf, planes.is_chroma)
        if g4:
            _chk(_lib.lib().hevcdbk_sao_filter_device_g4(self.handle, C.byref(planes), params_ptr, params_stride, params_frame_stride,
                                                         ctb_log2, lh, keep_ptr, keep_stride, keep_frame_stride,
                                                         None if borders is None else C.byref(borders), None), self.handle)
            return
        if borders is not None:
            _chk(_lib.lib().hevcdbk_sao_filter_device_nox(self.handle, C.byref(planes), params_ptr, params_stride, params_frame_stride,
                                                          ctb_log2, lh, keep_ptr, keep_stride, keep_frame_stride, C.byref(borders), None),
                 self.handle)
            return
        if cf == _lib.CHROMA_420 and lh == ctb_log2:
            rc = _lib.lib().hevc_sao_filter_device(self.handle, C.byref(planes), params_ptr, params_stride, params_frame_stride,
                                                   ctb_log2, keep_ptr, keep_stride, keep_frame_stride, None)
        else:
            rc = _lib.lib().hevcdbk_sao_filter_device_cf(self.handle, C.byref(planes), params_ptr, params_stride, params_frame_stride,
                                                      ctb_log2, lh, keep_ptr, keep_stride, keep_frame_stride, None)
        _chk(rc, self.handle)

    def sao_stats_device(self, planes, org_ptr, ctb_log2, *, org_pitch=None, org_frame_stride=None, ctb_log2_h=None, chroma_format="420",
                         keep_ptr=None, keep_stride=0, keep_frame_stride=0, borders=None, out_ptr, out_stride, out_frame_stride=0,
                         stream=None, semi_planar=False, out_cr_ptr=None):
        """hevcdbk_sao_stats_device: per-CTB SAO statistics of the deblocked plane planes.src against the original at org_ptr (device
        memory, the same geometry and container; pitch and frame stride default to the plane's).  out_ptr: device memory for one
        _lib.SaoStats (numpy: _lib.SAO_STATS_DTYPE) per CTB, out_stride entries per CTB row, out_frame_stride entries between frames;
        every entry of the grid is written, nothing needs clearing.  ctb_log2 = log2 of this plane's CTB width; the height follows
        from chroma_format as for sao_device unless ctb_log2_h says.  keep_ptr, borders: as for sao_device(g4=True).
        semi_planar=True: hevcdbk_sao_stats_device_sp -- `planes` and the original are planes of interleaved Cb / Cr pairs of a 4:2:0
        picture (plane_w x plane_h per component, multiples of 4); out_ptr takes Cb's statistics (the even samples), out_cr_ptr
        (needed) Cr's, with one stride and one frame stride; the keep map and borders serve both components; square CTBs of
        ctb_log2 3..5."""
        cf = _lib.chroma_format_idc(chroma_format)
        if semi_planar:
            if cf != _lib.CHROMA_420:
                raise ValueError("semi_planar is 4:2:0 only")
            if out_cr_ptr is None:
                raise ValueError("semi_planar needs out_cr_ptr: the statistics of the odd samples")
            if ctb_log2_h is not None and ctb_log2_h != ctb_log2:
                raise ValueError("semi_planar takes square CTBs")
            _chk(_lib.lib().hevcdbk_sao_stats_device_sp(self.handle, C.byref(planes), org_ptr, planes.pitch if org_pitch is None else org_pitch,
                                                        planes.frame_stride if org_frame_stride is None else org_frame_stride, ctb_log2,
                                                        keep_ptr, keep_stride, keep_frame_stride, None if borders is None else C.byref(borders),
                                                        out_ptr, out_cr_ptr, out_stride, out_frame_stride, stream), self.handle)
            return
        if out_cr_ptr is not None:
            raise ValueError("out_cr_ptr belongs to semi_planar=True")
        lh = _ctb_log2_h(ctb_log2, ctb_log2_h, cf, planes.is_chroma)
        _chk(_lib.lib().hevcdbk_sao_stats_device(self.handle, C.byref(planes), org_ptr, planes.pitch if org_pitch is None else org_pitch,
                                                 planes.frame_stride if org_frame_stride is None else org_frame_stride, ctb_log2, lh,
                                                 keep_ptr, keep_stride, keep_frame_stride, None if borders is None else C.byref(borders),
                                                 out_ptr, out_stride, out_frame_stride, stream), self.handle)

    def sao_pick_device(self, stats_ptr, stats_stride, ctbs_x, ctbs_y, bit_depth, lambda_q8, *, out_ptr, out_stride, n_frames=1,
                        stats_frame_stride=0, out_frame_stride=0, stats_b_ptr=None, out_b_ptr=None, delta_d_ptr=None, stream=None,
                        log2_offset_scale=None):
        """hevcdbk_sao_pick_device: one hevcdbk_sao_ctb per CTB (out_ptr, out_stride entries per row) from the statistics at stats_ptr,
        by the rule of include/hevc_deblock.h with lambda_q8 = lambda * 256.  stats_b_ptr / out_b_ptr: Cr beside Cb -- one type and
        one edge class for both.  delta_d_ptr: ctbs_x * ctbs_y * n_frames int64, the predicted change of the SSE per CTB.
        log2_offset_scale: an integer, 0 included, calls hevcdbk_sao_pick_device_os with it (log2_sao_offset_scale: offsets in units
        of 2^k, k at most Max(0, bit_depth - 10) and at most 2); None calls hevcdbk_sao_pick_device."""
        if log2_offset_scale is not None:
            _chk(_lib.lib().hevcdbk_sao_pick_device_os(self.handle, stats_ptr, stats_b_ptr, stats_stride, stats_frame_stride, ctbs_x, ctbs_y,
                                                       n_frames, bit_depth, int(log2_offset_scale), lambda_q8, out_ptr, out_b_ptr, out_stride,
                                                       out_frame_stride, delta_d_ptr, stream), self.handle)
            return
        _chk(_lib.lib().hevcdbk_sao_pick_device(self.handle, stats_ptr, stats_b_ptr, stats_stride, stats_frame_stride, ctbs_x, ctbs_y,
                                                n_frames, bit_depth, lambda_q8, out_ptr, out_b_ptr, out_stride, out_frame_stride,
                                                delta_d_ptr, stream), self.handle)

    def sao_decide_device(self, stats_ptr, stats_stride, ctbs_x, ctbs_y, bit_depth, lambda_q8, *, out_ptr, out_stride, decision_ptr,
                          decision_stride, n_frames=1, stats_frame_stride=0, out_frame_stride=0, decision_frame_stride=0, stats_cb_ptr=None,
                          stats_cr_ptr=None, out_cb_ptr=None, out_cr_ptr=None, bit_depth_chroma=None, lambda_q8_chroma=None,
                          slice_idx_ptr=None, tile_idx_ptr=None, idx_stride=0, idx_frame_stride=0, stream=None, log2_offset_scale=None,
                          log2_offset_scale_chroma=None, slice_flags_ptr=None, n_slices=None, slice_flags_frame_stride=0):
        """hevcdbk_sao_decide_device: per CTB own parameters, merge left or merge up (H.265 7.3.8.3) over Y, Cb and Cr at once, by the
        rule of include/hevc_deblock.h.  stats_ptr: luma's statistics; stats_cb_ptr / stats_cr_ptr (both or neither): the chroma
        components' on the same grid, with the same strides.  out_ptr / out_cb_ptr / out_cr_ptr: the final hevcdbk_sao_ctb per CTB, as
        sao_device reads them.  decision_ptr: one _lib.SaoDecision (numpy: _lib.SAO_DECISION_DTYPE) per CTB.  bit_depth_chroma and
        lambda_q8_chroma default to luma's.  slice_idx_ptr, tile_idx_ptr: uint16 per CTB, as sao_borders_device takes them; a CTB
        merges only with a neighbour of its own slice and tile.  log2_offset_scale: an integer, 0 included, calls
        hevcdbk_sao_decide_device_os with it for luma and log2_offset_scale_chroma (defaults to luma's) for Cb and Cr; None calls
        hevcdbk_sao_decide_device.  slice_flags_ptr (with n_slices): one byte per slice on the device, bit 0 slice_sao_luma_flag, bit 1
        slice_sao_chroma_flag -- calls hevcdbk_sao_decide_device_sf, with a log2_offset_scale of 0 where none is given."""
        if log2_offset_scale is None and log2_offset_scale_chroma is not None:
            raise ValueError("log2_offset_scale_chroma needs log2_offset_scale")
        if slice_flags_ptr is not None:
            if n_slices is None:
                raise ValueError("slice_flags_ptr needs n_slices")
            kl = 0 if log2_offset_scale is None else int(log2_offset_scale)
            kc = kl if log2_offset_scale_chroma is None else int(log2_offset_scale_chroma)
            _chk(_lib.lib().hevcdbk_sao_decide_device_sf(self.handle, stats_ptr, stats_cb_ptr, stats_cr_ptr, stats_stride, stats_frame_stride,
                                                         ctbs_x, ctbs_y, n_frames, bit_depth, bit_depth if bit_depth_chroma is None else bit_depth_chroma,
                                                         kl, kc, lambda_q8, lambda_q8 if lambda_q8_chroma is None else lambda_q8_chroma,
                                                         slice_idx_ptr, tile_idx_ptr, idx_stride, idx_frame_stride, out_ptr, out_cb_ptr, out_cr_ptr,
                                                         out_stride, out_frame_stride, decision_ptr, decision_stride, decision_frame_stride,
                                                         slice_flags_ptr, n_slices, slice_flags_frame_stride, stream), self.handle)
            return
        if log2_offset_scale is not None:
            kc = log2_offset_scale if log2_offset_scale_chroma is None else log2_offset_scale_chroma
            _chk(_lib.lib().hevcdbk_sao_decide_device_os(self.handle, stats_ptr, stats_cb_ptr, stats_cr_ptr, stats_stride, stats_frame_stride,
                                                         ctbs_x, ctbs_y, n_frames, bit_depth, bit_depth if bit_depth_chroma is None else bit_depth_chroma,
                                                         int(log2_offset_scale), int(kc), lambda_q8,
                                                         lambda_q8 if lambda_q8_chroma is None else lambda_q8_chroma, slice_idx_ptr, tile_idx_ptr,
                                                         idx_stride, idx_frame_stride, out_ptr, out_cb_ptr, out_cr_ptr, out_stride,
                                                         out_frame_stride, decision_ptr, decision_stride, decision_frame_stride, stream), self.handle)
            return
        _chk(_lib.lib().hevcdbk_sao_decide_device(self.handle, stats_ptr, stats_cb_ptr, stats_cr_ptr, stats_stride, stats_frame_stride, ctbs_x,
                                                  ctbs_y, n_frames, bit_depth, bit_depth if bit_depth_chroma is None else bit_depth_chroma,
                                                  lambda_q8, lambda_q8 if lambda_q8_chroma is None else lambda_q8_chroma, slice_idx_ptr,
                                                  tile_idx_ptr, idx_stride, idx_frame_stride, out_ptr, out_cb_ptr, out_cr_ptr, out_stride,
                                                  out_frame_stride, decision_ptr, decision_stride, decision_frame_stride, stream), self.handle)

    @staticmethod
    def sao_slice_flags_workspace(ctbs_x, ctbs_y, n_frames=1, n_slices=1):
        """hevcdbk_sao_slice_flags_workspace: the bytes of device memory sao_slice_flags_device needs as its workspace"""
        return int(_lib.lib().hevcdbk_sao_slice_flags_workspace(ctbs_x, ctbs_y, n_frames, n_slices))

    def sao_slice_flags_device(self, stats_ptr, stats_stride, ctbs_x, ctbs_y, bit_depth, lambda_q8, *, out_ptr, out_stride, decision_ptr,
                               decision_stride, n_slices, slice_flags_ptr, workspace_ptr, workspace_bytes, slice_flags_frame_stride=0,
                               slice_record_ptr=None, slice_record_frame_stride=0, n_frames=1, stats_frame_stride=0, out_frame_stride=0,
                               decision_frame_stride=0, stats_cb_ptr=None, stats_cr_ptr=None, out_cb_ptr=None, out_cr_ptr=None,
                               bit_depth_chroma=None, lambda_q8_chroma=None, slice_idx_ptr=None, tile_idx_ptr=None, idx_stride=0,
                               idx_frame_stride=0, stream=None, log2_offset_scale=0, log2_offset_scale_chroma=None):
        """hevcdbk_sao_slice_flags_device: slice_sao_luma_flag / slice_sao_chroma_flag chosen per slice (bit 0 / bit 1 of one byte per
        slice and frame at slice_flags_ptr) and the decision of sao_decide_device under them, by the rule of include/hevc_deblock.h.
        The operands of sao_decide_device; slice_record_ptr: one _lib.SaoSliceRecord (numpy: _lib.SAO_SLICE_RECORD_DTYPE) per slice and
        frame, or None; workspace_ptr: device memory, 16-byte aligned, of at least sao_slice_flags_workspace(...) bytes."""
        kc = log2_offset_scale if log2_offset_scale_chroma is None else log2_offset_scale_chroma
        _chk(_lib.lib().hevcdbk_sao_slice_flags_device(self.handle, stats_ptr, stats_cb_ptr, stats_cr_ptr, stats_stride, stats_frame_stride, ctbs_x,
                                                       ctbs_y, n_frames, bit_depth, bit_depth if bit_depth_chroma is None else bit_depth_chroma,
                                                       int(log2_offset_scale), int(kc), lambda_q8,
                                                       lambda_q8 if lambda_q8_chroma is None else lambda_q8_chroma, slice_idx_ptr, tile_idx_ptr,
                                                       idx_stride, idx_frame_stride, out_ptr, out_cb_ptr, out_cr_ptr, out_stride, out_frame_stride,
                                                       decision_ptr, decision_stride, decision_frame_stride, n_slices, slice_flags_ptr,
                                                       slice_flags_frame_stride, slice_record_ptr, slice_record_frame_stride, workspace_ptr,
                                                       workspace_bytes, stream), self.handle)

    def sse_device(self, planes, org_ptr, ctb_log2, *, org_pitch=None, org_frame_stride=None, ctb_log2_h=None, chroma_format="420",
                   out_ptr, out_stride, out_frame_stride=0, stream=None, semi_planar=False, out_cr_ptr=None):
        """hevcdbk_sse_device: the sum of squared errors of the plane planes.src against the original at org_ptr (device memory, the
        same geometry and container; pitch and frame stride default to the plane's), exact, one uint64 per CTB at out_ptr (device
        memory, 8-byte aligned), out_stride entries per CTB row, out_frame_stride entries between frames.  Every sample counts: no keep
        map, no borders.  ctb_log2 / ctb_log2_h / chroma_format as for sao_stats_device.  semi_planar=True: hevcdbk_sse_device_sp --
        planes of interleaved Cb / Cr pairs (plane_w x plane_h per component); out_ptr takes Cb's sums (the even samples), out_cr_ptr
        (needed) Cr's; square CTBs of ctb_log2 3..5."""
        cf = _lib.chroma_format_idc(chroma_format)
        pitch = planes.pitch if org_pitch is None else org_pitch
        fstride = planes.frame_stride if org_frame_stride is None else org_frame_stride
        if semi_planar:
            if cf != _lib.CHROMA_420:
                raise ValueError("semi_planar is 4:2:0 only")
            if out_cr_ptr is None:
                raise ValueError("semi_planar needs out_cr_ptr: the sums of the odd samples")
            if ctb_log2_h is not None and ctb_log2_h != ctb_log2:
                raise ValueError("semi_planar takes square CTBs")
            _chk(_lib.lib().hevcdbk_sse_device_sp(self.handle, C.byref(planes), org_ptr, pitch, fstride, ctb_log2, out_ptr, out_cr_ptr, out_stride,
                                                  out_frame_stride, stream), self.handle)
            return
        if out_cr_ptr is not None:
            raise ValueError("out_cr_ptr belongs to semi_planar=True")
        lh = _ctb_log2_h(ctb_log2, ctb_log2_h, cf, planes.is_chroma)
        _chk(_lib.lib().hevcdbk_sse_device(self.handle, C.byref(planes), org_ptr, pitch, fstride, ctb_log2, lh, out_ptr, out_stride,
                                           out_frame_stride, stream), self.handle)

    def sse_totals_device(self, sse_ptr, sse_stride, ctbs_x, ctbs_y, *, n_frames=1, sse_frame_stride=0, slice_idx_ptr=None, idx_stride=0,
                          idx_frame_stride=0, n_slices=1, slice_total_ptr=None, slice_total_frame_stride=0, frame_total_ptr=None, stream=None):
        """hevcdbk_sse_totals_device: the sums of sse_device's array (or of any uint64 per CTB) per slice and per frame, modulo 2^64.
        slice_idx_ptr: uint16 per CTB as sao_decide_device takes it, None = every CTB in slice 0.  slice_total_ptr: n_slices uint64 per
        frame, slice_total_frame_stride entries apart; frame_total_ptr: one uint64 per frame, CTBs with an index >= n_slices included.
        Either may be None, not both.  At most 600 slices."""
        _chk(_lib.lib().hevcdbk_sse_totals_device(self.handle, sse_ptr, sse_stride, sse_frame_stride, ctbs_x, ctbs_y, n_frames, slice_idx_ptr,
                                                  idx_stride, idx_frame_stride, n_slices, slice_total_ptr, slice_total_frame_stride,
                                                  frame_total_ptr, stream), self.handle)

    def deblock_sao_device(self, planes, qp, params_ptr, params_stride, ctb_log2, *, params_frame_stride=0, keep_ptr=None,
                           keep_stride=0, keep_frame_stride=0, tc_table=None, beta_table=None, fused=_lib.FUSED_AUTO, stream=None):
        """hevc_deblock_sao_device: reference-exact deblocking followed by SAO, src -> dst, one kernel where it applies.
        stream: a hipStream_t handle of the caller (int), None = the context's compute stream."""
        t, _k = _tables(tc_table, beta_table)
        _chk(_lib.lib().hevc_deblock_sao_device(self.handle, C.byref(planes), int(qp), None if t is None else C.byref(t), params_ptr,
                                                params_stride, params_frame_stride, ctb_log2, keep_ptr, keep_stride, keep_frame_stride,
                                                fused, stream), self.handle)

    def deblock_sao_h265_device(self, planes, qp, params_ptr, params_stride, ctb_log2, *, c_idx=0, tc_offset_div2=0,
                                beta_offset_div2=0, cb_qp_offset=0, cr_qp_offset=0, params_frame_stride=0, keep_ptr=None,
                                keep_stride=0, keep_frame_stride=0, fused=_lib.FUSED_AUTO, chroma_format="420", ctb_log2_h=None,
                                borders=None, slice_offsets=None, g4=False, semi_planar=False, params_cr_ptr=None, one_kernel=False):
        """hevc_deblock_sao_h265_device[_cf]: spec-exact deblocking (8.7.2) followed by SAO (8.7.3), src -> dst; chroma_format,
        ctb_log2 / ctb_log2_h and borders (hevcdbk_h265_deblock_sao_device_nox) as for sao_device; slice_offsets as for
        filter_device_h265 (hevcdbk_h265_deblock_sao_device_sl); g4=True: hevcdbk_h265_deblock_sao_device_g4 (a chroma plane
        sized in multiples of 4).  semi_planar=True: hevcdbk_h265_deblock_sao_device_sp -- a plane of interleaved Cb / Cr pairs as
        for filter_device_h265 and sao_device (c_idx is not used; params_cr_ptr is needed); fused=FUSED_ON is refused.  one_kernel=True
        (with semi_planar=True only): hevcdbk_h265_deblock_sao_device_sp_fused -- the same result from ONE kernel where its guards allow
        (fused=FUSED_AUTO), or nothing else (FUSED_ON); FUSED_OFF is the two launches."""
        if one_kernel and not semi_planar:
            raise ValueError("one_kernel belongs to semi_planar=True")
        cf = _lib.chroma_format_idc(chroma_format)
        prm = _lib.H265Params(tc_offset_div2, beta_offset_div2, cb_qp_offset, cr_qp_offset)
        if semi_planar:
            if cf != _lib.CHROMA_420:
                raise ValueError("semi_planar is 4:2:0 only")
            if params_cr_ptr is None:
                raise ValueError("semi_planar needs params_cr_ptr: the parameters of the odd samples")
            entry = _lib.lib().hevcdbk_h265_deblock_sao_device_sp_fused if one_kernel else _lib.lib().hevcdbk_h265_deblock_sao_device_sp
            _chk(entry(self.handle, C.byref(planes), int(qp), C.byref(prm), params_ptr, params_cr_ptr, params_stride, params_frame_stride,
                       ctb_log2, keep_ptr, keep_stride, keep_frame_stride, fused, None if borders is None else C.byref(borders),
                       None if slice_offsets is None else C.byref(slice_offsets), None), self.handle)
            return
        if params_cr_ptr is not None:
            raise ValueError("params_cr_ptr belongs to semi_planar=True")
        lh = _ctb_log2_h(ctb_log2, ctb_log2_h, cf, c_idx != 0)
        if g4:
            _chk(_lib.lib().hevcdbk_h265_deblock_sao_device_g4(self.handle, C.byref(planes), c_idx, cf, int(qp), C.byref(prm), params_ptr,
                                                               params_stride, params_frame_stride, ctb_log2, lh, keep_ptr, keep_stride,
                                                               keep_frame_stride, fused, None if borders is None else C.byref(borders),
                                                               None if slice_offsets is None else C.byref(slice_offsets), None),
                 self.handle)
            return
        if slice_offsets is not None:
            _chk(_lib.lib().hevcdbk_h265_deblock_sao_device_sl(self.handle, C.byref(planes), c_idx, cf, int(qp), C.byref(prm), params_ptr,
                                                               params_stride, params_frame_stride, ctb_log2, lh, keep_ptr, keep_stride,
                                                               keep_frame_stride, fused, None if borders is None else C.byref(borders),
                                                               C.byref(slice_offsets), None), self.handle)
            return
        if borders is not None:
            _chk(_lib.lib().hevcdbk_h265_deblock_sao_device_nox(self.handle, C.byref(planes), c_idx, cf, int(qp), C.byref(prm), params_ptr,
                                                                params_stride, params_frame_stride, ctb_log2, lh, keep_ptr, keep_stride,
                                                                keep_frame_stride, fused, C.byref(borders), None), self.handle)
            return
        if cf == _lib.CHROMA_420 and lh == ctb_log2:
            rc = _lib.lib().hevc_deblock_sao_h265_device(self.handle, C.byref(planes), c_idx, int(qp), C.byref(prm), params_ptr,
                                                         params_stride, params_frame_stride, ctb_log2, keep_ptr, keep_stride,
                                                         keep_frame_stride, fused, None)
        else:
            rc = _lib.lib().hevcdbk_h265_deblock_sao_device_cf(self.handle, C.byref(planes), c_idx, cf, int(qp), C.byref(prm), params_ptr,
                                                            params_stride, params_frame_stride, ctb_log2, lh, keep_ptr, keep_stride,
                                                            keep_frame_stride, fused, None)
        _chk(rc, self.handle)

    def deblock_sao_device_planes(self, planes_list, qp, sao_list, *, h265=None, fused=_lib.FUSED_AUTO, tc_table=None, beta_table=None,
                                  chroma_format="420", borders=None, slice_offsets=None, g4=False):
        """hevc_deblock_sao_device_planes / hevc_deblock_sao_h265_device_planes: deblocking + SAO of Y, U, V of a batch in one
        call (one launch where the fused kernel takes every plane).  sao_list[i] = (params_ptr, params_stride, ctb_log2) or a
        dict with the optional params_frame_stride / keep / keep_stride / keep_frame_stride; h265 = None (reference-exact
        deblocking) or a dict of tc_offset_div2, beta_offset_div2, cb_qp_offset, cr_qp_offset (spec-exact).  chroma_format
        (spec-exact mode only): '400' / '420' / '422' / '444'; ctb_log2 = log2 of the plane's CTB width, its height follows
        from the format (or a ctb_log2_h entry of the dict).  borders (spec-exact mode only): ONE _lib.SaoBorders for the
        picture (hevcdbk_h265_deblock_sao_device_planes_nox).  slice_offsets (spec-exact mode only): ONE _lib.SliceOffsets for the
        picture (hevcdbk_h265_deblock_sao_device_planes_sl).  g4=True (spec-exact mode only): hevcdbk_h265_deblock_sao_device_planes_g4,
        whose chroma planes may be sized in multiples of 4 (Y 1920x1080 with Cb, Cr 960x540)."""
        cf = _lib.chroma_format_idc(chroma_format)
        if g4 and h265 is None:
            raise ValueError("the reference-exact mode takes multiples of 8 only: g4 needs h265=")
        if cf != _lib.CHROMA_420 and h265 is None:
            raise ValueError("the reference-exact mode is 4:2:0 only: chroma_format needs h265=")
        if borders is not None and h265 is None:
            raise ValueError("the reference-exact mode has no slice / tile boundaries: borders needs h265=")
        if slice_offsets is not None and h265 is None:
            raise ValueError("the reference-exact mode has no slices: slice_offsets needs h265=")
        arr = (_lib.DevicePlanes * len(planes_list))(*planes_list)
        if g4 or borders is not None or slice_offsets is not None or cf != _lib.CHROMA_420 or any(isinstance(so, dict) and "ctb_log2_h" in so for so in sao_list):
            spc = (_lib.SaoPlaneCf * len(sao_list))()
            for i, so in enumerate(sao_list):
                d = so if isinstance(so, dict) else {"params": so[0], "params_stride": so[1], "ctb_log2": so[2]}
                spc[i].params, spc[i].params_stride, spc[i].ctb_log2_w = d["params"], d["params_stride"], d["ctb_log2"]
                spc[i].ctb_log2_h = _ctb_log2_h(d["ctb_log2"], d.get("ctb_log2_h"), cf, i > 0)
                spc[i].params_frame_stride = d.get("params_frame_stride", 0)
                spc[i].keep, spc[i].keep_stride, spc[i].keep_frame_stride = d.get("keep"), d.get("keep_stride", 0), d.get("keep_frame_stride", 0)
            prm = _lib.H265Params(h265.get("tc_offset_div2", 0), h265.get("beta_offset_div2", 0), h265.get("cb_qp_offset", 0),
                                  h265.get("cr_qp_offset", 0))
            if g4:
                _chk(_lib.lib().hevcdbk_h265_deblock_sao_device_planes_g4(self.handle, arr, len(planes_list), cf, int(qp), C.byref(prm), spc,
                                                                          fused, None if borders is None else C.byref(borders),
                                                                          None if slice_offsets is None else C.byref(slice_offsets),
                                                                          None), self.handle)
                return
            if slice_offsets is not None:
                _chk(_lib.lib().hevcdbk_h265_deblock_sao_device_planes_sl(self.handle, arr, len(planes_list), cf, int(qp), C.byref(prm), spc,
                                                                          fused, None if borders is None else C.byref(borders),
                                                                          C.byref(slice_offsets), None), self.handle)
                return
            if borders is not None:
                _chk(_lib.lib().hevcdbk_h265_deblock_sao_device_planes_nox(self.handle, arr, len(planes_list), cf, int(qp), C.byref(prm), spc,
                                                                           fused, C.byref(borders), None), self.handle)
                return
            _chk(_lib.lib().hevcdbk_h265_deblock_sao_device_planes_cf(self.handle, arr, len(planes_list), cf, int(qp), C.byref(prm), spc,
                                                                   fused, None), self.handle)
            return
        sp = (_lib.SaoPlane * len(sao_list))()
        for i, so in enumerate(sao_list):
            d = so if isinstance(so, dict) else {"params": so[0], "params_stride": so[1], "ctb_log2": so[2]}
            sp[i].params, sp[i].params_stride, sp[i].ctb_log2 = d["params"], d["params_stride"], d["ctb_log2"]
            sp[i].params_frame_stride = d.get("params_frame_stride", 0)
            sp[i].keep, sp[i].keep_stride, sp[i].keep_frame_stride = d.get("keep"), d.get("keep_stride", 0), d.get("keep_frame_stride", 0)
        if h265 is None:
            t, _k = _tables(tc_table, beta_table)
            rc = _lib.lib().hevc_deblock_sao_device_planes(self.handle, arr, len(planes_list), int(qp), None if t is None else C.byref(t),
                                                           sp, fused, None)
        else:
            prm = _lib.H265Params(h265.get("tc_offset_div2", 0), h265.get("beta_offset_div2", 0), h265.get("cb_qp_offset", 0),
                                  h265.get("cr_qp_offset", 0))
            rc = _lib.lib().hevc_deblock_sao_h265_device_planes(self.handle, arr, len(planes_list), int(qp), C.byref(prm), sp, fused, None)
        _chk(rc, self.handle)

    def deblock_sao_nv12(self, luma_planes, pair_planes, qp, sao_luma, sao_pairs, *, h265, fused=_lib.FUSED_AUTO, borders=None,
                         slice_offsets=None):
        """hevcdbk_h265_deblock_sao_device_nv12: spec-exact deblocking + SAO of a whole semi-planar 4:2:0 picture -- the Y plane
        (DeviceBatch(...).planes()) and the plane of interleaved Cb / Cr pairs (DeviceBatch(..., semi_planar=True).planes()) -- in ONE
        launch where both fused kernels apply, else plane by plane.  sao_luma: a dict as deblock_sao_device_planes takes (params,
        params_stride, ctb_log2, optional params_frame_stride / keep / keep_stride / keep_frame_stride); sao_pairs: a dict with
        params_cb, params_cr, params_stride, ctb_log2 (= the luma ctb_log2 - 1) and the same optional entries.  h265: a dict of
        tc_offset_div2, beta_offset_div2, cb_qp_offset, cr_qp_offset.  borders / slice_offsets: ONE operand each on the luma CTB grid."""
        if h265 is None:
            raise ValueError("a semi-planar picture is filtered in the spec-exact mode: h265= is needed")
        for d, keys in ((sao_luma, ("params", "params_stride", "ctb_log2")), (sao_pairs, ("params_cb", "params_cr", "params_stride", "ctb_log2"))):
            missing = [k for k in keys if not isinstance(d, dict) or d.get(k) is None]
            if missing:
                raise ValueError("SAO operands missing: %s" % ", ".join(missing))
        sl = _lib.SaoPlaneCf(sao_luma["params"], sao_luma["params_stride"], sao_luma.get("params_frame_stride", 0), sao_luma["ctb_log2"],
                             sao_luma.get("ctb_log2_h", sao_luma["ctb_log2"]), sao_luma.get("keep"), sao_luma.get("keep_stride", 0),
                             sao_luma.get("keep_frame_stride", 0))
        sp = _lib.SaoPlaneSp(sao_pairs["params_cb"], sao_pairs["params_cr"], sao_pairs["params_stride"], sao_pairs.get("params_frame_stride", 0),
                             sao_pairs["ctb_log2"], sao_pairs.get("keep"), sao_pairs.get("keep_stride", 0), sao_pairs.get("keep_frame_stride", 0))
        prm = _lib.H265Params(h265.get("tc_offset_div2", 0), h265.get("beta_offset_div2", 0), h265.get("cb_qp_offset", 0),
                              h265.get("cr_qp_offset", 0))
        _chk(_lib.lib().hevcdbk_h265_deblock_sao_device_nv12(self.handle, C.byref(luma_planes), C.byref(pair_planes), int(qp), C.byref(prm),
                                                             C.byref(sl), C.byref(sp), fused, None if borders is None else C.byref(borders),
                                                             None if slice_offsets is None else C.byref(slice_offsets), None), self.handle)

    def filter_device_planes(self, planes_list, qp, *, tc_table=None, beta_table=None, variant=KERNEL_AUTO):
        """hevc_deblocking_filter_device_planes: Y, U, V of a batch in one call (one fused launch where that applies)."""
        arr = (_lib.DevicePlanes * len(planes_list))(*planes_list)
        t, _k = _tables(tc_table, beta_table)
        _chk(_lib.lib().hevc_deblocking_filter_device_planes(self.handle, arr, len(planes_list), int(qp),
                                                             None if t is None else C.byref(t), variant, None), self.handle)

    def run_timed(self, planes_list, qp, steps, *, variant=KERNEL_AUTO, tc_table=None, beta_table=None):
        """`steps` back-to-back launches of every plane in planes_list; per-step kernel ms (HIP events)."""
        arr = (_lib.DevicePlanes * len(planes_list))(*planes_list)
        ms = (C.c_float * steps)()
        t, _k = _tables(tc_table, beta_table)
        rc = _lib.lib().hevcdbk_device_run_timed(self.handle, arr, len(planes_list), int(qp),
                                                 None if t is None else C.byref(t), variant, steps, ms)
        _chk(rc, self.handle)
        return np.array(ms, np.float64)

    def replay(self, planes_list, qp, steps, *, warmup=0, settle_min_ms=150.0, settle_max_ms=2000.0, settle_tolerance=0.005,
               settle_window=32, variant=KERNEL_AUTO, tc_table=None, beta_table=None):
        """hevcdbk_device_replay: ONE uninterrupted stream of [settle by time][warmup][steps timed] launches, one
        synchronisation at the end.  Returns (per-launch kernel ms of the timed launches, dict of the replay's outputs)."""
        arr = (_lib.DevicePlanes * len(planes_list))(*planes_list)
        ms = (C.c_float * max(steps, 1))()
        t, _k = _tables(tc_table, beta_table)
        r = _lib.Replay(settle_min_ms=settle_min_ms, settle_max_ms=settle_max_ms, settle_tolerance=settle_tolerance,
                        settle_window=settle_window, warmup=warmup, steps=steps)
        rc = _lib.lib().hevcdbk_device_replay(self.handle, arr, len(planes_list), int(qp),
                                              None if t is None else C.byref(t), variant, C.byref(r), ms)
        _chk(rc, self.handle)
        info = {k: getattr(r, k) for k in ("settle_launches", "settled", "settle_ms", "settle_tail_mean_ms", "t_begin", "t_end",
                                           "wall_ms", "span_ms")}
        return np.array(ms[:steps], np.float64), info

    def pci_bus_id(self):
        """'0000:0a:00.0' of this context's device (hevcdbk_device_pci_bus_id), lower case"""
        buf = C.create_string_buffer(64)
        _chk(_lib.lib().hevcdbk_device_pci_bus_id(self.handle, buf, 64), self.handle)
        return buf.value.decode().lower()


def _ctb_log2_h(ctb_log2_w, ctb_log2_h, cf, chroma):
    """log2 of a plane's CTB height: given, or from the format (4:2:2 chroma CTBs are twice as tall as wide, 6.5.1)"""
    if ctb_log2_h is not None:
        return int(ctb_log2_h)
    return int(ctb_log2_w) + (1 if chroma and cf == _lib.CHROMA_422 else 0)


class DeviceBatch:
    """n_frames planes of identical geometry resident in HBM (src and dst), plus their bS arrays -- any plane geometry: a
    luma plane, or a chroma plane of any chroma format ((W / SubWidthC) x (H / SubHeightC), is_chroma=True).
    This is the layout bench.py times: frame f at base + f*frame_stride, tight pitch."""

    def __init__(self, ctx, plane_w, plane_h, n_frames, *, bit_depth=8, sample_bytes=None, is_chroma=False,
                 in_place=False, per_frame_bs=True, pitch=None, storage=None, semi_planar=False):
        """storage = (src_buffer, dst_buffer) of another batch: lay this batch out in that device memory instead of
        allocating (a decoder's frame pool serving another geometry); free() then leaves those buffers alone.
        semi_planar=True: a plane of interleaved Cb / Cr pairs (semi_planar= on filter_device_h265): plane_w x plane_h are
        the samples per component, a row holds 2 * plane_w samples, and frames are uploaded and downloaded as (plane_h, plane_w, 2)."""
        self.ctx = ctx
        self.w, self.h, self.n = plane_w, plane_h, n_frames
        self.bit_depth = bit_depth
        self.sb = sample_bytes or (1 if bit_depth == 8 else 2)
        self.dtype = np.uint8 if self.sb == 1 else np.uint16
        self.semi_planar = bool(semi_planar)
        self.is_chroma = is_chroma or self.semi_planar
        self.row_w = plane_w * (2 if self.semi_planar else 1)            # samples a row holds
        self.pitch = self.row_w * self.sb if pitch is None else int(pitch)  # bytes; > width*sb leaves row padding
        assert self.pitch >= self.row_w * self.sb and self.pitch % self.sb == 0
        self.frame_bytes = self.pitch * plane_h
        self._borrowed = storage is not None
        if storage is not None:
            self.src, self.dst = storage
            assert self.src.nbytes >= self.frame_bytes * n_frames and self.dst.nbytes >= self.frame_bytes * n_frames
        else:
            self.src = ctx.alloc(self.frame_bytes * n_frames)
            self.dst = self.src if in_place else ctx.alloc(self.frame_bytes * n_frames)
        self.per_frame_bs = per_frame_bs
        nb = n_frames if per_frame_bs else 1
        if plane_w % 8 or plane_h % 8 or self.semi_planar:
            # a plane sized in multiples of 4 (the g4= calls of the spec-exact mode): the reference-exact mode and its default bS do
            # not exist for it; the arrays are the spec-exact mode's 4-sample-granular ones, all zero until set_bs()
            L = _lib.lib()
            self.nv, self.nh = int(L.hevcdbk_h265_num_vert_bs(plane_w, plane_h)), int(L.hevcdbk_h265_num_hor_bs(plane_w, plane_h))
            dv, dh = np.zeros(self.nv, np.uint8), np.zeros(self.nh, np.uint8)
        else:
            self.nv, self.nh = num_vert_bs(plane_w, plane_h), num_hor_bs(plane_w, plane_h)
            dv, dh = default_bs(plane_w, plane_h)
        self.vert = ctx.alloc(self.nv * nb)
        self.hor = ctx.alloc(self.nh * nb)
        self.vert.upload(np.tile(dv, nb))
        self.hor.upload(np.tile(dh, nb))
        self.qp_map = None
        self.map_stride = 0
        self.map_frame_stride = 0
        self.ctu_log2 = 6

    @property
    def keep_shape(self):
        """(rows, columns) of the plane's SAO keep map, one byte per 8 x 8 samples: by ceiling, so that the last byte of a row or
        column of a plane sized in multiples of 4 (the g4= calls) speaks for 4 samples; plane / 8 for multiples of 8"""
        return (self.h + 7) // 8, (self.w + 7) // 8

    def ctb_shape(self, ctb_log2_w, ctb_log2_h=None):
        """(rows, columns) of the plane's CTB grid for CTBs of (1 << ctb_log2_w) x (1 << ctb_log2_h) samples, by ceiling: the last
        CTB of a row or column may be cut"""
        lh = ctb_log2_w if ctb_log2_h is None else ctb_log2_h
        return (self.h + (1 << lh) - 1) >> lh, (self.w + (1 << ctb_log2_w) - 1) >> ctb_log2_w

    def _pitched(self, a, fill=0):
        """(.., h, w) samples -> (.., h, pitch/sb) with `fill` in the row padding"""
        ps = self.pitch // self.sb
        if ps == self.row_w:
            return np.ascontiguousarray(a, self.dtype)
        out = np.full(a.shape[:-1] + (ps,), fill, self.dtype)
        out[..., : self.row_w] = a
        return out

    def _rows(self, a, lead):
        """frames as rows of samples: (.., h, w), or (.., h, w, 2) pairs of a semi-planar batch -> (.., h, row_w)"""
        a = np.asarray(a, self.dtype)
        want = lead + ((self.h, self.w, 2) if self.semi_planar else (self.h, self.w))
        assert a.shape == want, (a.shape, want)
        return a.reshape(lead + (self.h, self.row_w))

    def upload_frame(self, f, plane, fill=0):
        self.src.upload(self._pitched(self._rows(plane, ()), fill), f * self.frame_bytes)

    def upload_all(self, frames, fill=0):
        self.src.upload(self._pitched(self._rows(frames, (self.n,)), fill))

    def set_bs(self, f, vert, hor):
        assert self.per_frame_bs or f == 0
        self.vert.upload(np.ascontiguousarray(vert, np.uint8), f * self.nv)
        self.hor.upload(np.ascontiguousarray(hor, np.uint8), f * self.nh)

    def set_qp_map(self, qmap, ctu_log2=6, frame_stride=None):
        """qmap: one (rows, cols) map for every frame, or (n_frames, rows, cols) = one map per frame, laid out tight or, with
        frame_stride (entries, >= rows * cols), with a gap between the frames' maps (left as allocated)"""
        m = np.ascontiguousarray(qmap, np.uint8)
        if m.ndim == 2:
            if frame_stride is not None:
                raise ValueError("frame_stride needs one map per frame")
            self.qp_map = self.ctx.alloc(m.nbytes)
            self.qp_map.upload(m)
            self.map_frame_stride = 0
        else:
            if m.ndim != 3 or m.shape[0] != self.n:
                raise ValueError("qmap must be (rows, cols) or (n_frames, rows, cols)")
            size = m.shape[1] * m.shape[2]
            self.map_frame_stride = size if frame_stride is None else int(frame_stride)
            if self.map_frame_stride < size:
                raise ValueError("frame_stride is smaller than one map")
            self.qp_map = self.ctx.alloc(self.map_frame_stride * (self.n - 1) + size)
            for f in range(self.n):
                self.qp_map.upload(m[f], f * self.map_frame_stride)
        self.map_stride, self.ctu_log2 = m.shape[-1], ctu_log2

    def planes(self):
        p = _lib.DevicePlanes()
        p.src, p.dst = self.src.ptr, self.dst.ptr
        p.pitch, p.frame_stride, p.n_frames = self.pitch, self.frame_bytes, self.n
        p.plane_w, p.plane_h = self.w, self.h
        p.bit_depth, p.sample_bytes, p.is_chroma = self.bit_depth, self.sb, int(self.is_chroma)
        p.vert_bs, p.hor_bs = self.vert.ptr, self.hor.ptr
        p.vert_bs_stride = self.nv if self.per_frame_bs else 0
        p.hor_bs_stride = self.nh if self.per_frame_bs else 0
        if self.qp_map is not None:
            p.qp_map, p.qp_map_stride, p.ctu_log2 = self.qp_map.ptr, self.map_stride, self.ctu_log2
            p.qp_map_frame_stride = self.map_frame_stride
        return p

    def download_frame(self, f, which="dst", with_padding=False):
        buf = self.dst if which == "dst" else self.src
        a = buf.download(self.frame_bytes, f * self.frame_bytes, self.dtype).reshape(self.h, self.pitch // self.sb)
        if with_padding:
            return a
        a = a[:, : self.row_w]
        return a.reshape(self.h, self.w, 2) if self.semi_planar else a

    def free(self):
        own = (self.vert, self.hor, self.qp_map) if self._borrowed else (self.src, self.dst, self.vert, self.hor, self.qp_map)
        for b in own:
            if b is not None and b.ptr:
                b.free()


class ReadYuvFrame:
    """Same call surface as the reference class (cpu.h:33), executed by the HIP library.

    ctor(file_name, width, height, Qp=20)            cpu.h:35
    SetBoundaryStrenght(vert_bs, hor_bs)              cpu.h:120  (luma only)
    DeblockingFilter()                                cpu.h:134  -> hevc_deblocking_filter on the GPU
    Save(output_file_name)                            cpu.h:995
    Errors are raised as DeblockError carrying the reference's message text.
    """

    def __init__(self, file_name, width, height, Qp=20, ctx=None):
        with open(file_name, "rb") as fh:
            buf = fh.read()
        if len(buf) != 3 * width * height // 2:            # cpu.h:43-45
            raise DeblockError(_lib.ERR_FILE_SIZE)
        if width % 8 != 0 or height % 8 != 0:               # cpu.h:46-48
            raise DeblockError(_lib.ERR_DIMENSIONS)
        a = np.frombuffer(buf, np.uint8)
        ysz, csz = width * height, width * height // 4
        self.y = a[:ysz].reshape(height, width).copy()
        self.u = a[ysz:ysz + csz].reshape(height // 2, width // 2).copy()
        self.v = a[ysz + csz:].reshape(height // 2, width // 2).copy()
        self.width, self.height, self.Qp = width, height, Qp
        self._vert = self._hor = None
        self._own_ctx = ctx is None
        self._ctx = ctx or Context(0)
        self.timing = None

    def SetBoundaryStrenght(self, vert_bs, hor_bs):
        vert_bs = np.ascontiguousarray(vert_bs, np.uint8)
        hor_bs = np.ascontiguousarray(hor_bs, np.uint8)
        if vert_bs.size != num_vert_bs(self.width, self.height) or hor_bs.size != num_hor_bs(self.width, self.height):
            raise DeblockError(_lib.ERR_BS_SIZE)              # cpu.h:122-123
        self._vert, self._hor = vert_bs.copy(), hor_bs.copy()

    def DeblockingFilter(self, num_threads=1):
        # num_threads is the reference's OpenMP knob (cpu.h:134-135); meaningless on the GPU, accepted and ignored
        self.timing = self._ctx.filter_frame(self.y, self.u, self.v, qp=self.Qp, vert_bs=self._vert, hor_bs=self._hor)

    def Save(self, output_file_name):
        with open(output_file_name, "wb") as fh:
            fh.write(self.tobytes())

    def tobytes(self):
        return self.y.tobytes() + self.u.tobytes() + self.v.tobytes()

    def close(self):
        if self._own_ctx and self._ctx:
            self._ctx.close()
            self._ctx = None
