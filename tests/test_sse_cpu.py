"""Measured distortion without a GPU: hevcdbk_sse_device, hevcdbk_sse_device_sp and hevcdbk_sse_totals_device exist everywhere they must
and refuse bad operands with the documented codes in the documented order; the numpy statement of tests/sse_ref.py agrees with a
sample-by-sample loop in Python integers; and csrc/sse.h, compiled into a stand-alone program (plain and under the address and
undefined-behaviour sanitizers) that runs a wave's procedure lane by lane and the butterfly step by step, on planes that end with
their last sample, reproduces the reference on every load path."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import sse_ref as R

CSRC = os.path.join(ROOT, "gpu_video_codec_amd", "csrc")
SIM_SRC = os.path.join(ROOT, "tests", "sse_sim", "sse_sim.cpp")
ENTRIES = ("hevcdbk_sse_device", "hevcdbk_sse_device_sp", "hevcdbk_sse_totals_device")
SHAPES = ((3, 3), (4, 4), (5, 5), (6, 6), (3, 4), (5, 6))
PLANES = ((8, 8), (12, 20), (72, 40), (136, 72), (200, 136))


@pytest.fixture(scope="module")
def L():
    from gpu_video_codec_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


# ---- the entries and their codes -------------------------------------------------------------------------------------------------

def test_entries_are_exported_declared_and_bound(L):
    import inspect
    from gpu_video_codec_amd import _lib, deblock
    hdr = open(os.path.join(ROOT, "include", "hevc_deblock.h")).read()
    for sym, n in zip(ENTRIES, (11, 11, 15)):
        assert re.search(r"HEVCDBK_API int %s\s*\(" % sym, hdr) and re.fullmatch(r"hevcdbk_[a-z0-9_]+", sym)
        assert sym in _lib.EXPORTS and hasattr(L, sym) and len(getattr(L, sym).argtypes) == n
    sig = inspect.signature(deblock.Context.sse_device).parameters
    assert sig["semi_planar"].default is False and sig["out_cr_ptr"].default is None and sig["out_ptr"].kind is inspect.Parameter.KEYWORD_ONLY
    assert "n_slices" in inspect.signature(deblock.Context.sse_totals_device).parameters
    for f in ("sse.hip", "sse.h", "sse_host.cpp", "sse_launch.h"):
        assert os.path.exists(os.path.join(CSRC, f))
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^HIP_SRCS :=.*\bsse\.hip", mk, re.M) and re.search(r"^CXX_SRCS :=.*\bsse_host\.cpp", mk, re.M) and "-o sse.s sse.hip" in mk


REC, ORG, OUT, OUT2, IDX, ST, FT = (0x100000 * k for k in range(1, 8))


def planes(src=REC, pitch=64, fstride=None, n=1, w=64, h=64, bd=8, sb=1, chroma=0):
    from gpu_video_codec_amd import _lib
    p = _lib.DevicePlanes()
    p.src, p.pitch, p.frame_stride, p.n_frames = src, pitch, pitch * h if fstride is None else fstride, n
    p.plane_w, p.plane_h, p.bit_depth, p.sample_bytes, p.is_chroma = w, h, bd, sb, chroma
    return p


def test_plane_entry_codes_and_their_order_without_a_device(L):
    """a context that no device stands behind (a zeroed block of memory: never looked into)"""
    from gpu_video_codec_amd import _lib
    ctx = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    ARG, DIM, UNS = _lib.ERR_ARG, _lib.ERR_DIMENSIONS, _lib.ERR_UNSUPPORTED

    def call(ctx=ctx, rec=True, org=ORG, opitch=None, ofs=0, lw=4, lh=4, out=OUT, stride=4, sfs=0, **kw):
        p = planes(**kw)
        return L.hevcdbk_sse_device(ctx, C.byref(p) if rec else None, org, p.pitch if opitch is None else opitch, ofs, lw, lh, out, stride, sfs, None)

    last = dict(bd=10, sb=2, pitch=129)               # everything else in order: the last check answers
    assert call(**last) == UNS and call(bd=10, sb=2, pitch=128, src=REC + 1) == UNS and call(bd=10, sb=2, pitch=128, org=ORG + 1) == UNS
    assert call(bd=10, sb=2, pitch=128, fstride=128 * 64 + 1) == UNS and call(bd=10, sb=2, pitch=128, opitch=131) == UNS
    assert call(bd=10, sb=2, pitch=128, ofs=3) == UNS
    assert call(ctx=None) == ARG and call(rec=False) == ARG and call(src=0) == ARG and call(org=None) == ARG and call(out=None) == ARG
    assert call(bd=7) == ARG and call(bd=17, sb=2) == ARG and call(bd=10, sb=1) == ARG and call(bd=8, sb=3) == ARG
    for w, h in ((0, 64), (64, 0), (4, 64), (64, 4), (66, 64), (64, 62)):
        assert call(w=w, h=h, pitch=128) == DIM, (w, h)
    for lw, lh in ((2, 2), (7, 7), (4, 3), (4, 6), (6, 7), (2, 3)):
        assert call(lw=lw, lh=lh) == ARG, (lw, lh)
    assert call(lw=5, lh=6, stride=2, **last) == UNS and call(lw=3, lh=4, stride=8, **last) == UNS
    assert call(pitch=63) == ARG and call(opitch=63) == ARG and call(n=65536, sfs=16) == ARG and call(h=65536, pitch=64) == ARG
    assert call(stride=3) == ARG and call(stride=0x80000000) == ARG and call(out=OUT + 4) == ARG and call(out=OUT + 1) == ARG
    assert call(n=2, sfs=15) == ARG and call(n=2, sfs=0) == ARG and call(n=2, sfs=16, **last) == UNS and call(n=1, sfs=0, **last) == UNS
    # the order: each refusal wins over every later one
    assert call(bd=7, w=66) == ARG and call(w=66, lw=2) == DIM and call(lw=2, **last) == ARG and call(stride=3, **last) == ARG
    assert call(out=OUT + 4, **last) == ARG and call(n=2, sfs=15, **last) == ARG and call(w=66, stride=0, out=OUT + 4, **last) == DIM
    assert call(bd=10, sb=2, pitch=127) == ARG                     # below a row, though odd as well
    # a 12 x 20 plane: multiples of 4, the grid by ceiling
    assert call(w=12, h=20, lw=3, lh=3, stride=2, **last) == UNS and call(w=12, h=20, lw=3, lh=3, stride=1, **last) == ARG


def test_pair_plane_entry_codes_and_their_order_without_a_device(L):
    from gpu_video_codec_amd import _lib
    ctx = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    ARG, DIM, UNS = _lib.ERR_ARG, _lib.ERR_DIMENSIONS, _lib.ERR_UNSUPPORTED

    def call(ctx=ctx, rec=True, org=ORG, opitch=None, ofs=0, lg=4, cb=OUT, cr=OUT2, stride=4, sfs=0, chroma=1, pitch=128, **kw):
        p = planes(chroma=chroma, pitch=pitch, **kw)
        return L.hevcdbk_sse_device_sp(ctx, C.byref(p) if rec else None, org, p.pitch if opitch is None else opitch, ofs, lg, cb, cr, stride, sfs, None)

    last = dict(bd=10, sb=2, pitch=257)
    assert call(**last) == UNS and call(bd=10, sb=2, pitch=256, org=ORG + 1) == UNS
    assert call(ctx=None) == ARG and call(rec=False) == ARG and call(src=0) == ARG and call(org=None) == ARG and call(cb=None) == ARG and call(cr=None) == ARG
    assert call(bd=7) == ARG and call(chroma=0) == ARG and call(chroma=0, **last) == ARG
    assert call(w=66) == DIM and call(h=4) == DIM and call(chroma=0, w=66) == ARG
    assert call(lg=2) == ARG and call(lg=6, stride=1) == ARG and call(lg=5, stride=2, **last) == UNS and call(lg=3, stride=8, **last) == UNS
    assert call(pitch=127) == ARG and call(opitch=127) == ARG and call(pitch=64) == ARG and call(n=65536, sfs=16) == ARG
    assert call(bd=10, sb=2, pitch=255) == ARG
    assert call(stride=3) == ARG and call(cb=OUT + 4) == ARG and call(cr=OUT2 + 4) == ARG and call(n=2, sfs=15) == ARG
    # two outputs whose extents meet: 4 x 4 entries of 8 bytes, from the first entry to the last
    for kw in (dict(cr=OUT), dict(cr=OUT + 8 * 15), dict(cr=OUT - 8 * 15), dict(n=2, sfs=16, cr=OUT + 8 * 31), dict(stride=6, cr=OUT + 8 * 21)):
        assert call(**kw, **last) == ARG, kw
    for kw in (dict(cr=OUT + 8 * 16), dict(cr=OUT - 8 * 16), dict(n=2, sfs=16, cr=OUT + 8 * 32), dict(stride=6, cr=OUT + 8 * 22)):
        assert call(**kw, **last) == UNS, kw
    assert call(lg=2, **last) == ARG and call(w=66, lg=2) == DIM and call(stride=3, cr=OUT) == ARG and call(n=2, sfs=15, cr=OUT, **last) == ARG


def test_totals_codes_and_their_order_without_a_device(L):
    from gpu_video_codec_amd import _lib
    ctx = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    ARG, DIM, UNS = _lib.ERR_ARG, _lib.ERR_DIMENSIONS, _lib.ERR_UNSUPPORTED

    def call(ctx=ctx, sse=OUT, stride=9, sfs=0, cx=9, cy=5, n=1, idx=IDX, istride=9, ifs=0, ns=601, st=ST, stfs=0, ft=FT):
        return L.hevcdbk_sse_totals_device(ctx, sse, stride, sfs, cx, cy, n, idx, istride, ifs, ns, st, stfs, ft, None)

    assert call() == UNS and call(ns=65536) == UNS and call(st=None) == UNS and call(ft=None) == UNS and call(idx=None, istride=0) == UNS
    assert call(n=3, sfs=45, stfs=601) == UNS and call(n=3, sfs=45, stfs=0, st=None) == UNS and call(n=0) == UNS
    assert call(ctx=None) == ARG and call(sse=None) == ARG and call(st=None, ft=None) == ARG
    assert call(cx=0) == DIM and call(cy=0) == DIM and call(cx=65536, stride=65536, istride=65536) == DIM and call(cy=65536) == DIM
    assert call(stride=8) == ARG and call(istride=8) == ARG and call(ns=0) == ARG and call(ns=65537) == ARG and call(n=65536, stfs=601) == ARG
    assert call(n=2, stfs=600) == ARG and call(n=2, stfs=0) == ARG
    assert call(sse=OUT + 4) == ARG and call(st=ST + 4) == ARG and call(ft=FT + 4) == ARG and call(idx=IDX + 1) == ARG
    for kw in (dict(ft=ST), dict(ft=ST + 8 * 600), dict(st=FT - 8 * 600), dict(st=OUT), dict(st=OUT + 8 * 44), dict(ft=OUT + 8 * 44),
               dict(ft=OUT + 8 * 134, n=3, sfs=45, stfs=601), dict(st=FT + 16, n=3, sfs=45, stfs=601), dict(sse=ST + 8 * 600)):
        assert call(**kw) == ARG, kw
    for kw in (dict(ft=ST + 8 * 601), dict(st=FT - 8 * 601), dict(st=OUT + 8 * 45), dict(ft=OUT + 8 * 135, n=3, sfs=45, stfs=601),
               dict(st=FT + 24, n=3, sfs=45, stfs=601)):
        assert call(**kw) == UNS, kw
    # the order
    assert call(st=None, ft=None, cx=0) == ARG and call(cx=0, stride=0) == DIM and call(stride=8, ns=0) == ARG and call(ns=0, ft=ST) == ARG
    assert call(ns=600, ft=ST) == ARG and call(ns=65537, cx=0) == DIM and call(sse=OUT + 4, ns=601) == ARG


# ---- the reference alone ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bd", [8, 10, 16])
def test_reference_is_the_sample_by_sample_loop(bd):
    rng = np.random.default_rng(bd)
    for w, h in PLANES[:3]:
        rec, org = R.planes(w, h, bd, rng)
        for lw, lh in SHAPES:
            a, b = R.sse_plane(rec[0], org[0], lw, lh), R.sse_plane_loop(rec[0], org[0], lw, lh)
            assert a.shape == b.shape == R.grid(w, h, lw, lh) and [[int(v) for v in r] for r in a] == b.tolist(), (w, h, lw, lh)
        assert int(R.sse_plane(rec[0], org[0], 3, 3).sum()) == int(((org[0].astype(np.int64) - rec[0]) ** 2).sum()) > 0
        prec, porg = R.planes(2 * w, h, bd, rng)
        cb, cr = R.sse_pairs(prec[0], porg[0], 3)
        assert cb.tobytes() == R.sse_plane(prec[0][:, 0::2], porg[0][:, 0::2], 3, 3).tobytes() and cb.tobytes() != cr.tobytes()


def test_reference_totals():
    rng = np.random.default_rng(1)
    sse = rng.integers(0, 1 << 44, (5, 9)).astype(np.uint64)
    idx = np.minimum(np.arange(45).reshape(5, 9) // 7, 5)
    st, ft = R.totals(sse, idx, 4)
    assert int(ft) == int(sse.sum()) and [int(v) for v in st] == [int(sse.ravel()[7 * s: 7 * s + 7].sum()) for s in range(4)]
    st, ft = R.totals(sse, None, 3)
    assert int(st[0]) == int(ft) and not st[1:].any()
    wrap = np.zeros((5, 9), np.uint64)
    wrap[0, 0] = wrap[4, 8] = (1 << 63) + 1
    st, ft = R.totals(wrap, None, 1)
    assert int(st[0]) == 2 == int(ft)
    assert R.load_mode(1, 0, 64, 0, 64) == 2 and R.load_mode(1, 4, 64, 0, 64) == 1 and R.load_mode(2, 8, 64, 0, 64) == 1
    assert R.load_mode(2, 4, 64, 0, 64) == 0 and R.load_mode(1, 0, 65, 0, 64) == 0


# ---- csrc/sse.h on the CPU ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=["plain", "sanitized"])
def sim(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("sse_sim_" + request.param)
    exe = str(d / "sse_sim")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas"] + flags + ["-I", CSRC, "-o", exe, SIM_SRC])
    return exe, str(d)


def placements(row, sb):
    """name -> (pitch, offset) in bytes of a plane whose rows hold `row` bytes: on 16 bytes, on four samples but not on 16 bytes, off
    by one sample, and tight"""
    q = 4 * sb
    up16 = (row + 15) // 16 * 16
    return {"wide": (up16, 0), "quad": (up16 + q, q), "odd": (row + sb, sb), "tight": (row, 0)}


def run_plane(sim, rec, org, lw, lh, bd, pairs, place_rec, place_org, mode=None):
    """rec, org: (h, samples per row).  Returns the grid (pairs: the two grids) as the program leaves it, and the mode it ran"""
    exe, d = sim
    sb = rec.itemsize
    h, per_row = rec.shape
    w = per_row // 2 if pairs else per_row
    row = per_row * sb
    (rp, ro), (op, oo) = placements(row, sb)[place_rec], placements(row, sb)[place_org]
    rule = R.load_mode(sb, ro, rp, oo, op)
    mode = rule if mode is None else mode
    assert mode <= rule
    blob = np.array([w, h, sb, lw, lh, int(pairs), mode, int(bd > 13), rp, op, ro, oo], "<i4").tobytes()
    for a, pitch, off in ((rec, rp, ro), (org, op, oo)):
        raw = bytearray(b"\xA5" * (off + pitch * (h - 1) + row))
        for y in range(h):
            raw[off + y * pitch: off + y * pitch + row] = a[y].tobytes()
        blob += bytes(raw)
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    open(fin, "wb").write(blob)
    r = subprocess.run([exe, "plane", fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    rows, cols = R.grid(w, h, lw, lh)
    out = np.fromfile(fout, np.uint64).reshape(2 if pairs else 1, rows, cols)
    return out, mode


@pytest.mark.parametrize("bd", [8, 10, 16])
@pytest.mark.parametrize("size", PLANES)
def test_wave_procedure_reproduces_the_reference(sim, size, bd):
    w, h = size
    rec, org = R.planes(w, h, bd, np.random.default_rng(w * 131 + bd))
    rec, org = rec[0], org[0]
    ran = set()
    for lw, lh in SHAPES:
        want = R.sse_plane(rec, org, lw, lh)
        for pr, po in (("wide", "wide"), ("quad", "quad"), ("odd", "odd"), ("tight", "tight"), ("wide", "quad"), ("odd", "wide")):
            got, mode = run_plane(sim, rec, org, lw, lh, bd, False, pr, po)
            ran.add(mode)
            assert got[0].tobytes() == want.tobytes(), (size, bd, lw, lh, pr, po, np.argwhere(got[0] != want)[:4].tolist())
        for mode in (0, 1):                                      # the narrower paths on the widest placement: the same result
            got, _ = run_plane(sim, rec, org, lw, lh, bd, False, "wide", "wide", mode)
            assert got[0].tobytes() == want.tobytes(), (size, bd, lw, lh, "forced", mode)
    assert ran == {0, 1, 2}


@pytest.mark.parametrize("bd", [8, 10, 16])
@pytest.mark.parametrize("size", PLANES[:4])
def test_wave_procedure_on_a_pair_plane(sim, size, bd):
    w, h = size
    rec, org = R.planes(2 * w, h, bd, np.random.default_rng(w * 137 + bd))
    rec, org = rec[0].copy(), org[0]
    rec[:, 1::2] = np.clip(rec[:, 1::2].astype(np.int64) + 1, 0, (1 << bd) - 1).astype(rec.dtype)      # the components carry different errors
    for lg in (3, 4, 5):
        cb, cr = R.sse_pairs(rec, org, lg)
        assert cb.tobytes() != cr.tobytes()
        for pr, po in (("wide", "wide"), ("quad", "quad"), ("odd", "odd"), ("tight", "quad")):
            got, _ = run_plane(sim, rec, org, lg, lg, bd, True, pr, po)
            assert got[0].tobytes() == cb.tobytes() and got[1].tobytes() == cr.tobytes(), (size, bd, lg, pr, po)
        for mode in (0, 1):
            got, _ = run_plane(sim, rec, org, lg, lg, bd, True, "wide", "wide", mode)
            assert got[0].tobytes() == cb.tobytes() and got[1].tobytes() == cr.tobytes(), (size, bd, lg, "forced", mode)


@pytest.mark.parametrize("bd", [8, 13, 14, 16])
def test_width_of_the_accumulators(sim, bd):
    """a 64 x 64 CTB at the extremes of the depth: a lane's 64 squares fit 32 bits up to 13 bit and do not above"""
    hi = (1 << bd) - 1
    dt = np.uint8 if bd == 8 else np.uint16
    rec, org = np.full((64, 64), hi, dt), np.zeros((64, 64), dt)
    assert (64 * hi * hi < 1 << 32) == (bd <= 13)
    for a, b in ((rec, org), (org, rec)):
        for place in ("wide", "quad", "odd"):
            got, _ = run_plane(sim, a, b, 6, 6, bd, False, place, place)
            assert got.tolist() == [[[4096 * hi * hi]]], (bd, place)
            got, _ = run_plane(sim, a, b, 3, 4, bd, False, place, place)
            assert (got == 128 * hi * hi).all() and got.shape == (1, 4, 8)
    prec = np.zeros((32, 64), dt)
    prec[:, 1::2] = hi
    got, _ = run_plane(sim, prec, np.zeros((32, 64), dt), 5, 5, bd, True, "wide", "wide")
    assert got.tolist() == [[[0]], [[1024 * hi * hi]]]


def run_totals(sim, sse, idx, n_slices, stride=None, istride=None):
    exe, d = sim
    rows, cols = sse.shape
    stride, istride = stride or cols, istride or cols

    def laid(a, s, dt, fill):
        out = np.full((rows - 1) * s + cols, fill, dt)
        for y in range(rows):
            out[y * s: y * s + cols] = a[y]
        return out

    blob = np.array([cols, rows, stride, int(idx is not None), istride, n_slices], "<i4").tobytes() + laid(sse, stride, np.uint64, 1 << 60).tobytes()
    if idx is not None:
        blob += laid(idx, istride, np.uint16, 0).tobytes()
    fin, fout = os.path.join(d, "tin.bin"), os.path.join(d, "tout.bin")
    open(fin, "wb").write(blob)
    r = subprocess.run([exe, "totals", fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    out = np.fromfile(fout, np.uint64)
    return out[:-1], out[-1]


def slice_layout(rows, cols, n_slices, rng, beyond=True):
    """irregular runs in raster order over slices 0 .. n_slices - 1 with one slice left empty and, with `beyond`, some CTBs at
    n_slices and above"""
    n = rows * cols
    used = min(n_slices, n)
    cuts = np.sort(rng.choice(np.arange(1, n), used - 1, replace=False)) if used > 1 else np.array([], int)
    idx = np.searchsorted(cuts, np.arange(n), side="right").astype(np.uint16)
    if n_slices > 2:
        idx[idx >= n_slices // 2] += 1                     # slice n_slices // 2 is empty; the last run moves beyond
    if beyond:
        idx[-2:] = (n_slices, 65535)
    return idx.reshape(rows, cols)


@pytest.mark.parametrize("n_slices", [1, 7, 600])
def test_totals_walk_reproduces_the_reference(sim, n_slices):
    rng = np.random.default_rng(n_slices)
    for rows, cols in ((5, 9), (1, 1), (34, 61), (135, 240)):
        sse = rng.integers(0, 1 << 44, (rows, cols)).astype(np.uint64)
        for idx in (None, slice_layout(rows, cols, n_slices, rng) if rows * cols > 2 else np.zeros((rows, cols), np.uint16)):
            want = R.totals(sse, idx, n_slices)
            got = run_totals(sim, sse, idx, n_slices, cols + 3, cols + 5)
            assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1], (rows, cols, n_slices, idx is None)
    idx = slice_layout(5, 9, n_slices, rng)
    if n_slices > 2:
        assert not (idx == n_slices // 2).any() and (idx >= n_slices).any()
    wrap = np.zeros((5, 9), np.uint64)
    wrap[0, 0] = wrap[4, 8] = (1 << 63) + 1
    st, ft = run_totals(sim, wrap, None, n_slices)
    assert int(st[0]) == 2 == int(ft)
