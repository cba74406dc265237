"""Measured distortion on the GPU through the Python layer: hevcdbk_sse_device, hevcdbk_sse_device_sp and hevcdbk_sse_totals_device,
equal as integers to the statement of tests/sse_ref.py.  Every output lands in a pre-filled buffer with guard entries before and
after, padding behind every CTB row and a gap between frames; EVERY uint64 of that buffer is compared.  Then the chain closed on the
device: deblocking -> statistics -> decision -> SAO, the distortion measured before and after against the decision's prediction."""
import numpy as np
import pytest

import sao_decide_ref as D
import sse_ref as R
from test_gpu_sao_stats import ctx, up  # noqa: F401 (ctx is the module's fixture)

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A5A5A5A5A
GUARD, PAD, GAP = 3, 2, 5     # entries before / after the grids, behind every CTB row, between frames
SHAPES = ((3, 3), (4, 4), (5, 5), (6, 6), (3, 4), (5, 6))
PLANES = ((8, 8), (12, 20), (72, 40), (136, 72), (200, 136))
PLACEMENTS = ("tight", "wide", "quad", "odd")


def placement(kind, row, sb):
    """(pitch, offset of the first sample) in samples for rows of `row` samples: tight pitch on a 16-byte-aligned base; pitch and
    base on 16 bytes; on four samples but not on 16 bytes; off by one sample"""
    per16 = 16 // sb
    up16 = (row + per16 - 1) // per16 * per16
    return {"tight": (row, 0), "wide": (up16, 0), "quad": (up16 + 4, 4), "odd": (row + 1, 1)}[kind]


def laid_out(frames, pitch, off, gap):
    """(n, h, row) samples -> one run of memory that ENDS with the last sample of the last row of the last frame"""
    n, h, row = frames.shape
    fs = h * pitch + gap
    out = np.full(off + (n - 1) * fs + (h - 1) * pitch + row, 0x5A5A & (0xFF if frames.itemsize == 1 else 0xFFFF), frames.dtype)
    for f in range(n):
        for y in range(h):
            at = off + f * fs + y * pitch
            out[at: at + row] = frames[f, y]
    return out, fs


def captured(call):
    from kernel_capture import kernels_enqueued, parse_kernel
    return [parse_kernel(x[0]) for x in kernels_enqueued(call)[1]]


def gpu_sse(ctx, recs, orgs, bd, lw, lh, *, rec_place="wide", org_place="wide", pairs=False, launched=None, rec_gap=0, org_gap=0):
    """recs (n, h, samples per row); orgs (n, ...) = per frame or (1, ...) = shared.  Returns (n, rows, cols) uint64 -- for a pair plane
    the even samples' and the odd samples' -- after comparing every other uint64 of the output buffers with the sentinel"""
    from gpu_video_codec_amd import _lib
    recs, orgs = np.asarray(recs), np.asarray(orgs)
    n, h, row = recs.shape
    sb = recs.itemsize
    w = row // 2 if pairs else row
    rows, cols = R.grid(w, h, lw, lh)
    stride, fstride = cols + PAD, rows * (cols + PAD) + GAP
    total = 2 * GUARD + fstride * n
    (rp, ro), (op, oo) = placement(rec_place, row, sb), placement(org_place, row, sb)
    per16 = 16 // sb
    rec_gap, org_gap = (g if k == "odd" else (g + per16 - 1) // per16 * per16 if k in ("wide", "tight") else g // 4 * 4
                        for g, k in ((rec_gap, rec_place), (org_gap, org_place)))
    hrec, rfs = laid_out(recs, rp, ro, rec_gap)
    horg, ofs = laid_out(orgs, op, oo, org_gap)
    drec, dorg = up(ctx, hrec), up(ctx, horg)
    douts = [up(ctx, np.full(total, SENTINEL, np.uint64)) for _ in range(2 if pairs else 1)]
    p = _lib.DevicePlanes()
    p.src, p.pitch, p.frame_stride, p.n_frames = drec.ptr + ro * sb, rp * sb, rfs * sb, n
    p.plane_w, p.plane_h, p.bit_depth, p.sample_bytes, p.is_chroma = w, h, bd, sb, int(pairs)
    kw = dict(semi_planar=True, out_cr_ptr=douts[1].ptr + GUARD * 8) if pairs else dict(ctb_log2_h=lh)

    def call(stream=None):
        ctx.sse_device(p, dorg.ptr + oo * sb, lw, org_pitch=op * sb, org_frame_stride=0 if orgs.shape[0] == 1 else ofs * sb,
                       out_ptr=douts[0].ptr + GUARD * 8, out_stride=stride, out_frame_stride=fstride, stream=stream, **kw)
    call()
    ctx.synchronize()
    if launched is not None:
        launched += captured(call)
    assert drec.download(hrec.nbytes).tobytes() == hrec.tobytes() and dorg.download(horg.nbytes).tobytes() == horg.tobytes(), "a source plane changed"
    res = []
    for d in douts:
        rest = d.download(total * 8).view(np.uint64).copy()
        got = np.zeros((n, rows, cols), np.uint64)
        for f in range(n):
            g = rest[GUARD + f * fstride: GUARD + f * fstride + rows * stride].reshape(rows, stride)
            got[f] = g[:, :cols]
            g[:, :cols] = SENTINEL
        assert (rest == SENTINEL).all(), "a uint64 outside the grid was written: %s" % np.argwhere(rest != SENTINEL)[:4].tolist()
        res.append(got)
    for b in [drec, dorg] + douts:
        b.free()
    return res if pairs else res[0]


def expected_mode(sb, row, rec_place, org_place):
    (rp, ro), (op, oo) = placement(rec_place, row, sb), placement(org_place, row, sb)
    return R.load_mode(sb, ro * sb, rp * sb, oo * sb, op * sb)


@pytest.fixture(scope="module")
def content():
    """(w, h, bd) -> (rec, org) of one frame, made once"""
    return {(w, h, bd): tuple(a[0] for a in R.planes(w, h, bd, np.random.default_rng([w, h, bd]))) for w, h in PLANES for bd in (8, 10, 16)}


@pytest.mark.parametrize("bd", [8, 10, 16])
@pytest.mark.parametrize("size", PLANES)
def test_planes_against_the_reference(ctx, content, size, bd):
    w, h = size
    rec, org = content[(w, h, bd)]
    sb = rec.itemsize
    modes = set()
    for i, (lw, lh) in enumerate(SHAPES):
        want = R.sse_plane(rec, org, lw, lh)
        assert want.any()
        # every placement at the first and the last shape; in between they rotate, and the two planes get different ones
        for pr, po in ([(p, p) for p in PLACEMENTS] + [("wide", "quad")] if i in (0, 5) else [(PLACEMENTS[i % 4], PLACEMENTS[(i + 1) % 4])]):
            ran = []
            got = gpu_sse(ctx, rec[None], org[None], bd, lw, lh, rec_place=pr, org_place=po, launched=ran)
            assert got[0].tobytes() == want.tobytes(), (size, bd, lw, lh, pr, po, np.argwhere(got[0] != want)[:4].tolist())
            mode = expected_mode(sb, w, pr, po)
            assert ran == [("sse_kernel", ("u8" if sb == 1 else "u16", mode, int(bd > 13), 0))], ran
            modes.add(mode)
    assert modes == {0, 1, 2}


@pytest.mark.parametrize("bd", [8, 13, 14, 16])
def test_width_of_the_accumulators(ctx, bd):
    """one 64 x 64 CTB at the extremes of the depth: 4096 * (2^bd - 1)^2; a lane's 64 squares fit 32 bits up to 13 bit, not above"""
    hi = (1 << bd) - 1
    dt = np.uint8 if bd == 8 else np.uint16
    rec, org = np.full((1, 64, 64), hi, dt), np.zeros((1, 64, 64), dt)
    for a, b in ((rec, org), (org, rec)):
        for place in ("wide", "quad", "odd"):
            assert gpu_sse(ctx, a, b, bd, 6, 6, rec_place=place, org_place=place).tolist() == [[[4096 * hi * hi]]], (bd, place)
    assert (gpu_sse(ctx, rec, org, bd, 3, 4) == 128 * hi * hi).all()


@pytest.mark.parametrize("shared", [False, True])
def test_batch_is_three_single_frame_calls(ctx, shared):
    w, h, bd, lw, lh = 136, 72, 10, 5, 5
    rec, org = R.planes(w, h, bd, np.random.default_rng(17), n=3)
    orgs = org[:1] if shared else org
    for place in ("wide", "odd"):
        got = gpu_sse(ctx, rec, orgs, bd, lw, lh, rec_place=place, org_place=place, rec_gap=24, org_gap=40)
        for f in range(3):
            o = orgs[0 if shared else f]
            one = gpu_sse(ctx, rec[f][None], o[None], bd, lw, lh, rec_place=place, org_place=place)
            assert got[f].tobytes() == one[0].tobytes() == R.sse_plane(rec[f], o, lw, lh).tobytes(), (shared, place, f)
        assert got[0].tobytes() != got[1].tobytes()


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("size", PLANES[:4])
def test_pair_plane(ctx, size, bd):
    """each output is hevcdbk_sse_device's ON THE DEVICE on the split planes, and the reference's; the components carry different errors"""
    w, h = size
    rec, org = R.planes(2 * w, h, bd, np.random.default_rng([w, h, bd, 2]))
    rec, org = rec[0].copy(), org[0]
    rec[:, 1::2] = np.clip(rec[:, 1::2].astype(np.int64) + 1, 0, (1 << bd) - 1).astype(rec.dtype)
    sb = rec.itemsize
    modes = set()
    for lg, places in ((3, [(p, p) for p in PLACEMENTS]), (4, [("wide", "quad")]), (5, [("quad", "odd"), ("wide", "wide")])):
        cb, cr = R.sse_pairs(rec, org, lg)
        assert cb.tobytes() != cr.tobytes()
        split = [gpu_sse(ctx, np.ascontiguousarray(rec[:, c::2])[None], np.ascontiguousarray(org[:, c::2])[None], bd, lg, lg) for c in (0, 1)]
        for pr, po in places:
            ran = []
            got = gpu_sse(ctx, rec[None], org[None], bd, lg, lg, rec_place=pr, org_place=po, pairs=True, launched=ran)
            for c, want in enumerate((cb, cr)):
                assert got[c][0].tobytes() == want.tobytes() == split[c][0].tobytes(), (size, bd, lg, pr, po, c)
            mode = expected_mode(sb, 2 * w, pr, po)
            assert ran == [("sse_kernel", ("u8" if sb == 1 else "u16", mode, 0, 1))], ran
            modes.add(mode)
    assert modes == {0, 1, 2}


# ---- totals -------------------------------------------------------------------------------------------------------------------------

def slice_layout(rows, cols, n_slices, rng):
    """irregular runs in raster order, slice n_slices // 2 left empty (n_slices > 2), two CTBs with an index >= n_slices"""
    n = rows * cols
    used = min(n_slices, n)
    cuts = np.sort(rng.choice(np.arange(1, n), used - 1, replace=False)) if used > 1 else np.array([], int)
    idx = np.searchsorted(cuts, np.arange(n), side="right").astype(np.uint16)
    if n_slices > 2:
        idx[idx >= n_slices // 2] += 1
    idx[-2:] = (n_slices, 65535)
    return idx.reshape(rows, cols)


def gpu_totals(ctx, sse, idx, n_slices, *, want_slices=True, want_frames=True, expect=None):
    """sse (n, rows, cols) uint64; idx None, (1, rows, cols) = shared or (n, rows, cols).  Returns (slice totals (n, n_slices) or None,
    frame totals (n,) or None); every other uint64 of the outputs must keep the sentinel.  expect: the error code the call must raise,
    with both outputs untouched"""
    from gpu_video_codec_amd import deblock
    n, rows, cols = sse.shape
    stride, fs = cols + PAD, rows * (cols + PAD) + GAP
    hin = np.full(n * fs, 1 << 60, np.uint64)
    for f in range(n):
        hin[f * fs: f * fs + rows * stride].reshape(rows, stride)[:, :cols] = sse[f]
    din = up(ctx, hin)
    bufs = [din]
    kw = {}
    if idx is not None:
        k = idx.shape[0]
        istride, ifs = cols + 3, rows * (cols + 3) + 7
        hidx = np.zeros(k * ifs, np.uint16)
        for f in range(k):
            hidx[f * ifs: f * ifs + rows * istride].reshape(rows, istride)[:, :cols] = idx[f]
        didx = up(ctx, hidx)
        bufs.append(didx)
        kw.update(slice_idx_ptr=didx.ptr, idx_stride=istride, idx_frame_stride=0 if k == 1 else ifs)
    stfs = n_slices + GAP
    dst, dft = up(ctx, np.full(2 * GUARD + n * stfs, SENTINEL, np.uint64)), up(ctx, np.full(2 * GUARD + n, SENTINEL, np.uint64))
    bufs += [dst, dft]
    if want_slices:
        kw.update(slice_total_ptr=dst.ptr + GUARD * 8, slice_total_frame_stride=stfs)
    if want_frames:
        kw.update(frame_total_ptr=dft.ptr + GUARD * 8)
    call = lambda: ctx.sse_totals_device(din.ptr, stride, cols, rows, n_frames=n, sse_frame_stride=fs, n_slices=n_slices, **kw)
    if expect is not None:
        with pytest.raises(deblock.DeblockError) as e:
            call()
        assert e.value.code == expect
    else:
        call()
    ctx.synchronize()
    assert din.download(hin.nbytes).tobytes() == hin.tobytes()
    st = dst.download().view(np.uint64).copy()
    ft = dft.download().view(np.uint64).copy()
    got_s = got_f = None
    if want_slices and expect is None:
        got_s = np.stack([st[GUARD + f * stfs: GUARD + f * stfs + n_slices].copy() for f in range(n)])
        for f in range(n):
            st[GUARD + f * stfs: GUARD + f * stfs + n_slices] = SENTINEL
    if want_frames and expect is None:
        got_f = ft[GUARD: GUARD + n].copy()
        ft[GUARD: GUARD + n] = SENTINEL
    assert (st == SENTINEL).all() and (ft == SENTINEL).all(), "a uint64 outside the outputs was written"
    for b in bufs:
        b.free()
    return got_s, got_f


@pytest.mark.parametrize("n_slices", [1, 7, 600])
def test_totals_against_the_reference(ctx, n_slices):
    rng = np.random.default_rng(n_slices)
    rows, cols, n = 5, 9, 3
    sse = rng.integers(0, 1 << 44, (n, rows, cols)).astype(np.uint64)
    idx = np.stack([slice_layout(rows, cols, n_slices, rng) for _ in range(n)])
    assert (idx >= n_slices).any() and (n_slices <= 2 or not (idx == n_slices // 2).any())
    for lay in (idx, idx[:1], None):
        want = [R.totals(sse[f], None if lay is None else lay[f if lay.shape[0] > 1 else 0], n_slices) for f in range(n)]
        ws, wf = np.stack([a for a, _ in want]), np.array([b for _, b in want], np.uint64)
        for slices, frames in ((True, True), (True, False), (False, True)):
            gs, gf = gpu_totals(ctx, sse, lay, n_slices, want_slices=slices, want_frames=frames)
            assert gs is None or gs.tobytes() == ws.tobytes(), (n_slices, slices, frames, lay is None)
            assert gf is None or gf.tobytes() == wf.tobytes(), (n_slices, slices, frames, lay is None)
        if n_slices > 2 and lay is not None:
            assert not ws[:, n_slices // 2].any() and (wf > ws.sum(axis=1, dtype=np.uint64)).all()


def test_totals_of_a_large_grid_and_the_wrap_rule(ctx):
    from gpu_video_codec_amd import _lib
    rng = np.random.default_rng(9)
    sse = rng.integers(0, 1 << 44, (1, 135, 240)).astype(np.uint64)        # a 3840 x 2160 picture in CTBs of 16
    idx = slice_layout(135, 240, 600, rng)[None]
    want = R.totals(sse[0], idx[0], 600)
    gs, gf = gpu_totals(ctx, sse, idx, 600)
    assert gs[0].tobytes() == want[0].tobytes() and gf[0] == want[1]
    wrap = np.zeros((1, 5, 9), np.uint64)
    wrap[0, 0, 0] = wrap[0, 4, 8] = (1 << 63) + 1
    gs, gf = gpu_totals(ctx, wrap, np.zeros((1, 5, 9), np.uint16), 4)
    assert gs.tolist() == [[2, 0, 0, 0]] and gf.tolist() == [2]
    gs, gf = gpu_totals(ctx, wrap, None, 1)
    assert gs.tolist() == [[2]] and gf.tolist() == [2]
    gpu_totals(ctx, wrap, None, 601, expect=_lib.ERR_UNSUPPORTED)            # refused, both outputs untouched


def test_the_same_bits_every_run(ctx, content):
    rec, org = content[(200, 136, 10)]
    a, b = (gpu_sse(ctx, rec[None], org[None], 10, 4, 4) for _ in range(2))
    assert a.tobytes() == b.tobytes()
    prec, porg = content[(136, 72, 8)]
    p, q = (gpu_sse(ctx, prec[None], porg[None], 8, 3, 3, pairs=True) for _ in range(2))
    assert p[0].tobytes() == q[0].tobytes() and p[1].tobytes() == q[1].tobytes()
    rng = np.random.default_rng(4)
    sse = rng.integers(0, 1 << 63, (2, 34, 61)).astype(np.uint64)
    idx = np.stack([slice_layout(34, 61, 7, rng) for _ in range(2)])
    s, t = (gpu_totals(ctx, sse, idx, 7) for _ in range(2))
    assert s[0].tobytes() == t[0].tobytes() and s[1].tobytes() == t[1].tobytes()


# ---- the chain closed on the device ------------------------------------------------------------------------------------------------------

def picture(case, rng):
    """Y, Cb, Cr of a 144 x 80 4:2:0 picture at 8 bit as (rec, org) per component: blocky reconstructions of a smooth original.
    "inside": every sample so far from both ends of the range that neither deblocking (a change of at most tC per sample, below 10
    at QP 30) nor an SAO offset (at most 7 at 8 bit) can take one to 0 or 255; "ends": an original at the ends of the range"""
    out = []
    for w, h in ((144, 80), (72, 40), (72, 40)):
        yy, xx = np.mgrid[0:h, 0:w]
        steps = rng.integers(-5, 6, (h // 8 + 1, w // 8 + 1))[yy // 8, xx // 8]
        if case == "inside":
            org = 128 + 60 * np.sin(xx / 9.0) * np.cos(yy / 7.0) + rng.integers(-4, 5, (h, w))
        else:
            # dark and bright fields of 16 x 16 whose borders lie between the 8 x 8 block edges; the reconstruction errs towards the
            # middle of the range, so the offsets SAO wants point at the ends -- where the samples nearest to them are clipped
            dark = (((xx + 4) // 16) + ((yy + 4) // 16)) % 2 == 0
            org = np.where(dark, 0, 255) + rng.integers(-2, 3, (h, w))
            steps = np.where(dark, np.abs(steps), -np.abs(steps))
        rec = org + steps + rng.integers(-2, 3, (h, w))
        out.append((np.clip(rec, 0, 255).astype(np.uint8), np.clip(org, 0, 255).astype(np.uint8)))
    return out


@pytest.mark.parametrize("case", ["inside", "ends"])
def test_closed_loop_wholly_on_the_device(ctx, case):
    """deblock -> statistics -> hevcdbk_sao_decide_device -> SAO for Y, Cb and Cr; the distortion measured on the device after
    deblocking and after SAO.  "inside": the clip of SAO never acts (asserted: an output sample of 0 or 255 is what a clip would
    leave, and there is none), and per CTB the measured change summed over the components IS the decision's delta_d.  "ends": the
    clip acts, the prediction misses in at least one CTB, and the measurement still is the reference's: what the entries are for."""
    from gpu_video_codec_amd import _lib, deblock
    L = _lib.lib()
    rng = np.random.default_rng(5)
    comps = picture(case, rng)
    lgs = (5, 4, 4)
    rows, cols = R.grid(144, 80, 5, 5)
    g = rows * cols
    dstats, dprm = [ctx.alloc(g * 384) for _ in range(3)], [ctx.alloc(g * 6) for _ in range(3)]
    ddec = ctx.alloc(g * 32)
    dsse = [[up(ctx, np.full(g, SENTINEL, np.uint64)) for _ in range(2)] for _ in range(3)]
    held, stages = [ddec] + dstats + dprm + [b for p in dsse for b in p], []
    for c, ((rec, org), lg) in enumerate(zip(comps, lgs)):
        h, w = rec.shape
        assert R.grid(w, h, lg, lg) == (rows, cols)
        drec, ddbk, dsao, dorg = up(ctx, rec), ctx.alloc(rec.nbytes), ctx.alloc(rec.nbytes), up(ctx, org)
        nv, nh = int(L.hevcdbk_h265_num_vert_bs(w, h)), int(L.hevcdbk_h265_num_hor_bs(w, h))
        dv, dh = up(ctx, rng.integers(0, 3, nv).astype(np.uint8)), up(ctx, rng.integers(0, 3, nh).astype(np.uint8))
        held += [drec, ddbk, dsao, dorg, dv, dh]
        p = _lib.DevicePlanes()
        p.src, p.dst, p.pitch, p.frame_stride, p.n_frames = drec.ptr, ddbk.ptr, w, w * h, 1
        p.plane_w, p.plane_h, p.bit_depth, p.sample_bytes, p.is_chroma = w, h, 8, 1, int(c > 0)
        p.vert_bs, p.hor_bs = dv.ptr, dh.ptr
        ctx.filter_device_h265(p, 30, c_idx=c)
        p.src, p.dst = ddbk.ptr, dsao.ptr                  # the deblocked plane: what is measured, what SAO reads
        ctx.sao_stats_device(p, dorg.ptr, lg, out_ptr=dstats[c].ptr, out_stride=cols)
        ctx.sse_device(p, dorg.ptr, lg, out_ptr=dsse[c][0].ptr, out_stride=cols)
        stages.append((p, dorg, ddbk, dsao, lg))
    ctx.sao_decide_device(dstats[0].ptr, cols, cols, rows, 8, 1024, out_ptr=dprm[0].ptr, out_stride=cols, decision_ptr=ddec.ptr,
                          decision_stride=cols, stats_cb_ptr=dstats[1].ptr, stats_cr_ptr=dstats[2].ptr, out_cb_ptr=dprm[1].ptr, out_cr_ptr=dprm[2].ptr)
    for c, (p, dorg, ddbk, dsao, lg) in enumerate(stages):
        ctx.sao_device(p, dprm[c].ptr, cols, lg)
        p.src = dsao.ptr                                   # a descriptor whose src is SAO's output
        ctx.sse_device(p, dorg.ptr, lg, out_ptr=dsse[c][1].ptr, out_stride=cols)
    ctx.synchronize()
    dec = ddec.download(g * 32).view(D.DECISION_DTYPE).reshape(rows, cols)
    measured = np.zeros((rows, cols), np.int64)
    clipped = False
    for c, ((rec, org), (p, dorg, ddbk, dsao, lg)) in enumerate(zip(comps, stages)):
        dbk, sao = (b.download(rec.nbytes).reshape(rec.shape) for b in (ddbk, dsao))
        before, after = (b.download(g * 8).view(np.uint64).reshape(rows, cols) for b in dsse[c])
        assert before.tobytes() == R.sse_plane(dbk, org, lg, lg).tobytes() and after.tobytes() == R.sse_plane(sao, org, lg, lg).tobytes(), c
        assert (dbk != rec).any() and (sao != dbk).any(), "a stage changed nothing"
        clipped |= bool(sao.min() == 0 or sao.max() == 255)
        measured += after.astype(np.int64) - before.astype(np.int64)
    missed = int((measured != dec["delta_d"]).sum())
    print(case, "delta SSE measured", int(measured.sum()), "predicted", int(dec["delta_d"].sum()), "CTBs that differ", missed, "of", g)
    if case == "inside":
        assert not clipped and missed == 0 and int(measured.sum()) < 0
    else:
        assert clipped and missed >= 1
    for b in held:
        b.free()
    assert isinstance(ctx, deblock.Context)
