"""SAO parameter estimation on the GPU through the Python layer: hevcdbk_sao_stats_device, bit for bit against the per-sample statement
of tests/sao_stats_ref.py, and hevcdbk_sao_pick_device against its plain-int statement.  Every output lands in a pre-filled buffer
with guard entries before and after, padding behind every CTB row and a gap between frames; EVERY int32 of that buffer is compared,
and the source planes must come back as they were uploaded.  PARITY UNPINNED, like the rest of SAO."""
import numpy as np
import pytest

import rext_oracle as ro
import sao_borders_ref as R
import sao_stats_ref as S

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
GUARD, PAD, GAP = 3, 2, 5     # entries before / after the grids, behind every CTB row, between frames
LAMBDAS = (0, 1024, 16384)


@pytest.fixture(scope="module")
def ctx():
    from gpu_video_codec_amd import deblock
    c = deblock.Context(0)
    yield c
    c.close()


def up(ctx, a):
    a = np.ascontiguousarray(a)
    d = ctx.alloc(max(a.nbytes, 1))
    d.upload(a.view(np.uint8).ravel())
    return d


def dev_planes(buf, n, w, h, depth, sb, pitch, dst=None):
    from gpu_video_codec_amd import _lib
    p = _lib.DevicePlanes()
    p.src, p.dst, p.pitch, p.frame_stride, p.n_frames = buf.ptr, 0 if dst is None else dst.ptr, pitch * sb, pitch * sb * h, n
    p.plane_w, p.plane_h, p.bit_depth, p.sample_bytes = w, h, depth, sb
    return p


def laid_out(frames, pitch, gap, off):
    """(n, h, w) samples -> one run of memory in which row y of frame f starts at sample off + f * (h * pitch + gap) + y * pitch;
    0x5A.. everywhere else, the row padding included"""
    frames = np.asarray(frames)
    n, h, w = frames.shape
    out = np.full(off + (n - 1) * (h * pitch + gap) + h * pitch, 0x5A5A & (0xFF if frames.itemsize == 1 else 0xFFFF), frames.dtype)
    for f in range(n):
        at = off + f * (h * pitch + gap)
        out[at: at + h * pitch].reshape(h, pitch)[:, :w] = frames[f]
    return out


def captured(call):
    """[(kernel, template arguments)] that call(stream) enqueues, from a stream capture (never instantiated, never launched)"""
    from kernel_capture import kernels_enqueued, parse_kernel
    _, k = kernels_enqueued(call)
    return [parse_kernel(x[0]) for x in k]


def gpu_stats(ctx, recs, orgs, bd, lw, lh, *, keeps=None, noxs=None, pitch=None, tight=False, org_pitch=None, rec_off=0, org_off=0, rec_gap=0,
              org_gap=0, launched=None):
    """recs (n, h, w); orgs, keeps, noxs: (n, ...) = per frame, (1, ...) = shared, None = absent; the stride of keeps and noxs is
    their last dimension, their frame stride their last two (columns and rows beyond the map's or the grid's: padding the entry
    must not read).  pitch, org_pitch (default: pitch), rec_off / org_off (how far the plane's first sample lies behind the start of
    its allocation) and rec_gap / org_gap (what a frame stride has beyond the rows of a frame) are in samples.  Returns (n, rows,
    cols) statistics after comparing every other int32 of the output buffer with the sentinel and the sources with what was uploaded.
    launched: a list that receives the kernels of a capture of the same call, on the same buffers"""
    from gpu_video_codec_amd import _lib
    recs = np.asarray(recs)
    n, h, w = recs.shape
    sb = recs.itemsize
    pitch = w if pitch is None else pitch
    org_pitch = pitch if org_pitch is None else org_pitch
    rows, cols = S.grid(w, h, lw, lh)
    stride, guard = (cols, 0) if tight else (cols + PAD, GUARD)
    fstride = rows * stride + (0 if tight else GAP)
    hrec, horg = laid_out(recs, pitch, rec_gap, rec_off), laid_out(orgs, org_pitch, org_gap, org_off)
    drec, dorg = up(ctx, hrec), up(ctx, horg)
    bufs = [drec, dorg]
    total = 2 * guard + fstride * n
    dout = up(ctx, np.full(total * 96, SENTINEL, np.uint32))
    bufs.append(dout)
    kw = {}
    if keeps is not None:
        keeps = np.ascontiguousarray(keeps, np.uint8)
        dk = up(ctx, keeps)
        bufs.append(dk)
        kw.update(keep_ptr=dk.ptr, keep_stride=keeps.shape[2], keep_frame_stride=0 if keeps.shape[0] == 1 else keeps.shape[1] * keeps.shape[2])
    if noxs is not None:
        noxs = np.ascontiguousarray(noxs, np.uint8)
        dn = up(ctx, noxs)
        bufs.append(dn)
        kw.update(borders=_lib.SaoBorders(dn.ptr, noxs.shape[2], 0 if noxs.shape[0] == 1 else noxs.shape[1] * noxs.shape[2]))
    p = dev_planes(drec, n, w, h, bd, sb, pitch)
    p.src, p.frame_stride = drec.ptr + rec_off * sb, (pitch * h + rec_gap) * sb
    def call(stream=None):
        ctx.sao_stats_device(p, dorg.ptr + org_off * sb, lw, ctb_log2_h=lh, org_pitch=org_pitch * sb,
                             org_frame_stride=0 if np.asarray(orgs).shape[0] == 1 else (org_pitch * h + org_gap) * sb,
                             out_ptr=dout.ptr + guard * 384, out_stride=stride, out_frame_stride=fstride, stream=stream, **kw)
    call()
    ctx.synchronize()
    if launched is not None:
        launched += captured(call)
    raw = dout.download(total * 384).view(np.uint32).reshape(total, 96)
    assert drec.download(hrec.nbytes).tobytes() == hrec.tobytes() and dorg.download(horg.nbytes).tobytes() == horg.tobytes(), "a source plane changed"
    got = np.zeros((n, rows, cols), S.STATS_DTYPE)
    rest = raw.copy()
    for f in range(n):
        g = rest[guard + f * fstride: guard + f * fstride + rows * stride].reshape(rows, stride, 96)
        got[f] = np.ascontiguousarray(g[:, :cols]).view(S.STATS_DTYPE).reshape(rows, cols)
        g[:, :cols] = SENTINEL
    assert (rest == SENTINEL).all(), "an int32 outside the grid was written: %s" % np.argwhere(rest != SENTINEL)[:4].tolist()
    for b in bufs:
        b.free()
    return got


def same(got, want, tag):
    assert got.tobytes() == want.tobytes(), (tag, [f for f in S.STATS_DTYPE.names if not np.array_equal(got[f], want[f])],
                                             np.argwhere(got["bo_count"] != want["bo_count"])[:3].tolist())


def border_bytes(v, kind):
    rows, cols = S.grid(v["w"], v["h"], v["lw"], v["lh"])
    if kind == "absent":
        return None
    if kind == "zero":
        return np.zeros((rows, cols), np.uint8)
    if kind == "random":
        return v["nox"]
    return R.expected_nox(R.layout(rows, cols, np.random.default_rng(5), col_starts=[max(cols // 2, 1)], row_starts=[max(rows // 2, 1)],
                                   mean_run=2, tiles_across=False))


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("name", list(S.GPU_SHAPES))
def test_statistics_are_the_references(ctx, name, keep):
    v = S.vector(name)
    for kind in ("absent", "zero", "random", "layout"):
        nox = border_bytes(v, kind)
        want = S.stats_plane(v["rec"], v["org"], v["lw"], v["lh"], v["bd"], keep=v["keep"] if keep else None, nox=nox)
        ran = []
        got = gpu_stats(ctx, v["rec"][None], v["org"][None], v["bd"], v["lw"], v["lh"], keeps=v["keep"][None] if keep else None,
                        noxs=None if nox is None else nox[None], pitch=S.pitch_of(name), launched=ran)
        same(got[0], want, (name, keep, kind))
        # which kernel ran, from a capture of the same call: rows of a multiple of four samples take four samples per load
        assert ran == [("sao_stats_kernel", ("u8" if v["bd"] == 8 else "u16", int(S.pitch_of(name) % 4 == 0)))], (name, ran)


@pytest.mark.parametrize("case", ["plus", "minus", "checkerboard"])
def test_width_of_the_accumulators(ctx, case):
    """one 64 x 64 CTB at 16 bit: 4096 * 65535 = 268,431,360 in one bin, either sign"""
    yy, xx = np.mgrid[0:64, 0:64]
    rec = {"plus": np.zeros((64, 64)), "minus": np.full((64, 64), 65535), "checkerboard": ((yy + xx) & 1) * 65535}[case].astype(np.uint16)
    org = (65535 - rec).astype(np.uint16)
    want = S.stats_plane(rec, org, 6, 6, 16)
    if case != "checkerboard":
        assert abs(int(want["bo_sum"].sum())) == 268431360 and int(np.abs(want["bo_sum"]).max()) == 268431360
    else:   # every sample with both neighbours inside is a valley or a peak under the horizontal and the vertical class (its diagonal
            # neighbours equal it: no category there): 31 * 64 samples of +-65535 in each of those four bins
        eo = want["eo_count"][0, 0]
        assert (eo[:2][:, (0, 3)] == 31 * 64).all() and not eo[:2][:, (1, 2)].any() and not eo[2:].any()
        assert int(np.abs(want["eo_sum"]).max()) == 31 * 64 * 65535 and int(np.abs(want["bo_sum"]).max()) == 2048 * 65535
    same(gpu_stats(ctx, rec[None], org[None], 16, 6, 6)[0], want, case)


@pytest.mark.parametrize("bd", [8, 10])
def test_flat_plane_all_lanes_on_one_bin(ctx, bd):
    rng = np.random.default_rng(bd)
    dt = np.uint8 if bd == 8 else np.uint16
    rec = np.full((128, 128), (1 << bd) // 3, dt)
    org = rng.integers(0, 1 << bd, (128, 128)).astype(dt)
    want = S.stats_plane(rec, org, 6, 6, bd)
    assert not want["eo_count"].any() and (np.count_nonzero(want["bo_count"], axis=-1) == 1).all()
    same(gpu_stats(ctx, rec[None], org[None], bd, 6, 6)[0], want, bd)


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("tight", [False, True])
def test_batch_is_three_single_frame_calls(ctx, shared, tight):
    """3 frames; org, keep and borders each shared or per frame; the output tight or padded"""
    w, h, bd, lw, lh = 136, 72, 10, 5, 5
    rng = np.random.default_rng(17)
    rec, org = S.planes(w, h, bd, rng, n=3)
    rows, cols = S.grid(w, h, lw, lh)
    k = 1 if shared else 3
    keeps = np.stack([S.keep_map(w, h, rng) for _ in range(k)])
    noxs = rng.integers(0, 256, (k, rows, cols)).astype(np.uint8)
    orgs = org[:k]
    got = gpu_stats(ctx, rec, orgs, bd, lw, lh, keeps=keeps, noxs=noxs, tight=tight)
    for f in range(3):
        i = 0 if shared else f
        one = gpu_stats(ctx, rec[f][None], orgs[i][None], bd, lw, lh, keeps=keeps[i][None], noxs=noxs[i][None])
        same(got[f], one[0], ("single call", f))
        same(got[f], S.stats_plane(rec[f], orgs[i], lw, lh, bd, keep=keeps[i], nox=noxs[i]), ("reference", f))
    assert got[0].tobytes() != got[1].tobytes()


def poisoned(st, pad, gap):
    """(n, rows, cols) statistics -> the same read through a stride of cols + pad and a frame stride with gap entries more; every
    int32 of the padding is the sentinel: statistics that would change any choice they entered"""
    n, rows, cols = st.shape
    out = np.full((n, rows * (cols + pad) + gap, 96), SENTINEL, np.uint32)
    for f in range(n):
        out[f, : rows * (cols + pad)].reshape(rows, cols + pad, 96)[:, :cols] = np.ascontiguousarray(st[f]).view(np.uint32).reshape(rows, cols, 96)
    return out


def gpu_pick(ctx, st_a, st_b, bd, lam, *, stats_pad=0, stats_gap=0):
    """(params_a, params_b, delta_d) of (n, rows, cols) statistics, the parameter rows padded and guarded; stats_pad, stats_gap: the
    statistics too lie behind a padded stride and frame stride (poisoned())"""
    n, rows, cols = st_a.shape
    stride = cols + PAD
    fstride = rows * stride + GAP
    total = 2 * GUARD + fstride * n
    da = up(ctx, poisoned(st_a, stats_pad, stats_gap))
    db = None if st_b is None else up(ctx, poisoned(st_b, stats_pad, stats_gap))
    outs = [up(ctx, np.full(total * 6, 0xA5, np.uint8)) for _ in range(1 if st_b is None else 2)]
    dd = up(ctx, np.full(n * rows * cols + 2, -7, np.int64))
    ctx.sao_pick_device(da.ptr, cols + stats_pad, cols, rows, bd, lam, out_ptr=outs[0].ptr + GUARD * 6, out_stride=stride, n_frames=n,
                        stats_frame_stride=rows * (cols + stats_pad) + stats_gap,
                        out_frame_stride=fstride, stats_b_ptr=None if db is None else db.ptr,
                        out_b_ptr=None if db is None else outs[1].ptr + GUARD * 6, delta_d_ptr=dd.ptr + 8)
    ctx.synchronize()
    res = []
    for o in outs:
        raw = o.download(total * 6).reshape(total, 6).copy()
        p = np.zeros((n, rows, cols), ro.SAO_CTB_DTYPE)
        for f in range(n):
            g = raw[GUARD + f * fstride: GUARD + f * fstride + rows * stride].reshape(rows, stride, 6)
            p[f] = np.ascontiguousarray(g[:, :cols]).view(ro.SAO_CTB_DTYPE).reshape(rows, cols)
            g[:, :cols] = 0xA5
        assert (raw == 0xA5).all(), "a byte outside the parameter grid was written"
        res.append(p)
    d = dd.download((n * rows * cols + 2) * 8).view(np.int64)
    assert d[0] == -7 and d[-1] == -7
    for b in [da, db, dd] + outs:
        if b is not None:
            b.free()
    return res[0], (res[1] if st_b is not None else None), d[1:-1].reshape(n, rows, cols)


@pytest.fixture(scope="module")
def own_stats(ctx):
    """the GPU's own statistics of two components, two frames each, per shape"""
    out = {}
    for name in ("8b_72x40_ctb16", "12b_136x72_ctb64", "10b_96x136_ctb32x64"):
        w, h, bd, lw, lh = S.GPU_SHAPES[name]
        rng = np.random.default_rng(len(name))
        comps = []
        for _ in range(2):
            rec, org = S.planes(w, h, bd, rng, n=2)
            comps.append(gpu_stats(ctx, rec, org, bd, lw, lh, tight=True))
        out[name] = (bd, comps)
    return out


@pytest.mark.parametrize("joint", [False, True])
@pytest.mark.parametrize("lam", LAMBDAS)
def test_pick_is_the_plain_int_statement(ctx, own_stats, lam, joint):
    for name, (bd, (sa, sb)) in own_stats.items():
        pa, pb, dd = gpu_pick(ctx, sa, sb if joint else None, bd, lam)
        for f in range(sa.shape[0]):
            wa, wb, wd = S.pick_plane(sa[f], sb[f] if joint else None, bd, lam)
            assert pa[f].tobytes() == wa.tobytes(), (name, f, lam, joint)
            if joint:
                assert pb[f].tobytes() == wb.tobytes(), (name, f, lam)
            assert np.array_equal(dd[f], wd), (name, f, lam, joint)
        assert (pa["type"] != 0).any()


@pytest.mark.parametrize("name", ["8b_72x40_ctb16", "12b_136x72_ctb64", "10b_96x136_ctb32x64"])
def test_closed_loop_on_the_device(ctx, name):
    """statistics -> pick -> the existing SAO entry with the same keep map and borders, on inputs the clip never reaches: the measured
    change of the SSE is the sum of delta_d, exactly, and not positive"""
    from gpu_video_codec_amd import _lib
    v = S.vector(name, seed=3)
    w, h, bd, lw, lh = v["w"], v["h"], v["bd"], v["lw"], v["lh"]
    rows, cols = S.grid(w, h, lw, lh)
    sb = v["rec"].itemsize
    drec, dorg, ddst = up(ctx, v["rec"]), up(ctx, v["org"]), up(ctx, np.zeros_like(v["rec"]))
    dk, dn = up(ctx, v["keep"]), up(ctx, v["nox"])
    dst, dprm, ddd = ctx.alloc(rows * cols * 384), ctx.alloc(rows * cols * 6), ctx.alloc(rows * cols * 8)
    borders = _lib.SaoBorders(dn.ptr, cols, 0)
    p = dev_planes(drec, 1, w, h, bd, sb, w, dst=ddst)
    for lam in (0, 1024):
        ctx.sao_stats_device(p, dorg.ptr, lw, ctb_log2_h=lh, keep_ptr=dk.ptr, keep_stride=v["keep"].shape[1], borders=borders, out_ptr=dst.ptr,
                             out_stride=cols)
        ctx.sao_pick_device(dst.ptr, cols, cols, rows, bd, lam, out_ptr=dprm.ptr, out_stride=cols, delta_d_ptr=ddd.ptr)
        ctx.sao_device(p, dprm.ptr, cols, lw, ctb_log2_h=lh, keep_ptr=dk.ptr, keep_stride=v["keep"].shape[1], borders=borders, g4=True)
        ctx.synchronize()
        out = ddst.download(v["rec"].nbytes).view(v["rec"].dtype).reshape(h, w)
        assert out.min() > 0 and out.max() < (1 << bd) - 1
        dd = ddd.download(rows * cols * 8).view(np.int64).reshape(rows, cols)
        measured = S.sse_per_ctb(v["org"], out, lw, lh) - S.sse_per_ctb(v["org"], v["rec"], lw, lh)
        print(name, lam, "delta SSE", int(measured.sum()))
        assert np.array_equal(measured, dd) and int(dd.sum()) < 0 and (dd <= 0).all(), (name, lam)
    # the pick has one kernel and nothing to select: named here from a capture of the call above, one workgroup per CTB
    from kernel_capture import kernels_enqueued, parse_kernel
    _, k = kernels_enqueued(lambda s: ctx.sao_pick_device(dst.ptr, cols, cols, rows, bd, 1024, out_ptr=dprm.ptr, out_stride=cols,
                                                          delta_d_ptr=ddd.ptr, stream=s))
    assert [(parse_kernel(x[0]), x[1], x[2]) for x in k] == [(("sao_pick_kernel", ()), (cols, rows, 1), (64, 1, 1))], k
    for b in (drec, dorg, ddst, dk, dn, dst, dprm, ddd):
        b.free()
