"""SAO statistics of a semi-planar chroma plane on the GPU through the Python layer: hevcdbk_sao_stats_device_sp, bit for bit against
tests/sao_stats_sp_ref.py (which is tests/sao_stats_ref.py per component), against the planar entry on the split planes, and closed
through hevcdbk_sao_pick_device and hevcdbk_sao_filter_device_sp.  Both outputs land in ONE pre-filled buffer with guard entries
before, between and after them, padding behind every CTB row and a gap between frames; EVERY int32 of that buffer is compared, and
the source planes and the small operands must come back as they were uploaded.  PARITY UNPINNED, like the rest of SAO."""
import numpy as np
import pytest

import rext_oracle as ro
import sao_stats_ref as S
import sao_stats_sp_ref as P
from test_gpu_sao_stats import GAP, GUARD, PAD, SENTINEL, captured, ctx, dev_planes, gpu_stats, laid_out, up  # noqa: F401 (ctx is the module's fixture)

pytestmark = pytest.mark.gpu

GPU_DEPTHS = ("8b", "10b", "14b", "16b")


def gpu_stats_sp(ctx, recs, orgs, bd, lg, *, keeps=None, noxs=None, pitch=None, org_pitch=None, rec_off=0, org_off=0, rec_gap=0, org_gap=0,
                 tight=False, launched=None):
    """recs (n, h, w, 2); orgs, keeps, noxs: (n, ...) = per frame, (1, ...) = shared, None = absent; the stride of keeps and noxs is
    their last dimension, their frame stride their last two.  pitch, org_pitch (default: pitch; default 2 w), rec_off / org_off and
    rec_gap / org_gap are in SAMPLES, as in gpu_stats.  Returns (n, 2, rows, cols) statistics, [:, 0] Cb's, after comparing every
    other int32 of the output buffer with the sentinel and every source with what was uploaded.  launched: a list that receives the
    kernels of a capture of the same call, on the same buffers"""
    from gpu_video_codec_amd import _lib
    recs, orgs = np.asarray(recs), np.asarray(orgs)
    n, h, w, _ = recs.shape
    sb = recs.itemsize
    pitch = 2 * w if pitch is None else pitch
    org_pitch = pitch if org_pitch is None else org_pitch
    rows, cols = S.grid(w, h, lg, lg)
    stride, guard = (cols, 0) if tight else (cols + PAD, GUARD)
    fstride = rows * stride + (0 if tight else GAP)
    hrec = laid_out(recs.reshape(n, h, 2 * w), pitch, rec_gap, rec_off)
    horg = laid_out(orgs.reshape(orgs.shape[0], h, 2 * w), org_pitch, org_gap, org_off)
    sources = [(up(ctx, hrec), hrec), (up(ctx, horg), horg)]
    one = guard + fstride * n                      # guard, then an array
    total = 2 * one + guard
    dout = up(ctx, np.full(total * 96, SENTINEL, np.uint32))
    kw = {}
    if keeps is not None:
        keeps = np.ascontiguousarray(keeps, np.uint8)
        sources.append((up(ctx, keeps), keeps))
        kw.update(keep_ptr=sources[-1][0].ptr, keep_stride=keeps.shape[2], keep_frame_stride=0 if keeps.shape[0] == 1 else keeps.shape[1] * keeps.shape[2])
    if noxs is not None:
        noxs = np.ascontiguousarray(noxs, np.uint8)
        sources.append((up(ctx, noxs), noxs))
        kw.update(borders=_lib.SaoBorders(sources[-1][0].ptr, noxs.shape[2], 0 if noxs.shape[0] == 1 else noxs.shape[1] * noxs.shape[2]))
    drec, dorg = sources[0][0], sources[1][0]
    p = dev_planes(drec, n, w, h, bd, sb, pitch)
    p.src, p.frame_stride, p.is_chroma = drec.ptr + rec_off * sb, (pitch * h + rec_gap) * sb, 1
    def call(stream=None):
        ctx.sao_stats_device(p, dorg.ptr + org_off * sb, lg, org_pitch=org_pitch * sb,
                             org_frame_stride=0 if orgs.shape[0] == 1 else (org_pitch * h + org_gap) * sb, out_ptr=dout.ptr + guard * 384,
                             out_cr_ptr=dout.ptr + (one + guard) * 384, out_stride=stride, out_frame_stride=fstride, semi_planar=True,
                             stream=stream, **kw)
    call()
    ctx.synchronize()
    if launched is not None:
        launched += captured(call)
    rest = dout.download(total * 384).view(np.uint32).reshape(total, 96).copy()
    for d, host in sources:
        assert d.download(host.nbytes).tobytes() == host.tobytes(), "a source or an operand changed"
    got = np.zeros((n, 2, rows, cols), S.STATS_DTYPE)
    for c in (0, 1):
        for f in range(n):
            at = c * one + guard + f * fstride
            g = rest[at: at + rows * stride].reshape(rows, stride, 96)
            got[f, c] = np.ascontiguousarray(g[:, :cols]).view(S.STATS_DTYPE).reshape(rows, cols)
            g[:, :cols] = SENTINEL
    assert (rest == SENTINEL).all(), "an int32 outside the two grids was written: %s" % np.argwhere(rest != SENTINEL)[:4].tolist()
    for d, _ in sources:
        d.free()
    dout.free()
    return got


def same(got, want, tag):
    for c, name in enumerate(("Cb", "Cr")):
        assert got[c].tobytes() == want[c].tobytes(), (tag, name, [f for f in S.STATS_DTYPE.names if not np.array_equal(got[c][f], want[c][f])],
                                                       np.argwhere(got[c]["bo_count"] != want[c]["bo_count"])[:3].tolist())


@pytest.mark.parametrize("lg", P.CTBS)
@pytest.mark.parametrize("depth", GPU_DEPTHS)
def test_statistics_are_the_references(ctx, depth, lg):
    """every plane, the no-clip and the full-range content, without and with a keep map and random border bytes"""
    bd = P.DEPTHS[depth][0]
    for (w, h) in P.PLANES:
        for kind in P.KINDS:
            rec, org = P.content(w, h, depth, kind)
            for small in (False, True):
                got = gpu_stats_sp(ctx, rec, org, bd, lg, keeps=P.keep_map(w, h) if small else None, noxs=P.border_bytes(w, h, lg) if small else None)
                same(got[0], P.reference(w, h, depth, kind, lg, small, small)[0], (w, h, depth, kind, lg, small))


@pytest.mark.parametrize("lg", P.CTBS)
@pytest.mark.parametrize("depth", ["8b", "10b"])
def test_pitch_of_2w_plus_10_samples_runs_sample_by_sample(ctx, depth, lg):
    w, h = P.PLANES[0]
    rec, org = P.content(w, h, depth, "full")
    ran = []
    got = gpu_stats_sp(ctx, rec, org, P.DEPTHS[depth][0], lg, keeps=P.keep_map(w, h), noxs=P.border_bytes(w, h, lg), pitch=2 * w + 10, launched=ran)
    assert ran == [("sao_stats_sp_kernel", ("u8" if depth == "8b" else "u16", 0))], (depth, lg, ran)
    same(got[0], P.reference(w, h, depth, "full", lg, True, True)[0], (depth, lg))


@pytest.mark.parametrize("lg", P.CTBS)
def test_every_block_kept_writes_zeros(ctx, lg):
    """nothing is counted, and still every int32 of both grids is written: gpu_stats_sp filled them with the sentinel"""
    for (w, h) in P.PLANES:
        for depth in ("8b", "10b"):
            rec, org = P.content(w, h, depth, "full")
            got = gpu_stats_sp(ctx, rec, org, P.DEPTHS[depth][0], lg, keeps=np.ones((1, -(-h // 8), -(-w // 8)), np.uint8), noxs=P.border_bytes(w, h, lg))
            assert got.shape[2:] == S.grid(w, h, lg, lg) and not got.tobytes().strip(b"\0"), (w, h, depth)


def test_width_of_the_accumulators(ctx):
    """one 32 x 32 CTB at 16 bit: rec 0 against org 65535 in Cb and the reverse in Cr -- 1024 * 65535 = 67,107,840 in one band per
    component, with opposite signs in the two outputs"""
    rec, org = np.zeros((1, 32, 32, 2), np.uint16), np.zeros((1, 32, 32, 2), np.uint16)
    org[..., 0], rec[..., 1] = 65535, 65535
    cb, cr = P.stats_pairs(rec[0], org[0], 5, 16)
    assert cb["bo_sum"][0, 0, 0] == 1024 * 65535 and cr["bo_sum"][0, 0, 31] == -1024 * 65535
    assert np.count_nonzero(cb["bo_sum"]) == 1 and np.count_nonzero(cr["bo_sum"]) == 1
    same(gpu_stats_sp(ctx, rec, org, 16, 5)[0], (cb, cr), "extremes")


@pytest.fixture(scope="module")
def aligned():
    """per depth: the planes of the load choice, their operands and the reference"""
    out = {}
    w, h, n, lg = P.ALIGN_W, P.ALIGN_H, P.ALIGN_FRAMES, P.ALIGN_LG
    for depth in ("8b", "10b"):
        rec, org = P.content(w, h, depth, "planes", n)
        out[depth] = (rec, org, P.keep_map(w, h, n), P.border_bytes(w, h, lg, n), P.reference(w, h, depth, "planes", lg, True, True, n))
    return out


@pytest.mark.parametrize("name", list(P.ALIGNMENTS))
@pytest.mark.parametrize("depth", ["8b", "10b"])
def test_load_choice(ctx, aligned, depth, name):
    """each of the six operands the load choice looks at -- base, pitch and frame stride of rec and of org -- misaligned ALONE by 1, 2
    and 3 pairs (a base also by one sample), and aligned pitches that differ between the planes: always the reference's statistics"""
    rec, org, keeps, noxs, want = aligned[depth]
    kw = P.ALIGNMENTS[name]
    assert P.takes_wide_loads(kw) == (name in P.WIDE_LOADS)            # a condition on the vectors: which side of the choice this is
    ran = []
    got = gpu_stats_sp(ctx, rec, org, P.DEPTHS[depth][0], P.ALIGN_LG, keeps=keeps, noxs=noxs, launched=ran, **kw)
    # which kernel ran, from a capture of the same call: four samples per load exactly for the layouts of WIDE_LOADS
    assert ran == [("sao_stats_sp_kernel", ("u8" if depth == "8b" else "u16", int(name in P.WIDE_LOADS)))], (depth, name, ran)
    for f in range(P.ALIGN_FRAMES):
        same(got[f], want[f], (depth, name, f))
    assert got[0].tobytes() != got[1].tobytes() and got[1].tobytes() != got[2].tobytes()


@pytest.fixture(scope="module")
def batch(ctx):
    """3 frames of 72x40 at 10 bit, their per-frame operands, and what three single-frame calls give"""
    w, h, lg = 72, 40, 4
    rec, org = P.content(w, h, "10b", "planes", 3)
    keeps, noxs = P.keep_map(w, h, 3), P.border_bytes(w, h, lg, 3)
    singles = {(f, fo, fk, fn): gpu_stats_sp(ctx, rec[f][None], org[fo][None], 10, lg, keeps=keeps[fk][None], noxs=noxs[fn][None])[0]
               for f in range(3) for (fo, fk, fn) in ((f, f, f), (f, 0, f), (f, f, 0), (0, f, f))}     # keys: frame, then whose org, keep, bytes
    return rec, org, keeps, noxs, singles


@pytest.mark.parametrize("nox_mode", ["shared", "tight", "padded"])
@pytest.mark.parametrize("keep_mode", ["shared", "tight", "padded"])
def test_batch_operands(ctx, batch, keep_mode, nox_mode):
    """keep and borders each shared, tight and padded (the excess poisoned: kept, everything forbidden); the outputs behind a padded
    stride and a frame stride with a gap: the batch is three single-frame calls"""
    rec, org, keeps, noxs, singles = batch
    k = {"shared": keeps[:1], "tight": keeps, "padded": P.padded(keeps, 3, 2, P.KEEP_POISON)}[keep_mode]
    b = {"shared": noxs[:1], "tight": noxs, "padded": P.padded(noxs, 5, 1, P.NOX_POISON)}[nox_mode]
    got = gpu_stats_sp(ctx, rec, org, 10, 4, keeps=k, noxs=b, rec_gap=16, org_gap=8)
    for f in range(3):
        fk, fn = 0 if keep_mode == "shared" else f, 0 if nox_mode == "shared" else f
        if (f, f, fk, fn) in singles:
            same(got[f], singles[(f, f, fk, fn)], ("single call", keep_mode, nox_mode, f))
        same(got[f], P.stats_pairs(rec[f], org[f], 4, 10, keep=keeps[fk], nox=noxs[fn]), ("reference", keep_mode, nox_mode, f))
    assert got[0].tobytes() != got[1].tobytes() and got[1].tobytes() != got[2].tobytes()


def test_batch_with_one_original(ctx, batch):
    rec, org, keeps, noxs, singles = batch
    got = gpu_stats_sp(ctx, rec, org[:1], 10, 4, keeps=keeps, noxs=noxs, tight=True)
    for f in range(3):
        same(got[f], singles[(f, 0, f, f)], ("single call", f))
        same(got[f], P.stats_pairs(rec[f], org[0], 4, 10, keep=keeps[f], nox=noxs[f]), ("reference", f))


@pytest.mark.parametrize("lg", P.CTBS)
@pytest.mark.parametrize("depth", ["8b", "10b"])
def test_planar_identity_on_the_device(ctx, depth, lg):
    """each output equals what hevcdbk_sao_stats_device returns ON THE DEVICE for the split plane of that component"""
    w, h = P.PLANES[0]
    bd = P.DEPTHS[depth][0]
    rec, org = P.content(w, h, depth, "full")
    keeps, noxs = P.keep_map(w, h), P.border_bytes(w, h, lg)
    got = gpu_stats_sp(ctx, rec, org, bd, lg, keeps=keeps, noxs=noxs)
    planar = [gpu_stats(ctx, np.ascontiguousarray(rec[..., c]), np.ascontiguousarray(org[..., c]), bd, lg, lg, keeps=keeps, noxs=noxs)[0] for c in (0, 1)]
    same(got[0], planar, (depth, lg))
    assert planar[0].tobytes() != planar[1].tobytes()


@pytest.mark.parametrize("joint", [True, False])
@pytest.mark.parametrize("vec", [(72, 40, "8b", 4), (96, 136, "10b", 5), (136, 72, "12b", 3)], ids=lambda v: "%dx%d_%s_ctb%d" % (v[0], v[1], v[2], 1 << v[3]))
def test_closed_loop_on_the_device(ctx, vec, joint):
    """statistics of the pair plane -> pick (joint: Cr beside Cb, one type and one edge class; else two independent calls, so that types
    differ inside a CTB and the general path of the pair SAO kernels runs) -> hevcdbk_sao_filter_device_sp with the same keep map and
    borders, on inputs the clip never reaches: per CTB the measured change of the SSE, both components summed, is delta_d exactly"""
    from gpu_video_codec_amd import _lib
    w, h, depth, lg = vec
    bd, sb = P.DEPTHS[depth]
    n = 2
    rec, org = P.content(w, h, depth, "planes", n)
    keeps, noxs = P.keep_map(w, h, n), P.border_bytes(w, h, lg, n)
    rows, cols = S.grid(w, h, lg, lg)
    g = rows * cols
    drec, dorg, ddst = up(ctx, rec), up(ctx, org), up(ctx, np.zeros_like(rec))
    dk, dn = up(ctx, keeps), up(ctx, noxs)
    dst = [ctx.alloc(n * g * 384) for _ in range(2)]
    dprm = [ctx.alloc(n * g * 6) for _ in range(2)]
    ddd = [ctx.alloc(n * g * 8) for _ in range(2)]
    borders = _lib.SaoBorders(dn.ptr, cols, g)
    kc, kr = keeps.shape[2], keeps.shape[1]
    p = dev_planes(drec, n, w, h, bd, sb, 2 * w, dst=ddst)
    p.is_chroma = 1
    mixed = 0
    for lam in (0, 1024):
        ctx.sao_stats_device(p, dorg.ptr, lg, keep_ptr=dk.ptr, keep_stride=kc, keep_frame_stride=kr * kc, borders=borders, out_ptr=dst[0].ptr,
                             out_cr_ptr=dst[1].ptr, out_stride=cols, out_frame_stride=g, semi_planar=True)
        if joint:
            ctx.sao_pick_device(dst[0].ptr, cols, cols, rows, bd, lam, out_ptr=dprm[0].ptr, out_stride=cols, n_frames=n, stats_frame_stride=g,
                                out_frame_stride=g, stats_b_ptr=dst[1].ptr, out_b_ptr=dprm[1].ptr, delta_d_ptr=ddd[0].ptr)
        else:
            for c in (0, 1):
                ctx.sao_pick_device(dst[c].ptr, cols, cols, rows, bd, lam, out_ptr=dprm[c].ptr, out_stride=cols, n_frames=n, stats_frame_stride=g,
                                    out_frame_stride=g, delta_d_ptr=ddd[c].ptr)
        ctx.sao_device(p, dprm[0].ptr, cols, lg, params_frame_stride=g, keep_ptr=dk.ptr, keep_stride=kc, keep_frame_stride=kr * kc, borders=borders,
                       semi_planar=True, params_cr_ptr=dprm[1].ptr)
        ctx.synchronize()
        out = ddst.download(rec.nbytes).view(rec.dtype).reshape(rec.shape)
        assert out.min() > 0 and out.max() < (1 << bd) - 1
        dd = ddd[0].download(n * g * 8).view(np.int64).reshape(n, rows, cols).copy()
        if not joint:
            dd += ddd[1].download(n * g * 8).view(np.int64).reshape(n, rows, cols)
        prm = [d.download(n * g * 6).view(ro.SAO_CTB_DTYPE).reshape(n, rows, cols) for d in dprm]
        measured = np.stack([sum(S.sse_per_ctb(org[f, :, :, c], out[f, :, :, c], lg, lg) - S.sse_per_ctb(org[f, :, :, c], rec[f, :, :, c], lg, lg)
                                 for c in (0, 1)) for f in range(n)])
        print(vec, joint, lam, "delta SSE", int(measured.sum()))
        assert np.array_equal(measured, dd) and int(dd.sum()) < 0 and (dd <= 0).all(), (vec, joint, lam)
        if joint:
            assert np.array_equal(prm[0]["type"], prm[1]["type"])
            edge = prm[0]["type"] == 2
            assert np.array_equal(prm[0]["cls"][edge], prm[1]["cls"][edge])       # edge CTBs: 9 and 2 per lambda on the 10- and 12-bit vectors
        else:
            mixed += int((prm[0]["type"] != prm[1]["type"]).sum())
    assert joint or mixed > 0                                          # a CTB whose components differ in type: the general path ran
    for b in [drec, dorg, ddst, dk, dn] + dst + dprm + ddd:
        b.free()
