"""SAO estimation with log2_sao_offset_scale on the GPU through the Python layer: hevcdbk_sao_pick_device_os and
hevcdbk_sao_decide_device_os, byte for byte against the plain-int statement of tests/sao_scale_ref.py in every output -- parameters,
delta_d and records -- on the vectors of tests/sao_scale_vectors.py, which tests/test_sao_scale_cpu.py holds to their conditions.  Every
output of the decision lands in a pre-filled buffer with guard entries before and after, padding behind every CTB row and a gap
between frames; EVERY byte of those buffers is compared.  At a scale of 0 the _os entries against the entries without a scale on the
same device buffers.  Then the chain closed on the device at 12 bit with a scale of 2: statistics -> decide -> SAO, the measured change
of the SSE per CTB against the record's delta_d.  PARITY UNPINNED, like the rest of SAO."""
import numpy as np
import pytest

import rext_oracle as ro
import sao_decide_ref as D
import sao_decide_vectors as DV
import sao_scale_ref as R
import sao_scale_vectors as V
import sao_stats_ref as S
from test_gpu_sao_decide import padded_idx
from test_gpu_sao_stats import GAP, GUARD, PAD, ctx, dev_planes, up  # noqa: F401 (ctx is the module's fixture)

pytestmark = pytest.mark.gpu

POISON = 0xA5
SMALL = ((1, 1), (1, 9), (9, 1), (5, 7))        # columns x rows; 61 x 34 runs once per configuration, with chroma


def gpu_decide(ctx, st, depths, lambdas, scales, *, sl=None, tl=None, tight=False, launched=None):
    """st: [Y] or [Y, Cb, Cr], each (n, rows, cols) statistics; sl, tl: None or (1 | n, rows, cols) uint16.  scales: (luma, chroma) or
    None = the entry without scales.  Returns ([params per component (n, rows, cols)], decision (n, rows, cols)) after comparing every
    byte outside the grids with the poison and every input with what was uploaded"""
    (bl, bc), (ll, lc) = depths, lambdas
    n, rows, cols = st[0].shape
    chroma = len(st) == 3
    guard = 0 if tight else GUARD
    pstride, dstride = (cols, cols) if tight else (cols + PAD, cols + PAD + 1)
    pfs, dfs = rows * pstride + (0 if tight else GAP), rows * dstride + (0 if tight else GAP + 2)
    total_p, total_d = 2 * guard + pfs * n, 2 * guard + dfs * n
    inputs = [(up(ctx, s), np.ascontiguousarray(s)) for s in st]
    outs = [up(ctx, np.full(total_p * 6, POISON, np.uint8)) for _ in st]
    ddec = up(ctx, np.full(total_d * 32, POISON, np.uint8))
    kw = {}
    if chroma:
        kw.update(stats_cb_ptr=inputs[1][0].ptr, stats_cr_ptr=inputs[2][0].ptr, out_cb_ptr=outs[1].ptr + guard * 6, out_cr_ptr=outs[2].ptr + guard * 6,
                  bit_depth_chroma=bc, lambda_q8_chroma=lc)
    if scales is not None:
        kw.update(log2_offset_scale=scales[0], log2_offset_scale_chroma=scales[1])
    for key, a in (("slice_idx_ptr", sl), ("tile_idx_ptr", tl)):
        if a is not None:
            flat, stride, fs = padded_idx(np.asarray(a, np.uint16), 0 if tight else 3, 5)
            inputs.append((up(ctx, flat), flat))
            kw.update({key: inputs[-1][0].ptr, "idx_stride": stride, "idx_frame_stride": fs})

    def call(stream=None):
        ctx.sao_decide_device(inputs[0][0].ptr, cols, cols, rows, bl, ll, out_ptr=outs[0].ptr + guard * 6, out_stride=pstride,
                              decision_ptr=ddec.ptr + guard * 32, decision_stride=dstride, n_frames=n, stats_frame_stride=rows * cols,
                              out_frame_stride=pfs, decision_frame_stride=dfs, stream=stream, **kw)
    call()
    ctx.synchronize()
    if launched is not None:
        from kernel_capture import kernels_enqueued, parse_kernel
        launched += [(parse_kernel(x[0]), x[1], x[2]) for x in kernels_enqueued(call)[1]]
    for d, host in inputs:
        assert d.download(host.nbytes).tobytes() == host.tobytes(), "an input changed"

    def grids(buf, total, stride, fs, dtype):
        raw = buf.download(total * dtype.itemsize).reshape(total, dtype.itemsize).copy()
        got = np.zeros((n, rows, cols), dtype)
        for f in range(n):
            g = raw[guard + f * fs: guard + f * fs + rows * stride].reshape(rows, stride, dtype.itemsize)
            got[f] = np.ascontiguousarray(g[:, :cols]).view(dtype).reshape(rows, cols)
            g[:, :cols] = POISON
        assert (raw == POISON).all(), "a byte outside the grid was written: entries %s" % np.argwhere(raw != POISON)[:4].tolist()
        return got
    params = [grids(o, total_p, pstride, pfs, np.dtype(ro.SAO_CTB_DTYPE)) for o in outs]
    dec = grids(ddec, total_d, dstride, dfs, D.DECISION_DTYPE)
    for b in [d for d, _ in inputs] + outs + [ddec]:
        b.free()
    return params, dec


def gpu_pick(ctx, st_a, st_b, bd, lam, k, *, launched=None):
    """(params_a, params_b, delta_d) of (n, rows, cols) statistics, the parameter rows padded and guarded.  k None: the entry without a
    scale"""
    n, rows, cols = st_a.shape
    stride = cols + PAD
    fstride = rows * stride + GAP
    total = 2 * GUARD + fstride * n
    da = up(ctx, st_a)
    db = None if st_b is None else up(ctx, st_b)
    outs = [up(ctx, np.full(total * 6, POISON, np.uint8)) for _ in range(1 if st_b is None else 2)]
    dd = up(ctx, np.full(n * rows * cols + 2, -7, np.int64))

    def call(stream=None):
        ctx.sao_pick_device(da.ptr, cols, cols, rows, bd, lam, out_ptr=outs[0].ptr + GUARD * 6, out_stride=stride, n_frames=n,
                            stats_frame_stride=rows * cols, out_frame_stride=fstride, stats_b_ptr=None if db is None else db.ptr,
                            out_b_ptr=None if db is None else outs[1].ptr + GUARD * 6, delta_d_ptr=dd.ptr + 8, stream=stream, log2_offset_scale=k)
    call()
    ctx.synchronize()
    if launched is not None:
        from kernel_capture import kernels_enqueued, parse_kernel
        launched += [(parse_kernel(x[0]), x[1], x[2]) for x in kernels_enqueued(call)[1]]
    res = []
    for o in outs:
        raw = o.download(total * 6).reshape(total, 6).copy()
        p = np.zeros((n, rows, cols), ro.SAO_CTB_DTYPE)
        for f in range(n):
            g = raw[GUARD + f * fstride: GUARD + f * fstride + rows * stride].reshape(rows, stride, 6)
            p[f] = np.ascontiguousarray(g[:, :cols]).view(ro.SAO_CTB_DTYPE).reshape(rows, cols)
            g[:, :cols] = POISON
        assert (raw == POISON).all(), "a byte outside the parameter grid was written"
        res.append(p)
    d = dd.download((n * rows * cols + 2) * 8).view(np.int64)
    assert d[0] == -7 and d[-1] == -7
    for b in [da, db, dd] + outs:
        if b is not None:
            b.free()
    return res[0], (res[1] if st_b is not None else None), d[1:-1].reshape(n, rows, cols)


def same(params, dec, f, res, tag):
    for c, p in enumerate(params):
        assert p[f].tobytes() == res["params"][c].tobytes(), (tag, "params", c, np.argwhere(p[f] != res["params"][c])[:4].tolist())
    want = res["decision"]
    assert dec[f].tobytes() == want.tobytes(), (tag, [k for k in D.DECISION_DTYPE.names if not np.array_equal(dec[f][k], want[k])],
                                                np.argwhere(dec[f]["merge"] != want["merge"])[:4].tolist())


def stats_of(dec, idx):
    st = dec.stats(idx)
    return [s[None] for s in (st if dec.chroma else st[:1])]


def operands(name):
    bl, bc, kl, kc, ll, lc, _ = V.SCALE_CONFIGS[name]
    return (bl, bc), (ll, lc), (kl, kc)


# ---- the decision -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chroma", [False, True])
@pytest.mark.parametrize("name", list(V.SCALE_CONFIGS))
def test_decision_is_the_reference(ctx, name, chroma):
    for cols, rows in SMALL + (((61, 34),) if chroma else ()):
        dec, idx, _, _, res = V.case(name, chroma, cols, rows)
        ran = []
        params, got = gpu_decide(ctx, stats_of(dec, idx), *operands(name), launched=ran)
        same(params, got, 0, res, (name, chroma, cols, rows))
        # one wave per CTB, then the merge walk of the entry without scales -- none for a grid of one CTB
        want = [(("sao_decide_new_os_kernel", ()), (cols, rows, 1), (64, 1, 1))]
        assert ran == want + ([(("sao_decide_merge_kernel", ()), (1, 1, 1), (256, 1, 1))] if cols * rows > 1 else []), ran


@pytest.mark.parametrize("kind", ["slices", "tiles"])
def test_decision_under_slices_and_tiles(ctx, kind):
    for name in ("12b_12b_k2_k2", "16b_12b_k2_lambdas_2p24_int32_ends"):
        for cols, rows in ((9, 1), (5, 7)):
            dec, idx, sl, tl, res = V.case(name, True, cols, rows, kind)
            params, got = gpu_decide(ctx, stats_of(dec, idx), *operands(name), sl=None if sl is None else sl[None], tl=None if tl is None else tl[None])
            same(params, got, 0, res, (name, cols, rows, kind))


@pytest.mark.parametrize("tight", [False, True])
def test_decision_of_two_frames_with_their_own_strides(ctx, tight):
    """2 frames with their own statistics and their own slices; outputs padded (the poison proves nothing beyond the CTB columns is
    written) or tight"""
    name, rows, cols = "11b_12b_k1_k2", 7, 9
    dec = V.decider(name, True)
    idx = [D.grid_of(rows, cols, DV.N_RECORDS, np.random.default_rng(70 + f), block=(2, 3)) for f in range(2)]
    lay = [D.layout(rows, cols, k) for k in ("slices", "both")]
    zero = np.zeros((rows, cols), np.uint16)
    sl = np.stack([zero if a is None else a for a, _ in lay])
    tl = np.stack([zero if b is None else b for _, b in lay])
    st = [np.stack([dec.stats(i)[c] for i in idx]) for c in range(3)]
    params, got = gpu_decide(ctx, st, *operands(name), sl=sl, tl=tl, tight=tight)
    for f in range(2):
        same(params, got, f, dec.decide(idx[f], sl[f], tl[f]), (tight, f))
    assert got[0].tobytes() != got[1].tobytes() and (got["merge"] != 0).sum() > 10


# ---- the pick ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(V.SCALE_CONFIGS))
def test_pick_is_the_reference(ctx, name):
    """luma alone and Cb with Cr, two frames: the 5 x 7 grid and its mirror image"""
    bl, bc, kl, kc, ll, lc, _ = V.SCALE_CONFIGS[name]
    st = [np.stack([s, s[::-1, ::-1]]) for s in V.picks(name, 5, 7)["stats"]]
    ran = []
    for a, b, bd, lam, k in ((st[0], None, bl, ll, kl), (st[1], st[2], bc, lc, kc)):
        pa, pb, dd = gpu_pick(ctx, a, b, bd, lam, k, launched=ran)
        for f in range(2):
            wa, wb, wd = R.pick_plane(a[f], None if b is None else b[f], bd, lam, k)
            assert pa[f].tobytes() == wa.tobytes() and (b is None or pb[f].tobytes() == wb.tobytes()), (name, f, b is not None)
            assert np.array_equal(dd[f], wd), (name, f, b is not None)
    assert ran == [(("sao_pick_os_kernel", ()), (5, 7, 2), (64, 1, 1))] * 2, ran


def test_pick_on_the_tie_vectors(ctx):
    for name, (st_a, st_b, bd, k, lam, want) in V.tie_vectors().items():
        a = np.array(st_a, S.STATS_DTYPE).reshape(1, 1, 1)
        b = None if st_b is None else np.array(st_b, S.STATS_DTYPE).reshape(1, 1, 1)
        pa, pb, dd = gpu_pick(ctx, a, b, bd, lam, k)
        out, ref_dd, _ = R.pick_ctb(st_a, st_b, bd, lam, k)
        for p, o, w in zip((pa, pb), out, want):
            assert (int(p[0, 0, 0]["type"]), int(p[0, 0, 0]["cls"])) == w and p[0, 0, 0]["offset"].tolist() == list(o[2]), (name, p, o)
        assert int(dd[0, 0, 0]) == ref_dd, name


def test_decision_on_the_tie_vectors(ctx):
    """the tie vectors as the Cb / Cr pair (or the luma) of a decision of one CTB: the NEW triple is the pick"""
    empty = np.zeros((), S.STATS_DTYPE)
    for name, (st_a, st_b, bd, k, lam, want) in V.tie_vectors().items():
        y, cb, cr = (empty, st_a, st_b) if st_b is not None else (st_a, empty, empty)
        dec = R.Decider([(y, cb, cr)], bd_luma=bd, lam_luma=lam, chroma=True, k_luma=k)
        idx = np.zeros((1, 1), np.int64)
        params, got = gpu_decide(ctx, stats_of(dec, idx), (bd, bd), (lam, lam), (k, k))
        same(params, got, 0, dec.decide(idx), name)
        for p, w in zip(params[1:] if st_b is not None else params[:1], want):
            assert (int(p[0, 0, 0]["type"]), int(p[0, 0, 0]["cls"])) == w, name


# ---- a scale of 0 is the entries without a scale ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(DV.CONFIGS))
def test_scale_0_is_the_entries_without_a_scale(ctx, name):
    """on the device, the same statistics: equal bytes in every output, luma alone and Y + Cb + Cr, on the configurations of
    tests/sao_decide_vectors.py"""
    bl, bc, ll, lc, _ = DV.CONFIGS[name]
    for chroma in (False, True):
        for cols, rows in ((5, 7), (61, 34)) if chroma else ((9, 1),):
            dec, idx, sl, tl, res = DV.case(name, chroma, cols, rows, "slices" if cols == 5 else "none")
            kw = dict(sl=None if sl is None else sl[None], tl=None if tl is None else tl[None])
            old = gpu_decide(ctx, stats_of(dec, idx), (bl, bc), (ll, lc), None, **kw)
            new = gpu_decide(ctx, stats_of(dec, idx), (bl, bc), (ll, lc), (0, 0), **kw)
            for a, b in zip(old[0] + [old[1]], new[0] + [new[1]]):
                assert a.tobytes() == b.tobytes(), (name, chroma, cols, rows)
            same(new[0], new[1], 0, res, (name, chroma, cols, rows))
    st = [s[None] for s in DV.case(name, True, 61, 34)[0].stats(DV.case(name, True, 61, 34)[1])]
    for a, b, bd, lam in ((st[0], None, bl, ll), (st[1], st[2], bc, lc)):
        old, new = gpu_pick(ctx, a, b, bd, lam, None), gpu_pick(ctx, a, b, bd, lam, 0)
        for x, y in zip(old, new):
            assert (x is None and y is None) or x.tobytes() == y.tobytes(), (name, b is not None)


# ---- the chain closed on the device ---------------------------------------------------------------------------------------------------

def biased_planes(w, h, rng, *, comps=None):
    """12-bit (rec, org): blocky content whose coding error carries a bias of up to +-100 per 8 x 8 block -- more than 31 takes away --
    with every sample of rec at least 256 away from 0 and 4095: no offset up to 31 << 2 reaches the clip.  comps = 2: (h, w, 2) pairs"""
    shape = (h, w) if comps is None else (h, w, comps)
    bh, bw = -(-h // 8), -(-w // 8)
    blocks = lambda lo, hi: np.stack([np.kron(rng.integers(lo, hi + 1, (bh, bw)), np.ones((8, 8), np.int64))[:h, :w] for _ in range(comps or 1)], -1).reshape(shape)
    org = np.clip(blocks(400, 3695) + rng.integers(-128, 129, shape), 300, 3795)
    rec = np.clip(org + rng.integers(-20, 21, shape) + blocks(-100, 100), 256, 4095 - 256)
    return rec.astype(np.uint16), org.astype(np.uint16)


@pytest.mark.parametrize("w,h,lg", [(72, 40, 4), (68, 36, 5)])
def test_closed_loop_at_12_bit_with_a_scale_of_2(ctx, w, h, lg):
    """hevcdbk_sao_stats_device -> hevcdbk_sao_decide_device_os (luma alone, scale 2) -> the SAO entry: per CTB the measured change of
    the SSE is the record's delta_d exactly, every written offset is a multiple of 4, and the scale takes away more than a scale of 0"""
    bd, lam = 12, 4096
    rows, cols = S.grid(w, h, lg, lg)
    g = rows * cols
    rec, org = biased_planes(w, h, np.random.default_rng([w, h, 12]))
    drec, dorg, ddst = up(ctx, rec), up(ctx, org), up(ctx, np.zeros_like(rec))
    dst, dprm, ddec = ctx.alloc(g * 384), ctx.alloc(g * 6), ctx.alloc(g * 32)
    p = dev_planes(drec, 1, w, h, bd, 2, w, dst=ddst)
    total = {}
    for k in (2, 0):
        ctx.sao_stats_device(p, dorg.ptr, lg, out_ptr=dst.ptr, out_stride=cols)
        ctx.sao_decide_device(dst.ptr, cols, cols, rows, bd, lam, out_ptr=dprm.ptr, out_stride=cols, decision_ptr=ddec.ptr, decision_stride=cols,
                              log2_offset_scale=k)
        ctx.sao_device(p, dprm.ptr, cols, lg, g4=True)
        ctx.synchronize()
        out = ddst.download(rec.nbytes).view(np.uint16).reshape(h, w)
        assert out.min() > 0 and out.max() < (1 << bd) - 1
        got = ddec.download(g * 32).view(D.DECISION_DTYPE).reshape(rows, cols)
        prm = dprm.download(g * 6).view(ro.SAO_CTB_DTYPE).reshape(rows, cols)
        measured = S.sse_per_ctb(org, out, lg, lg) - S.sse_per_ctb(org, rec, lg, lg)
        total[k] = int(measured.sum())
        print(w, h, "scale", k, "delta SSE", total[k], "largest |o|", int(np.abs(prm["offset"].astype(int)).max()))
        assert np.array_equal(measured, got["delta_d"]) and total[k] < 0, (w, h, k)
        assert (prm["offset"].astype(int) % (1 << k) == 0).all() and (prm["type"] != 0).any()
        st = dst.download(g * 384).view(S.STATS_DTYPE)
        ref = R.Decider([(st[i], st[i], st[i]) for i in range(g)], bd_luma=bd, lam_luma=lam, chroma=False, k_luma=k).decide(np.arange(g).reshape(rows, cols))
        assert got.tobytes() == ref["decision"].tobytes() and prm.tobytes() == ref["params"][0].tobytes(), (w, h, k)
    assert total[2] < total[0]
    for b in (drec, dorg, ddst, dst, dprm, ddec):
        b.free()


def test_closed_loop_nv12_shaped(ctx):
    """72 x 40 luma and 36 x 20 Cb / Cr pairs at 12 bit: hevcdbk_sao_stats_device (luma) and _sp (pairs) -> the decision with scales of 2
    and 1 -> hevcdbk_sao_filter_device_g4 and _sp.  Per CTB the measured change of the SSE, the three components summed, is the
    record's delta_d; the outputs are the reference's on the device's own statistics"""
    bd, w, h, lg, ll, lc, kl, kc = 12, 72, 40, 4, 4096, 3000, 2, 1
    cw, ch, clg = w // 2, h // 2, lg - 1
    rows, cols = S.grid(w, h, lg, lg)
    assert (rows, cols) == S.grid(cw, ch, clg, clg)
    g = rows * cols
    rng = np.random.default_rng(1240)
    rec, org = biased_planes(w, h, rng)
    prec, porg = biased_planes(cw, ch, rng, comps=2)
    drec, dorg, ddst = up(ctx, rec), up(ctx, org), up(ctx, np.zeros_like(rec))
    dprec, dporg, dpdst = up(ctx, prec), up(ctx, porg), up(ctx, np.zeros_like(prec))
    dst, dprm = [ctx.alloc(g * 384) for _ in range(3)], [ctx.alloc(g * 6) for _ in range(3)]
    ddec = ctx.alloc(g * 32)
    py = dev_planes(drec, 1, w, h, bd, 2, w, dst=ddst)
    pc = dev_planes(dprec, 1, cw, ch, bd, 2, 2 * cw, dst=dpdst)
    pc.is_chroma = 1
    ctx.sao_stats_device(py, dorg.ptr, lg, out_ptr=dst[0].ptr, out_stride=cols)
    ctx.sao_stats_device(pc, dporg.ptr, clg, out_ptr=dst[1].ptr, out_cr_ptr=dst[2].ptr, out_stride=cols, semi_planar=True)
    ctx.sao_decide_device(dst[0].ptr, cols, cols, rows, bd, ll, out_ptr=dprm[0].ptr, out_stride=cols, decision_ptr=ddec.ptr, decision_stride=cols,
                          stats_cb_ptr=dst[1].ptr, stats_cr_ptr=dst[2].ptr, out_cb_ptr=dprm[1].ptr, out_cr_ptr=dprm[2].ptr, lambda_q8_chroma=lc,
                          log2_offset_scale=kl, log2_offset_scale_chroma=kc)
    ctx.sao_device(py, dprm[0].ptr, cols, lg, g4=True)
    ctx.sao_device(pc, dprm[1].ptr, cols, clg, semi_planar=True, params_cr_ptr=dprm[2].ptr)
    ctx.synchronize()
    out = ddst.download(rec.nbytes).view(np.uint16).reshape(h, w)
    pout = dpdst.download(prec.nbytes).view(np.uint16).reshape(ch, cw, 2)
    assert min(out.min(), pout.min()) > 0 and max(out.max(), pout.max()) < (1 << bd) - 1
    got = ddec.download(g * 32).view(D.DECISION_DTYPE).reshape(rows, cols)
    measured = S.sse_per_ctb(org, out, lg, lg) - S.sse_per_ctb(org, rec, lg, lg)
    for c in (0, 1):
        measured = measured + S.sse_per_ctb(porg[:, :, c], pout[:, :, c], clg, clg) - S.sse_per_ctb(porg[:, :, c], prec[:, :, c], clg, clg)
    assert np.array_equal(measured, got["delta_d"]) and int(measured.sum()) < 0
    st = [d.download(g * 384).view(S.STATS_DTYPE) for d in dst]
    ref = R.Decider([(st[0][i], st[1][i], st[2][i]) for i in range(g)], bd_luma=bd, lam_luma=ll, lam_chroma=lc, k_luma=kl, k_chroma=kc)
    res = ref.decide(np.arange(g).reshape(rows, cols))
    assert got.tobytes() == res["decision"].tobytes()
    prm = [d.download(g * 6).view(ro.SAO_CTB_DTYPE).reshape(rows, cols) for d in dprm]
    for c in range(3):
        assert prm[c].tobytes() == res["params"][c].tobytes(), c
        assert (prm[c]["offset"].astype(int) % (1 << (kl if c == 0 else kc)) == 0).all()
    assert max(int(np.abs(p["offset"].astype(int)).max()) for p in prm) > 31
    for b in [drec, dorg, ddst, dprec, dporg, dpdst, ddec] + dst + dprm:
        b.free()
