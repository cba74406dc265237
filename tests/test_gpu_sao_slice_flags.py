"""slice_sao_luma_flag / slice_sao_chroma_flag in SAO estimation on the GPU through the Python layer: hevcdbk_sao_decide_device_sf and
hevcdbk_sao_slice_flags_device, byte for byte against the plain-int statement of tests/sao_slice_ref.py in every output -- parameters,
records, flag bytes and slice records -- on the vectors of tests/sao_slice_vectors.py, which tests/test_sao_slice_flags_cpu.py holds to
their conditions.  Every output and the workspace lie in pre-filled buffers with guards, padded rows and gaps between frames; EVERY
byte of the outputs is compared, the guards behind the workspace's declared size included.  The two entries against each other and
against hevcdbk_sao_decide_device_os ON THE DEVICE.  Then the chain closed: statistics -> slice flags -> SAO, the measured change of the
SSE per CTB against the record's delta_d.  PARITY UNPINNED, like the rest of SAO."""
import numpy as np
import pytest

import rext_oracle as ro
import sao_decide_ref as D
import sao_slice_ref as R
import sao_slice_vectors as V
import sao_stats_ref as S
import sao_stats_sp_ref as P
from test_gpu_sao_decide import padded_idx
from test_gpu_sao_stats import GAP, GUARD, PAD, ctx, dev_planes, up  # noqa: F401 (ctx is the module's fixture)

pytestmark = pytest.mark.gpu

POISON = 0xA5
FGUARD, FGAP = 19, 5        # bytes before and after the flag bytes, and between the frames' runs
NEW_SF, NEW_OS, MERGE = "sao_decide_new_sf_kernel", "sao_decide_new_os_kernel", "sao_decide_merge_kernel"


def gpu_run(ctx, st, name, n_slices, *, sl=None, tl=None, flags=None, mode="choose", tight=False, launched=None):
    """st: [Y] or [Y, Cb, Cr], each (n, rows, cols) statistics; sl, tl: None or (1 | n, rows, cols) uint16.  mode "choose": the choosing
    entry; "given": the decision under flags, (1 | n, n_slices) bytes; "null": the same entry without flag bytes; "os": the entry
    without flags.  Returns {"params": [per component (n, rows, cols)], "decision", and for "choose" "flags" (n, n_slices), "records"}
    after comparing every byte outside the outputs with the poison and every input with what was uploaded"""
    bl, bc, kl, kc, ll, lc, _ = V.CONFIGS[name]
    n, rows, cols = st[0].shape
    chroma = len(st) == 3
    guard = 0 if tight else GUARD
    pstride, dstride = (cols, cols) if tight else (cols + PAD, cols + PAD + 1)
    pfs, dfs = rows * pstride + (0 if tight else GAP), rows * dstride + (0 if tight else GAP + 2)
    total_p, total_d = 2 * guard + pfs * n, 2 * guard + dfs * n
    inputs = [(up(ctx, s), np.ascontiguousarray(s)) for s in st]
    outs = [up(ctx, np.full(total_p * 6, POISON, np.uint8)) for _ in st]
    ddec = up(ctx, np.full(total_d * 32, POISON, np.uint8))
    kw = dict(log2_offset_scale=kl, log2_offset_scale_chroma=kc)
    if chroma:
        kw.update(stats_cb_ptr=inputs[1][0].ptr, stats_cr_ptr=inputs[2][0].ptr, out_cb_ptr=outs[1].ptr + guard * 6, out_cr_ptr=outs[2].ptr + guard * 6,
                  bit_depth_chroma=bc, lambda_q8_chroma=lc)
    for key, a in (("slice_idx_ptr", sl), ("tile_idx_ptr", tl)):
        if a is not None:
            flat, stride, fs = padded_idx(np.asarray(a, np.uint16), 0 if tight else 3, 5)
            inputs.append((up(ctx, flat), flat))
            kw.update({key: inputs[-1][0].ptr, "idx_stride": stride, "idx_frame_stride": fs})
    extra = []
    ffs, rfs = n_slices + FGAP, n_slices + 1
    if mode == "choose":
        need = ctx.sao_slice_flags_workspace(cols, rows, n, n_slices)
        assert need % 16 == 0 and need >= n * rows * cols * 150
        dfl = up(ctx, np.full(2 * FGUARD + ffs * n, POISON, np.uint8))
        drec = up(ctx, np.full((2 + rfs * n) * 72, POISON, np.uint8))
        dws = up(ctx, np.full(need + 4096, POISON, np.uint8))
        extra = [dfl, drec, dws]
    elif mode == "given":
        fl = np.ascontiguousarray(flags, np.uint8)
        host = np.full((fl.shape[0], ffs), 0x5B, np.uint8)               # 0x5B = pair 3: a read beside a frame's bytes shows
        host[:, :n_slices] = fl
        inputs.append((up(ctx, host), host))
        kw.update(slice_flags_ptr=inputs[-1][0].ptr, n_slices=n_slices, slice_flags_frame_stride=ffs if fl.shape[0] > 1 else 0)

    def call(stream=None):
        common = dict(out_ptr=outs[0].ptr + guard * 6, out_stride=pstride, decision_ptr=ddec.ptr + guard * 32, decision_stride=dstride, n_frames=n,
                      stats_frame_stride=rows * cols, out_frame_stride=pfs, decision_frame_stride=dfs, stream=stream, **kw)
        if mode == "choose":
            ctx.sao_slice_flags_device(inputs[0][0].ptr, cols, cols, rows, bl, ll, n_slices=n_slices, slice_flags_ptr=dfl.ptr + FGUARD,
                                       slice_flags_frame_stride=ffs, slice_record_ptr=drec.ptr + 72, slice_record_frame_stride=rfs,
                                       workspace_ptr=dws.ptr, workspace_bytes=need, **common)
        elif mode == "null":                            # the Python layer never passes NULL flag bytes on: the C entry itself
            from gpu_video_codec_amd import _lib
            rc = _lib.lib().hevcdbk_sao_decide_device_sf(
                ctx.handle, inputs[0][0].ptr, kw.get("stats_cb_ptr"), kw.get("stats_cr_ptr"), cols, rows * cols, cols, rows, n, bl, bc, kl, kc, ll, lc,
                kw.get("slice_idx_ptr"), kw.get("tile_idx_ptr"), kw.get("idx_stride", 0), kw.get("idx_frame_stride", 0), common["out_ptr"],
                kw.get("out_cb_ptr"), kw.get("out_cr_ptr"), pstride, pfs, common["decision_ptr"], dstride, dfs, None, 0, 0, stream)
            assert rc == 0, rc
        else:
            ctx.sao_decide_device(inputs[0][0].ptr, cols, cols, rows, bl, ll, **common)
    call()
    ctx.synchronize()
    if launched is not None:
        from kernel_capture import kernels_enqueued, parse_kernel
        launched += [(parse_kernel(x[0])[0], x[1], x[2], x[3]) for x in kernels_enqueued(call)[1]]
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
    out = {"params": [grids(o, total_p, pstride, pfs, np.dtype(ro.SAO_CTB_DTYPE)) for o in outs], "decision": grids(ddec, total_d, dstride, dfs, D.DECISION_DTYPE)}
    if mode == "choose":
        raw = dfl.download(2 * FGUARD + ffs * n).copy()
        body = raw[FGUARD: FGUARD + ffs * n].reshape(n, ffs)
        out["flags"] = body[:, :n_slices].copy()
        body[:, :n_slices] = POISON
        assert (raw == POISON).all(), "a byte beside the flag bytes was written"
        raw = drec.download((2 + rfs * n) * 72).reshape(2 + rfs * n, 72).copy()
        body = raw[1: 1 + rfs * n].reshape(n, rfs, 72)
        out["records"] = body[:, :n_slices].copy().view(R.SLICE_RECORD_DTYPE).reshape(n, n_slices)
        body[:, :n_slices] = POISON
        assert (raw == POISON).all(), "a byte beside the slice records was written"
        assert (dws.download(need + 4096)[need:] == POISON).all(), "a byte behind the workspace's declared size was written"
    for b in [d for d, _ in inputs] + outs + [ddec] + extra:
        b.free()
    return out


def same(got, f, res, tag):
    for c, p in enumerate(got["params"]):
        assert p[f].tobytes() == res["params"][c].tobytes(), (tag, "params", c, np.argwhere(p[f] != res["params"][c])[:4].tolist())
    want = res["decision"]
    assert got["decision"][f].tobytes() == want.tobytes(), (tag, [k for k in D.DECISION_DTYPE.names if not np.array_equal(got["decision"][f][k], want[k])],
                                                           np.argwhere(got["decision"][f]["merge"] != want["merge"])[:4].tolist())
    if "flags" in got:
        assert got["flags"][f].tolist() == res["flags"], (tag, got["flags"][f].tolist(), res["flags"])
        rec = R.records(res)
        assert got["records"][f].tobytes() == rec.tobytes(), (tag, [k for k in R.SLICE_RECORD_DTYPE.names if not np.array_equal(got["records"][f][k], rec[k])])


def equal(a, b, tag):
    for x, y in zip(a["params"] + [a["decision"]], b["params"] + [b["decision"]]):
        assert x.tobytes() == y.tobytes(), tag


def stats_of(dec, idx):
    st = dec.stats(idx)
    return [s[None] for s in (st if dec.chroma else st[:1])]


def lead(a):
    return None if a is None else a[None]


def choose_launches(cols, rows, n, n_slices):
    return [("sao_slice_new_kernel", (cols, rows, n), (64, 1, 1), 0), ("sao_slice_walk_kernel", (n, 1, 1), (256, 1, 1), n_slices * 100),
            ("sao_slice_final_kernel", (-(-cols * rows // 256), n, 1), (256, 1, 1), 0)]


# ---- both entries on the grids ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chroma", [False, True])
@pytest.mark.parametrize("name", list(V.CONFIGS))
def test_both_entries_are_the_reference(ctx, name, chroma):
    """1x1 to 61x34 in slices: the choice against the reference; the decision under the flag bytes the choice wrote against the choice's
    own outputs, on the device; under other flag bytes, higher bits set, against the reference"""
    for cols, rows in D.GRIDS:
        lay = "slices" if cols * rows > 1 else "none"
        dec, idx, sl, tl, n = V.case(name, chroma, cols, rows, lay)
        st = stats_of(dec, idx)
        ran = []
        got = gpu_run(ctx, st, name, n, sl=lead(sl), launched=ran)
        same(got, 0, V.chosen(name, chroma, cols, rows, lay), (name, chroma, cols, rows))
        assert ran == choose_launches(cols, rows, 1, n), ran
        ran = []
        again = gpu_run(ctx, st, name, n, sl=lead(sl), flags=got["flags"], mode="given", launched=ran)
        equal(again, got, (name, chroma, cols, rows, "the decision under the chosen flags"))
        assert ran == [(NEW_SF, (cols, rows, 1), (64, 1, 1), 0)] + ([(MERGE, (1, 1, 1), (256, 1, 1), 0)] if cols * rows > 1 else []), ran
        flags = V.given_flags(n, cols)
        same(gpu_run(ctx, st, name, n, sl=lead(sl), flags=flags[None], mode="given"), 0, dec.decide(idx, sl, tl, [int(f) for f in flags], n),
             (name, chroma, cols, rows, "given"))


@pytest.mark.parametrize("lay", ["tiles", "both", "ctb_slices"])
def test_slices_and_tiles(ctx, lay):
    for name in ("12b_k2_unequal", "10b_lambdas_2p24_int32_ends"):
        for cols, rows in ((5, 7), (61, 34)):
            dec, idx, sl, tl, n = V.case(name, True, cols, rows, lay)
            st = stats_of(dec, idx)
            flags = V.given_flags(n, rows)
            got = gpu_run(ctx, st, name, n, sl=lead(sl), tl=lead(tl), flags=flags[None], mode="given")
            same(got, 0, dec.decide(idx, sl, tl, [int(f) for f in flags], n), (name, cols, rows, lay))
            if n <= V.MAX_SLICES:                        # one CTB per slice on 61x34 passes 600 slices: the entry under given flags alone
                same(gpu_run(ctx, st, name, n, sl=lead(sl), tl=lead(tl)), 0, V.chosen(name, True, cols, rows, lay), (name, cols, rows, lay, "choice"))


def test_ctbs_beyond_n_slices(ctx):
    for chroma in (False, True):
        dec, idx, sl, tl, n = V.case("8b_equal", chroma, 5, 7, "slices", short=True)
        got = gpu_run(ctx, stats_of(dec, idx), "8b_equal", n, sl=lead(sl))
        same(got, 0, V.chosen("8b_equal", chroma, 5, 7, "slices", short=True), chroma)
        assert not got["decision"][0][sl >= n].view(np.uint8).any()
        flags = np.full((1, n), 3, np.uint8)
        same(gpu_run(ctx, stats_of(dec, idx), "8b_equal", n, sl=lead(sl), flags=flags, mode="given"), 0, dec.decide(idx, sl, tl, 3, n), (chroma, "given"))


@pytest.mark.parametrize("name", ["12b_k2_unequal", "12b_k2_lambdas_2p20_2p24_int32_ends"])
def test_all_flags_3_and_no_flags_are_the_entry_without_flags(ctx, name):
    """on the device, the same statistics: equal bytes in every output; without flag bytes the kernels of that entry run"""
    for chroma, cols, rows, lay in ((True, 61, 34, "both"), (False, 9, 1, "slices"), (True, 5, 7, "slices")):
        dec, idx, sl, tl, n = V.case(name, chroma, cols, rows, lay)
        st = stats_of(dec, idx)
        kw = dict(sl=lead(sl), tl=lead(tl))
        base = gpu_run(ctx, st, name, n, mode="os", **kw)
        equal(gpu_run(ctx, st, name, n, flags=np.full((1, n), 3, np.uint8), mode="given", **kw), base, (name, cols, rows, "all 3"))
        equal(gpu_run(ctx, st, name, n, flags=np.full((1, n), 0xFF, np.uint8), mode="given", **kw), base, (name, cols, rows, "all 0xFF"))
        ran = []
        equal(gpu_run(ctx, st, name, n, mode="null", launched=ran, **kw), base, (name, cols, rows, "NULL"))
        assert ran == [(NEW_OS, (cols, rows, 1), (64, 1, 1), 0), (MERGE, (1, 1, 1), (256, 1, 1), 0)], ran
        same(base, 0, dec.decide(idx, sl, tl), (name, cols, rows))


@pytest.mark.parametrize("tight", [False, True])
@pytest.mark.parametrize("shared", [False, True])
def test_three_frames(ctx, shared, tight):
    """3 frames with their own statistics; the index arrays per frame or shared; for the decision under given flags the flag bytes
    per frame or shared"""
    name, rows, cols = "10b_unequal", 11, 13
    dec = V.decider(name, True)
    lay = [D.layout(rows, cols, "both")] * 3 if shared else [D.layout(rows, cols, k) for k in ("slices", "tiles", "both")]
    zero = np.zeros((rows, cols), np.uint16)
    sls = [zero if a is None else a for a, _ in lay]
    tls = [zero if b is None else b for _, b in lay]
    n = max(int(a.max()) for a in sls) + 2
    idx = [V.dealt(D.grid_of(rows, cols, 18, np.random.default_rng(40 + f), block=(2, 3)), sls[f]) for f in range(3)]
    st = [np.stack([dec.stats(i)[c] for i in idx]) for c in range(3)]
    sl, tl = np.stack(sls)[: 1 if shared else 3], np.stack(tls)[: 1 if shared else 3]
    ran = []
    got = gpu_run(ctx, st, name, n, sl=sl, tl=tl, tight=tight, launched=ran)
    assert ran == choose_launches(cols, rows, 3, n), ran
    pairs = set()
    for f in range(3):
        res = dec.choose(idx[f], sls[f], tls[f], n)
        same(got, f, res, (shared, tight, f))
        pairs |= set(res["flags"])
    assert pairs == {0, 1, 2, 3}
    flags = np.stack([V.given_flags(n, f) for f in range(1 if shared else 3)])
    given = gpu_run(ctx, st, name, n, sl=sl, tl=tl, flags=flags, mode="given", tight=tight)
    for f in range(3):
        same(given, f, dec.decide(idx[f], sls[f], tls[f], [int(b) for b in flags[0 if shared else f]], n), (shared, tight, f, "given"))
    equal(gpu_run(ctx, st, name, n, sl=sl, tl=tl, flags=got["flags"], mode="given", tight=tight), got, (shared, tight, "the chosen flags"))


def test_diagonals_longer_than_the_workgroup(ctx):
    """300 x 290 CTBs, luma alone, in 29 slices: diagonals of up to 290 CTBs, taken in two chunks of the 256 threads"""
    cols, rows, name = 300, 290, "8b_equal"
    dec = V.decider(name, False)
    sl = (np.arange(rows * cols).reshape(rows, cols) // 3000).astype(np.uint16)
    idx = V.dealt(D.grid_of(rows, cols, 18, np.random.default_rng(300)), sl)
    assert sl.max() == 28
    got = gpu_run(ctx, stats_of(dec, idx), name, 29, sl=sl[None])
    res = dec.choose(idx, sl, None, 29)
    same(got, 0, res, "300x290")
    assert set(res["flags"]) == {0, 1}


def test_600_slices(ctx):
    """n_slices of exactly 600 on the 61x34 grid: the most the choosing entry takes, 60000 bytes of LDS"""
    cols, rows, name = 61, 34, "10b_unequal"
    dec = V.decider(name, True)
    raster = np.arange(rows * cols).reshape(rows, cols)
    sl = np.minimum(raster * 600 // (rows * cols) + (raster % 7 == 0) * 2, 601).astype(np.uint16)     # 3 or 4 CTBs each, some beyond 599
    idx = V.dealt(D.grid_of(rows, cols, 18, np.random.default_rng(600)), sl)
    ran = []
    got = gpu_run(ctx, stats_of(dec, idx), name, 600, sl=sl[None], launched=ran)
    assert ran == choose_launches(cols, rows, 1, 600) and ran[1][3] == 60000, ran
    res = dec.choose(idx, sl, None, 600)
    same(got, 0, res, "600 slices")
    assert (sl >= 600).any() and set(res["flags"]) == {0, 1, 2, 3}


# ---- the chain closed on the device ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth", ["8b", "10b"])
def test_closed_loop_on_the_device(ctx, depth):
    """an NV12-shaped picture, 200x264 luma and 100x132 pairs in three slices of three CTB rows: hevcdbk_sao_stats_device (luma) and _sp
    (pairs) -> hevcdbk_sao_slice_flags_device -> hevcdbk_sao_filter_device_g4 and _sp.  In slice 0 the original's luma IS the
    reconstruction -- nothing to gain in luma --, in slice 1 its chroma.  Per CTB the measured change of the SSE, the three components
    summed, is the record's delta_d exactly; a plane of a slice whose flag came out 0 is byte for byte its input"""
    bd, sb = P.DEPTHS[depth]
    w, h, lg = 200, 264, 5
    cw, ch, clg = w // 2, h // 2, lg - 1
    rows, cols = S.grid(w, h, lg, lg)
    assert (rows, cols) == S.grid(cw, ch, clg, clg) == (9, 7)
    g = rows * cols
    rec, org = S.planes(w, h, bd, np.random.default_rng([bd, 200, 264]))
    prec, porg = P.content(cw, ch, depth, "planes", 1)
    org, porg = org.copy(), porg.copy()
    org[0, : 3 << lg] = rec[0, : 3 << lg]
    porg[0, 3 << clg: 6 << clg] = prec[0, 3 << clg: 6 << clg]
    sl = np.repeat(np.arange(3, dtype=np.uint16), 3 * cols).reshape(rows, cols)
    ll, lc = 1024, 1024
    drec, dorg, ddst = up(ctx, rec[0]), up(ctx, org[0]), up(ctx, np.zeros_like(rec[0]))
    dprec, dporg, dpdst = up(ctx, prec), up(ctx, porg), up(ctx, np.zeros_like(prec))
    dst, dprm = [ctx.alloc(g * 384) for _ in range(3)], [ctx.alloc(g * 6) for _ in range(3)]
    ddec, dsl, dfl, dsr = ctx.alloc(g * 32), up(ctx, sl), ctx.alloc(16), ctx.alloc(3 * 72)
    need = ctx.sao_slice_flags_workspace(cols, rows, 1, 3)
    dws = ctx.alloc(need)
    py = dev_planes(drec, 1, w, h, bd, sb, w, dst=ddst)
    pc = dev_planes(dprec, 1, cw, ch, bd, sb, 2 * cw, dst=dpdst)
    pc.is_chroma = 1
    sse = lambda o, p, L: S.sse_per_ctb(o, p, L, L)
    ctx.sao_stats_device(py, dorg.ptr, lg, out_ptr=dst[0].ptr, out_stride=cols)
    ctx.sao_stats_device(pc, dporg.ptr, clg, out_ptr=dst[1].ptr, out_cr_ptr=dst[2].ptr, out_stride=cols, semi_planar=True)
    ctx.sao_slice_flags_device(dst[0].ptr, cols, cols, rows, bd, ll, out_ptr=dprm[0].ptr, out_stride=cols, decision_ptr=ddec.ptr, decision_stride=cols,
                               stats_cb_ptr=dst[1].ptr, stats_cr_ptr=dst[2].ptr, out_cb_ptr=dprm[1].ptr, out_cr_ptr=dprm[2].ptr, lambda_q8_chroma=lc,
                               slice_idx_ptr=dsl.ptr, idx_stride=cols, n_slices=3, slice_flags_ptr=dfl.ptr, slice_record_ptr=dsr.ptr,
                               workspace_ptr=dws.ptr, workspace_bytes=need)
    ctx.sao_device(py, dprm[0].ptr, cols, lg, g4=True)
    ctx.sao_device(pc, dprm[1].ptr, cols, clg, semi_planar=True, params_cr_ptr=dprm[2].ptr)
    ctx.synchronize()
    out = ddst.download(rec[0].nbytes).view(rec.dtype).reshape(h, w)
    pout = dpdst.download(prec.nbytes).view(prec.dtype).reshape(ch, cw, 2)
    assert min(out.min(), pout.min()) > 0 and max(out.max(), pout.max()) < (1 << bd) - 1
    got = ddec.download(g * 32).view(D.DECISION_DTYPE).reshape(rows, cols)
    flags = dfl.download(3).tolist()
    measured = sse(org[0], out, lg) - sse(org[0], rec[0], lg)
    for c in (0, 1):
        measured = measured + sse(porg[0, :, :, c], pout[:, :, c], clg) - sse(porg[0, :, :, c], prec[0, :, :, c], clg)
    print(depth, "flags", flags, "delta SSE", int(measured.sum()), "merged", int((got["merge"] != 0).sum()), "of", g)
    assert np.array_equal(measured, got["delta_d"]) and int(measured.sum()) < 0
    assert flags == [2, 1, 3], flags
    for s, fl in enumerate(flags):
        if not fl & 1:
            assert np.array_equal(out[(3 * s) << lg: (3 * s + 3) << lg], rec[0, (3 * s) << lg: (3 * s + 3) << lg]), s
        if not fl & 2:
            assert np.array_equal(pout[(3 * s) << clg: (3 * s + 3) << clg], prec[0, (3 * s) << clg: (3 * s + 3) << clg]), s
    # the reference on the statistics the device gathered: one record per CTB
    st = [d.download(g * 384).view(S.STATS_DTYPE) for d in dst]
    ref = R.Decider([(st[0][k], st[1][k], st[2][k]) for k in range(g)], bd_luma=bd, lam_luma=ll, lam_chroma=lc)
    res = ref.choose(np.arange(g).reshape(rows, cols), sl, None, 3)
    assert res["flags"] == flags and got.tobytes() == res["decision"].tobytes()
    assert dsr.download(3 * 72).tobytes() == R.records(res).tobytes()
    for c in range(3):
        assert dprm[c].download(g * 6).tobytes() == res["params"][c].tobytes(), c
    for b in [drec, dorg, ddst, dprec, dporg, dpdst, ddec, dsl, dfl, dsr, dws] + dst + dprm:
        b.free()
