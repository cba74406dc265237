"""The SAO decision per CTB on the GPU through the Python layer: hevcdbk_sao_decide_device, byte for byte against the serial statement
of tests/sao_decide_ref.py in every output -- the three parameter arrays and the records -- on the vectors of
tests/sao_decide_vectors.py, which tests/test_sao_decide_cpu.py holds to their conditions.  Every output lands in a pre-filled buffer
with guard entries before and after, padding behind every CTB row and a gap between frames; EVERY byte of those buffers is compared.
Then the chain closed on the device: statistics (planar luma, semi-planar chroma) -> decide -> SAO, the measured change of the SSE per
CTB against the record's delta_d.  PARITY UNPINNED, like the rest of SAO."""
import numpy as np
import pytest

import rext_oracle as ro
import sao_decide_ref as D
import sao_stats_ref as S
import sao_stats_sp_ref as P
from sao_decide_vectors import CONFIGS, LAYOUTS, N_RECORDS, case, decider
from test_gpu_sao_stats import GAP, GUARD, PAD, ctx, dev_planes, up  # noqa: F401 (ctx is the module's fixture)

pytestmark = pytest.mark.gpu

POISON = 0xA5


def padded_idx(a, pad, gap):
    """(k, rows, cols) uint16 -> the same behind a stride of cols + pad and, for k > 1, a frame stride with gap entries more; 0xFFFF in
    the padding.  Returns (flat array, stride, frame stride)"""
    k, rows, cols = a.shape
    out = np.full((k, rows * (cols + pad) + gap), 0xFFFF, np.uint16)
    for f in range(k):
        out[f, : rows * (cols + pad)].reshape(rows, cols + pad)[:, :cols] = a[f]
    return out, cols + pad, 0 if k == 1 else rows * (cols + pad) + gap


def gpu_decide(ctx, st, name, *, sl=None, tl=None, tight=False, launched=None):
    """st: [Y] or [Y, Cb, Cr], each (n, rows, cols) statistics; sl, tl: None or (1 | n, rows, cols) uint16, the same leading size.
    Returns ([params per component (n, rows, cols)], decision (n, rows, cols)) after comparing every byte outside the grids with the
    poison and every input with what was uploaded"""
    bl, bc, ll, lc, _ = CONFIGS[name]
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


def same(params, dec, f, res, tag):
    for c, p in enumerate(params):
        assert p[f].tobytes() == res["params"][c].tobytes(), (tag, "params", c, np.argwhere(p[f] != res["params"][c])[:4].tolist())
    want = res["decision"]
    assert dec[f].tobytes() == want.tobytes(), (tag, [k for k in D.DECISION_DTYPE.names if not np.array_equal(dec[f][k], want[k])],
                                                np.argwhere(dec[f]["merge"] != want["merge"])[:4].tolist())


def stats_of(dec, idx):
    st = dec.stats(idx)
    return [s[None] for s in (st if dec.chroma else st[:1])]


@pytest.mark.parametrize("chroma", [False, True])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_grids_are_the_references(ctx, name, chroma):
    for cols, rows in D.GRIDS:
        dec, idx, _, _, res = case(name, chroma, cols, rows)
        ran = []
        params, got = gpu_decide(ctx, stats_of(dec, idx), name, launched=ran)
        same(params, got, 0, res, (name, chroma, cols, rows))
        # one wave per CTB, then one workgroup of 256 per frame -- none for a grid of one CTB
        want = [(("sao_decide_new_kernel", ()), (cols, rows, 1), (64, 1, 1))]
        assert ran == want + ([(("sao_decide_merge_kernel", ()), (1, 1, 1), (256, 1, 1))] if cols * rows > 1 else []), ran


@pytest.mark.parametrize("chroma", [False, True])
@pytest.mark.parametrize("kind", LAYOUTS)
def test_slices_and_tiles(ctx, kind, chroma):
    for name in ("8b_8b_equal", "10b_12b_lambdas_2p24_int32_ends"):
        for cols, rows in ((9, 1), (5, 7), (61, 34)):
            dec, idx, sl, tl, res = case(name, chroma, cols, rows, kind)
            params, got = gpu_decide(ctx, stats_of(dec, idx), name, sl=None if sl is None else sl[None], tl=None if tl is None else tl[None])
            same(params, got, 0, res, (name, chroma, cols, rows, kind))


@pytest.mark.parametrize("tight", [False, True])
@pytest.mark.parametrize("shared", [False, True])
def test_batch_of_three_frames(ctx, shared, tight):
    """3 frames with their own statistics; slice_idx / tile_idx per frame or shared (a frame stride of 0); outputs padded (the
    poison proves nothing beyond the CTB columns is written) or tight"""
    name, rows, cols = "10b_10b_unequal", 11, 13
    dec = decider(name, True)
    idx = [D.grid_of(rows, cols, N_RECORDS, np.random.default_rng(40 + f), block=(2, 3)) for f in range(3)]
    lay = [D.layout(rows, cols, "both")] * 3 if shared else [D.layout(rows, cols, k) for k in ("slices", "tiles", "both")]
    zero = np.zeros((rows, cols), np.uint16)
    sl = np.stack([zero if a is None else a for a, _ in lay])[: 1 if shared else 3]
    tl = np.stack([zero if b is None else b for _, b in lay])[: 1 if shared else 3]
    st = [np.stack([dec.stats(i)[c] for i in idx]) for c in range(3)]
    params, got = gpu_decide(ctx, st, name, sl=sl, tl=tl, tight=tight)
    merges = 0
    for f in range(3):
        res = dec.decide(idx[f], *lay[f])
        same(params, got, f, res, (shared, tight, f))
        merges += int((res["decision"]["merge"] != 0).sum())
    assert merges > 30 and got[0].tobytes() != got[1].tobytes()


def test_diagonals_longer_than_the_workgroup(ctx):
    """300 x 290 CTBs, luma alone: diagonals of up to 290 CTBs, taken in two chunks of the 256 threads, 589 diagonals"""
    dec, idx, _, _, res = case("8b_8b_equal", False, 300, 290)
    params, got = gpu_decide(ctx, stats_of(dec, idx), "8b_8b_equal")
    same(params, got, 0, res, "300x290")


@pytest.mark.parametrize("name", ["8b_12b_unequal", "10b_12b_lambdas_2p24_int32_ends"])
def test_without_candidates_the_outputs_are_the_picks(ctx, name):
    """one CTB per slice: nothing to merge with, and the parameter arrays are hevcdbk_sao_pick_device's ON THE DEVICE, byte for byte;
    with candidates, on the same statistics, no CTB's chosen J exceeds its NEW J"""
    bl, bc, ll, lc, _ = CONFIGS[name]
    cols, rows = 61, 34
    dec, idx, sl, _, _ = case(name, True, cols, rows, "ctb_slices")
    st = stats_of(dec, idx)
    params, lone = gpu_decide(ctx, st, name, sl=sl[None], tight=True)
    assert not lone["merge"].any() and not lone["cand"].any() and not lone["flag_bits"].any()
    dst = [up(ctx, s) for s in st]
    dprm = [up(ctx, np.full(rows * cols * 6, POISON, np.uint8)) for _ in st]
    ddd = [up(ctx, np.zeros(rows * cols, np.int64)) for _ in range(2)]
    ctx.sao_pick_device(dst[0].ptr, cols, cols, rows, bl, ll, out_ptr=dprm[0].ptr, out_stride=cols, delta_d_ptr=ddd[0].ptr)
    ctx.sao_pick_device(dst[1].ptr, cols, cols, rows, bc, lc, out_ptr=dprm[1].ptr, out_stride=cols, stats_b_ptr=dst[2].ptr, out_b_ptr=dprm[2].ptr,
                        delta_d_ptr=ddd[1].ptr)
    ctx.synchronize()
    for c in range(3):
        assert dprm[c].download(rows * cols * 6).tobytes() == params[c][0].tobytes(), (name, c)
    dd = sum(d.download(rows * cols * 8).view(np.int64).reshape(rows, cols) for d in ddd)
    assert np.array_equal(lone["delta_d"][0], dd)
    for b in dst + dprm + ddd:
        b.free()
    # J in Python ints from the records: NEW's costs are those of the run without candidates
    _, _, _, _, res = case(name, True, cols, rows)
    _, got = gpu_decide(ctx, st, name)
    J = lambda r, F: lc * int(r["cost_luma"]) + ll * int(r["cost_chroma"]) + ll * lc * int(F)
    worse = merged = 0
    for cy in range(rows):
        for cx in range(cols):
            r, new = got[0, cy, cx], lone[0, cy, cx]
            j, j_new = J(r, r["flag_bits"]), J(new, (int(r["cand"]) & 1) + (int(r["cand"]) >> 1))
            worse += j > j_new
            merged += r["merge"] != 0
            assert r["merge"] != 0 or j == j_new
    assert worse == 0 and merged > 100, (worse, merged)
    assert got[0].tobytes() == res["decision"].tobytes()


@pytest.mark.parametrize("depth", ["8b", "10b"])
def test_closed_loop_on_the_device(ctx, depth):
    """an NV12-shaped picture, 200x264 luma and 100x132 pairs, on content the final clip never reaches: hevcdbk_sao_stats_device (luma)
    and _sp (pairs) -> decide -> hevcdbk_sao_filter_device_g4 and _sp.  Per CTB the measured change of the SSE, the three components
    summed, is the record's delta_d exactly; the outputs are the reference's on the device's own statistics"""
    bd, sb = P.DEPTHS[depth]
    w, h, lg = 200, 264, 5
    cw, ch, clg = w // 2, h // 2, lg - 1
    rows, cols = S.grid(w, h, lg, lg)
    assert (rows, cols) == S.grid(cw, ch, clg, clg)
    g = rows * cols
    rec, org = S.planes(w, h, bd, np.random.default_rng([bd, 200, 264]))
    prec, porg = P.content(cw, ch, depth, "planes", 1)
    drec, dorg, ddst = up(ctx, rec[0]), up(ctx, org[0]), up(ctx, np.zeros_like(rec[0]))
    dprec, dporg, dpdst = up(ctx, prec), up(ctx, porg), up(ctx, np.zeros_like(prec))
    dst, dprm = [ctx.alloc(g * 384) for _ in range(3)], [ctx.alloc(g * 6) for _ in range(3)]
    ddec = ctx.alloc(g * 32)
    py = dev_planes(drec, 1, w, h, bd, sb, w, dst=ddst)
    pc = dev_planes(dprec, 1, cw, ch, bd, sb, 2 * cw, dst=dpdst)
    pc.is_chroma = 1
    sse = lambda o, p, L: S.sse_per_ctb(o, p, L, L)
    merged = 0
    # the second pair: lambdas at which this content merges (distortions grow 16-fold from 8 to 10 bit, so do the lambdas)
    for ll, lc in ((1024, 1024), (30000, 50000) if bd == 8 else (400000, 600000)):
        ctx.sao_stats_device(py, dorg.ptr, lg, out_ptr=dst[0].ptr, out_stride=cols)
        ctx.sao_stats_device(pc, dporg.ptr, clg, out_ptr=dst[1].ptr, out_cr_ptr=dst[2].ptr, out_stride=cols, semi_planar=True)
        ctx.sao_decide_device(dst[0].ptr, cols, cols, rows, bd, ll, out_ptr=dprm[0].ptr, out_stride=cols, decision_ptr=ddec.ptr, decision_stride=cols,
                              stats_cb_ptr=dst[1].ptr, stats_cr_ptr=dst[2].ptr, out_cb_ptr=dprm[1].ptr, out_cr_ptr=dprm[2].ptr, lambda_q8_chroma=lc)
        ctx.sao_device(py, dprm[0].ptr, cols, lg, g4=True)
        ctx.sao_device(pc, dprm[1].ptr, cols, clg, semi_planar=True, params_cr_ptr=dprm[2].ptr)
        ctx.synchronize()
        out = ddst.download(rec[0].nbytes).view(rec.dtype).reshape(h, w)
        pout = dpdst.download(prec.nbytes).view(prec.dtype).reshape(ch, cw, 2)
        assert min(out.min(), pout.min()) > 0 and max(out.max(), pout.max()) < (1 << bd) - 1
        got = ddec.download(g * 32).view(D.DECISION_DTYPE).reshape(rows, cols)
        measured = sse(org[0], out, lg) - sse(org[0], rec[0], lg)
        for c in (0, 1):
            measured = measured + sse(porg[0, :, :, c], pout[:, :, c], clg) - sse(porg[0, :, :, c], prec[0, :, :, c], clg)
        print(depth, ll, lc, "delta SSE", int(measured.sum()), "merged", int((got["merge"] != 0).sum()), "of", g)
        assert np.array_equal(measured, got["delta_d"]) and int(measured.sum()) < 0, (depth, ll, lc)
        # the reference on the statistics the device gathered: one record per CTB
        st = [d.download(g * 384).view(S.STATS_DTYPE) for d in dst]
        ref = D.Decider([(st[0][k], st[1][k], st[2][k]) for k in range(g)], bd_luma=bd, lam_luma=ll, lam_chroma=lc)
        res = ref.decide(np.arange(g).reshape(rows, cols))
        assert got.tobytes() == res["decision"].tobytes()
        for c in range(3):
            assert dprm[c].download(g * 6).tobytes() == res["params"][c].tobytes(), c
        merged += int((got["merge"] != 0).sum())
    assert merged > 0
    for b in [drec, dorg, ddst, dprec, dporg, dpdst, ddec] + dst + dprm:
        b.free()
