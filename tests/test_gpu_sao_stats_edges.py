"""SAO parameter estimation on the GPU at its edges (vectors: tests/sao_stats_vectors.py; their conditions are asserted in
tests/test_sao_stats_edges_cpu.py): every CTB shape the entry accepts -- 64, 32 and 8 CTBs per 64x64 region, regions that are not
square in CTBs, two replicas per histogram -- on full-range content at every depth and container; padded and shared small
operands; every side of the vector / scalar load choice; every boundary byte; and hevcdbk_sao_pick_device on extreme, tie-prone,
sparse and plain statistics and on a hand-built table whose expected output is written out.  Every comparison is byte for byte
against tests/sao_stats_ref.py, through gpu_stats / gpu_pick of tests/test_gpu_sao_stats.py: every int32 outside the grid stays the
sentinel and the sources come back unchanged.  PARITY UNPINNED, like the rest of SAO."""
import numpy as np
import pytest

import sao_stats_ref as S
import sao_stats_vectors as V
from test_gpu_sao_stats import ctx, gpu_pick, gpu_stats, same  # noqa: F401 (ctx is the module's fixture)

pytestmark = pytest.mark.gpu

SETS = [(d, lw, lh) for d in V.DEPTHS for (lw, lh) in V.CTB_SHAPES]


def set_id(s):
    return "%s_ctb%dx%d" % (s[0], 1 << s[1], 1 << s[2])


def shape_id(s):
    return "ctb%dx%d" % (1 << s[0], 1 << s[1])


@pytest.mark.parametrize("s", SETS, ids=set_id)
def test_every_shape_full_range(ctx, s):
    depth, lw, lh = s
    for (w, h, keep) in V.shape_set(depth, lw, lh):
        rec, org = V.content(w, h, depth)
        for nox in (True, False):
            got = gpu_stats(ctx, rec, org, V.DEPTHS[depth][0], lw, lh, keeps=V.keep_map(w, h) if keep else None,
                            noxs=V.border_bytes(w, h, lw, lh) if nox else None)
            same(got[0], V.reference(w, h, depth, lw, lh, keep, nox)[0], (s, w, h, keep, nox))


@pytest.mark.parametrize("shape", V.CTB_SHAPES, ids=shape_id)
def test_every_block_kept_writes_zeros(ctx, shape):
    """nothing is counted, and still every int32 of the grid is written: gpu_stats filled it with the sentinel"""
    lw, lh = shape
    w, h = V.PLANES[0]
    rec, org = V.content(w, h, "10b")
    got = gpu_stats(ctx, rec, org, 10, lw, lh, keeps=np.ones((1, -(-h // 8), -(-w // 8)), np.uint8), noxs=V.border_bytes(w, h, lw, lh))
    assert got.shape[1:] == S.grid(w, h, lw, lh) and not got.tobytes().strip(b"\0")


@pytest.mark.parametrize("shape", [(3, 4), (4, 5), (6, 6)], ids=shape_id)
@pytest.mark.parametrize("depth", ["8b", "10b"])
def test_padded_and_shared_small_operands(ctx, depth, shape):
    """the keep map and the bytes behind strides larger than their columns and frame strides with a gap, the excess poisoned (kept /
    everything forbidden); then one keep map, then one byte array, for both frames.  The planes' frame strides have a gap too"""
    lw, lh = shape
    w, h = V.PLANES[0]
    bd = V.DEPTHS[depth][0]
    rec, org = V.content(w, h, depth, 2)
    keeps, noxs = V.keep_map(w, h, 2), V.border_bytes(w, h, lw, lh, 2)
    assert keeps[0].tobytes() != keeps[1].tobytes() and noxs[0].tobytes() != noxs[1].tobytes()
    pk, pn = V.padded(keeps, 3, 2, V.KEEP_POISON), V.padded(noxs, 5, 1, V.NOX_POISON)
    for tag, k, n, fk, fn in (("per frame", pk, pn, (0, 1), (0, 1)), ("shared keep", pk[:1], pn, (0, 0), (0, 1)),
                              ("shared bytes", pk, pn[:1], (0, 1), (0, 0)), ("tight", keeps, noxs, (0, 1), (0, 1))):
        got = gpu_stats(ctx, rec, org, bd, lw, lh, keeps=k, noxs=n, pitch=w + 4, org_pitch=w + 12, rec_gap=8, org_gap=16)
        for f in range(2):
            same(got[f], S.stats_plane(rec[f], org[f], lw, lh, bd, keep=keeps[fk[f]], nox=noxs[fn[f]]), (depth, shape, tag, f))


@pytest.fixture(scope="module")
def aligned(ctx):
    """per depth: the planes of the alignment matrix, their operands, the reference and what the all-aligned call gives"""
    out = {}
    lw, lh = V.ALIGN_SHAPE
    w, h, n = V.ALIGN_W, V.ALIGN_H, V.ALIGN_FRAMES
    for depth in ("8b", "8b_in_16", "10b"):
        bd = V.DEPTHS[depth][0]
        rec, org = V.content(w, h, depth, n)
        keeps, noxs = V.keep_map(w, h, n), V.border_bytes(w, h, lw, lh, n)
        want = np.stack([S.stats_plane(rec[f], org[f], lw, lh, bd, keep=keeps[f], nox=noxs[f]) for f in range(n)])
        got = gpu_stats(ctx, rec, org, bd, lw, lh, keeps=keeps, noxs=noxs)
        out[depth] = (rec, org, keeps, noxs, want, got)
    return out


@pytest.mark.parametrize("name", list(V.ALIGNMENTS))
@pytest.mark.parametrize("depth", ["8b", "8b_in_16", "10b"])
def test_alignment_matrix(ctx, aligned, depth, name):
    """each of the six operands the load choice looks at misaligned ALONE -- a base, a pitch, a frame stride, of rec or of org -- and
    aligned pitches that differ between the planes: the reference's statistics, and those of the all-aligned call"""
    lw, lh = V.ALIGN_SHAPE
    rec, org, keeps, noxs, want, base = aligned[depth]
    kw = V.ALIGNMENTS[name]
    quad = lambda v: v % 4 == 0                                      # noqa: E731
    vec = all(quad(kw.get(k, 0)) for k in ("rec_off", "org_off", "rec_gap", "org_gap")) and quad(kw.get("pitch", V.ALIGN_W)) and \
        quad(kw.get("org_pitch", kw.get("pitch", V.ALIGN_W)))
    assert vec == (name in V.VECTOR_LOADS)                            # a condition on the vectors: which side of the choice this is
    ran = []
    got = gpu_stats(ctx, rec, org, V.DEPTHS[depth][0], lw, lh, keeps=keeps, noxs=noxs, launched=ran, **kw)
    # which kernel ran, from a capture of the same call: four samples per load exactly for the layouts of VECTOR_LOADS
    assert ran == [("sao_stats_kernel", ("u8" if depth == "8b" else "u16", int(name in V.VECTOR_LOADS)))], (depth, name, ran)
    for f in range(V.ALIGN_FRAMES):
        same(got[f], want[f], (depth, name, "reference", f))
        same(got[f], base[f], (depth, name, "aligned call", f))
    assert got[0].tobytes() != got[1].tobytes() and got[1].tobytes() != got[2].tobytes()


@pytest.mark.parametrize("shape", list(V.EVERY_BYTE), ids=shape_id)
def test_every_byte(ctx, shape):
    lw, lh = shape
    v = V.every_byte(lw, lh)
    got = gpu_stats(ctx, v["rec"], v["org"], v["bd"], lw, lh, noxs=v["nox"])
    want = V.every_byte_reference(lw, lh)
    for f in range(len(want)):
        same(got[f], want[f], (shape, f))


def check_pick(got, want, tag):
    (pa, pb, dd), (wa, wb, wd) = got, want
    assert pa.tobytes() == wa.tobytes(), (tag, "a", pa, wa)
    assert (pb is None) == (wb is None)
    if wb is not None:
        assert pb.tobytes() == wb.tobytes(), (tag, "b", pb, wb)
    assert np.array_equal(dd, wd), (tag, dd, wd)


@pytest.mark.parametrize("bd", V.PICK_DEPTHS)
@pytest.mark.parametrize("kind", V.PICK_KINDS)
def test_pick_tables(ctx, kind, bd):
    """two frames, one component and Cb beside Cr, every lambda; the statistics tight, and behind a padded stride and frame stride"""
    for joint in (False, True):
        a, b = V.pick_table(kind, bd), V.pick_table(kind, bd, 1) if joint else None
        for lam in V.PICK_LAMBDAS:
            want = V.pick_expected(kind, bd, lam, joint)
            for pad, gap in ((0, 0), (2, 3)):
                pa, pb, dd = gpu_pick(ctx, a, b, bd, lam, stats_pad=pad, stats_gap=gap)
                for f in range(a.shape[0]):
                    check_pick((pa[f], None if pb is None else pb[f], dd[f]), want[f], (kind, bd, lam, joint, pad, f))


@pytest.mark.parametrize("name", list(V.HAND))
def test_hand_table_gives_the_literals(ctx, name):
    """the tie orders, the clamp, M per depth and the largest bin under the largest lambda, against values written out by hand from
    the header's text"""
    c = V.HAND[name]
    a, b = V.hand_stats(c["a"]), None if c["b"] is None else V.hand_stats(c["b"])
    got = gpu_pick(ctx, a, b, c["bd"], c["lam"])
    check_pick(got, (V.hand_params(c["want_a"]), None if b is None else V.hand_params(c["want_b"]), np.full((1, 1, 1), c["dd"], np.int64)), name)
