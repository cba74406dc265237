"""The per-sample statement of SAO at slice / tile boundaries (tests/sao_borders_ref.py, H.265 8.7.3.2) pinned to what is already
trusted -- rext_oracle.sao_plane and the C checker's dbko_h265_sao_plane, whose picture-border rule is the same sentence -- and a
census showing that the vectors of tests/test_gpu_sao_borders.py bite.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import bs_vectors as bv
import rext_oracle as rx
import sao_borders_ref as R


@pytest.fixture(scope="module")
def h265():
    from oracle import h265 as h
    return h


def _c_sao(h265, plane, params, lw, lh, depth):
    """dbko_h265_sao_plane; CTBs twice as tall as wide as two square ones with the same parameters"""
    if lh != lw:
        params = np.repeat(params, 2, axis=0)[: -(-plane.shape[0] >> lw)]
    return h265.sao_plane(plane, params, lw, bit_depth=depth)


GEOM = [(4, 4), (5, 5), (6, 6), (5, 6)]


@pytest.mark.parametrize("depth", [8, 10, 12])
@pytest.mark.parametrize("lw,lh", GEOM)
def test_nothing_forbidden_is_the_trusted_result(h265, depth, lw, lh):
    rng = np.random.default_rng(depth + lw * 10 + lh)
    w, h = 200, 264
    plane = rng.integers(0, 1 << depth, (h, w)).astype(np.uint8 if depth == 8 else np.uint16)
    rows, cols = -(-h >> lh), -(-w >> lw)
    prm = R.edge_params(rows, cols, rng, depth)
    all_on = R.layout(rows, cols, rng, col_starts=[cols // 2], row_starts=[rows // 2], flags=1, tiles_across=True)
    for lay in (R.one_slice(rows, cols), all_on):
        got = R.sao_plane(plane, prm, lw, lh, lay, bit_depth=depth)
        assert np.array_equal(got, rx.sao_plane(plane, prm, lw, lh, bit_depth=depth))
        assert np.array_equal(got, _c_sao(h265, plane, prm, lw, lh, depth))
        assert not R.expected_nox(lay).any()


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("lw,lh", GEOM)
def test_forbidden_tiles_and_slices_are_pictures_of_their_own(h265, depth, lw, lh):
    rng = np.random.default_rng(100 + depth + lw + lh)
    rows, cols = 5, 6
    w, h = (cols << lw) - 8, (rows << lh) - 8     # the last CTB row and column are partial
    plane = rng.integers(0, 1 << depth, (h, w)).astype(np.uint8 if depth == 8 else np.uint16)
    prm = R.edge_params(rows, cols, rng, depth)
    cs, rs = [2, 5], [3]
    tile, order = R.tile_scan(rows, cols, cs, rs)
    starts = [int(order[tile == t].min()) for t in range(int(tile.max()) + 1)]     # one slice per tile
    lay = R.layout(rows, cols, rng, col_starts=cs, row_starts=rs, slice_starts=starts, flags=1, tiles_across=False)
    got = R.sao_plane(plane, prm, lw, lh, lay, bit_depth=depth)
    for (r0, r1) in ((0, 3), (3, rows)):
        for (c0, c1) in ((0, 2), (2, 5), (5, cols)):
            ys, xs = slice(r0 << lh, min(r1 << lh, h)), slice(c0 << lw, min(c1 << lw, w))
            crop = _c_sao(h265, np.ascontiguousarray(plane[ys, xs]), np.ascontiguousarray(prm[r0:r1, c0:c1]), lw, lh, depth)
            assert np.array_equal(got[ys, xs], crop), (r0, c0)
    # slices of whole CTB rows, flag 0, one tile
    lay = R.layout(rows, cols, rng, slice_starts=[2 * cols, 3 * cols], flags=0, tiles_across=True)
    got = R.sao_plane(plane, prm, lw, lh, lay, bit_depth=depth)
    for (r0, r1) in ((0, 2), (2, 3), (3, rows)):
        ys = slice(r0 << lh, min(r1 << lh, h))
        crop = _c_sao(h265, np.ascontiguousarray(plane[ys]), np.ascontiguousarray(prm[r0:r1]), lw, lh, depth)
        assert np.array_equal(got[ys], crop), r0


def test_the_later_slice_governs_the_boundary():
    """slices A < B: A's flag changes no sample along A | B, B's flag changes samples on both sides of it"""
    rng = np.random.default_rng(3)
    rows, cols, lg = 4, 4, 4
    plane = rng.integers(0, 256, (rows << lg, cols << lg)).astype(np.uint8)
    prm = R.edge_params(rows, cols, rng, p_edge=1.0)
    res = {}
    for fa in (0, 1):
        for fb in (0, 1):
            lay = R.layout(rows, cols, rng, slice_starts=[2 * cols], flags=[fa, fb], tiles_across=True)
            res[fa, fb] = R.sao_plane(plane, prm, lg, lg, lay)
    y = 2 << lg
    assert np.array_equal(res[0, 1], res[1, 1]) and np.array_equal(res[0, 0], res[1, 0])
    d = res[1, 0] != res[1, 1]
    assert d[y - 1].any() and d[y].any()                  # the last row of A and the first row of B
    assert not d[: y - 1].any() and not d[y + 1:].any()   # and nothing else


def test_only_the_rim_of_edge_offset_ctbs_changes():
    rng = np.random.default_rng(4)
    for (lw, lh) in GEOM:
        rows, cols = 6, 7
        h, w = rows << lh, cols << lw
        plane = rng.integers(0, 256, (h, w)).astype(np.uint8)
        prm = R.edge_params(rows, cols, rng)
        lay = R.layout(rows, cols, rng, col_starts=[3], row_starts=[2, 4], mean_run=3, tiles_across=False)
        got, free = R.sao_plane(plane, prm, lw, lh, lay), rx.sao_plane(plane, prm, lw, lh)
        yy, xx = np.mgrid[0:h, 0:w]
        ry, rxx = yy & ((1 << lh) - 1), xx & ((1 << lw) - 1)
        rim = (ry == 0) | (ry == (1 << lh) - 1) | (rxx == 0) | (rxx == (1 << lw) - 1)
        edge = (prm["type"] == 2)[yy >> lh, xx >> lw]
        diff = got != free
        assert diff.any() and not (diff & ~(rim & edge)).any()
        # a changed sample's CTB looks, by its class, across a border its byte forbids
        nox = R.expected_nox(lay)[yy >> lh, xx >> lw]
        cls = prm["cls"].astype(np.int64)[yy >> lh, xx >> lw]
        looks = np.zeros((h, w), np.int64)
        for c, nbs in R.HV.items():
            for (dy, dx) in nbs:
                bits = R.NOX_BITS[(dy, dx)] | (R.NOX_BITS[(dy, 0)] if dy and dx else 0) | (R.NOX_BITS[(0, dx)] if dy and dx else 0)
                looks = np.where(cls == c, looks | bits, looks)
        assert not (diff & ((nox & looks) == 0)).any()


def test_layout_of_coded_pictures_is_the_generators():
    """coded_picture_layout redraws what bs_vectors.coded_picture drew: the units' NOX flags follow from it"""
    for (w, h, seed, lg) in [(416, 240, 3, 6), (256, 192, 5, 4), (384, 256, 11, 5), (192, 128, 8, 5)]:
        flags = bv.coded_picture(w, h, seed, lg)[0].astype(np.int64)
        lay = R.coded_picture_layout(w, h, seed, lg)
        S, F, T = R.membership(lay, h // 4, w // 4, lg - 2, lg - 2)     # per 4x4 unit
        left = np.zeros_like(S, bool)
        left[:, 1:] = ((S[:, 1:] != S[:, :-1]) & (F[:, 1:] == 0)) | ((T[:, 1:] != T[:, :-1]) & (not lay["tiles_across"]))
        top = np.zeros_like(S, bool)
        top[1:] = ((S[1:] != S[:-1]) & (F[1:] == 0)) | ((T[1:] != T[:-1]) & (not lay["tiles_across"]))
        assert np.array_equal((flags & bv.U_NOX_LEFT) != 0, left) and np.array_equal((flags & bv.U_NOX_TOP) != 0, top), (w, h, seed)


def test_census_of_the_gpu_vectors():
    tot = R._empty()
    for spec in R.SMALL_SAO_CASES:
        c = R.sao_case(spec)
        for f in range(len(c["planes"])):
            lay = R.case_layout(c, f)
            cs = R.census(c["planes"][f], c["params"][f], c["lw"], c["lh"], lay, bit_depth=c["depth"])
            if R.expected_nox(lay).any():
                want = R.case_expected(c, f)
                free = rx.sao_plane(c["planes"][f], c["params"][f], c["lw"], c["lh"], bit_depth=c["depth"],
                                    keep=None if c["keeps"] is None else c["keeps"][f])
                assert (want != free).any(), (spec[0], f, "a library ignoring the operand would pass this vector")
            tot = R.merge(tot, cs)
    for cl, nbs in R.HV.items():
        for d in nbs:
            for what in ("forbidden", "allowed"):
                assert tot[(cl, R.NOX_NAMES[d], what)] >= 8, (cl, R.NOX_NAMES[d], what, tot)
    for cl in (2, 3):
        assert tot[(cl, "corner_diag_only")] >= 1 and tot[(cl, "corner_sides_only")] >= 1, tot
    assert tot["slice_only"] >= 1 and tot["tile_only"] >= 1 and tot["both"] >= 1


def test_large_vectors_bite():
    """the 3840x2160 vectors: checked on a crop around the tile / slice borders of the first CTB rows (the whole picture is the GPU test's)"""
    for spec in [s for s in R.SAO_CASES if s not in R.SMALL_SAO_CASES]:
        c = R.sao_case(spec)
        lay = R.case_layout(c, 0)
        assert R.expected_nox(lay).any()
        sub = dict(lay, slice_idx=lay["slice_idx"][:4], tile_idx=lay["tile_idx"][:4])
        crop, prm = c["planes"][0][:256], c["params"][0][:4]
        assert (R.sao_plane(crop, prm, 6, 6, sub, bit_depth=c["depth"]) != rx.sao_plane(crop, prm, 6, 6, bit_depth=c["depth"])).any()


def test_entries_refuse_bad_arguments_without_a_device():
    from gpu_video_codec_amd import _lib
    L = _lib.lib()
    planes = (_lib.DevicePlanes * 3)()
    sp = (_lib.SaoPlaneCf * 3)()
    b = _lib.SaoBorders()
    assert L.hevcdbk_sao_filter_device_nox(None, planes, None, 0, 0, 6, 6, None, 0, 0, C.byref(b), None) == _lib.ERR_ARG
    assert L.hevcdbk_h265_deblock_sao_device_nox(None, planes, 0, 1, 30, None, None, 0, 0, 6, 6, None, 0, 0, _lib.FUSED_AUTO, C.byref(b), None) == _lib.ERR_ARG
    assert L.hevcdbk_h265_deblock_sao_device_planes_nox(None, planes, 3, 1, 30, None, sp, _lib.FUSED_AUTO, C.byref(b), None) == _lib.ERR_ARG
    assert L.hevcdbk_h265_sao_borders_device(None, None, None, None, 1, 4, 4, 4, None, 4, None) == _lib.ERR_ARG
    assert C.sizeof(_lib.SaoBorders) == 24
    assert (_lib.SAO_NOX_L, _lib.SAO_NOX_R, _lib.SAO_NOX_U, _lib.SAO_NOX_D, _lib.SAO_NOX_UL, _lib.SAO_NOX_UR, _lib.SAO_NOX_DL,
            _lib.SAO_NOX_DR) == tuple(R.NOX_BITS[d] for d in ((0, -1), (0, 1), (-1, 0), (1, 0), (-1, -1), (-1, 1), (1, -1), (1, 1)))
