"""Per-slice deblocking offsets without a GPU: the reference of tests/slice_offsets_ref.py is tied to the oracles it is composed
of, every vector of test_gpu_slice_offsets.py is shown to bite (the census), the producer's expected bytes are derived a second
way, and the C ABI and the Python structure are checked as far as they go without a device."""
import ctypes as C

import numpy as np
import pytest

import rext_oracle as rx
import slice_offsets_ref as R
import slice_offsets_vectors as V


@pytest.fixture(scope="module")
def h265():
    from oracle import h265 as h
    return h


@pytest.fixture(scope="module")
def L():
    from gpu_video_codec_amd import _lib
    return _lib.lib()


# ---- the reference ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spec", [V.CASES[i] for i in (0, 1, 3, 6, 9, 14, 17, 22, 25, 29)], ids=lambda s: s[0])
def test_one_pair_composes_to_the_oracle(h265, spec):
    c = V.case(spec)
    for (beta, tc) in R.PAIRS + [(0, 0)]:
        got = V.expected(c, pairs=V.uniform((beta, tc)))
        if c["c_idx"] == 0 or c["cf"] == 1:
            want = h265.filter_plane(c["planes"][0], c["qp"], c["vb"], c["hb"], c_idx=c["c_idx"], bit_depth=c["depth"], qp_map=c["qp_map"],
                                     unit_log2=3, tc_offset_div2=tc, beta_offset_div2=beta, c_qp_offset=c["c_qp_offset"])
        else:
            want = rx.filter_chroma_plane(c["planes"][0], c["vb"], c["hb"], c["cf"], qp=c["qp"], qp_map=c["qp_map"], unit_log2=3,
                                          bit_depth=c["depth"], c_qp_offset=c["c_qp_offset"], tc_offset_div2=tc)
        assert np.array_equal(got, want), (spec[0], beta, tc)
        assert not np.array_equal(got, c["planes"][0])


def test_vertical_and_horizontal_passes_are_transposes():
    """as tests/test_h265_oracle.py shows it of the oracle: vertical edges with per-CTB pairs = horizontal edges of the transposed
    plane with the transposed pair array"""
    rng = np.random.default_rng(9)
    w, h, lg = 64, 96, 4
    y = V.blocky(rng, h, w, 8)
    pairs = R.ctb_pairs(R.slices_raster(h >> lg, w >> lg, 3), R.table_for(8))
    vb = np.zeros((h // 4, w // 8 + 1), np.uint8)
    vb[:, 1:w // 8] = rng.integers(0, 3, (h // 4, w // 8 - 1))
    a = R.expected(y, vb.ravel(), np.zeros((h // 8 + 1) * (w // 4), np.uint8), pairs, lg, qp=33)
    b = R.expected(np.ascontiguousarray(y.T), np.zeros((w // 4) * (h // 8 + 1), np.uint8), np.ascontiguousarray(vb.T).ravel(),
                   np.ascontiguousarray(pairs.transpose(1, 0, 2)), lg, qp=33)
    assert np.array_equal(a, b.T)
    assert not np.array_equal(a, y)
    assert not np.array_equal(a, R.expected(y, vb.ravel(), np.zeros((h // 8 + 1) * (w // 4), np.uint8), pairs, lg, qp=33, selector="p"))


# ---- the census: every vector of the GPU file differs, in every 32 x 32 cell, from what a wrong implementation would give -------

@pytest.mark.parametrize("spec", V.CASES, ids=lambda s: s[0])
def test_census_of_the_gpu_vectors(spec):
    c = V.case(spec)
    want = V.expected(c)
    assert R.cells_differ(want, V.expected(c, pairs=V.uniform((0, 0)))), "offsets 0"
    for pr in sorted({tuple(p) for p in c["tables"][0].tolist()}):
        assert R.cells_differ(want, V.expected(c, pairs=V.uniform(pr))), ("one slice's pair everywhere", pr)
    assert R.cells_differ(want, V.expected(c, selector="p")), "the CTB on the P side"


def test_census_of_the_batch_vectors():
    """the frames of a batch carry different tables: every frame differs from every other frame's pairs applied to it"""
    for spec in (V.CASES[1], V.CASES[9]):
        c = V.case(spec, frames=3)
        for f in range(3):
            want = V.expected(c, f)
            for g in range(3):
                if g != f:
                    assert R.cells_differ(want, V.expected(c, f, pairs=c["pairs"][g])), (spec[0], f, g)
            poison = V.expected(c, f, pairs=V.uniform((6, 6)))
            assert R.cells_differ(want, poison), (spec[0], f, "poison")


def test_clip_vectors_reach_both_ends_of_both_clips():
    """Clip3(0, 51, qPL + 2 beta_offset_div2) and Clip3(0, 53, qPL + 2 (bS - 1) + 2 tc_offset_div2)"""
    (b0, _b1), (t0, _t1) = V.index_range(V.clip_case(True))
    assert b0 < 0 and t0 < 0
    (_b0, b1), (_t0, t1) = V.index_range(V.clip_case(False))
    assert b1 > 51 and t1 > 53
    # the high end changes samples (tC' of index 53 against that of 50..53); at the low end beta and tC are 0 with or without the
    # offsets, so nothing is filtered: what the case shows there is that a negative index reads nothing out of range
    c = V.clip_case(False)
    assert not np.array_equal(V.expected(c), V.expected(c, pairs=V.uniform((0, 0))))
    c = V.clip_case(True)
    assert np.array_equal(V.expected(c), c["planes"][0])


# ---- the producer ----------------------------------------------------------------------------------------------------------

def test_producer_bytes_from_per_sample_membership():
    rng = np.random.default_rng(4)
    for (w, h, lg, run) in [(256, 192, 4, 5), (416, 240, 6, 3), (200, 120, 5, 2), (64, 64, 6, 1)]:
        rows, cols = -(-h >> lg), -(-w >> lg)
        sidx = R.slices_raster(rows, cols, run)
        n = int(sidx.max()) + 1
        table = rng.integers(-6, 7, (n, 2)).astype(np.int8)
        # every sample's slice, then the pair of every CTB from its samples: all samples of a CTB agree
        per_sample = np.kron(sidx, np.ones((1 << lg, 1 << lg), np.uint16))[:h, :w]
        want = np.zeros((rows, cols, 2), np.int8)
        for cy in range(rows):
            for cx in range(cols):
                blk = per_sample[cy << lg:(cy + 1) << lg, cx << lg:(cx + 1) << lg]
                assert (blk == blk[0, 0]).all()
                want[cy, cx] = table[blk[0, 0]]
        assert np.array_equal(R.ctb_pairs(sidx, table), want)
        assert np.array_equal(R.ctb_pairs_per_sample(per_sample, table, lg), want)
        short = R.ctb_pairs(sidx, table[: n // 2])
        assert np.array_equal(short[sidx < n // 2], want[sidx < n // 2]) and not short[sidx >= n // 2].any()


# ---- the C ABI and the bindings ---------------------------------------------------------------------------------------------

NEW = ["hevcdbk_h265_slice_offsets_device", "hevcdbk_h265_filter_device_sl", "hevcdbk_h265_deblock_sao_device_sl",
       "hevcdbk_h265_deblock_sao_device_planes_sl"]


def test_new_symbols_are_exported(L):
    from gpu_video_codec_amd import _lib
    for s in NEW:
        assert s in _lib.EXPORTS and hasattr(L, s), s


def test_slice_offsets_structure_has_the_c_layout():
    from gpu_video_codec_amd import _lib
    S = _lib.SliceOffsets
    assert [f[0] for f in S._fields_] == ["offs", "stride", "frame_stride", "ctb_log2"]
    # const int8_t *; unsigned; size_t; unsigned on LP64
    assert (S.offs.offset, S.stride.offset, S.frame_stride.offset, S.ctb_log2.offset, C.sizeof(S)) == (0, 8, 16, 24, 32)
    assert S.stride.size == 4 and S.ctb_log2.size == 4 and S.frame_stride.size == C.sizeof(C.c_size_t)


def _plane(w=256, h=192, chroma=False):
    from gpu_video_codec_amd import _lib
    p = _lib.DevicePlanes()
    p.src = p.dst = 0x1000
    p.pitch, p.frame_stride, p.n_frames, p.plane_w, p.plane_h = w, w * h, 1, w, h
    p.bit_depth, p.sample_bytes, p.is_chroma = 8, 1, int(chroma)
    p.vert_bs = p.hor_bs = 0x1000
    return p


def test_argument_errors_come_before_the_device(L):
    """a context that no device stands behind (a zeroed block of memory: never looked into) and operands that are wrong: every new
    entry answers HEVCDBK_ERR_ARG, not HEVCDBK_ERR_HIP, and a NULL context is refused"""
    from gpu_video_codec_amd import _lib
    ctx = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    hp = _lib.H265Params(0, 0, 0, 0)
    p = _plane()
    dst = _plane()
    dst.dst = 0x200000
    cols = 256 >> 4
    bad = [_lib.SliceOffsets(None, cols, 0, 4),          # no pairs
           _lib.SliceOffsets(0x1000, cols - 1, 0, 4),     # stride below the CTB columns
           _lib.SliceOffsets(0x1000, cols, 0, 3), _lib.SliceOffsets(0x1000, cols, 0, 7),   # CtbLog2SizeY outside 4..6
           _lib.SliceOffsets(0x1001, cols, 0, 4), _lib.SliceOffsets(0x1000, cols, 3, 4)]   # pairs that are not 16-bit words
    sp = (_lib.SaoPlaneCf * 1)()
    sp[0].params, sp[0].params_stride, sp[0].ctb_log2_w, sp[0].ctb_log2_h = 0x1000, cols, 4, 4
    for so in bad:
        assert L.hevcdbk_h265_filter_device_sl(ctx, C.byref(p), 0, 1, 30, C.byref(hp), 0, C.byref(so), None) == _lib.ERR_ARG
        assert L.hevcdbk_h265_deblock_sao_device_sl(ctx, C.byref(dst), 0, 1, 30, C.byref(hp), 0x1000, cols, 0, 4, 4, None, 0, 0, _lib.FUSED_AUTO,
                                                    None, C.byref(so), None) == _lib.ERR_ARG
        assert L.hevcdbk_h265_deblock_sao_device_planes_sl(ctx, C.byref(dst), 1, 1, 30, C.byref(hp), sp, _lib.FUSED_AUTO, None, C.byref(so),
                                                           None) == _lib.ERR_ARG
    # a chroma plane of 4:2:0: the stride is measured on the LUMA grid (128 chroma columns = 256 luma = 16 CTBs)
    pc = _plane(128, 96, True)
    assert L.hevcdbk_h265_filter_device_sl(ctx, C.byref(pc), 1, 1, 30, C.byref(hp), 0, C.byref(_lib.SliceOffsets(0x1000, 15, 0, 4)), None) == _lib.ERR_ARG
    # the entries' own argument checks still come first
    good = _lib.SliceOffsets(0x1000, cols, 0, 4)
    assert L.hevcdbk_h265_filter_device_sl(ctx, C.byref(p), 1, 1, 30, C.byref(hp), 0, C.byref(good), None) == _lib.ERR_ARG   # c_idx 1 on luma
    assert L.hevcdbk_h265_filter_device_sl(ctx, C.byref(p), 0, 1, 30, C.byref(hp), 77, C.byref(good), None) == _lib.ERR_ARG  # no such kernel
    assert L.hevcdbk_h265_deblock_sao_device_sl(ctx, C.byref(dst), 0, 1, 30, C.byref(hp), 0x1000, cols, 0, 4, 4, None, 0, 0, 9, None,
                                                C.byref(good), None) == _lib.ERR_ARG
    for so in (good, None):
        assert L.hevcdbk_h265_filter_device_sl(None, C.byref(p), 0, 1, 30, C.byref(hp), 0, None if so is None else C.byref(so), None) == _lib.ERR_ARG
    # the producer
    assert L.hevcdbk_h265_slice_offsets_device(None, 0x1000, 4, 0x1000, 2, 4, 4, 0x1000, 4, None) == _lib.ERR_ARG
    assert L.hevcdbk_h265_slice_offsets_device(ctx, None, 4, 0x1000, 2, 4, 4, 0x1000, 4, None) == _lib.ERR_ARG
    assert L.hevcdbk_h265_slice_offsets_device(ctx, 0x1000, 3, 0x1000, 2, 4, 4, 0x1000, 4, None) == _lib.ERR_ARG
    assert L.hevcdbk_h265_slice_offsets_device(ctx, 0x1000, 4, 0x1000, 2, 4, 4, 0x1000, 3, None) == _lib.ERR_ARG
    assert L.hevcdbk_h265_slice_offsets_device(ctx, 0x1000, 4, None, 2, 4, 4, 0x1000, 4, None) == _lib.ERR_ARG
    assert L.hevcdbk_h265_slice_offsets_device(ctx, 0x1000, 4, 0x1000, 2, 0, 4, 0x1000, 4, None) == _lib.ERR_ARG
    assert L.hevcdbk_h265_slice_offsets_device(ctx, 0x1000, 4, 0x1000, 2, 4, 4, 0x1001, 4, None) == _lib.ERR_ARG


def test_python_keyword_needs_the_spec_exact_mode():
    from gpu_video_codec_amd import _lib, deblock
    ctx = deblock.Context.__new__(deblock.Context)   # no device: the check comes before any call
    ctx.handle = None
    with pytest.raises(ValueError):
        ctx.deblock_sao_device_planes([_plane()], 30, [(0x1000, 16, 4)], slice_offsets=_lib.SliceOffsets(0x1000, 16, 0, 4))


# ---- the kernels' rule and per-block procedure, on the CPU -----------------------------------------------------------------------

@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    import os
    import subprocess
    from conftest import ROOT
    out = str(tmp_path_factory.mktemp("sl_sim") / "libsl_sim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", out,
                           os.path.join(ROOT, "tests", "sl_sim", "sl_sim.cpp")])
    L = C.CDLL(out)
    L.sl_sim_filter_plane.restype = C.c_int
    return L


def _run_sim(sim, c, pairs, packed, f=0):
    out = np.ascontiguousarray(c["planes"][f]).copy()
    h, w = out.shape
    m = c["qp_map"]
    pr = np.ascontiguousarray(pairs, np.int8)
    rc = sim.sl_sim_filter_plane(out.ctypes.data_as(C.c_void_p), w, h, C.c_long(out.strides[0]), out.itemsize, c["depth"],
                                 0 if c["c_idx"] == 0 else c["cf"], c["vb"].ctypes.data_as(C.c_void_p), c["hb"].ctypes.data_as(C.c_void_p),
                                 int(c["qp"]), None if m is None else m.ctypes.data_as(C.c_void_p), 0 if m is None else m.shape[1], 3,
                                 c["c_qp_offset"], pr.ctypes.data_as(C.c_void_p), pr.shape[1], V.CTB_LOG2, packed)
    assert rc == 0
    return out


@pytest.mark.parametrize("spec", V.CASES, ids=lambda s: s[0])
def test_kernel_rule_matches_the_reference(sim, spec):
    """the 32-bit kernel's form, the packed kernels' per-lane values and (luma) their table rows"""
    c = V.case(spec)
    want = V.expected(c)
    for packed in ((0, 1, 2) if c["c_idx"] == 0 else (0, 1)):
        got = _run_sim(sim, c, c["pairs"][0], packed)
        assert np.array_equal(got, want), (spec[0], packed, int((got != want).sum()))


def test_kernel_rule_at_the_clips(sim):
    for low in (True, False):
        for depth in (8, 10):
            c = V.clip_case(low, depth)
            want = V.expected(c)
            for packed in (0, 1, 2):
                assert np.array_equal(_run_sim(sim, c, c["pairs"][0], packed), want), (low, depth, packed)
