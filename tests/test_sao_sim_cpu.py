"""csrc/sao_packed.h -- the packed SAO arithmetic and the boundary-mask rule shared by the SAO pass and every fused deblocking +
SAO kernel -- compiled for the CPU by tests/sao_sim and checked without a GPU: every primitive over its whole operand range
against 8.7.3 in plain integers, and the block procedure over whole planes, bit for bit, against the by-byte reference
(sao_borders_ref.sao_plane_by_bytes) on the vectors of tests/sao_bytes_vectors.py and against the references the suite already
trusts on its existing vectors.  Every plane runs twice, surrounded by samples of 0 and of max_v: a result that depends on a
sample outside the picture differs between the two."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import batch_vectors as bvx
import h265_vectors as hv
import rext_oracle as rx
import sao_borders_ref as R
import sao_bytes_vectors as V

SIM_SRC = os.path.join(ROOT, "tests", "sao_sim", "sao_sim.cpp")
CSRC = os.path.join(ROOT, "gpu_video_codec_amd", "csrc")
FILL = 0xA5


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("sao_sim") / "libsao_sim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-I", CSRC, "-o", out, SIM_SRC])
    L = C.CDLL(out)
    L.sao_sim_plane.restype = C.c_int
    L.sao_sim_block_mask.restype = C.c_uint32
    return L


# ---- B1: the primitives, exhaustively --------------------------------------------------------------------------------------------

DEPTH_SAMPLES = sum(1 << d for d in range(8, 13))     # rec 0..max_v for bit depths 8..12
PRIMITIVES = {                                         # entry -> operand tuples, each visited in both orders of the halves
    "edge_idx8": 256 ** 3,
    "edge_idx16": 4096 * 4096 * 5,
    "apply8": 256 * 256 * 5,
    "apply16": DEPTH_SAMPLES * 256 * 5,
    "band_sel": DEPTH_SAMPLES * 32,                    # shift 3..7 = bit depth 8..12
}


@pytest.mark.parametrize("name", list(PRIMITIVES))
def test_primitive_over_its_whole_range(sim, name):
    out = (C.c_uint64 * 8)()
    getattr(sim, "sao_sim_" + name)(out)
    visited, bad = int(out[0]), int(out[1])
    print("%s: %d operand tuples, %d mismatches" % (name, visited, bad))
    assert visited == 2 * PRIMITIVES[name], (name, visited)
    assert bad == 0, (name, bad, "first mismatching operands", [int(v) for v in out[2:]])


# ---- B2: blocks over whole planes ------------------------------------------------------------------------------------------------

def run(sim, plane, params, ctb_log2, depth, *, keep=None, nox=None, border=2, force=0, nrows=8, g4=False, poison=0):
    src = np.ascontiguousarray(plane)
    h, w = src.shape
    dst = np.full((h, w), FILL * 0x0101 & (0xFF if src.itemsize == 1 else 0xFFFF), src.dtype)
    prm = np.ascontiguousarray(params, rx.SAO_CTB_DTYPE)
    k = None if keep is None else np.ascontiguousarray(keep, np.uint8)
    n = None if nox is None else np.ascontiguousarray(nox, np.uint8)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = sim.sao_sim_plane(ptr(src), ptr(dst), w, h, src.itemsize, depth, ptr(prm), prm.shape[1], ctb_log2, ptr(k), 0 if k is None else k.shape[1],
                           ptr(n), 0 if n is None else n.shape[1], border, force, nrows, int(g4), poison)
    assert rc == 0, rc
    return dst


def both_poisons(sim, want, plane, params, ctb_log2, depth, tag, **kw):
    for poison in (0, (1 << depth) - 1):
        got = run(sim, plane, params, ctb_log2, depth, poison=poison, **kw)
        assert np.array_equal(got, want), (tag, kw.get("border", 2), kw.get("force", 0), kw.get("nrows", 8), poison, int((got != want).sum()),
                                           np.argwhere(got != want)[:4].tolist())


@pytest.mark.parametrize("nrows,force", [(8, 0), (8, 1), (2, 0), (2, 1)])
@pytest.mark.parametrize("name", list(V.CASES))
def test_blocks_on_arbitrary_bytes(sim, name, nrows, force):
    """the mask of every block from saonox::block_mask as the fused kernels compute it, lanes of 8 and of 2 rows; CTBs twice as
    tall as wide as the library runs them (square CTBs, parameters and bytes rewritten); planes that end in a block of 4 columns
    / rows with the _g4 forms"""
    c = V.case(name)
    g4 = bool(c["w"] % 8 or c["h"] % 8)
    for f in range(len(c["planes"])):
        prm, nox = c["params"][f], c["nox"][f]
        if c["lh"] != c["lw"]:
            prm, nox = bvx.rows_x2(prm), bvx.nox_rows_x2(nox)
        both_poisons(sim, V.expected(name, f), c["planes"][f], prm, c["lw"], c["depth"], (name, f), keep=V.keep_of(c, f), nox=nox, nrows=nrows,
                     force=force, g4=g4)


@pytest.mark.parametrize("name", ["every_8b_ctb16", "every_10b_ctb32", "every_8b_g4_ctb8", "mixed_8b", "mixed_12b"])
def test_no_bytes_and_bytes_of_zero_are_the_border_less_result(sim, name):
    c = V.case(name)
    g4 = bool(c["w"] % 8 or c["h"] % 8)
    for f in range(len(c["planes"])):
        want = V.free(name, f)
        for nrows in (8, 2):
            for force in (0, 1):
                kw = dict(keep=V.keep_of(c, f), nrows=nrows, force=force)
                both_poisons(sim, want, c["planes"][f], c["params"][f], c["lw"], c["depth"], (name, f, "zero"), nox=np.zeros_like(c["nox"][f]), g4=g4, **kw)
                both_poisons(sim, want, c["planes"][f], c["params"][f], c["lw"], c["depth"], (name, f, "none"), nox=None, g4=g4, **kw)
                if not g4:   # the picture border alone: the form of the kernels without the operand
                    both_poisons(sim, want, c["planes"][f], c["params"][f], c["lw"], c["depth"], (name, f, "border"), border=1, **kw)


LAYOUT_CASES = [s for s in R.SMALL_SAO_CASES if s[3] <= 12]     # the packed forms take up to 12 bit


@pytest.mark.parametrize("spec", LAYOUT_CASES, ids=[s[0] for s in LAYOUT_CASES])
def test_blocks_on_the_layout_vectors(sim, spec):
    """the vectors of tests/test_gpu_sao_borders.py against the per-sample slice / tile statement"""
    c = R.sao_case(spec)
    for f in range(len(c["planes"])):
        prm, nox = c["params"][f], R.expected_nox(R.case_layout(c, f))
        if c["lh"] != c["lw"]:
            prm, nox = bvx.rows_x2(prm), bvx.nox_rows_x2(nox)
        want = R.case_expected(c, f)
        for nrows in (8, 2):
            both_poisons(sim, want, c["planes"][f], prm, c["lw"], c["depth"], (spec[0], f), keep=None if c["keeps"] is None else c["keeps"][f],
                         nox=nox, nrows=nrows)


@pytest.mark.parametrize("bd,container", [(8, 1), (8, 2), (10, 2), (12, 2)])
def test_blocks_on_the_full_range_vectors(sim, bd, container):
    """h265_vectors.sao_full_range: 0 and max_v side by side, every band position, offsets up to the int8 ends; 8-bit samples also
    in 16-bit containers"""
    rng = np.random.default_rng(900 + bd + container)
    for ctb_log2 in (4, 5, 6):
        p, prm, keep = hv.sao_full_range(bd, ctb_log2, rng, w=192, h=136)
        p = np.ascontiguousarray(p).astype(np.uint8 if container == 1 else np.uint16)
        want = rx.sao_plane(p, prm, ctb_log2, ctb_log2, bit_depth=bd, keep=keep)
        zero = np.zeros(prm.shape, np.uint8)
        for nrows in (8, 2):
            for force in (0, 1):
                both_poisons(sim, want, p, prm, ctb_log2, bd, (bd, ctb_log2), keep=keep, border=1, nrows=nrows, force=force)
                both_poisons(sim, want, p, prm, ctb_log2, bd, (bd, ctb_log2), keep=keep, nox=zero, nrows=nrows, force=force)
        # and under bytes of every value
        nox = rng.integers(0, 256, prm.shape).astype(np.uint8)
        want = R.sao_plane_by_bytes(p, prm, ctb_log2, ctb_log2, nox, bit_depth=bd, keep=keep)
        assert (want != rx.sao_plane(p, prm, ctb_log2, ctb_log2, bit_depth=bd, keep=keep)).any()
        for nrows in (8, 2):
            both_poisons(sim, want, p, prm, ctb_log2, bd, (bd, ctb_log2, "bytes"), keep=keep, nox=nox, nrows=nrows)


def test_block_mask_of_a_ctb_that_is_one_block(sim):
    """CTB == block (ctb_log2 3): every side and corner of the block is the CTB's, so the mask inside the picture is the byte"""
    for byte in range(256):
        assert sim.sao_sim_block_mask(8, byte, 16, 24, 64, 64, 3) == byte
        # a corner of a larger CTB that is not the block's corner follows the side (the diagonal neighbour lies beside, not across)
        m = sim.sao_sim_block_mask(8, byte, 16, 16, 64, 64, 4)      # the top-left block of a CTB of 16
        want = (byte & (V.L | V.U | V.UL)) | (V.UR if byte & V.U else 0) | (V.DL if byte & V.L else 0)
        assert m == want, (byte, m, want)
