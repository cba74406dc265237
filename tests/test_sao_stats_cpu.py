"""SAO parameter estimation without a GPU: the two entries exist everywhere they must and refuse bad operands with the documented
codes; the statement of the statistics (tests/sao_stats_ref.py) satisfies, to the last unit, the identity that ties it to the SAO
statements the suite already holds -- for random parameters and for picked ones; the picked parameters are legal syntax; and
csrc/sao_stats.h, compiled into a stand-alone program (plain and under the address and undefined-behaviour sanitizers), reproduces
the reference's integers on the planes the GPU tests use."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import rext_oracle as ro
import sao_borders_ref as R
import sao_stats_ref as S

CSRC = os.path.join(ROOT, "gpu_video_codec_amd", "csrc")
SIM_SRC = os.path.join(ROOT, "tests", "sao_stats_sim", "sao_stats_sim.cpp")
LAMBDAS = (0, 1024, 16384)


@pytest.fixture(scope="module")
def L():
    from gpu_video_codec_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


# ---- entries and codes ----------------------------------------------------------------------------------------------------------

def test_entries_are_exported_declared_and_bound(L):
    from gpu_video_codec_amd import _lib, deblock
    hdr = open(os.path.join(ROOT, "include", "hevc_deblock.h")).read()
    for sym in ("hevcdbk_sao_stats_device", "hevcdbk_sao_pick_device"):
        assert re.search(r"\b%s\s*\(" % sym, hdr), sym
        assert sym in _lib.EXPORTS and hasattr(L, sym), sym
        assert getattr(L, sym).argtypes is not None, sym
    assert "typedef struct hevcdbk_sao_stats" in hdr
    assert C.sizeof(_lib.SaoStats) == 384 and np.dtype(_lib.SAO_STATS_DTYPE).itemsize == 384
    assert np.dtype(_lib.SAO_STATS_DTYPE) == S.STATS_DTYPE
    assert callable(deblock.Context.sao_stats_device) and callable(deblock.Context.sao_pick_device)


def _planes(w=64, h=64, depth=8, sb=1, pitch=None, n=1):
    from gpu_video_codec_amd import _lib
    p = _lib.DevicePlanes()
    p.src, p.dst = 0x10000, 0
    p.pitch = w * sb if pitch is None else pitch
    p.frame_stride = p.pitch * h
    p.n_frames, p.plane_w, p.plane_h, p.bit_depth, p.sample_bytes = n, w, h, depth, sb
    return p


def test_documented_codes_without_a_device(L):
    """a context that no device stands behind (a zeroed block of memory: never looked into): every bad operand is refused with the
    documented code before the device is asked for anything"""
    from gpu_video_codec_amd import _lib
    ctx = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    ARG, DIM, UNS = _lib.ERR_ARG, _lib.ERR_DIMENSIONS, _lib.ERR_UNSUPPORTED
    ORG, OUT, KEEP = 0x20000, 0x30000, 0x40000

    def stats(p, org=ORG, org_pitch=None, lw=4, lh=4, keep=None, keep_stride=0, borders=None, out=OUT, stride=4, frame_stride=0):
        return L.hevcdbk_sao_stats_device(ctx, C.byref(p), org, p.pitch if org_pitch is None else org_pitch, p.frame_stride, lw, lh, keep,
                                          keep_stride, 0, None if borders is None else C.byref(borders), out, stride, frame_stride, None)

    assert stats(_planes(), org=None) == ARG
    assert stats(_planes(), out=None) == ARG
    assert L.hevcdbk_sao_stats_device(ctx, None, ORG, 64, 0, 4, 4, None, 0, 0, None, OUT, 4, 0, None) == ARG
    for w, h in ((62, 64), (64, 66), (4, 64), (64, 0)):            # not multiples of 4, or below 8
        assert stats(_planes(w, h), stride=8) == DIM, (w, h)
    for lw, lh in ((2, 2), (7, 7), (2, 3), (4, 6), (5, 4), (6, 7)):
        assert stats(_planes(), lw=lw, lh=lh, stride=8) == ARG, (lw, lh)
    for depth, sb in ((7, 1), (17, 2), (10, 1), (8, 3), (8, 0)):
        assert stats(_planes(depth=depth, sb=sb)) == ARG, (depth, sb)
    assert stats(_planes(), stride=3) == ARG                        # four CTB columns
    assert stats(_planes(72, 40), lw=4, lh=4, stride=4) == ARG      # five, by ceiling
    assert stats(_planes(n=2), frame_stride=15) == ARG              # the second frame's grid would overlap the first
    assert stats(_planes(), keep=KEEP, keep_stride=7) == ARG
    assert stats(_planes(), org_pitch=63) == ARG
    assert stats(_planes(pitch=63)) == ARG
    assert stats(_planes(64, 64, 10, 2, pitch=129)) == UNS          # a sample at an odd address
    assert stats(_planes(), borders=_lib.SaoBorders(None, 4, 0)) == ARG
    assert stats(_planes(), borders=_lib.SaoBorders(0x50000, 3, 0)) == ARG
    assert stats(_planes(72, 40), lw=4, lh=4, stride=5, borders=_lib.SaoBorders(0x50000, 4, 0)) == ARG

    def pick(a=OUT, b=None, stride=4, cx=4, cy=4, n=1, depth=8, lam=1024, pa=ORG, pb=None, pstride=4, pfs=0):
        return L.hevcdbk_sao_pick_device(ctx, a, b, stride, 0, cx, cy, n, depth, lam, pa, pb, pstride, pfs, None, None)

    assert pick(a=None) == ARG and pick(pa=None) == ARG
    assert pick(b=0x60000) == ARG and pick(pb=0x60000) == ARG       # Cr's statistics and Cr's parameters come together
    assert pick(depth=7) == ARG and pick(depth=17) == ARG
    assert pick(lam=(1 << 24) + 1) == ARG
    assert pick(stride=3) == ARG and pick(pstride=3) == ARG
    assert pick(n=2, pfs=15) == ARG
    assert pick(cx=0) == DIM and pick(cy=0) == DIM
    for code in (ARG, DIM, UNS):
        assert L.hevcdbk_strerror(code)


# ---- the identity ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def vectors():
    """per shape: the vector, its statistics under (keep, bytes), and those of a second component of the same geometry"""
    out = {}
    for name in S.SHAPES:
        v, v2 = S.vector(name), S.vector(name, seed=1)
        for x in (v, v2):
            x["stats"] = S.stats_plane(x["rec"], x["org"], x["lw"], x["lh"], x["bd"], keep=v["keep"], nox=v["nox"])
        out[name] = (v, v2)
    return out


def real_delta(v, x, params):
    """SSE(org, SAO(rec)) - SSE(org, rec) per CTB under the by-bytes statement of SAO; no output sample at 0 or max"""
    got = R.sao_plane_by_bytes(x["rec"], params, v["lw"], v["lh"], v["nox"], bit_depth=v["bd"], keep=v["keep"])
    assert got.min() > 0 and got.max() < (1 << v["bd"]) - 1
    return S.sse_per_ctb(x["org"], got, v["lw"], v["lh"]) - S.sse_per_ctb(x["org"], x["rec"], v["lw"], v["lh"])


@pytest.mark.parametrize("name", list(S.SHAPES))
def test_identity_for_random_parameters(vectors, name):
    v, _ = vectors[name]
    changed = 0
    for i in range(2):
        prm = ro.random_sao_params(v["w"], v["h"], v["lw"], v["lh"], np.random.default_rng(70 + i), v["bd"])
        want = real_delta(v, v, prm)
        got = S.predicted_delta(v["stats"], prm)
        print(name, i, "sum of delta", int(want.sum()))
        assert np.array_equal(got, want), (name, i, np.argwhere(got != want)[:4].tolist())
        changed += int((want != 0).sum())
    assert changed > 0


@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("name", list(S.SHAPES))
def test_picked_parameters(vectors, name, lam):
    v, v2 = vectors[name]
    M = S.max_offset(v["bd"])
    pa, _, dd = S.pick_plane(v["stats"], None, v["bd"], lam)
    assert np.array_equal(dd, real_delta(v, v, pa)), name
    assert (dd <= 0).all()
    ja, jb, jd = S.pick_plane(v["stats"], v2["stats"], v["bd"], lam)
    assert np.array_equal(jd, real_delta(v, v, ja) + real_delta(v, v2, jb)), name
    assert (jd <= 0).all()
    assert np.array_equal(ja["type"], jb["type"])
    edge = ja["type"] == 2
    assert np.array_equal(ja["cls"][edge], jb["cls"][edge])
    for p in (pa, ja, jb):
        assert (np.abs(p["offset"].astype(int)) <= M).all()
        assert set(np.unique(p["type"])) <= {0, 1, 2}
        e = p["type"] == 2
        assert (p["offset"][e][:, :2] >= 0).all() and (p["offset"][e][:, 2:] <= 0).all()      # 7.4.9.3.2
        assert (p["cls"][e] < 4).all() and (p["cls"][p["type"] == 1] < 32).all()
        assert (p["offset"][p["type"] == 0] == 0).all()
    if lam == 0:
        assert (pa["type"] != 0).any()


@pytest.mark.parametrize("name", list(S.SHAPES))
def test_census(vectors, name):
    """conditions on the vectors, not measurements: every edge bin and at least 16 bands are hit; borders and the keep map bite"""
    v, _ = vectors[name]
    st = v["stats"]
    assert (st["eo_count"].sum(axis=(0, 1)) > 0).all()
    assert int((st["bo_count"].sum(axis=(0, 1)) > 0).sum()) >= 16
    free = S.stats_plane(v["rec"], v["org"], v["lw"], v["lh"], v["bd"], keep=v["keep"])
    assert (free["eo_count"] != st["eo_count"]).any() and np.array_equal(free["bo_count"], st["bo_count"])
    unkept = S.stats_plane(v["rec"], v["org"], v["lw"], v["lh"], v["bd"], nox=v["nox"])
    assert (unkept["bo_count"] != st["bo_count"]).any()
    zero = S.stats_plane(v["rec"], v["org"], v["lw"], v["lh"], v["bd"], keep=v["keep"], nox=np.zeros_like(v["nox"]))
    assert zero.tobytes() == free.tobytes()


# ---- csrc/sao_stats.h on the CPU ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=["plain", "sanitized"])
def sim(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("sao_stats_sim_" + request.param)
    exe = str(d / "sao_stats_sim")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas"] + flags + ["-I", CSRC, "-o", exe, SIM_SRC])
    return exe, str(d)


def sim_stats(sim, v, name, *, keep, nox):
    exe, d = sim
    pitch = S.pitch_of(name)
    sb = v["rec"].itemsize

    def pitched(a):
        out = np.full((v["h"], pitch), 0x5A, a.dtype)
        out[:, : v["w"]] = a
        return out.tobytes()

    blob = np.array([v["w"], v["h"], sb, v["bd"], v["lw"], v["lh"], int(keep), int(nox), pitch], "<i4").tobytes()
    blob += pitched(v["rec"]) + pitched(v["org"]) + (v["keep"].tobytes() if keep else b"") + (v["nox"].tobytes() if nox else b"")
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    open(fin, "wb").write(blob)
    r = subprocess.run([exe, "stats", fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return np.fromfile(fout, S.STATS_DTYPE).reshape(S.grid(v["w"], v["h"], v["lw"], v["lh"]))


@pytest.mark.parametrize("name", list(S.GPU_SHAPES))
def test_block_procedure_reproduces_the_reference(sim, name):
    v = S.vector(name)
    for keep in (False, True):
        for nox in (False, True):
            want = S.stats_plane(v["rec"], v["org"], v["lw"], v["lh"], v["bd"], keep=v["keep"] if keep else None, nox=v["nox"] if nox else None)
            got = sim_stats(sim, v, name, keep=keep, nox=nox)
            assert got.tobytes() == want.tobytes(), (name, keep, nox, [f for f in S.STATS_DTYPE.names if not np.array_equal(got[f], want[f])])


@pytest.mark.parametrize("joint", [False, True])
def test_pick_procedure_reproduces_the_reference(sim, vectors, joint):
    exe, d = sim
    for name in ("8b_72x40_ctb16", "12b_136x72_ctb64"):
        v, v2 = vectors[name]
        n = v["stats"].size
        for lam in LAMBDAS:
            blob = np.array([v["bd"], lam, n, int(joint)], "<i4").tobytes() + v["stats"].tobytes() + (v2["stats"].tobytes() if joint else b"")
            fin, fout = os.path.join(d, "pick_in.bin"), os.path.join(d, "pick_out.bin")
            open(fin, "wb").write(blob)
            r = subprocess.run([exe, "pick", fin, fout], capture_output=True, text=True)
            assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
            raw = open(fout, "rb").read()
            k = 2 if joint else 1
            got = np.frombuffer(raw[: n * 6 * k], ro.SAO_CTB_DTYPE).reshape((k,) + v["stats"].shape)
            dd = np.frombuffer(raw[n * 6 * k:], "<i8").reshape(v["stats"].shape)
            pa, pb, want_dd = S.pick_plane(v["stats"], v2["stats"] if joint else None, v["bd"], lam)
            assert got[0].tobytes() == pa.tobytes(), (name, lam)
            if joint:
                assert got[1].tobytes() == pb.tobytes(), (name, lam)
            assert np.array_equal(dd, want_dd), (name, lam)
