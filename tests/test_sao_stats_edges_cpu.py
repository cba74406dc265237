"""SAO parameter estimation at its edges, without a GPU: the conditions the vectors of tests/sao_stats_vectors.py must meet, asserted
from the reference alone -- they are conditions, not measurements; csrc/sao_stats.h as a stand-alone program (plain and under the
address and undefined-behaviour sanitizers) against tests/sao_stats_ref.py on every CTB shape, depth and container, on every
boundary byte and on every synthetic statistics table; and the hand-built table, whose literals the reference must give too.
Every comparison is exact."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import rext_oracle as ro
import sao_bytes_vectors as B
import sao_stats_ref as S
import sao_stats_vectors as V

CSRC = os.path.join(ROOT, "gpu_video_codec_amd", "csrc")
SIM_SRC = os.path.join(ROOT, "tests", "sao_stats_sim", "sao_stats_sim.cpp")
SETS = [(d, lw, lh) for d in V.DEPTHS for (lw, lh) in V.CTB_SHAPES]


def set_id(s):
    return "%s_ctb%dx%d" % (s[0], 1 << s[1], 1 << s[2])


# ---- conditions on the vectors ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("s", SETS, ids=set_id)
def test_conditions_on_a_set(s):
    """per (shape, depth): all 32 bands and all 16 edge bins are hit, some |org - rec| is the whole range, sums of both signs occur;
    and the keep map and the bytes bite"""
    depth, lw, lh = s
    max_v = (1 << V.DEPTHS[depth][0]) - 1
    bands, edges, neg, pos, full = np.zeros(32, np.int64), np.zeros((4, 4), np.int64), 0, 0, 0
    for (w, h, keep) in V.shape_set(depth, lw, lh):
        st = V.reference(w, h, depth, lw, lh, keep, True)
        bands += st["bo_count"].sum(axis=(0, 1, 2))
        edges += st["eo_count"].sum(axis=(0, 1, 2))
        neg += int((st["bo_sum"] < 0).sum()) + int((st["eo_sum"] < 0).sum())
        pos += int((st["bo_sum"] > 0).sum()) + int((st["eo_sum"] > 0).sum())
        rec, org = V.content(w, h, depth)
        assert rec.dtype.itemsize == V.DEPTHS[depth][1] and int(rec.max()) <= max_v and int(org.max()) <= max_v
        full += int((np.abs(org.astype(np.int64) - rec.astype(np.int64)) == max_v).sum())
    assert (bands > 0).all() and (edges > 0).all(), (bands, edges)
    assert full > 0 and neg > 0 and pos > 0
    w, h = V.PLANES[0]
    rec = V.content(w, h, depth)[0][0].astype(np.int64)
    for k in range(8, w, 8):        # 0 against max across every column and row that is a multiple of 8, hence of 64 and of every CTB size
        assert ((rec[:, k - 1] == max_v) & (rec[:, k] == 0)).any(), k
    for k in range(8, h, 8):
        assert ((rec[k - 1] == max_v) & (rec[k] == 0)).any(), k
    both, free, unkept = (V.reference(w, h, depth, lw, lh, *kn) for kn in ((True, True), (True, False), (False, True)))
    assert (both["eo_count"] != free["eo_count"]).any() and (both["bo_count"] != unkept["bo_count"]).any()


@pytest.mark.parametrize("shape", list(V.EVERY_BYTE), ids=lambda s: "ctb%dx%d" % (1 << s[0], 1 << s[1]))
def test_every_byte_every_relevant_bit_bites(shape):
    """every byte value sits on a CTB with all eight neighbours; for each of them, every class k and every bit RELEVANT[k], turning
    the bit over changes the CTB's eo_count[k] -- and no other bit does, and nothing changes a band.  A CTB's statistics depend on
    no byte but its own (the reference's definition), so one run with the bit turned over in EVERY byte decides it for all"""
    lw, lh = shape
    v = V.every_byte(lw, lh)
    assert sorted(v["nox"][:, 1:-1, 1:-1].ravel().tolist()) == list(range(256))
    base = V.every_byte_reference(lw, lh)
    assert (base["eo_count"][:, 1:-1, 1:-1].sum(axis=-1) > 0).all()
    for b in range(8):
        flipped = V.every_byte_reference(lw, lh, 1 << b)
        assert np.array_equal(flipped["bo_count"], base["bo_count"]) and np.array_equal(flipped["bo_sum"], base["bo_sum"])
        for k in range(4):
            changed = (flipped["eo_count"][..., k, :] != base["eo_count"][..., k, :]).any(axis=-1)[:, 1:-1, 1:-1]
            assert changed.all() if B.RELEVANT[k] & (1 << b) else not changed.any(), (shape, b, k, int(changed.sum()))


def test_pick_census():
    """over the random tables, alone and jointly: every type, a wrapped band position and an offset of magnitude M occur"""
    for joint in (False, True):
        c = V.pick_census(joint)
        print("pick census, %s:" % ("Cb beside Cr" if joint else "one component"), c)
        assert all(n > 0 for n in c.values()), (joint, c)


def test_pick_tables_are_what_they_claim():
    for bd in V.PICK_DEPTHS:
        t = V.pick_table("extreme", bd)
        n = np.concatenate([t["eo_count"].ravel(), t["bo_count"].ravel()]).astype(np.int64)
        s = np.concatenate([t["eo_sum"].ravel(), t["bo_sum"].ravel()]).astype(np.int64)
        assert set(np.unique(n)) == {0, 1, 4096} and int(s.max()) == 268431360 and int(s.min()) == -268431360
        assert set(np.unique(np.abs(s[n > 0]) // n[n > 0])) == {0, 1, 65535}
        t = V.pick_table("tie", bd)
        n, s = t["bo_count"].astype(np.int64), t["bo_sum"].astype(np.int64)
        assert ((2 * s + n) % (2 * n) == 0).all()                       # 2s = n (2o - 1)
        t = V.pick_table("sparse", bd)
        assert (t["bo_count"] == 0).mean() > 0.75 and (t["eo_count"] == 0).mean() > 0.75
        assert V.pick_table("plain", bd).tobytes() != V.pick_table("plain", bd, 1).tobytes()


# ---- the hand-built table ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(V.HAND))
def test_hand_table_reference_gives_the_literals(name):
    c = V.HAND[name]
    a, b = V.hand_stats(c["a"]), None if c["b"] is None else V.hand_stats(c["b"])
    pa, pb, dd = S.pick_plane(a[0], None if b is None else b[0], c["bd"], c["lam"])
    assert pa.tobytes() == V.hand_params(c["want_a"])[0].tobytes(), (name, pa)
    if b is not None:
        assert pb.tobytes() == V.hand_params(c["want_b"])[0].tobytes(), (name, pb)
    assert int(dd[0, 0]) == c["dd"], (name, dd)


def test_hand_table_covers_the_header():
    kinds = {(c["b"] is not None, c["lam"] > 0) for c in V.HAND.values()}
    assert {(False, False), (False, True), (True, False)} <= kinds
    assert {c["bd"] for c in V.HAND.values()} == {8, 9, 10, 16}
    assert any(c["want_a"][0] == 1 and c["want_a"][1] >= 29 for c in V.HAND.values())


# ---- csrc/sao_stats.h on the CPU --------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=["plain", "sanitized"])
def sim(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("sao_stats_edges_sim_" + request.param)
    exe = str(d / "sao_stats_sim")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas"] + flags + ["-I", CSRC, "-o", exe, SIM_SRC])
    return exe, str(d)


def sim_stats(sim, rec, org, bd, lw, lh, keep=None, nox=None):
    """one plane through the program, tight pitch"""
    exe, d = sim
    h, w = rec.shape
    blob = np.array([w, h, rec.itemsize, bd, lw, lh, keep is not None, nox is not None, w], "<i4").tobytes()
    blob += rec.tobytes() + org.tobytes() + (b"" if keep is None else keep.tobytes()) + (b"" if nox is None else nox.tobytes())
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    open(fin, "wb").write(blob)
    r = subprocess.run([exe, "stats", fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return np.fromfile(fout, S.STATS_DTYPE).reshape(S.grid(w, h, lw, lh))


def sim_pick(sim, a, b, bd, lam):
    """(params_a, params_b or None, delta_d), each of a's shape"""
    exe, d = sim
    blob = np.array([bd, lam, a.size, b is not None], "<i4").tobytes() + a.tobytes() + (b"" if b is None else b.tobytes())
    fin, fout = os.path.join(d, "pick_in.bin"), os.path.join(d, "pick_out.bin")
    open(fin, "wb").write(blob)
    r = subprocess.run([exe, "pick", fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw = open(fout, "rb").read()
    k = 1 if b is None else 2
    got = np.frombuffer(raw[: a.size * 6 * k], ro.SAO_CTB_DTYPE).reshape((k,) + a.shape)
    return got[0], (got[1] if k == 2 else None), np.frombuffer(raw[a.size * 6 * k:], "<i8").reshape(a.shape)


def names_of(got, want):
    return [f for f in S.STATS_DTYPE.names if not np.array_equal(got[f], want[f])]


@pytest.mark.parametrize("s", SETS, ids=set_id)
def test_block_procedure_on_every_shape(sim, s):
    depth, lw, lh = s
    for (w, h, keep) in V.shape_set(depth, lw, lh):
        rec, org = V.content(w, h, depth)
        for nox in (True, False):
            want = V.reference(w, h, depth, lw, lh, keep, nox)[0]
            got = sim_stats(sim, rec[0], org[0], V.DEPTHS[depth][0], lw, lh, V.keep_map(w, h)[0] if keep else None,
                            V.border_bytes(w, h, lw, lh)[0] if nox else None)
            assert got.tobytes() == want.tobytes(), (s, w, h, keep, nox, names_of(got, want))


def test_block_procedure_every_block_kept(sim):
    w, h = V.PLANES[0]
    rec, org = V.content(w, h, "10b")
    keep = np.ones((-(-h // 8), -(-w // 8)), np.uint8)
    got = sim_stats(sim, rec[0], org[0], 10, 4, 5, keep, V.border_bytes(w, h, 4, 5)[0])
    assert got.shape == S.grid(w, h, 4, 5) and not got.tobytes().strip(b"\0")


@pytest.mark.parametrize("shape", list(V.EVERY_BYTE), ids=lambda s: "ctb%dx%d" % (1 << s[0], 1 << s[1]))
def test_block_procedure_on_every_byte(sim, shape):
    lw, lh = shape
    v = V.every_byte(lw, lh)
    want = V.every_byte_reference(lw, lh)
    for f in range(len(v["rec"])):
        got = sim_stats(sim, v["rec"][f], v["org"][f], v["bd"], lw, lh, None, v["nox"][f])
        assert got.tobytes() == want[f].tobytes(), (shape, f, names_of(got, want[f]))


@pytest.mark.parametrize("bd", V.PICK_DEPTHS)
@pytest.mark.parametrize("kind", V.PICK_KINDS)
def test_pick_procedure_on_every_table(sim, kind, bd):
    for joint in (False, True):
        a, b = V.pick_table(kind, bd), V.pick_table(kind, bd, 1) if joint else None
        for lam in V.PICK_LAMBDAS:
            pa, pb, dd = sim_pick(sim, a, b, bd, lam)
            for f, (wa, wb, wd) in enumerate(V.pick_expected(kind, bd, lam, joint)):
                assert pa[f].tobytes() == wa.tobytes(), (kind, bd, lam, joint, f)
                if joint:
                    assert pb[f].tobytes() == wb.tobytes(), (kind, bd, lam, f)
                assert np.array_equal(dd[f], wd), (kind, bd, lam, joint, f)


def test_pick_procedure_gives_the_literals(sim):
    for name, c in V.HAND.items():
        a, b = V.hand_stats(c["a"]), None if c["b"] is None else V.hand_stats(c["b"])
        pa, pb, dd = sim_pick(sim, a, b, c["bd"], c["lam"])
        assert pa.tobytes() == V.hand_params(c["want_a"]).tobytes(), (name, pa)
        if b is not None:
            assert pb.tobytes() == V.hand_params(c["want_b"]).tobytes(), (name, pb)
        assert int(dd[0, 0, 0]) == c["dd"], (name, dd)
