"""The batch-operand vectors (tests/batch_vectors.py) checked on the CPU: the census that makes a wrong frame index visible in
every cell of every frame, the coverage of kernel families x operands x states (from the dispatch restatement, not by hand), the
generator's own invariants, and a numpy restatement of the two 4:2:2 rewrites tied to tests/sao_borders_ref.py."""
import collections
import itertools

import numpy as np
import pytest

import batch_vectors as bv
import dispatch_cases as dc
import rext_oracle as rx
import sao_borders_ref as R

CASES = bv.cases()
BY_NAME = {c.name: c for c in CASES}


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_census(name):
    """every per-frame operand of every case: frame g's operand (and, padded, the operand read at the tight stride) changes
    frame f's output in every cell -- no pair, no cell exempt"""
    c = BY_NAME[name]
    bad, exp, wrong = bv.census(c, bv.make_operands(c, bv.seed_of(c)))
    assert not bad, (name, [(x, i, f, g, cells[:3]) for x, i, f, g, cells in bad][:6])
    per_frame = [x for x in bv.OPERANDS if c.state(x) in bv.PER_FRAME]
    want = c.n_planes * len(per_frame) * c.n * (c.n - 1) + c.n_planes * (c.n - 1) * sum(c.state(x) == "padded" for x in per_frame)
    assert len(wrong) == want and len(exp) == c.n_planes * c.n, (name, len(wrong), want)


def _table():
    t = collections.defaultdict(list)
    for c in CASES:
        for fam, x, s in bv.attribution(c):
            t[fam, x, s].append(c)
    return t


def test_coverage_of_families_operands_and_states():
    t = _table()

    def have(fam, x, s, pred=lambda c: True):
        return [c for c in t.get((fam, x, s), []) if pred(c)]

    missing = []

    def need(what, found):
        if not found:
            missing.append(what)

    dbk = ("generic", "packed rows", "packed linear", "fused", "fused multi")
    for mode in ("ref", "h265"):
        for fam in dbk:
            need(("map per frame", mode, fam), [c for s in ("tight", "padded") for c in have(fam, "map", s, lambda c: c.mode == mode)])
    for s in ("tight", "padded"):
        need(("map", s), [c for fam in dbk for c in have(fam, "map", s)])
        for fam in dbk:
            need(("bs", "h265", fam, s), have(fam, "bs", s, lambda c: c.h265))
    for fam in ("packed rows", "packed linear", "multi", "fused", "fused multi"):
        need(("bs padded", "ref", fam), have(fam, "bs", "padded", lambda c: not c.h265))
    # the packed QP-map kernels by plane kind: 8-bit luma, 8-bit chroma, 16-bit containers, the 12-bit WIDE variant, _cf chroma
    pk = ("packed rows", "packed linear")
    kinds = {"8-bit luma": lambda c: c.bd == 8 and c.planes == "Y", "8-bit 4:2:0 chroma": lambda c: c.bd == 8 and c.planes == "C" and c.cf == 1,
             "10-bit luma": lambda c: c.bd == 10 and c.planes == "Y", "12-bit luma (WIDE)": lambda c: c.bd == 12 and c.planes == "Y",
             "16-bit chroma": lambda c: c.bd == 10 and c.planes == "C" and c.cf == 1}
    for mode in ("ref", "h265"):
        for kind, pred in kinds.items():
            need(("map per frame", mode, kind), [c for fam in pk for s in ("tight", "padded")
                                                 for c in have(fam, "map", s, lambda c: c.mode == mode and c.entry == "filter" and pred(c))])
    for cf in (2, 3):
        for bd in (8, 10):
            need(("map per frame, _cf chroma", cf, bd), [c for fam in pk for s in ("tight", "padded")
                                                           for c in have(fam, "map", s, lambda c: c.planes == "C" and c.cf == cf and c.bd == bd)])
        need(("map per frame, fused multi", cf), [c for s in ("tight", "padded") for c in have("fused multi", "map", s, lambda c: c.cf == cf)])
    for bd in (8, 10):
        for mode in ("ref", "h265"):
            need(("map per frame, fused", mode, bd), [c for s in ("tight", "padded")
                                                      for c in have("fused", "map", s, lambda c: c.bd == bd and c.mode == mode)])
    need("map per frame through hevc_deblocking_filter_device_planes", [c for c in CASES if c.entry == "filter_planes" and c.state("map") in bv.PER_FRAME])
    units = {c.unit_log2 for c in CASES if c.state("map") in bv.PER_FRAME}
    assert {3, 4, 6, 8} <= units, units
    # SAO parameters x keep map x borders: all 27 combinations for each of these families
    for fam, pred in (("sao8<swz>", None), ("sao<u16,pk16>", None), ("fused", lambda c: c.bd == 8), ("fused", lambda c: c.bd == 10),
                      ("fused multi", None)):
        for combo in itertools.product(("shared", "tight", "padded"), repeat=3):
            found = [c for c in CASES if fam in bv.families(c) and (pred is None or pred(c)) and
                     (c.state("params"), c.state("keep"), c.state("borders")) == combo]
            need((fam, combo), found)
    # both 4:2:2 rewrite kernels with padded and with shared sources
    for x, k in (("params", 0), ("borders", 1)):
        for s in ("padded", "shared", "tight"):
            need(("4:2:2 rewrite of", x, s), [c for c in CASES if bv.rewrites_422(c)[k] and c.state(x) == s])
    need("4:2:2 rewrites in the multi-plane launch", [c for c in CASES if c.planes == "YUV" and bv.rewrites_422(c) == (2, 2) and c.state("borders") == "padded"])
    # every operand in every state; every entry that takes an operand appears with it per frame
    for x in bv.OPERANDS:
        for s in ("shared", "tight", "padded"):
            need((x, s), [c for c in CASES if c.state(x) == s])
    takes = {"map": ["filter", "filter_planes", "dbk_sao", "dbk_sao_planes"], "bs": ["filter", "filter_planes", "dbk_sao", "dbk_sao_planes"],
             "params": ["sao", "dbk_sao", "dbk_sao_planes"], "keep": ["sao", "dbk_sao", "dbk_sao_planes"], "borders": ["sao", "dbk_sao", "dbk_sao_planes"]}
    for x, entries in takes.items():
        for e in entries:
            for mode in ("ref", "h265"):
                if (e == "sao" or x == "borders") and mode == "ref" or (e == "filter_planes" and mode == "h265"):
                    continue   # SAO alone has no mode; the reference-exact entries have no borders; filter_planes is reference-exact
                need((x, "per frame through", e, mode), [c for c in CASES if c.entry == e and c.mode == mode and c.state(x) in bv.PER_FRAME])
    # frame counts; the far strides
    assert {1, 2, 3, 5} <= {c.n for c in CASES}
    # one count above three per family (frames f and f + 3 differ by the generators' seeded step), with a per-frame operand
    for fam in ("generic", "packed rows", "packed linear", "multi", "fused", "fused multi", "sao8<swz>", "sao<u16,pk16>"):
        need(("more than three frames", fam), [c for c in CASES if c.n > 3 and any(f == fam and s in bv.PER_FRAME for f, _, s in bv.attribution(c))])
    need("more than three frames, _cf chroma", [c for c in CASES if c.n > 3 and c.planes == "C" and c.cf in (2, 3) and c.state("map") in bv.PER_FRAME])
    # the exported entries without a borders argument, each with per-frame SAO operands
    for e, pred in (("hevc_sao_filter_device", lambda c: c.entry == "sao" and c.geom(0)[2] == c.geom(0)[3]),
                    ("hevcdbk_sao_filter_device_cf", lambda c: c.entry == "sao" and c.geom(0)[2] != c.geom(0)[3]),
                    ("hevc_deblock_sao_h265_device", lambda c: c.entry == "dbk_sao" and c.cf == 1),
                    ("hevcdbk_h265_deblock_sao_device_cf", lambda c: c.entry == "dbk_sao" and c.cf != 1),
                    ("hevcdbk_h265_deblock_sao_device_planes_cf", lambda c: c.entry == "dbk_sao_planes")):
        need(e, [c for c in CASES if c.plain_entry and c.h265 and pred(c) and c.state("params") in bv.PER_FRAME and c.state("keep") in bv.PER_FRAME])
    assert not [c.name for c in CASES if c.plain_entry and c.uses("borders")]
    need("far map", [c for c in CASES if c.state("map") == "far"])
    need("far vert", [c for c in CASES if c.state("bs") == "far" and c.far_which == "vert"])
    need("far hor", [c for c in CASES if c.state("bs") == "far" and c.far_which == "hor"])
    assert bv.FAR_STRIDE % 2 == 1 and 2 * bv.FAR_STRIDE >= 1 << 32
    assert not missing, missing


def test_packed_linear_cases_have_padding_workgroups_and_a_partial_last_one():
    """the larger frame counts: the linear map's grid is rounded up to 8 workgroups and the last frame's last workgroup is partial;
    the fused grid likewise is not filled by the tiles"""
    lin = [c for c in CASES if "packed linear" in bv.families(c)]
    assert lin
    for c in lin:
        p = bv.dispatch_case(c).planes[0]
        nb = p.nbx * p.nby
        wpf = -(-nb // dc.WG_CAP)
        assert nb % dc.WG_CAP != 0 and (wpf * c.n) % 8 != 0, (c.name, nb, wpf)
    fused = [c for c in CASES if c.n == 5 and "fused" in bv.families(c)]
    assert fused
    for c in fused:
        p = bv.dispatch_case(c).planes[0]
        assert (dc.fused_tiles(p)[2] * c.n) % 8 != 0, c.name


def test_padded_gaps_hold_poison_and_odd_strides_occur():
    odd = 0
    for c in CASES:
        ops = bv.make_operands(c, bv.seed_of(c))
        for x in bv.OPERANDS:
            if c.state(x) != "padded":
                continue
            for i in range(1 if x in ("map", "borders") else c.n_planes):
                for which in ((0, 1) if x == "bs" else (0,)):
                    arrs = bv.operand_arrays(c, ops, x, i, which)
                    buf, stride = bv.lay_out(arrs, "padded", bv.poison_entry(x, c.bd), bv.operand_dtype(x))
                    size = np.asarray(arrs[0]).size
                    assert stride > size and buf.size == stride * c.n
                    odd += (x == "map" and stride % 2 == 1)
                    for f in range(c.n):
                        assert np.array_equal(buf[f * stride:f * stride + size], np.ascontiguousarray(arrs[f], bv.operand_dtype(x)).ravel())
                        gap = buf[f * stride + size:(f + 1) * stride]
                        assert gap.size and (gap == np.array(bv.poison_entry(x, c.bd), bv.operand_dtype(x))).all(), (c.name, x, f)
    assert odd


def test_shared_operands_are_one_array_and_equal_their_replication():
    """a shared operand is one object for all frames, lays out with stride 0, and the expected output equals that of the same case
    with the operand replicated tight"""
    import dataclasses
    picked = {}
    for c in CASES:
        for x in bv.OPERANDS:
            if c.state(x) == "shared":
                picked.setdefault((x, c.entry, c.mode), c)
    assert {k[0] for k in picked} == set(bv.OPERANDS)
    for (x, _, _), c in picked.items():
        ops = bv.make_operands(c, bv.seed_of(c))
        arrs = bv.operand_arrays(c, ops, x)
        assert all(a is arrs[0] for a in arrs), (c.name, x)
        buf, stride = bv.lay_out(arrs, "shared", bv.poison_entry(x, c.bd), bv.operand_dtype(x))
        assert stride == 0 and buf.size == np.asarray(arrs[0]).size
        t = dataclasses.replace(c, st=dict(c.st, **{x: "tight"}))
        tops = bv.replicate(c, ops, x)
        for i in range(c.n_planes):
            for f in range(c.n):
                assert np.array_equal(bv.expected(c, ops, i, f), bv.expected(t, tops, i, f)), (c.name, x, i, f)


@pytest.mark.parametrize("kind", ["tiles", "slices", "mixed", "random", "every"])
@pytest.mark.parametrize("lw,lh", [(4, 4), (3, 4), (5, 6)])
def test_sao_from_nox_bytes_and_the_422_rewrites(kind, lw, lh):
    """sao_plane_nox on the bytes of a layout = the per-sample statement on the layout; and tall CTBs = their square halves with the
    parameter rows doubled (sao_rows_x2_kernel) and the NOX bytes re-aimed (sao_nox_rows_x2_kernel), on per-frame layouts"""
    rng = np.random.default_rng(lw * 100 + lh * 10 + len(kind))
    w, h = 9 << lw, 5 << lh
    w, h = w // 8 * 8, h // 8 * 8
    rows, cols = -(-h >> lh), -(-w >> lw)
    for f in range(3):
        lay = R._layout_of(kind, rows, cols, rng)
        prm = R.edge_params(rows, cols, rng)
        plane = rng.integers(0, 256, (h, w)).astype(np.uint8)
        keep = (rng.integers(0, 6, (h // 8, w // 8)) == 0).astype(np.uint8)
        want = R.sao_plane(plane, prm, lw, lh, lay, keep=keep)
        nox = R.expected_nox(lay)
        assert np.array_equal(bv.sao_plane_nox(plane, prm, lw, lh, nox, keep=keep), want), (kind, f)
        assert (want != rx.sao_plane(plane, prm, lw, lh, keep=keep)).any() or kind == "none"
        if lh == lw + 1:
            p2, n2 = bv.rows_x2(prm), bv.nox_rows_x2(nox)
            assert p2.shape == (2 * rows, cols) and n2.shape == (2 * rows, cols)
            assert np.array_equal(bv.sao_plane_nox(plane, p2, lw, lw, n2, keep=keep), want), (kind, f, "rewritten")


def test_rewritten_strides():
    """what the launchers hand on after a rewrite: rows * cols per frame for per-frame sources, 0 for shared ones"""
    for c in CASES:
        if not any(bv.rewrites_422(c)):
            continue
        rows, cols = c.grid()
        for x in ("params", "borders"):
            if c.uses(x):
                assert bv.rewritten_stride(c, x) == (2 * rows * cols if c.state(x) in bv.PER_FRAME else 0)


# ---- sao8<3d>: two frames on a plane just past the guard of the renumbered SAO grid ---------------------------------------------

@pytest.mark.parametrize("name", [g.name for g in bv.giants()])
def test_giant_3d_family_and_census(name):
    """the plane is the first past the swz guard for its frame count, the launch is sao8<3d> with the frame in the grid's z, and
    frame g's parameters, keep map or borders (padded: the operand read at the tight stride) change frame f in every check window"""
    g = {x.name: x for x in bv.giants()}[name]
    assert g.n > 1 and g.families() == ["sao8<3d>"]
    (launch,) = dc.predict(g.dispatch_case())
    assert launch.kernel == "sao8_kernel" and launch.args[0] == 0 and launch.grid[2] == g.n
    assert dc.sao_swz(dc.Plane(g.w, g.h - 64, n=g.n)) and not dc.sao_swz(g.plane())
    p = g.plane()
    assert 2 * p.nbytes() < 4 << 30     # source + destination: below the 6.07 GiB the dispatch tests already need
    ops = bv.giant_operands(g)
    assert len(ops["windows"][0].check(64)) >= 9
    for x in ("params", "keep", "borders"):
        a, b = bv.giant_arrays(g, ops, x)[:2]
        assert a.shape == b.shape and (np.asarray(a).view(np.uint8) != np.asarray(b).view(np.uint8)).any()
    assert (ops["params"][0]["type"] != 0).all() and (ops["keep"][0] != ops["keep"][1]).mean() > 0.5
    bad = bv.giant_census(g, ops)
    assert not bad, [(x, f, k, e[:2]) for x, f, k, e in bad]


def test_giant_3d_states():
    assert {g.state for g in bv.giants()} == {"tight", "padded"}
