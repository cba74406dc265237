"""The batch-operand vectors (tests/batch_vectors.py) checked on the CPU: the census that makes a wrong frame index visible in
every cell of every frame, the coverage of kernel families x operands x states (from the dispatch restatement, not by hand), the
generator's own invariants, and a numpy restatement of the two 4:2:2 rewrites tied to tests/sao_borders_ref.py."""
import collections
import dataclasses
import itertools

import numpy as np
import pytest

import batch_vectors as bv
import dispatch_cases as dc
import g4_ref as G
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
    # every plane reads every operand in the state that plane has it in; a plane of pairs adds one reading per frame (Cb <-> Cr)
    want = 0
    for i in range(c.n_planes):
        per_frame = [x for x in bv.OPERANDS if c.state(x, i) in bv.PER_FRAME]
        want += len(per_frame) * c.n * (c.n - 1) + (c.n - 1) * sum(c.state(x, i) == "padded" for x in per_frame)
        want += c.n * (c.pair(i) and c.has_sao())
    assert len(wrong) == want == bv.census_readings(c) and len(exp) == c.n_planes * c.n, (name, len(wrong), want)
    for i in range(c.n_planes):   # a plane of pairs is compared per component: cells of Cb and cells of Cr
        assert exp[i, 0].shape == ((c.geom(i)[1], c.geom(i)[0], 2) if c.pair(i) else (c.geom(i)[1], c.geom(i)[0]))


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


def test_pinned_cases_predict_their_kernel():
    """the cases written for one instantiation each: the dispatch restatement predicts exactly that kernel with those template
    arguments (the GPU test holds the capture against the same table), the six row-major ones on a grid of 513 blocks per row with
    QP-map units of 16 or 32 luma samples, as the older row-major cases have them"""
    assert set(bv.PINNED) <= set(BY_NAME) and len({v for v in bv.PINNED.values()}) == len(bv.PINNED)
    for name, (kernel, args) in bv.PINNED.items():
        c = BY_NAME[name]
        got = [(l.kernel, l.args) for l in dc.predict(bv.dispatch_case(c)) if l.family != "sao rows x2"]
        assert got == [(kernel, args)], (name, got)
    lin = [BY_NAME[n] for n, (k, _) in bv.PINNED.items() if k.startswith("dbk_packed")]
    assert len(lin) == len(bv.LINEAR_QM) == 6 and {c.n for c in lin} == {3, 5}
    for c in lin:
        p = bv.dispatch_case(c).planes[0]
        assert p.w == 4096 and p.nbx == 513 > dc.WG_CAP and c.state("map") in bv.PER_FRAME and c.unit_log2 in (4, 5), c.name
        assert bv.families(c) == ["packed linear"]
    multi = BY_NAME["map_ref_multi_cf1_12_padded"]
    assert (multi.mode, multi.planes, multi.w, multi.h, multi.bd, multi.fused, multi.state("map")) == ("ref", "YUV", 256, 128, 12, dc.FUSED_ON, "padded")


def test_padded_gaps_hold_poison_and_odd_strides_occur():
    odd = 0
    for c in CASES:
        ops = bv.make_operands(c, bv.seed_of(c))
        for x in bv.OPERANDS:
            for i in range(1 if x in ("borders", "sl") or (x == "map" and c.planes != "NV") else c.n_planes):
                if c.state(x, i) != "padded":
                    continue
                for which in ((0, 1) if x == "bs" or (x == "params" and c.pair(i)) else (0,)):
                    arrs = bv.operand_arrays(c, ops, x, i, which)
                    buf, stride = bv.lay_out(arrs, "padded", bv.poison_entry(x, c.bd), bv.operand_dtype(x))
                    size = np.asarray(arrs[0]).size
                    assert stride > size and buf.size == stride * c.n
                    if x == "sl":   # 16-bit words: the stride in bytes is even whatever the stride in words; the gap holds SL_POISON
                        assert buf.dtype == np.uint16 and buf[size:stride].view(np.int8).reshape(-1, 2).tolist() == [list(bv.SL_POISON)] * (stride - size)
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
    p = g.plane()
    tx, tpf, total = dc.sao_strips(p)
    launch = g.launch()
    assert (launch.kernel, launch.args) == g.kernel and launch.grid == (tx, tpf // tx, g.n) and dc.api_align_ok(p), (name, launch)
    if not g.kind:
        assert g.n > 1 and g.families() == ["sao8<3d>"]
        (l0,) = dc.predict(g.dispatch_case())
        assert l0.kernel == "sao8_kernel" and l0.args[0] == 0 and l0.grid[2] == g.n
        assert dc.sao_swz(dc.Plane(g.w, g.h - 64, n=g.n)) and not dc.sao_swz(p)
        assert 2 * p.nbytes() < 4 << 30     # source + destination: below the 6.07 GiB the dispatch tests already need
    else:
        # the smallest plane of its kind past the guard: the most strip rows an entry takes, one strip per row fewer passes the guard,
        # and the last strip holds one block column of 4 (g4, pairs) or 8 samples
        assert g.n > 1 or g.bd > 8
        assert tpf // tx == g.strip_rows and g.w == 256 * (tx - 1) + g.unit and g.ctb_log2 == (5 if g.kind == "sp" else 6)
        if g.kind == "sp":   # two rows of strips, the second one block row: the same guard, half the bytes of 1024 rows of strips
            assert g.strip_rows == 2 and g.h == 64 + g.unit and p.nbytes() < bv.Giant("x", "tight", kind="sp", pad=g.pad).plane().nbytes() * 0.55
        else:
            assert g.strip_rows == bv.GIANT_STRIP_ROWS and g.h <= 65535 < g.h + g.unit
        assert not dc.sao_swz(p) and dc.sao_swz(dc.Plane(256 * (tx - 1), g.h, n=g.n))
        assert (g.kind == "nox") == (g.w % 8 == 0 and g.h % 8 == 0) and g.w % 4 == 0 and g.h % 4 == 0
        assert 2 * (p.nbytes() + 256) < 6.07 * (1 << 30)     # source + destination: what the dispatch tests already need
        assert p.P * p.h < 1 << 31 or g.bd > 8               # the 8-bit packed kernels' own guard
    ops = bv.giant_operands(g)
    checks = ops["windows"][0][0].check(1 << g.ctb_log2)
    assert len(checks) >= 9
    if g.kind:   # a check window on each of the four plane borders; the last block column and the last block row in content windows
        content = ops["windows"][0][0].content
        assert {0} <= {r[0] for r in checks} and {0} <= {r[2] for r in checks} and g.h in {r[1] for r in checks} and g.w in {r[3] for r in checks}
        assert any(r[1] == g.h for r in content) and any(r[3] == g.w for r in content)
    for x in ("params", "keep", "borders"):
        for which in range(g.comps if x == "params" else 1):
            arrs = bv.giant_arrays(g, ops, x, which)
            assert len(arrs) == g.n
            for a, b in itertools.permutations(arrs, 2):
                assert a.shape == b.shape and (np.asarray(a).view(np.uint8) != np.asarray(b).view(np.uint8)).any()
    first = ops["params"][0] if g.comps == 1 else ops["params"][0][0]
    assert (first["type"] != 0).all() and (g.n == 1 or (ops["keep"][0] != ops["keep"][1]).mean() > 0.5)
    if g.comps == 2:   # Cb and Cr differ in type in CTBs of a check window: the pair kernels' general path
        cb, cr = ops["params"][0]
        assert ((cb["type"] != cr["type"]) & ops["touch"]).sum() >= 9 and not ((cb["type"] != cr["type"]) & ~ops["touch"]).any()
    bad = bv.giant_census(g, ops)
    assert not bad, [(x, f, k, e[:2]) for x, f, k, e in bad]


def test_giant_3d_states():
    gs = bv.giants()
    assert {g.state for g in gs} == {"tight", "padded"} and len({g.name for g in gs}) == len(gs)
    assert {g.state for g in gs if g.n > 1 and g.kind} == {"tight", "padded"}
    # the seven 3-D forms beside sao8_nox_kernel<false, 4>; the two semi-planar 16-bit forms need more than 4e9 bytes per buffer
    assert {g.kernel for g in gs if g.kind} == {("sao8_g4_kernel", (0, 4)), ("sao_g4_kernel", ("u8", 0, 0)), ("sao_nox_kernel", ("u8", 0, 0)),
                                                ("sao8_sp_kernel", (0,)), ("sao_sp_kernel", ("u8", 0)), ("sao_g4_kernel", ("u16", 0, 0)),
                                                ("sao_nox_kernel", ("u16", 0, 0))}


def test_unreached_pair_forms_need_more_than_4e9_bytes():
    """sao_sp_kernel<u16, false> and sao16_sp_kernel<false> in the giants' construction (the most strip rows, the first strip count or
    frame count past the guard), from the restated guards: the figures of profiles/launch_select/branch_census.md"""
    one = bv.Giant("x", "tight", n=1, kind="sp", ctb_log2=5, bd=10, pad=8)
    p = one.plane()
    assert (one.launch().kernel, one.launch().args) == ("sao_sp_kernel", ("u16", 0)) and (one.w, one.h) == (16132, 65532) and p.nbytes() > 4.2e9
    assert p.P * p.h >= 1 << 31        # ... and far past what the packed form addresses
    # the packed 16-bit form needs pitch * plane_h < 2^31: at 65532 rows at most 8192 pairs a row, 32 strips; the guard fails by frames
    w = dc.first_false(lambda k: 16 * k * one.h < 1 << 31, 1, 1 << 16) * 4 - 4
    n = dc.first_false(lambda k: dc.sao_swz(dc.Plane(w, one.h, bd=10, pitch=4 * w, n=k)), 1, 1 << 16)
    l = dc.sao_sp_launch(dc.Plane(w, one.h, bd=10, pitch=4 * w, n=n))
    assert (w, n) == (8192, 4) and (l.kernel, l.args) == ("sao16_sp_kernel", (0,)) and n * 4 * w * one.h > 8.5e9


# ---- the _sl, _g4, _sp and NV12 families ---------------------------------------------------------------------------------------------

NEW = [c for c in CASES if c.fam]
LISTED = {"sl": set(bv.K_SL.values()), "g4": set(bv.K_G4.values()), "sp": set(bv.K_SP.values())}
TAKES = {"dbk": ("map", "bs", "sl"), "sao": ("params", "keep", "borders")}


def _operands_of(kernel):
    return (TAKES["dbk"] if kernel.startswith("dbk") else ()) + (TAKES["sao"] if "sao" in kernel else ())


def test_new_families_see_every_operand_in_every_state():
    """every kernel of the three lists is some case's, and reads each operand it takes shared, tight and padded (from the cases'
    own kernel lists, which the GPU test holds against the stream capture)"""
    t = collections.Counter(k for c in NEW for k in bv.attribution(c))
    missing = [(k, x, s) for fam in LISTED.values() for k in sorted(fam) for x in _operands_of(k) for s in bv.THREE if not t[k, x, s]]
    # the _sl deblocking kernels take sl tight here: sl alone, in every state, is test_gpu_slice_offsets.py's
    missing = [m for m in missing if not (m[0] in (bv.K_SL["g"], bv.K_SL[8], bv.K_SL[16]) and m[1] == "sl" and m[2] != "tight")]
    assert not missing, missing
    for c in NEW:
        assert set(c.kernels) <= set().union(*LISTED.values()), c.name
        assert all(s in bv.THREE + ("far",) for s in bv.all_states(c)), c.name


def test_new_families_shapes_frame_counts_and_combinations():
    by = collections.defaultdict(list)
    for c in NEW:
        for k in c.kernels:
            by[k].append(c)
    assert {1, 2, 3, 5, 7} <= {c.n for c in NEW}
    for k in (bv.K_SL["f8"], bv.K_SL["f16"], bv.K_SL["multi"], bv.K_G4["f8"], bv.K_G4["f16"], bv.K_G4["multi"], bv.K_SP["f8"], bv.K_SP["f16"],
              bv.K_SP["multi"]):
        assert any(c.n == 5 and any(s in bv.PER_FRAME for s in bv.all_states(c)) for c in by[k]), ("a five-frame case", k)
    # the fused grids are whole multiples of 8 workgroups: the tiles of the three- and five-frame cases, counted from the plane and
    # the kernels' tile sizes (pairs 96 / 64 x 128, luma 192 / 128 x 128; the NV12 kernel rounds its luma part and its pair part each)
    def tiles(c, i):
        pw, ph = c.geom(i)[:2]
        tw = {1: 96, 2: 64}[c.sb] if c.pair(i) else dc.FUSED_TILE[c.sb][0]
        return -(-pw // tw) * -(-ph // 128)
    seen = collections.Counter()
    for c in NEW:
        if c.planes in ("P", "NV") and c.has_deblock() and c.has_sao() and any("fused" in k for k in c.kernels):
            per_frame = [tiles(c, i) for i in range(c.n_planes)]
            assert per_frame == ([6, 4] if c.planes == "NV" else [4]), (c.name, per_frame)
            if c.n in (3, 5):
                assert all((t * c.n) % 8 != 0 for t in per_frame), (c.name, per_frame)   # padding workgroups exist in every part
                seen[c.kernels, c.n] += 1
    for k in (bv.K_SP["f8"], bv.K_SP["f16"], bv.K_SP["multi"]):
        assert seen[(k,), 3] and seen[(k,), 5], k
    for k in (bv.K_SL["f8"], bv.K_G4["f8"], bv.K_SP["f8"], bv.K_SP["f16"]):   # five frames with keep map and borders padded
        assert any(c.n == 5 and c.state("keep") == c.state("borders") == "padded" for c in by[k]), k
    for k, entry, with_sl in ((bv.K_SL["f8"], "dbk_sao_sl", True), (bv.K_G4["sao8"], "sao_g4", False), (bv.K_SP["sao8"], "sao_sp", False)):
        for combo in itertools.product(bv.THREE, repeat=3):
            assert [c for c in by[k] if c.entry == entry and (c.state("params"), c.state("keep"), c.state("borders")) == combo and
                    (not with_sl or c.state("sl") == "padded")], (k, combo)
    # planes: pairs 100 x 132, NV12 luma 200 x 264, planar g4 chroma 100 x 132, _sl in multiples of 8; SAO CTBs of 8 on the pair plane
    for c in NEW:
        if c.fam in ("sp", "nv12"):
            i = c.n_planes - 1
            assert c.pair(i) and c.geom(i) == (100, 132, 3, 3) and c.pitch(i) >= 200 * c.sb and c.offs[2] != c.offs[3], c.name
        if c.fam == "nv12":
            assert c.geom(0) == (200, 264, 4, 4) and c.st1 is not None and not c.pair(0)
        if c.fam == "g4":
            assert G.is_g4(*c.geom(c.n_planes - 1)[:2]) and (c.linear or c.geom(c.n_planes - 1)[:2] == (100, 264 if c.cf == 2 else 132)), c.name
        if c.fam == "sl":
            assert all(c.geom(i)[0] % 8 == 0 and c.geom(i)[1] % 8 == 0 for i in range(c.n_planes)), c.name
        if c.fam != "nv12" or c.name != "nv12_plane_by_plane":
            assert all(c.pitch(i) % 32 == 0 and c.frame_stride(i) % 32 == 0 for i in range(c.n_planes)), c.name
    # the row-major block map of the packed _sl / _g4 kernels: rows of more blocks than a workgroup holds, a grid with padding
    lin = [c for c in NEW if c.linear]
    assert {c.kernels for c in lin} == {(bv.K_SL[8],), (bv.K_SL[16],), (bv.K_G4[8],), (bv.K_G4[16],)}
    for c in lin:
        pw, ph = c.geom(0)[:2]
        nbx, nby = pw // 8 + 1, ph // 8 + 1
        wpf = -(-nbx * nby // dc.WG_CAP)
        assert nbx > dc.WG_CAP and wpf >= 2 and (wpf * c.n) % 8 != 0 and (pw, ph) == ((4100, 20) if c.fam == "g4" else (4096, 16)), c.name
    nv = [c for c in NEW if c.fam == "nv12"]
    assert {c.bd for c in nv} == {8, 10} and {3, 5} <= {c.n for c in nv}
    for c in nv:   # the two operand sets in different states; the three picture operands in every state over the list
        if c.name not in ("nv12_pair_only", "nv12_luma_only"):
            assert sum(c.state(x, 0) != c.state(x, 1) for x in bv.PLANE_OPERANDS) >= 2, c.name
    for x in ("sl", "borders"):
        assert {c.state(x) for c in nv} >= set(bv.THREE), x
    only = {c.name: ([c.state(x, 0) in bv.PER_FRAME for x in bv.PLANE_OPERANDS], [c.state(x, 1) in bv.PER_FRAME for x in bv.PLANE_OPERANDS]) for c in nv}
    assert only["nv12_pair_only"] == ([False] * 4, [True] * 4) and only["nv12_luma_only"] == ([True] * 4, [False] * 4)
    assert any(c.fused == dc.FUSED_AUTO and len(c.kernels) == 3 and c.pitch(1) % 16 for c in nv), "the plane-by-plane fallback"
    assert bv.FAR_STRIDE_SL % 2 == 0 and 2 * bv.FAR_STRIDE_SL >= 1 << 32
    far = {(x, c.far_which, c.kernels) for c in NEW for x in bv.OPERANDS if c.state(x) == "far"}
    both = [(bv.K_SP[8],), (bv.K_SP["f8"],)]   # map, vert bS and hor bS through the packed and the fused pair kernel, sl through the fused one
    assert far == {(x, w, k) for x, w in (("map", ""), ("bs", "vert"), ("bs", "hor")) for k in both} | {("sl", "", (bv.K_SP["f8"],))}, far


def test_slice_offsets_tell_the_frames_apart_by_tc_alone():
    """chroma deblocking ignores beta: frame f's tC offsets occur in no other frame's array, and the poison's in none"""
    seen = 0
    for c in NEW:
        if c.state("sl") not in bv.PER_FRAME:
            continue
        ops = bv.make_operands(c, bv.seed_of(c))
        tcs = [set(np.unique(a[..., 1]).tolist()) for a in ops["sl"]]
        assert all(a.shape == c.sl_grid() + (2,) and a.dtype == np.int8 for a in ops["sl"]), c.name
        for f, g in itertools.combinations(range(c.n), 2):
            assert not tcs[f] & tcs[g], (c.name, f, g)
            assert (ops["sl"][f][..., 1] != ops["sl"][g][..., 1]).all()
        assert all(bv.SL_POISON[1] not in t and len(t) == 2 for t in tcs), c.name
        seen += 1
    assert seen >= 20


def test_pair_parameters_are_two_contents_behind_one_stride():
    for c in NEW:
        for i in range(c.n_planes):
            if c.pair(i) and c.has_sao():
                ops = bv.make_operands(c, bv.seed_of(c))
                cb, cr = bv.operand_arrays(c, ops, "params", i, 0), bv.operand_arrays(c, ops, "params", i, 1)
                st = c.state("params", i) if c.state("params", i) != "far" else "tight"
                a, b = (bv.lay_out(x, st, bv.poison_entry("params", c.bd), bv.SAO_DT) for x in (cb, cr))
                assert a[1] == b[1] and a[0].shape == b[0].shape and (a[0] != b[0]).any(), c.name
                break


def test_pair_chain_is_the_feature_tests_expectation(monkeypatch):
    """the chain of this module on the vector of test_gpu_fused_sp.py = sao_sp_ref.chain_expected: sp_ref.dbk_expected, then
    sao_sp_ref.sao, with the per-slice pairs and the layout"""
    import sao_sp_ref as P
    import sp_ref as S
    v = P.chain_case(P.spec_of("140x132"))
    monkeypatch.setattr(bv, "QP", S.QP)
    c = bv.Case("tie", "dbk_sao_sp_fused", "h265", "P", 2 * v["w"], 2 * v["h"], fam="sp", n=2, unit_log2=S.UNIT_LOG2, ctb_log2=v["lg"] + 1,
                offs=(S.TC_DIV2, 0, S.CB_OFF, S.CR_OFF))
    for f in range(2):
        for sl in (False, True):
            dbk, want = P.chain_expected(v, f, sl, v["layout"])
            got = bv.oracle_frame(c, 0, v["planes"][f], qmap=v["qp_map"], bs=v["bs"][f], sl=v["pairs"] if sl else None,
                                  params=(v["pcb"][f], v["pcr"][f]), keep=v["keep"][f], layout=v["layout"])
            assert np.array_equal(got, want) and (want != dbk).any() and (dbk != v["planes"][f]).any(), (f, sl)
        d = dataclasses.replace(c, entry="filter_sp")
        assert np.array_equal(bv.oracle_frame(d, 0, v["planes"][f], qmap=v["qp_map"], bs=v["bs"][f], sl=v["pairs"]), S.dbk_expected(v, f, True, True))


def test_g4_chain_is_the_feature_tests_expectation(monkeypatch):
    """likewise on a vector of test_gpu_g4.py: g4_ref.dbk_expected (direct and per slice), then g4_ref.sao_direct"""
    spec = next(s for s in G.TILES8 if s[0] == "196x132")
    v, s_ = G.dbk_case(spec, frames=2), G.sao_case(spec, frames=2)
    monkeypatch.setattr(bv, "QP", G.QP)
    c = bv.Case("tie", "dbk_sao_g4", "h265", "C", 2 * v["w"], 2 * v["h"], fam="g4", n=2, unit_log2=G.UNIT_LOG2, ctb_log2=s_["lw"] + 1,
                offs=(G.TC_DIV2, 0, G.CQP, G.CQP))
    lay = G.sao_layout(s_, 0)
    for f in range(2):
        for sl in (False, True):
            mid = G.dbk_expected(v, f, sl)
            want = G.sao_direct(mid, s_["params"][f], s_["lw"], s_["lh"], bit_depth=v["depth"], keep=s_["keep"][f], layout=lay)
            got = bv.oracle_frame(c, 0, v["planes"][f], qmap=v["qp_map"], bs=v["bs"][f], sl=v["pairs"] if sl else None, params=s_["params"][f],
                                  keep=s_["keep"][f], layout=lay)
            assert np.array_equal(got, want) and (mid != v["planes"][f]).any() and (want != mid).any(), (f, sl)


def test_luma_sl_chain_is_the_slice_offset_statement():
    """the _sl luma cases: slice_offsets_ref.expected, then sao_borders_ref.sao_plane, composed by hand on the case's own operands"""
    import slice_offsets_ref as SR
    c = BY_NAME["sl_fused8_n2_shared_tight"]
    ops = bv.make_operands(c, bv.seed_of(c))
    for f in range(c.n):
        mid = SR.expected(ops["frames"][0][f], *ops["bs"][0][f], ops["sl"][f], bv.SL_LOG2, qp=bv.QP, c_idx=0, qp_map=ops["map"][f],
                          unit_log2=c.unit_log2, bit_depth=8)
        want = R.sao_plane(mid, ops["params"][0][f], 4, 4, ops["borders"][f], keep=ops["keep"][0][f])
        assert np.array_equal(bv.expected(c, ops, 0, f), want) and (mid != ops["frames"][0][f]).any() and (want != mid).any()
