"""The restated dispatch guards (tests/dispatch_cases.py) without a GPU: every clause is met on both sides by the case list,
every kernel family is reached, the solved bounds are the ones the arithmetic gives, and the windowed oracle construction used
for giant planes equals the whole-plane oracle."""
import collections

import numpy as np
import pytest

import dispatch_cases as dc

# clauses the public entries cannot drive to one side, and why
UNREACHABLE = {
    ("dbk_packed_supports", "8-bit max_v == 255"): "an 8-bit container holds 8-bit samples only (bad_depth)",
    ("dbk_packed_h265_supports", "8-bit max_v == 255"): "an 8-bit container holds 8-bit samples only (bad_depth)",
    ("plan_packed", "nbx >= 2"): "plane_w >= 8 gives nbx >= 2",
    ("plan_packed", "total < 2^31"): "implied by total * wpf < 2^32 with wpf >= 2",
    ("sao swz", "total + 8 < 2^31"): "implied by (total + 8) * tpf < 2^32 unless tpf = 1; n_frames <= 65535",
    ("dbk_multi_supports", "same n_frames"): "hevc_deblocking_filter_device_planes returns ERR_ARG first (planes_mixed_n)",
    ("dbk_deblock_sao_supports", "n_frames <= 65535"): "sao_args / planes_to_args reject n_frames > 65535 first",
    ("dbk_deblock_sao_supports", "pitch * h < 2^31"): "dbk_packed_supports checks the same product first",
    ("dbk_deblock_sao_supports", "tiles * n + 8 < 2^31"): "implied by (tiles * n + 8) * tiles < 2^32 unless tiles = 1",
}
for g in ("dbk_packed_supports", "dbk_packed_h265_supports"):
    for c in ("pitch % 8", "frame_stride % 8", "src % 8", "dst % 8"):
        UNREACHABLE[(g, c)] = "16-bit operands: the argument checks require 8-byte alignment already"
for c in ("pitch % 4", "frame_stride % 4", "src % 4", "dst % 4"):
    UNREACHABLE[("sao pk16", c)] = "16-bit operands: sao_args requires 8-byte alignment already"
for c in ("dst % 4", "dst % 8"):
    UNREACHABLE[("dbk_deblock_sao_supports", c)] = "sao_args requires the same alignment already"

FAMILIES = ["sao8<swz>", "sao8<3d>", "sao<u8>", "sao<u8,3d>", "sao<u16,pk16>", "sao<u16>", "sao<u16,3d>", "packed linear",
            "packed rows", "generic", "multi", "fused", "fused multi", "sao rows x2"]


def _walk():
    census, fam, errs = dc.Census(), collections.defaultdict(list), collections.Counter()
    for c in dc.cases():
        r = dc.predict(c, census)
        if isinstance(r, int):
            errs[r] += 1
            continue
        for launch in r:
            fam[launch.family].append(c.name)
    return census, fam, errs


def test_census_both_sides_of_every_clause():
    census, fam, errs = _walk()
    one_sided = []
    for guard, clauses in sorted(census.seen.items()):
        for name, vals in sorted(clauses.items()):
            key = (guard, name)
            if len(vals) < 2 and key not in UNREACHABLE:
                one_sided.append((key, vals))
            if len(vals) == 2:
                assert key not in UNREACHABLE, ("listed as unreachable but reached", key)
    assert not one_sided, one_sided
    print()
    for f in FAMILIES:
        names = fam.get(f, [])
        print("%-16s %4d  %s" % (f, len(names), ", ".join(names[:3]) + (" ..." if len(names) > 3 else "")))
    print("errors          ", dict(errs))
    missing = [f for f in FAMILIES if not fam.get(f)]
    assert not missing, missing
    assert not set(fam) - set(FAMILIES), set(fam) - set(FAMILIES)
    assert errs[dc.ERR_UNSUPPORTED] and errs[dc.ERR_ARG]


def test_gpu_cases_reach_every_family():
    """what the GPU file runs reaches every family (the 16-bit 3-D SAO grid through the 16-bit 2 GiB planes)"""
    fam = set()
    for c in dc.cases():
        r = dc.predict(c)
        if c.gpu and not isinstance(r, int):
            fam |= {x.family for x in r}
    assert set(FAMILIES) == fam, set(FAMILIES) ^ fam


def test_every_entry_is_driven():
    """each public device entry of the issue's list has GPU cases, with AUTO / FUSED_AUTO among them"""
    auto = {c.entry for c in dc.cases() if c.gpu and c.variant == dc.KERNEL_AUTO and c.fused == dc.FUSED_AUTO}
    assert auto == {"filter", "filter_planes", "filter_h265", "sao", "dbk_sao", "dbk_sao_h265", "dbk_sao_planes",
                    "dbk_sao_h265_planes", "dbk_sao_h265_planes_cf"}, auto
    cf_forms = {(c.entry, c.cf) for c in dc.cases() if c.gpu and c.cf != 1}
    assert {("filter_h265", 2), ("sao", 2), ("dbk_sao_h265", 2), ("dbk_sao_h265_planes_cf", 2)} <= cf_forms
    assert any(c.entry == "dbk_sao_h265_planes_cf" and c.cf == 1 for c in dc.cases())


def test_limits_match_the_hand_arithmetic():
    # 2 GiB plane: 8-bit 32768 x 65528 at pitch 32768 is 2,147,221,504 bytes (inside); pitch 32776 is outside
    assert dc.plane_h_2g(32768) == 65528 and 32768 * 65528 == 2147221504
    assert dc.packed_supports(dc.Plane(32768, 65528, pitch=32768))
    assert not dc.packed_supports(dc.Plane(32768, 65528, pitch=32776))
    assert dc.packed_supports(dc.Plane(16384, 65528, bd=10, pitch=32768))
    assert not dc.packed_supports(dc.Plane(16384, 65528, bd=10, pitch=32776))
    # SAO swz: 8-bit, h = 64, one frame: tx = 65532 renumbered, 65533 not
    assert dc.sao_swz_tx_limit() == 65533
    assert dc.sao_launch(dc.Plane(65532 * 256, 64)).family == "sao8<swz>"
    assert dc.sao_launch(dc.Plane(65533 * 256, 64)).family == "sao8<3d>"
    # fused tiles: 192 x 128, one tile row: 65532 fused, 65533 not
    assert dc.fused_tile_limit() == 65533
    assert dc.fused_supports(dc.Plane(65532 * 192, 128)) and not dc.fused_supports(dc.Plane(65533 * 192, 128))
    # plan_packed at w = 32768: the (nb + 1024) * nbx clause trips at about 2 K rows
    assert dc.linear_height_limit(32768) == 2040
    assert (4097 * 255 + 1024) * 4097 < 1 << 32 <= (4097 * 256 + 1024) * 4097
    # Y+U+V in one launch up to luma nbx = 1024: width 8184 inside, 8192 outside
    assert dc.multi_width_limit() == 8192
    # frame count and plane height limits of the argument checks
    assert dc.predict(dc.Case("n", "dbk_sao", [dc.Plane(8, 8, n=65535)], ctb_log2=3))[0].family == "fused"
    assert dc.predict(dc.Case("n", "dbk_sao", [dc.Plane(8, 8, n=65536)], ctb_log2=3)) == dc.ERR_ARG
    assert dc.predict(dc.Case("n", "filter", [dc.Plane(8, 8, n=65536)])) == dc.ERR_UNSUPPORTED


def test_case_names_unique_and_gpu_cases_fit_the_budget():
    cs = dc.cases()
    assert len({c.name for c in cs}) == len(cs)
    for c in cs:
        if c.gpu:
            # src + dst + the two-launch scratch plane, the largest case included
            assert 3 * sum(p.nbytes() for p in c.planes) < 9 << 30, c.name


# ---- windowed oracle ---------------------------------------------------------------------------------------------------------

def _check_windowed(win, op, ctb_log2=None):
    full_in = win.dense()
    full = op(full_in, 0, 0)
    mask = np.zeros(full.shape, bool)
    for (y0, y1, x0, x1), want in dc.windowed(win, op, ctb_log2):
        assert np.array_equal(full[y0:y1, x0:x1], want), (y0, y1, x0, x1)
        mask[y0:y1, x0:x1] = True
    assert np.all(full[~mask] == win.flat)


@pytest.mark.parametrize("bd", [8, 10])
def test_windowed_oracle_equals_whole_plane(bd):
    w, h = 2048, 1024
    flat = 128 << (bd - 8)
    # windows near every border, the middle, and (pretending the pitch is large) the row holding byte offset 2^31
    win = dc.standard_windows(w, h, bd, flat, pitch_bytes=(1 << 31) // 600, seed=bd)
    assert len(win.content) >= 10
    for qp in (30, 45):
        _check_windowed(win, dc.op_filter_ref(qp, bd, W=w, H=h))
        _check_windowed(win, dc.op_filter_h265(qp, bd, W=w, H=h))
    for ctb in (4, 5, 6):
        prm = dc.sao_params_for(w, h, ctb, seed=ctb + bd, bd=bd, win=win)
        assert (prm["type"] == 1).any()
        _check_windowed(win, dc.op_sao(prm, ctb, bd), ctb)
        _check_windowed(win, dc.op_chain(dc.op_filter_h265(40, bd, W=w, H=h), dc.op_sao(prm, ctb, bd)), ctb)
        _check_windowed(win, dc.op_chain(dc.op_filter_ref(40, bd, W=w, H=h), dc.op_sao(prm, ctb, bd)), ctb)


def test_band_offset_only_near_windows():
    w, h = 2048, 1024
    win = dc.standard_windows(w, h, 8, 128, pitch_bytes=w)
    prm = dc.sao_params_for(w, h, 6, seed=3, bd=8, win=win)
    s = 64
    for y, x in zip(*np.nonzero(prm["type"] == 1)):
        assert any(y0 < (y + 1) * s and y * s < y1 and x0 < (x + 1) * s and x * s < x1 for y0, y1, x0, x1 in win.check(s))
