"""Which kernel the device entries launch: the launchers' guards restated in Python, and operand sets on both sides of each.

Every guard below restates a predicate of the C++ launchers clause by clause; each names the function or helper it restates.  predict()
walks an operand set through the public entry it names (argument checks, AUTO / FUSED_AUTO choice, launcher) and returns the
error the entry returns, or the launches it enqueues: kernel name, template arguments, grid, block and dynamic LDS.  The GPU
tests (test_gpu_dispatch.py) compare that with what a captured call really enqueues, so a change to a guard or to the launch
geometry fails there.

Bounds in the case list are solved from the restatement (first_false), never typed in.  Planes too large to filter whole on
the CPU (2 GiB planes, a 65533-strip SAO row, a 65533-tile fused row) are flat except for random windows; windowed_* give
their expected output from the oracle run on each window with a halo."""
import dataclasses
import itertools

import numpy as np

ERR_ARG, ERR_UNSUPPORTED = -5, -8  # include/hevc_deblock.h
TWO31, TWO32 = 1 << 31, 1 << 32

WG_CAP = 512                                   # deblock_kernels.hip wg_cap()
FUSED_TILE = {1: (192, 128), 2: (128, 128)}    # kFusedTileW x kFusedTile, kFused16Tile (deblock_sao_fused.inc)
FUSED_THREADS = {1: 448, 2: 320}               # kFusedThreads, kFused16Threads: fused_shape
FUSED_LDS = {1: (128 + 8) * 208, 2: (128 + 8) * 288}  # kFusedLds, kFused16Lds: fused_shape
SAO_STRIP = 256                                # dbksel::sao_grid: 4 waves of 64-sample regions


# ---- operands ------------------------------------------------------------------------------------------------------------

@dataclasses.dataclass
class Plane:
    w: int
    h: int
    bd: int = 8
    pitch: int = 0           # bytes; 0 = tight
    n: int = 1
    src_off: int = 0         # bytes added to an aligned base pointer
    dst_off: int = 0
    chroma: bool = False
    fs_pad: int = 0          # frame_stride = pitch * h + fs_pad
    qpmap: int = 0           # log2 of the QP-map unit (3 .. 8); 0 = one QP for the plane

    @property
    def sb(self):
        return 1 if self.bd == 8 else 2

    @property
    def P(self):
        return self.pitch or self.w * self.sb

    @property
    def fs(self):
        return self.P * self.h + self.fs_pad

    @property
    def max_v(self):
        return (1 << self.bd) - 1

    @property
    def nbx(self):  # planes_to_args
        return self.w // 8 + 1

    @property
    def nby(self):  # planes_to_args
        return self.h // 8 + 1

    def nbytes(self):
        return self.fs * (self.n - 1) + self.P * self.h


@dataclasses.dataclass
class Case:
    name: str
    entry: str                  # filter, filter_planes, filter_h265, sao, dbk_sao, dbk_sao_h265, dbk_sao_planes,
    #                             dbk_sao_h265_planes, dbk_sao_h265_planes_cf
    planes: list
    variant: int = 0            # KERNEL_AUTO / _GENERIC / _PACKED
    fused: int = 0              # FUSED_AUTO / _OFF / _ON
    ctb_log2: int = 6
    cf: int = 1                 # chroma_format_idc (the _cf entries)
    params_pad: int = 0         # params_stride = CTB columns + params_pad
    params_per_frame: bool = False
    giant: bool = False         # flat content with random windows (windowed_* oracles)
    gpu: bool = True            # run by test_gpu_dispatch (False: census only)


KERNEL_AUTO, KERNEL_GENERIC, KERNEL_PACKED = 0, 1, 2
FUSED_AUTO, FUSED_OFF, FUSED_ON = 0, 1, 2


@dataclasses.dataclass(frozen=True)
class Launch:
    kernel: str
    args: tuple
    grid: tuple
    block: tuple
    lds: int = 0

    @property
    def family(self):
        return family_of(self.kernel, self.args)


def family_of(kernel, args):
    """short name of a kernel family, as the issue and the census table use"""
    if kernel == "sao8_kernel":
        return "sao8<%s>" % ("swz" if args[0] else "3d")
    if kernel == "sao_kernel":
        t = args[0]
        return "sao<%s%s%s>" % (t, ",pk16" if len(args) > 2 and args[2] else "", "" if args[1] else ",3d")
    if kernel in ("dbk_generic_kernel", "dbk_h265_kernel", "dbk_h265_cf_kernel"):
        return "generic"
    if kernel in ("dbk_packed_multi_kernel", "dbk_packed16_multi_kernel"):
        return "multi"
    if kernel.startswith("dbk_sao_fused_multi"):
        return "fused multi"
    if kernel.startswith("dbk_sao_fused"):
        return "fused"
    if kernel == "sao_rows_x2_kernel":
        return "sao rows x2"
    if kernel.startswith("dbk_packed"):
        lin = {"dbk_packed_kernel": 3, "dbk_packed16_kernel": 2, "dbk_packed16c_kernel": 0, "dbk_packed_h265_kernel": 1,
               "dbk_packed16_h265_kernel": 1, "dbk_packed_h265_cf_kernel": 0, "dbk_packed16_h265_cf_kernel": 0}[kernel]
        return "packed linear" if args[lin] else "packed rows"
    return kernel


# ---- the census: every clause evaluated, with its value ---------------------------------------------------------------

class Census:
    """clause -> set of values seen; guard -> clauses.  predict() records into the one passed to it"""

    def __init__(self):
        self.seen = {}

    def clause(self, guard, name, value):
        self.seen.setdefault(guard, {}).setdefault(name, set()).add(bool(value))
        return bool(value)


_NULL = Census()


def _all(census, guard, clauses):
    ok = True
    for name, v in clauses:
        ok = census.clause(guard, name, v) and ok
    return ok


# ---- restated guards ------------------------------------------------------------------------------------------------------

def api_align_ok(p, census=_NULL):
    """planes_to_args (deblock_host.cpp) and sao_args (deblock_host_h265.cpp): one 4-sample word"""
    al = 4 * p.sb
    return _all(census, "api alignment", [("pitch %% %d" % al, p.P % al == 0), ("frame_stride %% %d" % al, p.fs % al == 0),
                                          ("src %% %d" % al, p.src_off % al == 0), ("dst %% %d" % al, p.dst_off % al == 0)])


def packed_supports(p, census=_NULL, guard="dbk_packed_supports"):
    """dbk_packed_supports with the default tables; dbk_packed_h265_supports is the same predicate (the Table 8-12 tc always
    fits)"""
    c = [("pitch * plane_h < 2^31", p.P * p.h < TWO31)]
    if p.sb == 1:
        c.append(("8-bit max_v == 255", p.max_v == 255))
    else:
        c += [("max_v <= 4095", p.max_v <= 4095), ("pitch % 8", p.P % 8 == 0),
              ("frame_stride % 8", p.fs % 8 == 0), ("src % 8", p.src_off % 8 == 0), ("dst % 8", p.dst_off % 8 == 0)]
    return _all(census, guard, c)


def plan_packed(p, census=_NULL):
    """plan_packed (deblock_kernels.hip) -> (linear, grid, block)"""
    cap, nbx, nby, n = WG_CAP, p.nbx, p.nby, p.n
    nb = nbx * nby
    wg = (nb + 63) // 64 * 64 if nb < cap else cap
    wpf = (nb + wg - 1) // wg
    total = (wpf * n + 7) // 8 * 8
    want = census.clause("plan_packed", "nbx > cap", nbx > cap)  # want_linear
    exact = _all(census, "plan_packed", [  # linear
        ("wpf >= 2", wpf >= 2), ("nbx >= 2", nbx >= 2), ("(nb + 1024) * nbx < 2^32", (nb + 1024) * nbx < TWO32),
        ("total * wpf < 2^32", total * wpf < TWO32), ("total < 2^31", total < TWO31)])
    linear = want and exact
    if linear:
        return True, (total, 1, 1), (wg, 1, 1)
    per_wg = min(nbx, cap)
    bx = (per_wg + 63) // 64 * 64
    return False, (nby, n, (nbx + bx - 1) // bx), (bx, 1, 1)


def generic_launch(p, h265, cf=1):
    """launch_generic_t (its own dim3), dbk_launch_h265 / dbk_launch_h265_cf (dbksel::generic_grid / generic_block)"""
    grid, block = ((p.nbx + 63) // 64, (p.nby + 3) // 4, p.n), (64, 4, 1)
    t = "u8" if p.sb == 1 else "u16"
    if not h265:
        return Launch("dbk_generic_kernel", (t, int(p.chroma), int(p.qpmap > 0)), grid, block)
    if p.chroma and cf != 1:
        return Launch("dbk_h265_cf_kernel", (t, cf), grid, block)
    return Launch("dbk_h265_kernel", (t, int(p.chroma)), grid, block)


def packed_launch(p, h265, census=_NULL, cf=1):
    """launch_packed_sel<Gen::kRef> / <Gen::kH265> after fold_operands (deblock_kernels.hip): the format is a template argument
    only for spec-exact chroma of 4:2:2 / 4:4:4 with a QP map (the _cf kernels); with one QP those planes take the 4:2:0 kernels"""
    lin, grid, block = plan_packed(p, census)
    L, wide, qm = int(lin), int(p.sb == 2 and not p.chroma and p.max_v > 2047), int(p.qpmap > 0)
    if h265 and p.chroma and cf != 1 and qm:
        return Launch("dbk_packed16_h265_cf_kernel" if p.sb == 2 else "dbk_packed_h265_cf_kernel", (L, cf), grid, block)
    if h265:
        if p.sb == 2:
            return Launch("dbk_packed16_h265_kernel", (int(p.chroma), L, qm, wide), grid, block)
        return Launch("dbk_packed_h265_kernel", (int(p.chroma), L, qm), grid, block)
    if p.sb == 2 and p.chroma:
        return Launch("dbk_packed16c_kernel", (L, qm), grid, block)
    if p.sb == 2:
        return Launch("dbk_packed16_kernel", (0, 0, L, qm, wide), grid, block)
    return Launch("dbk_packed_kernel", (int(p.chroma), 0, 0, L, qm), grid, block)


def deblock_launch(p, h265, variant=KERNEL_AUTO, cf=1, census=_NULL):
    """launch (deblock_host.cpp) / launch_h265 (deblock_host_h265.cpp): a launch or an error code"""
    ok = packed_supports(p, census, "dbk_packed_h265_supports" if h265 else "dbk_packed_supports")
    if variant == KERNEL_PACKED and not ok:
        return ERR_UNSUPPORTED
    if variant == KERNEL_GENERIC or not ok:
        return generic_launch(p, h265, cf)
    return packed_launch(p, h265, census, cf)


def multi_supports(planes, census=_NULL):
    """dbk_multi_supports after planes_fuse's own checks (deblock_host.cpp)"""
    if not (2 <= len(planes) <= 3) or planes[0].chroma or not all(q.chroma for q in planes[1:]):
        return False
    p0 = planes[0]
    each = all([packed_supports(q, census) for q in planes])
    return _all(census, "dbk_multi_supports", [
        ("same sample width", all(q.sb == p0.sb for q in planes)), ("no QP map", not any(q.qpmap for q in planes)),
        ("same max_v", all(q.max_v == p0.max_v for q in planes)), ("same n_frames", all(q.n == p0.n for q in planes)),
        ("chroma nbx <= luma nbx", all(q.nbx <= p0.nbx for q in planes)), ("each plane packed", each),
        ("luma nbx <= 1024", p0.nbx <= 1024)])


def multi_launch(planes):
    """dbk_launch_packed_multi"""
    p0 = planes[0]
    rows = sum(q.nby for q in planes)
    bx = (min(p0.nbx, WG_CAP) + 63) // 64 * 64
    grid = (rows, p0.n, (p0.nbx + bx - 1) // bx)
    if p0.sb == 1:
        return Launch("dbk_packed_multi_kernel", (0,), grid, (bx, 1, 1))
    return Launch("dbk_packed16_multi_kernel", (int(p0.max_v > 2047),), grid, (bx, 1, 1))


def sao_strips(p):
    """(tx, tpf, total) of dbk_launch_sao's strip grid: dbksel::sao_strips"""
    tx = (p.w + SAO_STRIP - 1) // SAO_STRIP
    tpf = tx * ((p.h + 63) // 64)
    return tx, tpf, tpf * p.n


def sao_swz(p, census=_NULL):
    tx, tpf, total = sao_strips(p)
    return _all(census, "sao swz", [("total + 8 < 2^31", total + 8 < TWO31),                     # dbksel::renumbered_grid: exact
                                    ("(total + 8) * tpf < 2^32", (total + 8) * tpf < TWO32),
                                    ("tpf * tx < 2^32", tpf * tx < TWO32)])


def sao_launch(p, census=_NULL):
    """dbk_launch_sao (launch_sao<false> in sao.hip), the product library"""
    tx, tpf, total = sao_strips(p)
    swz = sao_swz(p, census)
    grid = ((total + 7) // 8 * 8, 1, 1) if swz else (tx, (p.h + 63) // 64, p.n)  # dbksel::sao_grid
    block = (SAO_STRIP, 1, 1)
    if p.sb == 1:
        a8 = _all(census, "sao aligned8", [  # launch_sao: aligned8
            ("pitch % 8", p.P % 8 == 0), ("frame_stride % 8", p.fs % 8 == 0), ("src % 8", p.src_off % 8 == 0),
            ("dst % 8", p.dst_off % 8 == 0), ("pitch * h < 2^31", p.P * p.h < TWO31)])
        if a8:
            return Launch("sao8_kernel", (int(swz), 4), grid, block)
        return Launch("sao_kernel", ("u8", int(swz), 0), grid, block)
    pk = _all(census, "sao pk16", [  # launch_sao: pk16
        ("max_v <= 4095", p.max_v <= 4095), ("pitch % 4", p.P % 4 == 0), ("frame_stride % 4", p.fs % 4 == 0),
        ("src % 4", p.src_off % 4 == 0), ("dst % 4", p.dst_off % 4 == 0), ("pitch * h < 2^31", p.P * p.h < TWO31)])
    return Launch("sao_kernel", ("u16", int(swz), int(swz and pk)), grid, block)


def sao_twin_launch(p, twin, census=_NULL):
    """launch_sao<false> with boundary bytes (twin "nox") and launch_sao<true> (twin "g4": dbk_launch_sao_g4, planes in multiples of
    4) in sao.hip: dbk_launch_sao's grid and predicates -- the demand for multiples of 8 is met by the first and waived for the second
    -- and the kernel's twin of that name"""
    l = sao_launch(p, census)
    return dataclasses.replace(l, kernel=l.kernel.replace("_kernel", "_%s_kernel" % twin))


def sao_sp_launch(p, census=_NULL):
    """dbk_launch_sao_sp (sao_sp.hip) on a plane of p.w x p.h Cb / Cr pairs (p.P, p.fs in bytes): the strips are 256 pairs by 64 rows,
    so dbksel::sao_grid is sao_launch's on the pair counts; dbk_sao_sp_packed_supports chooses the packed kernels"""
    tx, tpf, total = sao_strips(p)
    swz = sao_swz(p, census)
    grid = ((total + 7) // 8 * 8, 1, 1) if swz else (tx, (p.h + 63) // 64, p.n)
    piece = 16 * p.sb  # a lane's row piece
    packed = _all(census, "sao sp packed", [
        ("pitch %% %d" % piece, p.P % piece == 0), ("frame_stride %% %d" % piece, p.fs % piece == 0), ("src %% %d" % piece, p.src_off % piece == 0),
        ("dst %% %d" % piece, p.dst_off % piece == 0), ("pitch * h < 2^31", p.P * p.h < TWO31), ("max_v", p.max_v == 255 if p.sb == 1 else p.max_v <= 4095)])
    if packed:
        return Launch("sao8_sp_kernel" if p.sb == 1 else "sao16_sp_kernel", (int(swz),), grid, (SAO_STRIP, 1, 1))
    return Launch("sao_sp_kernel", ("u8" if p.sb == 1 else "u16", int(swz)), grid, (SAO_STRIP, 1, 1))


def fused_tiles(p):
    tw, th = FUSED_TILE[p.sb]
    tx, ty = (p.w + tw - 1) // tw, (p.h + th - 1) // th
    return tx, ty, tx * ty


def fused_supports(p, census=_NULL):
    """dbk_deblock_sao_supports for operands that passed sao_args / planes_to_args: by_count 0,
    equal max_v, band_shift = bit depth - 5 and equal geometry always hold there"""
    if not census.clause("dbk_deblock_sao_supports", "max_v <= 4095", p.max_v <= 4095):
        return False
    if not packed_supports(p, census):
        return False
    al = 4 * p.sb
    tiles = fused_tiles(p)[2]
    return _all(census, "dbk_deblock_sao_supports", [
        ("n_frames <= 65535", p.n <= 65535),
        ("pitch * h < 2^31", p.P * p.h < TWO31), ("dst %% %d" % al, p.dst_off % al == 0),
        ("tiles * n + 8 < 2^31", tiles * p.n + 8 < TWO31), ("tiles^2 < 2^32", tiles * tiles < TWO32),
        ("(tiles * n + 8) * tiles < 2^32", (tiles * p.n + 8) * tiles < TWO32)])


def fused_grid(p):
    """fused_grid -> dbksel::renumbered_grid: 1-D, a multiple of 8"""
    total = fused_tiles(p)[2] * p.n
    return (total + 7) // 8 * 8


def fused_launch(p, h265, cf=1):
    """launch_fused<Gen::kRef> / <Gen::kH265> (dbk_launch_deblock_sao / _h265_cf), scalar QP"""
    k = "dbk_sao_fused%s%s_kernel" % ("" if p.sb == 1 else "16", "_h265" if h265 else "")
    args = (int(p.chroma), 0) if p.sb == 1 else (int(p.chroma), int(not p.chroma and p.max_v > 2047), 0)
    return Launch(k, args, (fused_grid(p), 1, 1), (FUSED_THREADS[p.sb], 1, 1), FUSED_LDS[p.sb])


def fused_multi_launch(planes, h265):
    """launch_fused_multi<Gen::kRef> / <Gen::kH265> (dbk_launch_deblock_sao_multi[_h265_cf]) of a 4:2:0 picture; QPMAP is folded
    from the luma plane's map (fold_operands)"""
    p0 = planes[0]
    k = "dbk_sao_fused_multi%s_kernel" % ("_h265" if h265 else "")
    return Launch(k, (p0.sb, int(p0.sb == 2 and p0.max_v > 2047), int(p0.qpmap > 0)), (sum(fused_grid(q) for q in planes), 1, 1),
                  (FUSED_THREADS[p0.sb], 1, 1), FUSED_LDS[p0.sb])


def rows_x2_launch(p, ctb_log2_w, per_frame):
    """dbk_launch_sao_rows_x2: one thread per square-CTB entry"""
    s = 1 << ctb_log2_w
    total = ((p.w + s - 1) // s) * ((p.h + s - 1) // s) * (p.n if per_frame else 1)
    return Launch("sao_rows_x2_kernel", (), ((total + 255) // 256, 1, 1), (256, 1, 1))


# ---- the entries ----------------------------------------------------------------------------------------------------------

def _sao_args_rc(p):
    """sao_args (deblock_host_h265.cpp) for the operands the cases vary"""
    if not api_align_ok(p):
        return ERR_UNSUPPORTED
    if p.n > 65535 or p.h > 65535:
        return ERR_ARG
    return 0


def _dbk_args_rc(p):
    """planes_to_args (deblock_host.cpp)"""
    if not api_align_ok(p):
        return ERR_UNSUPPORTED
    if p.n > 65535:
        return ERR_UNSUPPORTED
    return 0


def _dbk_sao_plane(p, h265, fused, cf, census):
    """deblock_sao_plane[_h265[_cf]] (deblock_host_h265.cpp)"""
    can = fused_supports(p, census)
    if fused == FUSED_ON and not can:
        return ERR_UNSUPPORTED
    if can and fused != FUSED_OFF:
        return [fused_launch(p, h265, cf)]
    first = dataclasses.replace(p, dst_off=0)  # the scratch plane: a fresh allocation
    second = dataclasses.replace(p, src_off=0)
    return [deblock_launch(first, h265, KERNEL_AUTO, cf, census), sao_launch(second, census)]


def predict(case, census=_NULL):
    """the error code the entry returns, or the list of Launch it enqueues"""
    pl, e = case.planes, case.entry
    h265 = "h265" in e
    if e in ("filter", "filter_h265"):
        p = pl[0]
        rc = _dbk_args_rc(p)
        if rc:
            return rc
        r = deblock_launch(p, h265, case.variant, case.cf, census)
        return r if isinstance(r, int) else [r]
    if e == "filter_planes":
        for p in pl:  # hevc_deblocking_filter_device_planes
            rc = _dbk_args_rc(p) or (ERR_ARG if p.n != pl[0].n else 0)
            if rc:
                return rc
        if case.variant in (KERNEL_AUTO, KERNEL_PACKED) and multi_supports(pl, census):
            return [multi_launch(pl)]
        out = [deblock_launch(p, False, case.variant, 1, census) for p in pl]
        bad = [r for r in out if isinstance(r, int)]
        return bad[0] if bad else out
    if e == "sao":
        p = pl[0]
        rc = _sao_args_rc(p)
        if rc:
            return rc
        out = [sao_launch(p, census)]
        if p.chroma and case.cf == 2:
            out.insert(0, rows_x2_launch(p, case.ctb_log2, case.params_per_frame))
        return out
    if e in ("dbk_sao", "dbk_sao_h265"):
        p = pl[0]
        rc = _sao_args_rc(p) or _dbk_args_rc(p)
        if rc:
            return rc
        out = _dbk_sao_plane(p, h265, case.fused, case.cf, census)
        if isinstance(out, list) and p.chroma and case.cf == 2:
            out.insert(0, rows_x2_launch(p, case.ctb_log2, case.params_per_frame))
        return out
    if e in ("dbk_sao_planes", "dbk_sao_h265_planes", "dbk_sao_h265_planes_cf"):
        for p in pl:
            rc = _sao_args_rc(p) or _dbk_args_rc(p)
            if rc:
                return rc
        can = [fused_supports(p, census) for p in pl]
        one = (len(pl) >= 2 and case.fused != FUSED_OFF and not pl[0].chroma and all(can) and
               all(q.sb == pl[0].sb and q.bd == pl[0].bd and q.chroma for q in pl[1:]))
        pre = [rows_x2_launch(q, case.ctb_log2 - (i > 0), case.params_per_frame)
               for i, q in enumerate(pl) if i > 0 and h265 and case.cf == 2]
        if one:
            return pre + [fused_multi_launch(pl, h265)]
        if case.fused == FUSED_ON and not all(can):
            return ERR_UNSUPPORTED
        out = pre
        for q in pl:
            out += _dbk_sao_plane(q, h265, case.fused, case.cf, census)
        return out
    raise ValueError(e)


# ---- bounds solved from the restatement -------------------------------------------------------------------------------------

def first_false(pred, lo, hi):
    """smallest x in (lo, hi] with pred(x) false, given pred(lo) true and pred(hi) false (pred monotone)"""
    assert pred(lo) and not pred(hi), (lo, hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if pred(mid):
            lo = mid
        else:
            hi = mid
    return hi


def plane_h_2g(width_bytes):
    """largest multiple-of-8 plane height whose plane stays under 2^31 bytes at this pitch"""
    return (TWO31 - 1) // width_bytes // 8 * 8


def sao_swz_tx_limit(h=64, n=1):
    """first strip count per row (8-bit, strips of 256) at which the SAO grid leaves the renumbered (swz) form"""
    return first_false(lambda tx: sao_swz(Plane(tx * SAO_STRIP, h, n=n)), 1, 1 << 20)


def fused_tile_limit(h=128, n=1):
    """first 8-bit tile count per row at which the fused kernel's tile guard fails"""
    tw = FUSED_TILE[1][0]
    return first_false(lambda t: fused_supports(Plane(t * tw, h, n=n)), 1, 1 << 20)


def linear_height_limit(w=32768):
    """first multiple-of-8 height at which plan_packed leaves the row-major map for an 8-bit plane of width w"""
    return 8 * first_false(lambda k: plan_packed(Plane(w, 8 * k))[0], 1, 1 << 16)


def multi_width_limit():
    """first luma width (multiple of 8) at which Y+U+V no longer go out as one launch"""
    ok = lambda k: multi_supports([Plane(8 * k, 16), Plane(8, 8, chroma=True), Plane(8, 8, chroma=True)])
    return 8 * first_false(ok, 1, 4096)


# ---- the case list ----------------------------------------------------------------------------------------------------------

def cases():
    out = []
    add = out.append
    # 2 GiB plane guard: 8-bit width 32768 at the largest height under 2^31, and the same plane 8 bytes wider in pitch
    H2 = plane_h_2g(32768)
    for pitch in (32768, 32776):
        inside = pitch * H2 < TWO31
        tag = "2g_%s" % ("in" if inside else "out")
        add(Case("filter_" + tag, "filter", [Plane(32768, H2, pitch=pitch)], giant=True))
        add(Case("filter_h265_" + tag, "filter_h265", [Plane(32768, H2, pitch=pitch)], giant=True))
        add(Case("sao_" + tag, "sao", [Plane(32768, H2, pitch=pitch)], giant=True))
        add(Case("dbk_sao_" + tag, "dbk_sao", [Plane(32768, H2, pitch=pitch)], giant=True))
        if not inside:
            add(Case("filter_packed_" + tag, "filter", [Plane(32768, H2, pitch=pitch)], variant=KERNEL_PACKED, giant=True))
            add(Case("dbk_sao_on_" + tag, "dbk_sao", [Plane(32768, H2, pitch=pitch)], fused=FUSED_ON, giant=True))
        # 16-bit: 16384 samples at the same byte pitches (SAO: the 3-D grid, (total + 8) * tpf = 65544 * 65536 >= 2^32)
        add(Case("filter16_" + tag, "filter", [Plane(16384, H2, bd=10, pitch=pitch)], giant=True))
        add(Case("sao16_" + tag, "sao", [Plane(16384, H2, bd=10, pitch=pitch)], giant=True))
    # SAO swz guard: one strip row, strips of 256 samples
    T = sao_swz_tx_limit()
    for tx in (T - 1, T):
        add(Case("sao_swz_%d" % tx, "sao", [Plane(tx * SAO_STRIP, 64)], giant=True))
    add(Case("sao_swz_65536", "sao", [Plane(65536 * SAO_STRIP, 64)], giant=True, gpu=False))  # tpf * tx = 2^32
    # fused tile guard: one tile row of 192 x 128 tiles
    F = fused_tile_limit()
    for t in (F - 1, F):
        add(Case("dbk_sao_h265_tiles_%d" % t, "dbk_sao_h265", [Plane(t * 192, 128)], giant=True))
        if t == F:
            add(Case("dbk_sao_h265_on_tiles_%d" % t, "dbk_sao_h265", [Plane(t * 192, 128)], fused=FUSED_ON, giant=True))
    add(Case("dbk_sao_h265_tiles_65536", "dbk_sao_h265", [Plane(65536 * 192, 128)], giant=True, gpu=False))  # tiles^2 = 2^32
    # plan_packed linear guard at width 32768: the (nb + 1024) * nbx clause
    HL = linear_height_limit(32768)
    for h in (HL - 8, HL):
        add(Case("filter_lin_w32768_h%d" % h, "filter", [Plane(32768, h)]))
        add(Case("filter_h265_lin_w32768_h%d" % h, "filter_h265", [Plane(32768, h)]))
    # nbx > cap: widths 8 * cap - 8 (nbx = cap) and 8 * cap (nbx = cap + 1); 1-row planes (wpf >= 2 fails)
    for w in (8 * WG_CAP - 8, 8 * WG_CAP):
        add(Case("filter_nbx%d" % (w // 8 + 1), "filter", [Plane(w, 64)]))
        add(Case("filter16_nbx%d" % (w // 8 + 1), "filter", [Plane(w, 32, bd=10)]))
        add(Case("filter_h265_nbx%d" % (w // 8 + 1), "filter_h265", [Plane(w, 32, bd=12)]))
    add(Case("filter_nbx513_wpf1", "filter", [Plane(8 * WG_CAP, 8)]))
    # alignment: 8-bit pitch residues {0, 4, 1}; 16-bit {0, 2, 4, 6} bytes; base offsets 1..7 on src and dst
    for r in (0, 4, 1):
        P = 264 + r
        add(Case("filter_pitch8_r%d" % r, "filter", [Plane(256, 64, pitch=P, n=2)]))
        add(Case("sao_pitch8_r%d" % r, "sao", [Plane(256, 64, pitch=P, n=2)]))
        add(Case("dbk_sao_pitch8_r%d" % r, "dbk_sao", [Plane(256, 64, pitch=P, n=2)]))
    for r in (0, 2, 4, 6):
        P = 2 * 264 + r
        add(Case("filter16_pitch_r%d" % r, "filter", [Plane(256, 64, bd=10, pitch=P, n=2)]))
        add(Case("sao16_pitch_r%d" % r, "sao", [Plane(256, 64, bd=10, pitch=P, n=2)]))
    for off in range(1, 8):
        for side in ("src", "dst"):
            kw = {side + "_off": off}
            add(Case("filter_%s%d" % (side, off), "filter", [Plane(128, 64, pitch=136, n=2, **kw)]))
            add(Case("sao_%s%d" % (side, off), "sao", [Plane(128, 64, pitch=136, n=2, **kw)]))
            add(Case("dbk_sao_h265_%s%d" % (side, off), "dbk_sao_h265", [Plane(128, 64, pitch=136, n=2, **kw)]))
            if off % 2 == 0:
                add(Case("sao16_%s%d" % (side, off), "sao", [Plane(128, 64, bd=10, pitch=272, n=2, **kw)]))
                add(Case("filter16_%s%d" % (side, off), "filter", [Plane(128, 64, bd=10, pitch=272, n=2, **kw)]))
    add(Case("filter16_fs_r4", "filter", [Plane(128, 64, bd=10, n=2, fs_pad=4)]))
    add(Case("filter16_fs_r8", "filter", [Plane(128, 64, bd=10, n=2, fs_pad=8)]))
    add(Case("sao_fs_r4", "sao", [Plane(128, 64, n=2, fs_pad=4)]))
    # Y+U+V in one launch: luma widths on both sides of nbx = 1024
    MW = multi_width_limit()
    for w in (MW - 8, MW):
        for bd in (8, 10):
            ys = [Plane(w, 16, bd=bd, n=2), Plane(4088, 8, bd=bd, n=2, chroma=True), Plane(4088, 8, bd=bd, n=2, chroma=True)]
            add(Case("planes_w%d_bd%d" % (w, bd), "filter_planes", ys))
    add(Case("planes_mixed_bd", "filter_planes", [Plane(64, 16), Plane(32, 8, bd=10, chroma=True), Plane(32, 8, bd=10, chroma=True)]))
    add(Case("planes_wide_chroma", "filter_planes", [Plane(64, 16), Plane(128, 8, chroma=True), Plane(32, 8, chroma=True)]))
    add(Case("planes_generic", "filter_planes", [Plane(64, 16), Plane(32, 8, chroma=True), Plane(32, 8, chroma=True)],
             variant=KERNEL_GENERIC))
    add(Case("planes_u16_bd13", "filter_planes", [Plane(64, 16, bd=13), Plane(32, 8, bd=13, chroma=True), Plane(32, 8, bd=13, chroma=True)]))
    add(Case("planes_mixed_maxv", "filter_planes", [Plane(64, 16, bd=10), Plane(32, 8, bd=12, chroma=True),
                                                    Plane(32, 8, bd=12, chroma=True)]))
    add(Case("planes_mixed_n", "filter_planes", [Plane(64, 16, n=2), Plane(32, 8, chroma=True), Plane(32, 8, chroma=True)]))
    add(Case("planes_qpmap", "filter_planes", [Plane(64, 16, n=2, qpmap=4), Plane(32, 8, n=2, chroma=True),
                                               Plane(32, 8, n=2, chroma=True)]))
    add(Case("planes_qpmap_bd10", "filter_planes", [Plane(64, 16, bd=10, qpmap=3), Plane(32, 8, bd=10, chroma=True),
                                                    Plane(32, 8, bd=10, chroma=True)]))
    add(Case("filter_qpmap_bd13", "filter", [Plane(128, 64, bd=13, n=2, qpmap=5)]))
    add(Case("planes_src4", "filter_planes", [Plane(64, 16, pitch=72), Plane(32, 8, chroma=True, src_off=4), Plane(32, 8, chroma=True)]))
    add(Case("dbk_sao_planes_w%d" % (MW - 8), "dbk_sao_planes",
             [Plane(MW - 8, 16), Plane(4088, 8, chroma=True), Plane(4088, 8, chroma=True)]))
    add(Case("dbk_sao_planes_bd13", "dbk_sao_planes", [Plane(64, 16, bd=13), Plane(32, 8, bd=13, chroma=True),
                                                       Plane(32, 8, bd=13, chroma=True)]))
    add(Case("dbk_sao_planes_on_bd13", "dbk_sao_planes", [Plane(64, 16, bd=13), Plane(32, 8, bd=13, chroma=True),
                                                          Plane(32, 8, bd=13, chroma=True)], fused=FUSED_ON))
    # spec-exact Y+U+V of a 4:2:0 batch: hevc_deblock_sao_h265_device_planes, and the _cf entry with chroma_format_idc 1
    yuv = lambda bd: [Plane(128, 64, bd=bd, n=2), Plane(64, 32, bd=bd, n=2, chroma=True), Plane(64, 32, bd=bd, n=2, chroma=True)]
    for entry in ("dbk_sao_h265_planes", "dbk_sao_h265_planes_cf"):
        for bd in (8, 10, 13):
            add(Case("%s_420_bd%d" % (entry, bd), entry, yuv(bd), ctb_log2=4))
        add(Case("%s_420_on_bd13" % entry, entry, yuv(13), ctb_log2=4, fused=FUSED_ON))
    # frame-count limit on 8 x 8 planes: 65535 frames are fused, 65536 rejected by the argument checks
    for n in (65535, 65536):
        add(Case("dbk_sao_n%d" % n, "dbk_sao", [Plane(8, 8, n=n)], ctb_log2=3))
        add(Case("dbk_sao_h265_n%d" % n, "dbk_sao_h265", [Plane(8, 8, n=n)], ctb_log2=3))
        add(Case("sao_n%d" % n, "sao", [Plane(8, 8, n=n)], ctb_log2=3))
        add(Case("filter_n%d" % n, "filter", [Plane(8, 8, n=n)]))
    # bit depths: SAO and the 16-bit paths at 10, 12 and 13..16 bit
    for bd in (10, 12, 13, 14, 15, 16):
        add(Case("filter_bd%d" % bd, "filter", [Plane(128, 64, bd=bd, n=2)]))
        add(Case("filter_packed_bd%d" % bd, "filter", [Plane(128, 64, bd=bd)], variant=KERNEL_PACKED))
        add(Case("filter_h265_bd%d" % bd, "filter_h265", [Plane(128, 64, bd=bd, n=2)]))
        add(Case("filter_h265_c_bd%d" % bd, "filter_h265", [Plane(64, 32, bd=bd, chroma=True)]))
        add(Case("sao_bd%d" % bd, "sao", [Plane(128, 64, bd=bd, n=2)], ctb_log2=4))
        add(Case("dbk_sao_bd%d" % bd, "dbk_sao", [Plane(128, 64, bd=bd)], ctb_log2=5))
        add(Case("dbk_sao_h265_bd%d" % bd, "dbk_sao_h265", [Plane(128, 64, bd=bd)], ctb_log2=5))
        add(Case("dbk_sao_h265_on_bd%d" % bd, "dbk_sao_h265", [Plane(128, 64, bd=bd)], ctb_log2=5, fused=FUSED_ON))
    for bd in (8, 10, 13):  # 4:2:2 chroma deblocking through the _cf entry
        add(Case("filter_h265_422_bd%d" % bd, "filter_h265", [Plane(96, 64, bd=bd, n=2, chroma=True)], cf=2))
    # 4:2:2 SAO parameters: tight and padded params_stride, shared and per-frame parameters
    for pad, per_frame in ((0, False), (3, False), (0, True), (5, True)):
        tag = "pad%d_%s" % (pad, "pf" if per_frame else "shared")
        add(Case("sao_422_" + tag, "sao", [Plane(96, 64, n=2, chroma=True)], cf=2, ctb_log2=4, params_pad=pad,
                 params_per_frame=per_frame))
        add(Case("sao16_422_" + tag, "sao", [Plane(96, 64, bd=10, n=2, chroma=True)], cf=2, ctb_log2=4, params_pad=pad,
                 params_per_frame=per_frame))
        add(Case("dbk_sao_h265_422_" + tag, "dbk_sao_h265", [Plane(96, 64, n=2, chroma=True)], cf=2, ctb_log2=4,
                 params_pad=pad, params_per_frame=per_frame))
        add(Case("dbk_sao_h265_planes_422_" + tag, "dbk_sao_h265_planes_cf",
                 [Plane(192, 64, n=2), Plane(96, 64, n=2, chroma=True), Plane(96, 64, n=2, chroma=True)], cf=2, ctb_log2=5,
                 params_pad=pad, params_per_frame=per_frame))
    return out


def by_name():
    return {c.name: c for c in cases()}


# ---- flat planes with random windows, and their expected output -----------------------------------------------------------

HALO = 16   # >= what any output sample depends on: 4 read + 3 written per edge, both directions, plus SAO's one neighbour


@dataclasses.dataclass
class Windows:
    """a plane of w x h samples, `flat` everywhere except random content in `content` (y0, y1, x0, x1) rectangles; output is
    checked against the oracle in `check` (content + HALO, clipped) and must equal `flat` elsewhere"""
    w: int
    h: int
    bd: int
    flat: int
    content: list
    seed: int = 1

    def grow(self, r, align):
        """rectangle r grown by HALO, outward to a multiple of align, clipped to the plane"""
        y0, y1, x0, x1 = r
        lo = lambda v: max(0, (v - HALO) // align * align)
        hi = lambda v, lim: min(lim, -(-(v + HALO) // align) * align)
        return lo(y0), hi(y1, self.h), lo(x0), hi(x1, self.w)

    def check(self, align=8):
        """content grown by HALO, outward to a multiple of align (whole CTBs for SAO), clipped to the plane"""
        return [self.grow(r, align) for r in self.content]

    def window_data(self, i):
        y0, y1, x0, x1 = self.content[i]
        rng = np.random.default_rng(self.seed * 1000 + i)
        top = (1 << self.bd) - 1
        # blocky content with steps at the 8-sample grid so that every filter decision is exercised
        base = rng.integers(top // 4, 3 * top // 4 + 1, ((y1 - y0) // 8 + 1, (x1 - x0) // 8 + 1))
        a = np.kron(base, np.ones((8, 8), np.int64))[: y1 - y0, : x1 - x0] + rng.integers(-3, 4, (y1 - y0, x1 - x0)) * (1 << (self.bd - 8))
        a[:8, :8] = rng.integers(0, top + 1, (8, 8))
        return np.clip(a, 0, top).astype(np.uint8 if self.bd == 8 else np.uint16)

    def dense(self):
        """the whole plane as an array (planes small enough to hold)"""
        a = np.full((self.h, self.w), self.flat, np.uint8 if self.bd == 8 else np.uint16)
        for i, (y0, y1, x0, x1) in enumerate(self.content):
            a[y0:y1, x0:x1] = self.window_data(i)
        return a

    def crop(self, y0, y1, x0, x1):
        """input samples of the rectangle (content windows overlaid on flat)"""
        a = np.full((y1 - y0, x1 - x0), self.flat, np.uint8 if self.bd == 8 else np.uint16)
        for i, (cy0, cy1, cx0, cx1) in enumerate(self.content):
            iy0, iy1, ix0, ix1 = max(y0, cy0), min(y1, cy1), max(x0, cx0), min(x1, cx1)
            if iy0 < iy1 and ix0 < ix1:
                a[iy0 - y0:iy1 - y0, ix0 - x0:ix1 - x0] = self.window_data(i)[iy0 - cy0:iy1 - cy0, ix0 - cx0:ix1 - cx0]
        return a


def standard_windows(w, h, bd, flat, pitch_bytes, seed=1, size=(64, 256), grid=8):
    """content around the first and last block rows and columns, the middle, and the row holding byte offset 2^31"""
    wy, wx = size
    al = lambda v: v // grid * grid
    ys = sorted({0, al(max(0, h - wy)), al(max(0, h // 2 - wy // 2))} |
                ({al(min(max(0, TWO31 // pitch_bytes - wy // 2), h - wy))} if pitch_bytes * h > TWO31 // 2 else set()))
    xs = sorted({0, al(max(0, w - wx)), al(max(0, w // 2 - wx // 2))})
    content = [(y, min(h, y + wy), x, min(w, x + wx)) for y, x in itertools.product(ys, xs)]
    if pitch_bytes * h > TWO31 // 2:  # the samples at byte offset 2^31 itself
        y = TWO31 // pitch_bytes
        x = (TWO31 - y * pitch_bytes) // ((bd > 8) + 1)
        if x < w:
            content.append((al(max(0, min(y - wy // 2, h - wy))), min(h, al(max(0, min(y - wy // 2, h - wy))) + wy),
                            al(max(0, min(x - wx // 2, w - wx))), min(w, al(max(0, min(x - wx // 2, w - wx))) + wx)))
    return Windows(w, h, bd, flat, content, seed)


def sao_params_for(w, h, ctb_log2, seed, bd, win=None):
    """SAO parameters of a windowed plane: random in CTBs that touch a check window, edge offset or off elsewhere"""
    from oracle import h265
    p = h265.random_sao_params(w, h, ctb_log2, seed, bit_depth=bd)
    if win is not None:
        s = 1 << ctb_log2
        touch = np.zeros(p.shape, bool)
        for y0, y1, x0, x1 in win.check(s):
            touch[y0 // s:(y1 + s - 1) // s, x0 // s:(x1 + s - 1) // s] = True
        band = (p["type"] == 1) & ~touch
        p["type"][band] = 2
        p["cls"][band] = p["cls"][band] & 3
        off = p["offset"][band].astype(np.int64)
        off[:, 0:2] = np.abs(off[:, 0:2])
        off[:, 2:4] = -np.abs(off[:, 2:4])
        p["offset"][band] = off
    return p


def windowed(win, op, ctb_log2=None):
    """expected output in each check window: op(crop) on the window grown by HALO (aligned to the 8-sample grid, or to the CTB
    grid for SAO, whose check windows are whole CTBs), compared on the window.  op(crop, y0, x0) -> filtered crop.  Returns [(rect, expected array)]"""
    align = 8 if ctb_log2 is None else max(8, 1 << ctb_log2)
    out = []
    for r in win.check(align):
        hy0, hy1, hx0, hx1 = win.grow(r, align)
        res = op(win.crop(hy0, hy1, hx0, hx1), hy0, hx0)
        y0, y1, x0, x1 = r
        out.append((r, res[y0 - hy0:y1 - hy0, x0 - hx0:x1 - hx0]))
    return out


def bs_arrays(h265, w, h, y0=0, x0=0, W=None, H=None):
    """bS 2 on every edge of a w x h crop at (y0, x0) of a W x H picture, 0 on the picture's own border edges and, in the
    reference mode, on horizontal edges of the first block column (flat content then stays flat in both modes: the reference
    mode otherwise filters those against zero padding).
    Layouts as load_block_bs reads them: vert[row][w / 8 + 1], hor[h / 8 + 1][cols] (rows / cols of 8, or of 4 for bS4)"""
    W, H = W or w, H or h
    u = 4 if h265 else 8
    vert = np.full((h // u, w // 8 + 1), 2, np.uint8)
    hor = np.full((h // 8 + 1, w // u), 2, np.uint8)
    gx = x0 // 8 + np.arange(w // 8 + 1)
    gy = y0 // 8 + np.arange(h // 8 + 1)
    vert[:, (gx == 0) | (gx == W // 8)] = 0
    hor[(gy == 0) | (gy == H // 8), :] = 0
    if not h265:  # the reference decides hor edges of the first block column on padding columns (ref_vectors: hor2's P/Q)
        hor[:, x0 // u + np.arange(w // u) == 0] = 0
    return vert.ravel(), hor.ravel()


def op_filter_ref(qp, bd, chroma=False, W=None, H=None, qp_map=None, ctu_log2=6):
    """reference-mode deblocking (oracle/oracle.py) with bs_arrays; a QP map only for whole planes (y0 = x0 = 0)"""
    from oracle import oracle as o

    def f(a, y0, x0):
        h, w = a.shape
        assert qp_map is None or y0 == x0 == 0
        vb, hb = bs_arrays(False, w, h, y0, x0, W or w, H or h)
        return o.filter_plane(a, qp, is_chroma=chroma, bit_depth=bd, vert_bs=vb, hor_bs=hb, qp_map=qp_map, ctu_log2=ctu_log2)
    return f


def op_filter_h265(qp, bd, c_idx=0, W=None, H=None):
    from oracle import h265

    def f(a, y0, x0):
        h, w = a.shape
        vb, hb = bs_arrays(True, w, h, y0, x0, W or w, H or h)
        return h265.filter_plane(a, qp, vb, hb, c_idx=c_idx, bit_depth=bd)
    return f


def op_sao(params, ctb_log2, bd):
    from oracle import h265
    s = 1 << ctb_log2

    def f(a, y0, x0):
        return h265.sao_plane(a, params[y0 // s:, x0 // s:], ctb_log2, bit_depth=bd)
    return f


def op_chain(*ops):
    def f(a, y0, x0):
        for op in ops:
            a = op(a, y0, x0)
        return a
    return f
