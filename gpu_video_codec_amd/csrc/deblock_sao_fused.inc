/*
 * deblock_sao_fused.inc -- included by deblock_kernels.hip (inside its anonymous namespace): deblocking and sample adaptive
 * offset (H.265 8.7.3) in ONE kernel, the deblocked samples handed from the first stage to the second through the
 * workgroup's LDS tile (SURVEY 8f rank 4: "SAO sharing the LDS-resident tile").  8-bit planes here, 16-bit containers
 * further down; one QP or a QP map.
 *
 * SAO of a sample needs the DEBLOCKED values of its eight neighbours, which other offset blocks -- other lanes, other waves --
 * produce, so the two stages cannot share registers.  A workgroup therefore owns a tile of 192 x 128 output samples:
 *   1. its 448 lanes deblock the 25 x 17 offset blocks that cover the tile plus one sample of halo all round (image columns
 *      X0-4 .. X0+195, rows Y0-4 .. Y0+131; the blocks on the tile's rim are deblocked by the neighbouring workgroup as well:
 *      425 blocks for 384 blocks' worth of output, 10.7 % more arithmetic, plus 23 idle lanes) exactly as the plain kernels do
 *      -- same per-block arithmetic (deblock_packed.h / deblock_packed_h265.h), same bS and border rules -- and write their
 *      8 x 8 results into the LDS tile (136 rows x 208 bytes = 28.3 KB: four workgroups per CU) instead of HBM;
 *   2. one workgroup barrier;
 *   3. waves 0..5 each take one 64 x 64 quadrant (one luma CTB when CTBs are 64 samples: one SAO type per wave), one lane per
 *      8 x 8 sample block, read the block's rows (16 bytes each) from the LDS tile as the three-row window slides down and run
 *      the SAO pass's own block procedure (sao_packed.h); the result goes to HBM.
 * Every sample is read from HBM once and written once for BOTH stages (the rim comes from the L2: tiles are numbered so that
 * neighbours run on one XCD); the deblocked picture never exists in memory.  Picture borders: out-of-image halves / rows of an
 * offset block are zeros (the reference's padding) and what the filter makes of them lands in LDS positions that SAO only
 * reads for samples whose neighbour is outside the picture -- which get no offset whatever was read (8.7.3.2).
 * Tile size, measured (tools/bench_deblock_sao.py, 64 x 4K 8-bit luma, one third of the CTBs each off / band / edge, ms per
 * call; the two launches it replaces: 0.45): 128x64 0.344, 128x128 0.321, 192x128 0.311, 128x192 0.315, 256x128 0.323,
 * 192x192 0.337, 256x192 0.374 -- a smaller rim does not pay for a workgroup whose waves wait longer at the barrier.
 */
constexpr int kFusedTile = 128;                       /* output rows per tile */
constexpr int kFusedTileW = 192;                      /* output columns per tile */
constexpr int kFusedBlocks = kFusedTile / 8 + 1;      /* 17 offset block rows per tile */
constexpr int kFusedBlocksX = kFusedTileW / 8 + 1;    /* 25 offset block columns per tile */
constexpr int kFusedPitch = 208;                      /* LDS row pitch in bytes (200 used) */
constexpr int kFusedThreads = 448;                    /* 7 waves >= 25 * 17 lanes */
constexpr int kFusedQuads = kFusedTile / 64;          /* 64 x 64 quadrants: kFusedQuadsX x kFusedQuads = 3 x 2 SAO waves */
constexpr int kFusedQuadsX = kFusedTileW / 64;
constexpr int kFusedLds = (kFusedTile + 8) * kFusedPitch;

template <bool CHROMA, int MODE, bool QPMAP, int CF = 1, bool NOX = false, bool SL = false, bool G4 = false> /* MODE 0 = reference-exact deblocking, 2 = spec-exact (H.265 8.7.2); QPMAP = QP per map unit;
                                                          CF = chroma_format_idc of a spec-exact chroma plane with a QP map;
                                                          NOX = stage 2 honours the slice / tile boundaries of nx (the _nox kernels);
                                                          SL = per-slice deblocking offsets from sl (the _sl kernels: MODE 2, QPMAP and NOX set,
                                                          the map and the bytes of nx may be absent);
                                                          G4 = with SL: a plane whose sizes are multiples of 4 (the _g4 kernels: g4_right /
                                                          g4_below in stage 1, partial blocks of 4 columns / 4 rows in stage 2) */
__device__ __forceinline__ void fused_body(const DbkArgs &a, const DbkH265Args *hx, const DbkSaoArgs &s, const DbkFusedGrid &g, uint8_t *tile,
                                           uint32_t id /* workgroup number inside this plane's part of the grid */, const DbkSaoNox *nx = nullptr,
                                           [[maybe_unused]] const DbkSlOffs *sl = nullptr)
{
    /* workgroups are dealt round-robin over the 8 XCDs (an observation used for speed only): renumber them so that each XCD
     * works through a contiguous range of tiles.  A tile's row pieces are 200 bytes at an odd alignment, so it shares 128-byte
     * lines with its left / right neighbours and its rim rows with the tiles above / below; with neighbours on one XCD those
     * are L2 hits (HBM reads 2.0 x the plane without the renumbering) */
    const uint32_t logical = (id & 7u) * g.per_xcd + (id >> 3);
    if (logical >= g.total) return; /* padding workgroup: the whole workgroup leaves before the barrier */
    const uint32_t fr = g.tiles_per_frame == 1u ? logical : __umulhi(logical, g.magic_tpf);
    const uint32_t in_frame = logical - fr * g.tiles_per_frame;
    const uint32_t trow = g.tiles_x == 1u ? in_frame : __umulhi(in_frame, g.magic_tx);
    const int t = (int)threadIdx.x, f = (int)fr;
    const int X0 = (int)(in_frame - trow * g.tiles_x) * kFusedTileW, Y0 = (int)trow * kFusedTile;
    const int lby = t / kFusedBlocksX; /* a constant divisor: multiply and shift */
    const int lbx = t - kFusedBlocksX * lby;
    const bool in_tile = t < kFusedBlocksX * kFusedBlocks;
    const int bx = (X0 >> 3) + lbx, by = (Y0 >> 3) + lby;
    const bool active = in_tile && bx < a.nbx && by < a.nby;
    const bool lv = active && bx > 0;
    bool rv, full; /* full: all 8 rows and both halves inside the picture */
    if constexpr (G4) {
        rv = active && g4_right(a, bx);
        full = lv && rv && by > 0 && g4_below(a, by);
    } else {
        rv = active && bx < a.nbx - 1;
        full = lv && rv && by > 0 && by < a.nby - 1;
    }
    const int y0 = by * 8 - 4;
    const uint32_t xoff = (uint32_t)(bx * 8 - 4);
    const uint32_t plane_bytes = (uint32_t)a.pitch * (uint32_t)a.plane_h;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint8_t *>(a.src) + (long long)f * a.frame_stride, 0, plane_bytes, 0x00020000);

    /* ---- stage 1: this lane's offset block, HBM -> registers -> deblocked -> LDS ---- */
#ifdef HEVCDBK_DIAG
    if (a.diag_prio & 1) __builtin_amdgcn_s_setprio(3); /* experiment: the loads of a new workgroup go out ahead of everybody's arithmetic */
#endif
    uint32_t L[8], R[8];
    if (__builtin_amdgcn_ballot_w64(active && !full) == 0ull) {
        /* no lane of the wave touches the picture border: one 8-byte access per row, the row in the scalar offset */
        const uint32_t voff = full ? (uint32_t)y0 * (uint32_t)a.pitch + xoff : kOob;
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const u32x2 w = __builtin_amdgcn_raw_buffer_load_b64(rs, voff, r * (int)a.pitch, 0);
            L[r] = w.x;
            R[r] = w.y;
        }
    } else {
        const uint32_t base = (uint32_t)(y0 * (int)a.pitch) + xoff;
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const bool yv = (unsigned)(y0 + r) < (unsigned)a.plane_h;
            const uint32_t off = base + (uint32_t)r * (uint32_t)a.pitch;
            L[r] = __builtin_amdgcn_raw_buffer_load_b32(rs, (yv && lv) ? off : kOob, 0, 0);
            R[r] = __builtin_amdgcn_raw_buffer_load_b32(rs, (yv && rv) ? off + 4u : kOob, 0, 0);
        }
    }
#ifdef HEVCDBK_DIAG
    if (a.diag_prio & 1) __builtin_amdgcn_s_setprio(0);
#endif
    /* the per-block operands exactly as the plain packed kernels derive them (packed_body): one QP, or the QP map */
    /* QP-map luma: the segments' operand sets come out of the workgroup's table (deblock_packed.h, ktab_build), built by the
     * first 54 lanes once every lane's loads are under way; 3.4 KB of static LDS beside the tile (five tiles per CU still fit;
     * the 16-bit twin below keeps the per-lane construction: with the table its 39 KB tile would fit three times, not four) */
    constexpr bool KT = QPMAP && !CHROMA;
    __shared__ uint32_t ktab_lds[KT ? dbk::kKTabDwords : 1];
    if constexpr (MODE == 0) {
        const dbk::BlockBs bs = load_bs_buffer<true>(a, f, by, bx, active);
        if constexpr (KT) {
            dbk::QsTable qs = block_qp_tab<false>(a, f, by, active ? bx : 0, nullptr);
            qs.tab = ktab_setup(ktab_lds, a);
            dbk::packed_filter_luma_block_src(L, R, bs, qs);
        } else {
            const dbk::BlockQp q = block_qp<QPMAP, CHROMA>(a, f, by, active ? bx : 0);
            dbk::packed_filter_block<CHROMA, !QPMAP>(L, R, bs, q);
        }
    } else {
        int entry[4];
        load_bs_buffer_h265<2, G4>(a, f, by, bx, active, entry);
        dbk::H265Seg sg;
        if constexpr (QPMAP && SL) {
            int qpl[4], tc_off[4], beta_off[4];
            sl_block_operands<CHROMA, CF, G4>(a, hx, sl, f, by, active ? bx : 0, qpl, tc_off, beta_off);
            const dbk::H265Prm prm = {0, 0, hx->c_qp_offset, 0, 255};
            if constexpr (KT) dbk::h265_seg_rows_sl(entry, qpl, prm, ktab_setup_h265(ktab_lds, 0), tc_off, beta_off, sg);
            else dbk::h265_seg_params_sl<CHROMA, CF>(entry, qpl, prm, tc_off, beta_off, sg);
        } else if constexpr (QPMAP) {
            int qpl[4];
            block_qpl4_dev<CHROMA, CF>(a, f, by, active ? bx : 0, qpl);
            const dbk::H265Prm prm = {hx->tc_off, hx->beta_off, hx->c_qp_offset, 0, 255};
            if constexpr (KT) dbk::h265_seg_rows(entry, qpl, prm, ktab_setup_h265(ktab_lds, 0), sg);
            else dbk::h265_seg_params<CHROMA, CF>(entry, qpl, prm, sg);
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                sg.entry[i] = entry[i];
                sg.beta[i] = hx->beta_s;
                sg.tc[i] = (entry[i] & dbk::kH265BsMask) == 2 ? hx->tc_bs2 : hx->tc_bs1;
            }
        }
        if constexpr (!QPMAP && !CHROMA) {
            const dbk::H265Uni u = dbk::h265_uni(hx->beta_s, hx->tc_bs1, hx->tc_bs2);
            dbk::packed_filter_block_h265<CHROMA>(L, R, sg, &u);
        } else {
            dbk::packed_filter_block_h265<CHROMA, KT>(L, R, sg);
        }
    }
    if (in_tile) {
        uint8_t *const p = tile + (lby * 8) * kFusedPitch + lbx * 8;
#pragma unroll
        for (int r = 0; r < 8; r++) *reinterpret_cast<uint2 *>(p + r * kFusedPitch) = make_uint2(L[r], R[r]);
    }
    __syncthreads();
#ifdef HEVCDBK_DIAG
    if (a.diag_prio & 2) __builtin_amdgcn_s_setprio(2); /* experiment: a workgroup past its barrier finishes ahead of the others' stage 1 */
#endif

    /* ---- stage 2: SAO of the tile out of LDS, one 64 x 64 quadrant per wave ---- */
    const int wv = t >> 6, l = t & 63;
    if (wv >= kFusedQuadsX * kFusedQuads) return;
    const int qr = wv / kFusedQuadsX;
    const int qx0 = (wv - kFusedQuadsX * qr) * 64, qy0 = qr * 64; /* the quadrant inside the tile */
    const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc(s.dst + (long long)f * s.frame_stride, 0,
                                                                        (uint32_t)s.pitch * (uint32_t)s.plane_h, 0x00020000);
    /* one block of 8 x NROWS samples at tile position (qx, qy) */
    auto sao_block = [&](auto nrows, int qx, int qy) {
        constexpr int NROWS = decltype(nrows)::value;
        const int x = X0 + qx, ys = Y0 + qy;
        if (x >= s.plane_w || ys >= s.plane_h) return;
        [[maybe_unused]] uint32_t nox_byte = 0u;
        if constexpr (NOX && SL) nox_byte = nx->nox ? saonox::ctb_byte(*nx, f, x, ys, s.ctb_log2) : 0u; /* no bytes: nothing forbidden */
        else if constexpr (NOX) nox_byte = saonox::ctb_byte(*nx, f, x, ys, s.ctb_log2);
        const DbkSaoCtb c = s.params[(long long)f * s.params_frame_stride + (long long)(ys >> s.ctb_log2) * s.params_stride + (x >> s.ctb_log2)];
        const bool kept = s.keep && s.keep[(long long)f * s.keep_frame_stride + (long long)(ys >> 3) * s.keep_stride + (x >> 3)];
        /* image (x - 4, ys - 1 + i) is tile (qx, qy + 3 + i): the tile's origin is image (X0 - 4, Y0 - 4) */
        const uint8_t *const q0 = tile + (qy + 3) * kFusedPitch + qx;
        auto fetch = [&](int i, auto /* halo: the LDS tile holds it anyway */) {
            const uint2 lo = *reinterpret_cast<const uint2 *>(q0 + i * kFusedPitch), hi = *reinterpret_cast<const uint2 *>(q0 + i * kFusedPitch + 8);
            sao8::SaoRaw q;
            q.lh = lo.x; q.cx = lo.y; q.cy = hi.x; q.rh = hi.y;
            return q;
        };
        const uint32_t vout = (uint32_t)ys * (uint32_t)s.pitch + (uint32_t)x;
        if constexpr (G4) {
            /* the last block of a row may be 4 samples wide, the last one of a column 4 rows tall (NROWS 8 only: a plane's height
             * is a multiple of 4).  Such a block is on the picture border, so its wave takes the masked procedure anyway: the
             * narrow block has the picture's edge behind sample 3 (saonox::W4) and stores its low dword alone, the short one runs
             * the procedure for 4 rows */
            const bool w4 = x + 8 > s.plane_w, h4 = NROWS == 8 && ys + 8 > s.plane_h;
            const bool any_w4 = __builtin_amdgcn_ballot_w64(w4) != 0ull;
            auto store4 = [&](int r, uint32_t lo, uint32_t hi) {
                u32x2 w;
                w.x = lo;
                w.y = hi;
                __builtin_amdgcn_raw_buffer_store_b64(w, rd, w4 ? kOob : vout, r * (int)s.pitch, 0);
                if (any_w4) __builtin_amdgcn_raw_buffer_store_b32(lo, rd, w4 ? vout : kOob, r * (int)s.pitch, 0);
            };
            const uint32_t m = (h4 ? saonox::block_mask<4>(nox_byte, x, ys, s.plane_w, s.plane_h, s.ctb_log2)
                                   : saonox::block_mask<NROWS>(nox_byte, x, ys, s.plane_w, s.plane_h, s.ctb_log2)) |
                               (w4 ? saonox::W4 : 0u);
            if (__builtin_amdgcn_ballot_w64(m != 0u) == 0ull) {
                sao8::block<false, NROWS>(fetch, store4, x, ys, s.plane_w, s.plane_h, c, kept);
            } else if constexpr (NROWS == 8) {
                if (h4) sao8::block<2, 4, true>(fetch, store4, x, ys, s.plane_w, s.plane_h, c, kept, m);
                else sao8::block<2, 8, true>(fetch, store4, x, ys, s.plane_w, s.plane_h, c, kept, m);
            } else {
                sao8::block<2, NROWS, true>(fetch, store4, x, ys, s.plane_w, s.plane_h, c, kept, m);
            }
            return;
        }
        auto store = [&](int r, uint32_t lo, uint32_t hi) {
            u32x2 w;
            w.x = lo;
            w.y = hi;
            __builtin_amdgcn_raw_buffer_store_b64(w, rd, vout, r * (int)s.pitch, 0);
        };
        if constexpr (NOX) { /* the block's mask of directions not to look in, the picture border among them (sao_packed.h) */
            const uint32_t m = saonox::block_mask<NROWS>(nox_byte, x, ys, s.plane_w, s.plane_h, s.ctb_log2);
            if (__builtin_amdgcn_ballot_w64(m != 0u) != 0ull) sao8::block<2, NROWS>(fetch, store, x, ys, s.plane_w, s.plane_h, c, kept, m);
            else sao8::block<false, NROWS>(fetch, store, x, ys, s.plane_w, s.plane_h, c, kept);
            return;
        }
        const bool border = x == 0 || x + 8 == s.plane_w || ys == 0 || ys + NROWS >= s.plane_h;
        if (__builtin_amdgcn_ballot_w64(border) != 0ull) sao8::block<true, NROWS>(fetch, store, x, ys, s.plane_w, s.plane_h, c, kept);
        else sao8::block<false, NROWS>(fetch, store, x, ys, s.plane_w, s.plane_h, c, kept);
    };
    if (s.ctb_log2 == 5) {
        /* 32-sample CTBs (the chroma planes of a 4:2:0 picture with 64-sample luma CTBs): the quadrant's four CTBs one after
         * the other, each by the whole wave -- a lane takes 8 x 2 samples, 4 lanes across, 16 down -- so that the wave runs ONE
         * SAO path at a time with all its lanes, instead of every path that occurs among four CTBs with a quarter of them.
         * (Requesting the parameters ahead -- before the filter, and one CTB ahead in this loop -- was measured slower: +6 %
         * on luma, registers held across stage 1.) */
#pragma unroll 1
        for (int i = 0; i < 4; i++)
            sao_block(std::integral_constant<int, 2>{}, qx0 + (i & 1) * 32 + (l & 3) * 8, qy0 + (i >> 1) * 32 + (l >> 2) * 2);
    } else {
        /* a lane = one 8 x 8 sample block (the keep map's unit): with 64-sample CTBs the wave holds one CTB */
        sao_block(std::integral_constant<int, 8>{}, qx0 + (l & 7) * 8, qy0 + (l >> 3) * 8);
    }
}

/* ---- 16-bit containers (bit depth 8..12): the same structure on a 128 x 128 tile ------------------------------------
 * 17 x 17 offset blocks = 289 lanes (320 threads, five waves), the tile in LDS at 2 bytes per sample: 136 rows x 288 bytes =
 * 39 KB, four workgroups per CU; stage 2 = the packed 16-bit SAO block procedure (sao_packed.h, sao16) on the tile's 2 x 2
 * quadrants, waves 0..3.  A block's row is 16 bytes: one buffer_load_dwordx4 in, one ds_write_b128 to the tile, two ds_read_b128
 * per SAO row (samples x-4 .. x+11), one buffer_store_dwordx4 out. */
constexpr int kFused16Tile = 128;
constexpr int kFused16Blocks = kFused16Tile / 8 + 1;   /* 17 */
constexpr int kFused16Pitch = 288;                     /* LDS row pitch in bytes (272 used), a multiple of 16 */
constexpr int kFused16Threads = 320;
constexpr int kFused16Quads = kFused16Tile / 64;       /* 2 x 2 SAO waves */
constexpr int kFused16Lds = (kFused16Tile + 8) * kFused16Pitch;

template <bool CHROMA, int MODE, bool WIDE, bool QPMAP, int CF = 1, bool NOX = false, bool SL = false, bool G4 = false /* fused_body */>
__device__ __forceinline__ void fused_body16(const DbkArgs &a, const DbkH265Args *hx, const DbkSaoArgs &s, const DbkFusedGrid &g, uint8_t *tile,
                                             uint32_t id, const DbkSaoNox *nx = nullptr, [[maybe_unused]] const DbkSlOffs *sl = nullptr)
{
    const uint32_t logical = (id & 7u) * g.per_xcd + (id >> 3);
    if (logical >= g.total) return;
    const uint32_t fr = g.tiles_per_frame == 1u ? logical : __umulhi(logical, g.magic_tpf);
    const uint32_t in_frame = logical - fr * g.tiles_per_frame;
    const uint32_t trow = g.tiles_x == 1u ? in_frame : __umulhi(in_frame, g.magic_tx);
    const int t = (int)threadIdx.x, f = (int)fr;
    const int X0 = (int)(in_frame - trow * g.tiles_x) * kFused16Tile, Y0 = (int)trow * kFused16Tile;
    const int lby = t / kFused16Blocks;
    const int lbx = t - kFused16Blocks * lby;
    const bool in_tile = t < kFused16Blocks * kFused16Blocks;
    const int bx = (X0 >> 3) + lbx, by = (Y0 >> 3) + lby;
    const bool active = in_tile && bx < a.nbx && by < a.nby;
    const bool lv = active && bx > 0;
    bool rv, full;
    if constexpr (G4) {
        rv = active && g4_right(a, bx);
        full = lv && rv && by > 0 && g4_below(a, by);
    } else {
        rv = active && bx < a.nbx - 1;
        full = lv && rv && by > 0 && by < a.nby - 1;
    }
    const int y0 = by * 8 - 4;
    const uint32_t xoff = (uint32_t)(bx * 16 - 8);
    const uint32_t plane_bytes = (uint32_t)a.pitch * (uint32_t)a.plane_h;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint8_t *>(a.src) + (long long)f * a.frame_stride, 0, plane_bytes, 0x00020000);

    /* ---- stage 1 ---- */
    uint32_t W[8][4];
    if (__builtin_amdgcn_ballot_w64(active && !full) == 0ull) {
        const uint32_t voff = full ? (uint32_t)y0 * (uint32_t)a.pitch + xoff : kOob;
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const u32x4 w = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, r * (int)a.pitch, 0);
            W[r][0] = w.x; W[r][1] = w.y; W[r][2] = w.z; W[r][3] = w.w;
        }
    } else {
        const uint32_t base = (uint32_t)(y0 * (int)a.pitch) + xoff;
        const uint32_t lbits = lv ? 0u : kOob, rbits = rv ? 0u : kOob;
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const uint32_t ob = (unsigned)(y0 + r) < (unsigned)a.plane_h ? 0u : kOob;
            const uint32_t off = base + (uint32_t)r * (uint32_t)a.pitch;
            const u32x2 l = __builtin_amdgcn_raw_buffer_load_b64(rs, off | lbits | ob, 0, 0);
            const u32x2 rr = __builtin_amdgcn_raw_buffer_load_b64(rs, (off + 8u) | rbits | ob, 0, 0);
            W[r][0] = l.x; W[r][1] = l.y; W[r][2] = rr.x; W[r][3] = rr.y;
        }
    }
    if constexpr (MODE == 0) {
        const dbk::BlockBs bs = load_bs_buffer<true>(a, f, by, bx, active);
        const dbk::BlockQp q = block_qp<QPMAP, CHROMA>(a, f, by, active ? bx : 0);
        if constexpr (CHROMA) dbk::packed_filter_chroma_block16(W, bs, q, a.max_v);
        else dbk::packed_filter_luma_block16<WIDE, !QPMAP>(W, bs, q, a.max_v);
    } else {
        int entry[4];
        load_bs_buffer_h265<2, G4>(a, f, by, bx, active, entry);
        dbk::H265Seg sg;
        if constexpr (QPMAP && SL) {
            int qpl[4], tc_off[4], beta_off[4];
            sl_block_operands<CHROMA, CF, G4>(a, hx, sl, f, by, active ? bx : 0, qpl, tc_off, beta_off);
            const dbk::H265Prm prm = {0, 0, hx->c_qp_offset, a.shift, a.max_v};
            dbk::h265_seg_params_sl<CHROMA, CF>(entry, qpl, prm, tc_off, beta_off, sg);
        } else if constexpr (QPMAP) {
            int qpl[4];
            block_qpl4_dev<CHROMA, CF>(a, f, by, active ? bx : 0, qpl);
            const dbk::H265Prm prm = {hx->tc_off, hx->beta_off, hx->c_qp_offset, a.shift, a.max_v};
            dbk::h265_seg_params<CHROMA, CF>(entry, qpl, prm, sg);
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                sg.entry[i] = entry[i];
                sg.beta[i] = hx->beta_s;
                sg.tc[i] = (entry[i] & dbk::kH265BsMask) == 2 ? hx->tc_bs2 : hx->tc_bs1;
            }
        }
        if constexpr (!QPMAP && !CHROMA) {
            const dbk::H265Uni u = dbk::h265_uni(hx->beta_s, hx->tc_bs1, hx->tc_bs2);
            dbk::packed_filter_block16_h265<CHROMA, WIDE>(W, sg, a.max_v, &u);
        } else {
            dbk::packed_filter_block16_h265<CHROMA, WIDE>(W, sg, a.max_v);
        }
    }
    if (in_tile) {
        uint8_t *const p = tile + (lby * 8) * kFused16Pitch + lbx * 16;
#pragma unroll
        for (int r = 0; r < 8; r++) *reinterpret_cast<uint4 *>(p + r * kFused16Pitch) = make_uint4(W[r][0], W[r][1], W[r][2], W[r][3]);
    }
    __syncthreads();

    /* ---- stage 2 ---- */
    const int wv = t >> 6, l = t & 63;
    if (wv >= kFused16Quads * kFused16Quads) return;
    const int qr = wv / kFused16Quads;
    const int qx0 = (wv - kFused16Quads * qr) * 64, qy0 = qr * 64; /* the quadrant inside the tile */
    const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc(s.dst + (long long)f * s.frame_stride, 0,
                                                                        (uint32_t)s.pitch * (uint32_t)s.plane_h, 0x00020000);
    auto sao_block = [&](auto nrows, int qx, int qy) { /* one block of 8 x NROWS samples at tile position (qx, qy) */
        constexpr int NROWS = decltype(nrows)::value;
        const int x = X0 + qx, ys = Y0 + qy;
        if (x >= s.plane_w || ys >= s.plane_h) return;
        [[maybe_unused]] uint32_t nox_byte = 0u;
        if constexpr (NOX && SL) nox_byte = nx->nox ? saonox::ctb_byte(*nx, f, x, ys, s.ctb_log2) : 0u; /* no bytes: nothing forbidden */
        else if constexpr (NOX) nox_byte = saonox::ctb_byte(*nx, f, x, ys, s.ctb_log2);
        const DbkSaoCtb c = s.params[(long long)f * s.params_frame_stride + (long long)(ys >> s.ctb_log2) * s.params_stride + (x >> s.ctb_log2)];
        const bool kept = s.keep && s.keep[(long long)f * s.keep_frame_stride + (long long)(ys >> 3) * s.keep_stride + (x >> 3)];
        /* image (x - 4, ys - 1 + i) is tile (column qx, row qy + 3 + i): the tile's origin is image (X0 - 4, Y0 - 4) */
        const uint8_t *const q0 = tile + (qy + 3) * kFused16Pitch + qx * 2;
        auto fetch = [&](int i, auto /* halo: the LDS tile holds it anyway */) {
            const uint4 lo = *reinterpret_cast<const uint4 *>(q0 + i * kFused16Pitch), hi = *reinterpret_cast<const uint4 *>(q0 + i * kFused16Pitch + 16);
            sao16::Raw q;
            q.d[0] = lo.x; q.d[1] = lo.y; q.d[2] = lo.z; q.d[3] = lo.w; q.d[4] = hi.x; q.d[5] = hi.y; q.d[6] = hi.z; q.d[7] = hi.w;
            return q;
        };
        const uint32_t vout = (uint32_t)ys * (uint32_t)s.pitch + (uint32_t)x * 2u;
        if constexpr (G4) { /* partial blocks as in fused_body: the narrow one stores its first 8 bytes alone */
            const bool w4 = x + 8 > s.plane_w, h4 = NROWS == 8 && ys + 8 > s.plane_h;
            const bool any_w4 = __builtin_amdgcn_ballot_w64(w4) != 0ull;
            auto store4 = [&](int r, uint32_t d0, uint32_t d1, uint32_t d2, uint32_t d3) {
                u32x4 w;
                w.x = d0; w.y = d1; w.z = d2; w.w = d3;
                __builtin_amdgcn_raw_buffer_store_b128(w, rd, w4 ? kOob : vout, r * (int)s.pitch, 0);
                if (any_w4) {
                    u32x2 h;
                    h.x = d0; h.y = d1;
                    __builtin_amdgcn_raw_buffer_store_b64(h, rd, w4 ? vout : kOob, r * (int)s.pitch, 0);
                }
                asm volatile("s_nop 1" : : "v"(w.x), "v"(w.y), "v"(w.z), "v"(w.w) : "memory"); /* the wait states of `store` below */
            };
            const uint32_t m = (h4 ? saonox::block_mask<4>(nox_byte, x, ys, s.plane_w, s.plane_h, s.ctb_log2)
                                   : saonox::block_mask<NROWS>(nox_byte, x, ys, s.plane_w, s.plane_h, s.ctb_log2)) |
                               (w4 ? saonox::W4 : 0u);
            if (__builtin_amdgcn_ballot_w64(m != 0u) == 0ull) {
                sao16::block<false, NROWS>(fetch, store4, x, ys, s.plane_w, s.plane_h, c, kept, s.max_v, s.band_shift);
            } else if constexpr (NROWS == 8) {
                if (h4) sao16::block<2, 4, true>(fetch, store4, x, ys, s.plane_w, s.plane_h, c, kept, s.max_v, s.band_shift, m);
                else sao16::block<2, 8, true>(fetch, store4, x, ys, s.plane_w, s.plane_h, c, kept, s.max_v, s.band_shift, m);
            } else {
                sao16::block<2, NROWS, true>(fetch, store4, x, ys, s.plane_w, s.plane_h, c, kept, s.max_v, s.band_shift, m);
            }
            return;
        }
        auto store = [&](int r, uint32_t d0, uint32_t d1, uint32_t d2, uint32_t d3) {
            u32x4 w;
            w.x = d0; w.y = d1; w.z = d2; w.w = d3;
            __builtin_amdgcn_raw_buffer_store_b128(w, rd, vout, r * (int)s.pitch, 0);
            /* Two wait states before the next VALU instruction may overwrite w: measured on MI355X (round 3,
             * profiles/r04/store_hazard.md), the FIRST launch of a process -- the card still at its idle clock -- wrote a
             * few hundred samples per 4K frame whose value was the LDS address the compiler computes into the same register right
             * behind the store (the next row's ds_read address).  The compiler's hazard table requires a wait state after a
             * 16-byte buffer store only when soffset is NOT an SGPR; this store's soffset is one.  tools/check_store_hazard.py
             * scans the product's ISA for the sequence. */
            asm volatile("s_nop 1" : : "v"(w.x), "v"(w.y), "v"(w.z), "v"(w.w) : "memory"); /* reads w: nothing that overwrites it moves above */
        };
        if constexpr (NOX) {
            const uint32_t m = saonox::block_mask<NROWS>(nox_byte, x, ys, s.plane_w, s.plane_h, s.ctb_log2);
            if (__builtin_amdgcn_ballot_w64(m != 0u) != 0ull)
                sao16::block<2, NROWS>(fetch, store, x, ys, s.plane_w, s.plane_h, c, kept, s.max_v, s.band_shift, m);
            else
                sao16::block<false, NROWS>(fetch, store, x, ys, s.plane_w, s.plane_h, c, kept, s.max_v, s.band_shift);
            return;
        }
        const bool border = x == 0 || x + 8 == s.plane_w || ys == 0 || ys + NROWS >= s.plane_h;
        if (__builtin_amdgcn_ballot_w64(border) != 0ull)
            sao16::block<true, NROWS>(fetch, store, x, ys, s.plane_w, s.plane_h, c, kept, s.max_v, s.band_shift);
        else
            sao16::block<false, NROWS>(fetch, store, x, ys, s.plane_w, s.plane_h, c, kept, s.max_v, s.band_shift);
    };
    if (s.ctb_log2 == 5) { /* 32-sample CTBs: the quadrant's four CTBs one after the other, each by the whole wave (see fused_body) */
#pragma unroll 1
        for (int i = 0; i < 4; i++)
            sao_block(std::integral_constant<int, 2>{}, qx0 + (i & 1) * 32 + (l & 3) * 8, qy0 + (i >> 1) * 32 + (l >> 2) * 2);
    } else {
        sao_block(std::integral_constant<int, 8>{}, qx0 + (l & 7) * 8, qy0 + (l >> 3) * 8);
    }
}

/* ---- kernels: one plane, or the planes of a 4:2:0 batch in ONE launch (the grid is the planes' grids one after the other,
 * each a multiple of 8 workgroups so that the per-XCD renumbering works inside every plane) ---- */
template <bool CHROMA, bool QPMAP>
__global__ __launch_bounds__(kFusedThreads) void dbk_sao_fused_kernel(const DbkFusedArgs fa)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t fused_tile[];
    fused_body<CHROMA, 0, QPMAP>(fa.d, nullptr, fa.s, fa.g, fused_tile, blockIdx.x);
}

template <bool CHROMA, bool QPMAP>
__global__ __launch_bounds__(kFusedThreads) void dbk_sao_fused_h265_kernel(const DbkFusedH265Args fa)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t fused_tile[];
    fused_body<CHROMA, 2, QPMAP>(fa.d.base, &fa.d, fa.s, fa.g, fused_tile, blockIdx.x);
}

template <bool CHROMA, bool WIDE, bool QPMAP>
__global__ __launch_bounds__(kFused16Threads) void dbk_sao_fused16_kernel(const DbkFusedArgs fa)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t fused_tile[];
    fused_body16<CHROMA, 0, WIDE, QPMAP>(fa.d, nullptr, fa.s, fa.g, fused_tile, blockIdx.x);
}

template <bool CHROMA, bool WIDE, bool QPMAP>
__global__ __launch_bounds__(kFused16Threads) void dbk_sao_fused16_h265_kernel(const DbkFusedH265Args fa)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t fused_tile[];
    fused_body16<CHROMA, 2, WIDE, QPMAP>(fa.d.base, &fa.d, fa.s, fa.g, fused_tile, blockIdx.x);
}

/* plane of this workgroup and its number inside the plane's part of the grid */
__device__ __forceinline__ int fused_plane(const uint32_t (&wg_end)[3], uint32_t &id)
{
    const uint32_t b = blockIdx.x;
    const int pl = b >= wg_end[0] ? (b >= wg_end[1] ? 2 : 1) : 0; /* scalar */
    id = b - (pl ? wg_end[pl - 1] : 0u);
    return pl;
}

/* QPMAP: every plane of the launch reads the (luma-unit) QP map */
template <int SB, bool WIDE, bool QPMAP>
__global__ __launch_bounds__(SB == 1 ? kFusedThreads : kFused16Threads) void dbk_sao_fused_multi_kernel(const DbkFusedMultiArgs m)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t fused_tile[];
    uint32_t id;
    const int pl = fused_plane(m.wg_end, id);
    const DbkFusedArgs &fa = m.pl[pl];
    if constexpr (SB == 1) {
        if (pl == 0) fused_body<false, 0, QPMAP>(fa.d, nullptr, fa.s, fa.g, fused_tile, id);
        else fused_body<true, 0, QPMAP>(fa.d, nullptr, fa.s, fa.g, fused_tile, id);
    } else {
        if (pl == 0) fused_body16<false, 0, WIDE, QPMAP>(fa.d, nullptr, fa.s, fa.g, fused_tile, id);
        else fused_body16<true, 0, false, QPMAP>(fa.d, nullptr, fa.s, fa.g, fused_tile, id);
    }
}

template <int SB, bool WIDE, bool QPMAP>
__global__ __launch_bounds__(SB == 1 ? kFusedThreads : kFused16Threads) void dbk_sao_fused_multi_h265_kernel(const DbkFusedMultiH265Args m)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t fused_tile[];
    uint32_t id;
    const int pl = fused_plane(m.wg_end, id);
    const DbkFusedH265Args &fa = m.pl[pl];
    if constexpr (SB == 1) {
        if (pl == 0) fused_body<false, 2, QPMAP>(fa.d.base, &fa.d, fa.s, fa.g, fused_tile, id);
        else fused_body<true, 2, QPMAP>(fa.d.base, &fa.d, fa.s, fa.g, fused_tile, id);
    } else {
        if (pl == 0) fused_body16<false, 2, WIDE, QPMAP>(fa.d.base, &fa.d, fa.s, fa.g, fused_tile, id);
        else fused_body16<true, 2, false, QPMAP>(fa.d.base, &fa.d, fa.s, fa.g, fused_tile, id);
    }
}

/* QP-map planes of 4:2:2 (CF 2) / 4:4:4 (CF 3) pictures: chroma with the format's map positions and QpC rule (one-QP planes of
 * every format take the kernels above; 4:2:2 SAO parameters arrive rewritten for square CTBs, dbk_launch_sao_rows_x2) */
template <int CF>
__global__ __launch_bounds__(kFusedThreads) void dbk_sao_fused_h265_cf_kernel(const DbkFusedH265Args fa)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t fused_tile[];
    fused_body<true, 2, true, CF>(fa.d.base, &fa.d, fa.s, fa.g, fused_tile, blockIdx.x);
}
template <int CF>
__global__ __launch_bounds__(kFused16Threads) void dbk_sao_fused16_h265_cf_kernel(const DbkFusedH265Args fa)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t fused_tile[];
    fused_body16<true, 2, false, true, CF>(fa.d.base, &fa.d, fa.s, fa.g, fused_tile, blockIdx.x);
}
template <int SB, bool WIDE, int CF>
__global__ __launch_bounds__(SB == 1 ? kFusedThreads : kFused16Threads) void dbk_sao_fused_multi_h265_cf_kernel(const DbkFusedMultiH265Args m)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t fused_tile[];
    uint32_t id;
    const int pl = fused_plane(m.wg_end, id);
    const DbkFusedH265Args &fa = m.pl[pl];
    if constexpr (SB == 1) {
        if (pl == 0) fused_body<false, 2, true>(fa.d.base, &fa.d, fa.s, fa.g, fused_tile, id);
        else fused_body<true, 2, true, CF>(fa.d.base, &fa.d, fa.s, fa.g, fused_tile, id);
    } else {
        if (pl == 0) fused_body16<false, 2, WIDE, true>(fa.d.base, &fa.d, fa.s, fa.g, fused_tile, id);
        else fused_body16<true, 2, false, true, CF>(fa.d.base, &fa.d, fa.s, fa.g, fused_tile, id);
    }
}

/* ---- the spec-exact kernels with the slice / tile boundaries SAO must not look across (H.265 8.7.3.2): the kernels above plus one
 * argument, DbkSaoNox (one per plane for the multi-plane launch).  Kernels of their own names, so that every kernel without the
 * operand keeps its argument layout and machine code; CF 1 = 4:2:0 and every one-QP plane (fused_body's CF enters through the QP
 * map only) ---- */
template <bool CHROMA, bool QPMAP, int CF>
__global__ __launch_bounds__(kFusedThreads) void dbk_sao_fused_h265_nox_kernel(const DbkFusedH265Args fa, const DbkSaoNox nx)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t fused_tile[];
    fused_body<CHROMA, 2, QPMAP, CF, true>(fa.d.base, &fa.d, fa.s, fa.g, fused_tile, blockIdx.x, &nx);
}
template <bool CHROMA, bool WIDE, bool QPMAP, int CF>
__global__ __launch_bounds__(kFused16Threads) void dbk_sao_fused16_h265_nox_kernel(const DbkFusedH265Args fa, const DbkSaoNox nx)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t fused_tile[];
    fused_body16<CHROMA, 2, WIDE, QPMAP, CF, true>(fa.d.base, &fa.d, fa.s, fa.g, fused_tile, blockIdx.x, &nx);
}
struct DbkSaoNox3 {
    DbkSaoNox pl[3];
};
template <int SB, bool WIDE, bool QPMAP, int CF>
__global__ __launch_bounds__(SB == 1 ? kFusedThreads : kFused16Threads) void dbk_sao_fused_multi_h265_nox_kernel(const DbkFusedMultiH265Args m,
                                                                                                                 const DbkSaoNox3 nx)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t fused_tile[];
    uint32_t id;
    const int pl = fused_plane(m.wg_end, id);
    const DbkFusedH265Args &fa = m.pl[pl];
    if constexpr (SB == 1) {
        if (pl == 0) fused_body<false, 2, QPMAP, 1, true>(fa.d.base, &fa.d, fa.s, fa.g, fused_tile, id, &nx.pl[0]);
        else fused_body<true, 2, QPMAP, CF, true>(fa.d.base, &fa.d, fa.s, fa.g, fused_tile, id, &nx.pl[pl]);
    } else {
        if (pl == 0) fused_body16<false, 2, WIDE, QPMAP, 1, true>(fa.d.base, &fa.d, fa.s, fa.g, fused_tile, id, &nx.pl[0]);
        else fused_body16<true, 2, false, QPMAP, CF, true>(fa.d.base, &fa.d, fa.s, fa.g, fused_tile, id, &nx.pl[pl]);
    }
}

/* ---- the spec-exact kernels with per-slice deblocking offsets (deblock_sl.h): the _nox kernels plus one argument, DbkSlOffs -- ONE
 * for all planes of the multi-plane launch, whose CTB grid is the luma grid.  Kernels of their own names again.  They take the
 * boundary bytes as well, which may be absent (nx.nox == NULL: stage 2 then masks the picture border only, the same bytes as the
 * kernels without the operand), and always run stage 1 in the per-lane form, with a constant qPL where the plane has no QP map:
 * neither choice is a template dimension, so there is one kernel per plane kind and format ---- */
template <bool CHROMA, int CF>
__global__ __launch_bounds__(kFusedThreads) void dbk_sao_fused_h265_sl_kernel(const DbkFusedH265Args fa, const DbkSaoNox nx, const DbkSlOffs sl)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t fused_tile[];
    fused_body<CHROMA, 2, true, CF, true, true>(fa.d.base, &fa.d, fa.s, fa.g, fused_tile, blockIdx.x, &nx, &sl);
}
template <bool CHROMA, bool WIDE, int CF>
__global__ __launch_bounds__(kFused16Threads) void dbk_sao_fused16_h265_sl_kernel(const DbkFusedH265Args fa, const DbkSaoNox nx, const DbkSlOffs sl)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t fused_tile[];
    fused_body16<CHROMA, 2, WIDE, true, CF, true, true>(fa.d.base, &fa.d, fa.s, fa.g, fused_tile, blockIdx.x, &nx, &sl);
}
template <int SB, bool WIDE, int CF>
__global__ __launch_bounds__(SB == 1 ? kFusedThreads : kFused16Threads) void dbk_sao_fused_multi_h265_sl_kernel(const DbkFusedMultiH265Args m,
                                                                                                                const DbkSaoNox3 nx,
                                                                                                                const DbkSlOffs sl)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t fused_tile[];
    uint32_t id;
    const int pl = fused_plane(m.wg_end, id);
    const DbkFusedH265Args &fa = m.pl[pl];
    if constexpr (SB == 1) {
        if (pl == 0) fused_body<false, 2, true, 1, true, true>(fa.d.base, &fa.d, fa.s, fa.g, fused_tile, id, &nx.pl[0], &sl);
        else fused_body<true, 2, true, CF, true, true>(fa.d.base, &fa.d, fa.s, fa.g, fused_tile, id, &nx.pl[pl], &sl);
    } else {
        if (pl == 0) fused_body16<false, 2, WIDE, true, 1, true, true>(fa.d.base, &fa.d, fa.s, fa.g, fused_tile, id, &nx.pl[0], &sl);
        else fused_body16<true, 2, false, true, CF, true, true>(fa.d.base, &fa.d, fa.s, fa.g, fused_tile, id, &nx.pl[pl], &sl);
    }
}

/* ---- the _sl kernels for planes whose sizes are multiples of 4 (the _g4 entries; deblock_h265.h load_block_bs_h265_g4): kernels of
 * their own names once more.  Chroma planes only have such sizes; in the multi-plane launch the luma plane runs the same body, for
 * which its multiple-of-8 size is the special case and which adds the launch's own (beta, tC) pair to the per-slice ones
 * (sl_block_operands): a call without per-slice offsets hands in an array of no bytes ---- */
template <int CF>
__global__ __launch_bounds__(kFusedThreads) void dbk_sao_fused_h265_g4_kernel(const DbkFusedH265Args fa, const DbkSaoNox nx, const DbkSlOffs sl)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t fused_tile[];
    fused_body<true, 2, true, CF, true, true, true>(fa.d.base, &fa.d, fa.s, fa.g, fused_tile, blockIdx.x, &nx, &sl);
}
template <int CF>
__global__ __launch_bounds__(kFused16Threads) void dbk_sao_fused16_h265_g4_kernel(const DbkFusedH265Args fa, const DbkSaoNox nx, const DbkSlOffs sl)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t fused_tile[];
    fused_body16<true, 2, false, true, CF, true, true, true>(fa.d.base, &fa.d, fa.s, fa.g, fused_tile, blockIdx.x, &nx, &sl);
}
template <int SB, bool WIDE, int CF>
__global__ __launch_bounds__(SB == 1 ? kFusedThreads : kFused16Threads) void dbk_sao_fused_multi_h265_g4_kernel(const DbkFusedMultiH265Args m,
                                                                                                                const DbkSaoNox3 nx,
                                                                                                                const DbkSlOffs sl)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t fused_tile[];
    uint32_t id;
    const int pl = fused_plane(m.wg_end, id);
    const DbkFusedH265Args &fa = m.pl[pl];
    if constexpr (SB == 1) {
        if (pl == 0) fused_body<false, 2, true, 1, true, true, true>(fa.d.base, &fa.d, fa.s, fa.g, fused_tile, id, &nx.pl[0], &sl);
        else fused_body<true, 2, true, CF, true, true, true>(fa.d.base, &fa.d, fa.s, fa.g, fused_tile, id, &nx.pl[pl], &sl);
    } else {
        if (pl == 0) fused_body16<false, 2, WIDE, true, 1, true, true, true>(fa.d.base, &fa.d, fa.s, fa.g, fused_tile, id, &nx.pl[0], &sl);
        else fused_body16<true, 2, false, true, CF, true, true, true>(fa.d.base, &fa.d, fa.s, fa.g, fused_tile, id, &nx.pl[pl], &sl);
    }
}
