/* sao8_kernel_body.inc -- the body of sao8_kernel / sao8_nox_kernel, included by sao.hip once for the kernel without the slice / tile boundary operand (NOX false: nx is
 * not looked at) and once for its _nox twin (NOX true; H.265 8.7.3.2), and a third time for the _nox twin's _g4 twin (G4 true: a plane
 * whose sizes are multiples of 4, whose boundary bytes may be absent).  Written once and compiled into two kernels of their own
 * argument lists, so that the kernel without the operand is the same machine code with or without the twin beside it (a shared
 * __device__ body taking the arguments by reference was compiled to other code than the kernel had before). */
    int wx, wy, f;
    if (!sao_strip<SWZ>(g, wx, wy, f)) return;
    const int wv = threadIdx.x >> 6, l = threadIdx.x & 63;
    /* Lane -> 8 x 8 block.  A wave takes one 64 x 64 region, i.e. with 64-sample CTBs one CTB and ONE path; its row pieces are
     * then 64 bytes, half a cache line.  Where the two CTBs of an aligned pair (waves 2k, 2k + 1 of the workgroup) take the
     * same path -- both edge offset of one class, or neither edge offset: SAO parameters are merged from the left / above
     * neighbour in most CTBs of a real stream -- the two waves split the pair the other way: each takes 32 rows of BOTH CTBs
     * (16 blocks across, 4 down), whole 128-byte lines, still one path per wave.  (Round 3 measured the wide shape for every
     * pair: +8 % where the paths agree, -7 % where they differ; per pair it only ever takes the gain.) */
    int x = (wx * WAVES + wv) * 64 + (l & 7) * 8;
    int y0 = wy * 64 + (l >> 3) * 8;
    bool zero_band = false;
    if constexpr (WAVES % 2 == 0) {
        const int px = (wx * WAVES + (wv & ~1)) * 64, py = wy * 64; /* the pair's origin */
        if (a.ctb_log2 == 6 && px + 128 <= a.plane_w && py + 64 <= a.plane_h) {
            const DbkSaoCtb *pc = a.params + (long long)f * a.params_frame_stride + (long long)(py >> 6) * a.params_stride + (px >> 6);
            /* "not applied" and band offset count as one path: in a wide wave the former runs as a band offset of zeros (below) */
            const bool e0 = pc[0].type == 2, e1 = pc[1].type == 2;
            const bool same = e0 == e1 && (!e0 || ((pc[0].cls ^ pc[1].cls) & 3) == 0);
            if (__builtin_amdgcn_readfirstlane(same ? 1 : 0)) { /* uniform by construction: every lane looked at the same two entries */
                x = px + (l & 15) * 8;
                y0 = py + (wv & 1) * 32 + (l >> 4) * 8;
                /* one CTB band offset, the other not applied: see below */
                zero_band = __builtin_amdgcn_readfirstlane((!e0 && (pc[0].type == 1) != (pc[1].type == 1)) ? 1 : 0) != 0;
            }
        }
    }
    if (x >= a.plane_w || y0 >= a.plane_h) return;
    const uint8_t *src = a.src + (long long)f * a.frame_stride;
    uint8_t *dst = a.dst + (long long)f * a.frame_stride;
    [[maybe_unused]] uint32_t nox_byte = 0u;
    if constexpr (NOX && G4) nox_byte = nx.nox ? saonox::ctb_byte(nx, f, x, y0, a.ctb_log2) : 0u; /* no bytes: nothing forbidden */
    else if constexpr (NOX) nox_byte = saonox::ctb_byte(nx, f, x, y0, a.ctb_log2);
    const DbkSaoCtb c = a.params[(long long)f * a.params_frame_stride + (long long)(y0 >> a.ctb_log2) * a.params_stride + (x >> a.ctb_log2)];
    const bool kept = a.keep && a.keep[(long long)f * a.keep_frame_stride + (long long)(y0 >> 3) * a.keep_stride + (x >> 3)];
    bool border = x == 0 || x + 8 == a.plane_w || y0 == 0 || y0 + 8 >= a.plane_h;
    uint32_t m = 0u;
    if constexpr (NOX) { /* per lane, so the wide shape needs no rule of its own: a pair with a boundary between or around its halves is a wave whose ballot is not zero */
        m = saonox::block_mask<8>(nox_byte, x, y0, a.plane_w, a.plane_h, a.ctb_log2); /* the picture border included */
        border = m != 0u;
    }
    if (__builtin_amdgcn_ballot_w64(border) == 0ull) {
        /* no lane of the wave touches the picture border (nearly every wave): the shared block procedure (sao_packed.h, the
         * edge class resolved once per block) on rows addressed through buffer resources -- a lane's byte offset once, the
         * row in the scalar offset, no per-row 64-bit address arithmetic and no clamping of row numbers */
        const uint32_t plane_bytes = (uint32_t)a.pitch * (uint32_t)a.plane_h; /* < 2^31: checked by the launcher */
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(src), 0, plane_bytes, 0x00020000);
        const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc(dst, 0, plane_bytes, 0x00020000);
        const int sp = __builtin_amdgcn_readfirstlane((int)a.pitch);
        const uint32_t vrow = (uint32_t)y0 * (uint32_t)a.pitch + (uint32_t)x; /* (x, y0); y0 >= 8 and x >= 8 here */
        const uint32_t vup = vrow - (uint32_t)a.pitch;                         /* raw row 0 = image row y0 - 1 */
        auto fetch = [&](int j, auto halo) {
            SaoRaw q;
            if constexpr (decltype(halo)::value) {
                const sao_u32x4b v = __builtin_amdgcn_raw_buffer_load_b128(rs, vup - 4u, j * sp, 0);
                q.lh = v.x; q.cx = v.y; q.cy = v.z; q.rh = v.w;
            } else {
                const sao_u32x2b v = __builtin_amdgcn_raw_buffer_load_b64(rs, vup, j * sp, 0);
                q.lh = q.rh = 0u;
                q.cx = v.x; q.cy = v.y;
            }
            return q;
        };
        auto store = [&](int r, uint32_t lo, uint32_t hi) {
            sao_u32x2b w;
            w.x = lo;
            w.y = hi;
            __builtin_amdgcn_raw_buffer_store_b64(w, rd, vrow, r * sp, 0);
        };
        if (zero_band) {
            /* a wide wave over one band-offset CTB and one without SAO: the latter's blocks (and kept ones) run as a band offset
             * of zeros (rec + 0, clipped: the same bytes) so that the two CTBs' lanes issue the SAME loads and stores -- whole
             * lines -- instead of each half of the wave its own.  (A pair without SAO in either CTB keeps the plain copy:
             * the arithmetic costs 5 % there.) */
            DbkSaoCtb z = c;
            if (kept || c.type != 1) {
                z.type = 1; z.cls = 0;
                z.offset[0] = z.offset[1] = z.offset[2] = z.offset[3] = 0;
            }
            sao8::block<false, 8>(fetch, store, x, y0, a.plane_w, a.plane_h, z, false);
            return;
        }
        sao8::block<false, 8>(fetch, store, x, y0, a.plane_w, a.plane_h, c, kept);
        return;
    }
    if constexpr (G4) {
        /* a wave that holds a block of 4 columns or 4 rows (the last column / row of blocks of a plane whose size is a multiple
         * of 4, not 8: border blocks all of them): the masked per-sample procedure for the whole wave.  Every other wave --
         * the border waves of whole blocks among them -- runs what it runs for a multiple of 8 */
        if (__builtin_amdgcn_ballot_w64(x + 8 > a.plane_w || y0 + 8 > a.plane_h) != 0ull) {
            sao_block_g4<uint8_t>(a, nox_byte, src, dst, x, y0, c, kept);
            return;
        }
    }
    if (kept || c.type == 0 || c.type > 2) {
#pragma unroll
        for (int r = 0; r < 8; r++)
            *reinterpret_cast<uint2 *>(dst + (long long)(y0 + r) * a.pitch + x) =
                *reinterpret_cast<const uint2 *>(src + (long long)(y0 + r) * a.pitch + x);
        return;
    }
    auto b = [](int v) { return (uint32_t)(v + 128) & 0xffu; };
    if (c.type == 1) { /* band offset: bandTable[(k + sao_band_position) & 31] = k + 1; index min(k, 4), entry 4 = no offset */
        const uint32_t tab_lo = b(c.offset[0]) | (b(c.offset[1]) << 8) | (b(c.offset[2]) << 16) | (b(c.offset[3]) << 24), tab_hi = b(0);
        const spk pos = s_splat((int)c.cls);
        auto band = [&](uint32_t rec) {
            return sao_apply(rec, sao8::band_sel(rec, 3, pos), tab_lo, tab_hi); /* 8 bit: bandShift = bitDepth - 5 = 3 */
        };
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const SaoRow m = sao_load_row<false, false>(src + (long long)(y0 + r) * a.pitch, x, a.plane_w);
            uint2 out;
            out.x = band(m.E0) | (band(m.O0) << 8);
            out.y = band(m.E1) | (band(m.O1) << 8);
            *reinterpret_cast<uint2 *>(dst + (long long)(y0 + r) * a.pitch + x) = out;
        }
        return;
    }
    /* edge offset: index 0 -> SaoOffsetVal[1], 1 -> [2], 2 -> none, 3 -> [3], 4 -> [4] */
    const uint32_t tab_lo = b(c.offset[0]) | (b(c.offset[1]) << 8) | (b(0) << 16) | (b(c.offset[2]) << 24), tab_hi = b(c.offset[3]);
    sao8_edge_block<NOX ? 2 : 1>(a, src, dst, x, y0, c.cls & 3, tab_lo, tab_hi, m); /* a wave with a lane on the picture border */
