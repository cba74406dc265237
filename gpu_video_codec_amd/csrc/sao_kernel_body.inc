/* sao_kernel_body.inc -- the body of sao_kernel / sao_nox_kernel, included by sao.hip once for the kernel without the slice / tile boundary operand (NOX false: nx is
 * not looked at) and once for its _nox twin (NOX true; H.265 8.7.3.2), and a third time for the _nox twin's _g4 twin (G4 true: a plane
 * whose sizes are multiples of 4, whose boundary bytes may be absent).  Written once and compiled into two kernels of their own
 * argument lists, so that the kernel without the operand is the same machine code with or without the twin beside it (a shared
 * __device__ body taking the arguments by reference was compiled to other code than the kernel had before). */
    /* a wave = the 8 x 8 blocks of one 64 x 64 region: with 64-sample CTBs every lane of a wave has the same SAO type and the
     * wave runs ONE of the three paths; a row-shaped wave (512 x 8) would span eight CTBs and run all of them */
    int wx, wy, f;
    if (!sao_strip<SWZ>(g, wx, wy, f)) return;
    const int wv = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int x = (wx * 4 + wv) * 64 + (l & 7) * 8;
    const int y0 = wy * 64 + (l >> 3) * 8;
    if (x >= a.plane_w || y0 >= a.plane_h) return;
    const uint8_t *src = a.src + (long long)f * a.frame_stride;
    uint8_t *dst = a.dst + (long long)f * a.frame_stride;
    const DbkSaoCtb c = a.params[(long long)f * a.params_frame_stride + (long long)(y0 >> a.ctb_log2) * a.params_stride + (x >> a.ctb_log2)];
    const bool kept = a.keep && a.keep[(long long)f * a.keep_frame_stride + (long long)(y0 >> 3) * a.keep_stride + (x >> 3)];
    if constexpr (PK16 && sizeof(T) == 2) {
        /* no lane of the wave on the picture border (nearly every wave): the packed 16-bit block procedure of the fused kernels
         * (sao_packed.h, sao16: the samples already are int16 pairs) on rows addressed through buffer resources, as the 8-bit
         * kernel below does; a region's row piece is a whole 128-byte line here, so the wave keeps its 64 x 64 shape */
        bool border = x == 0 || x + 8 == a.plane_w || y0 == 0 || y0 + 8 >= a.plane_h;
        if constexpr (NOX && G4) border = saonox::block_mask<8>(nx.nox ? saonox::ctb_byte(nx, f, x, y0, a.ctb_log2) : 0u, x, y0, a.plane_w, a.plane_h, a.ctb_log2) != 0u; /* a block of 4 columns / rows is a border block */
        else if constexpr (NOX) border = saonox::block_mask<8>(saonox::ctb_byte(nx, f, x, y0, a.ctb_log2), x, y0, a.plane_w, a.plane_h, a.ctb_log2) != 0u; /* the picture border included */
        if (__builtin_amdgcn_ballot_w64(border) == 0ull) {
            typedef uint32_t u32x4b __attribute__((ext_vector_type(4)));
            const uint32_t plane_bytes = (uint32_t)a.pitch * (uint32_t)a.plane_h; /* < 2^31: checked by the launcher */
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(src), 0, plane_bytes, 0x00020000);
            const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc(dst, 0, plane_bytes, 0x00020000);
            const int sp = __builtin_amdgcn_readfirstlane((int)a.pitch);
            const uint32_t vrow = (uint32_t)y0 * (uint32_t)a.pitch + (uint32_t)x * 2u;
            const uint32_t vup = vrow - (uint32_t)a.pitch; /* raw row 0 = image row y0 - 1 */
            auto fetch = [&](int j, auto halo) {
                sao16::Raw q;
                const u32x4b m = __builtin_amdgcn_raw_buffer_load_b128(rs, vup, j * sp, 0); /* samples x .. x+7 */
                q.d[0] = q.d[7] = 0u;
                q.d[2] = m.x; q.d[3] = m.y; q.d[4] = m.z; q.d[5] = m.w;
                if constexpr (decltype(halo)::value) {
                    q.d[1] = __builtin_amdgcn_raw_buffer_load_b32(rs, vup - 4u, j * sp, 0);  /* s[-2], s[-1] */
                    q.d[6] = __builtin_amdgcn_raw_buffer_load_b32(rs, vup + 16u, j * sp, 0); /* s8, s9 */
                } else {
                    q.d[1] = q.d[6] = 0u;
                }
                return q;
            };
            auto store = [&](int r, uint32_t d0, uint32_t d1, uint32_t d2, uint32_t d3) {
                u32x4b w;
                w.x = d0; w.y = d1; w.z = d2; w.w = d3;
                __builtin_amdgcn_raw_buffer_store_b128(w, rd, vrow, r * sp, 0);
                /* the wait states of the fused 16-bit kernel's stores (deblock_sao_fused.inc): a 16-byte buffer store with an SGPR
                 * offset followed at once by a VALU write of its data registers */
                asm volatile("s_nop 1" : : "v"(w.x), "v"(w.y), "v"(w.z), "v"(w.w) : "memory");
            };
            sao16::block<false, 8>(fetch, store, x, y0, a.plane_w, a.plane_h, c, kept, a.max_v, a.band_shift);
            return;
        }
    }
    if constexpr (G4) { /* the same procedure for blocks of 8 or 4 columns and rows (sao_block_g4) */
        sao_block_g4<T>(a, nx.nox ? saonox::ctb_byte(nx, f, x, y0, a.ctb_log2) : 0u, src, dst, x, y0, c, kept);
        return;
    }
    if (kept || c.type == 0 || c.type > 2) {
#pragma unroll
        for (int r = 0; r < 8; r++) {
            int o[8];
            load8<T>(src + (long long)(y0 + r) * a.pitch, x, o);
            store8<T>(dst + (long long)(y0 + r) * a.pitch, x, o);
        }
        return;
    }
    if (c.type == 1) { /* band offset: bandTable[(k + sao_band_position) & 31] = k + 1 */
#pragma unroll
        for (int r = 0; r < 8; r++) {
            int o[8];
            load8<T>(src + (long long)(y0 + r) * a.pitch, x, o);
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const int k = ((o[i] >> a.band_shift) - (int)c.cls) & 31;
                const int off = k == 0 ? c.offset[0] : (k == 1 ? c.offset[1] : (k == 2 ? c.offset[2] : (k == 3 ? c.offset[3] : 0)));
                const int v = o[i] + off;
                o[i] = v < 0 ? 0 : (v > a.max_v ? a.max_v : v);
            }
            store8<T>(dst + (long long)(y0 + r) * a.pitch, x, o);
        }
        return;
    }
    /* edge offset, Table 8-13: class 0 (-1,0)/(1,0); 1 (0,-1)/(0,1); 2 (-1,-1)/(1,1); 3 (1,-1)/(-1,1) */
    const int cls = c.cls & 3;
    const int dxa = cls == 1 ? 0 : (cls == 3 ? 1 : -1);
    const bool vertical = cls != 0; /* neighbours in the rows above and below */
    auto row_at = [&](int y) { return src + (long long)(y < 0 ? 0 : (y >= a.plane_h ? a.plane_h - 1 : y)) * a.pitch; };
    [[maybe_unused]] uint32_t nox = 0u; /* the CTB's byte: the lane's 8 x 8 block lies inside one CTB */
    if constexpr (NOX) nox = nx.nox[(long long)f * nx.frame_stride + (long long)(y0 >> a.ctb_log2) * nx.stride + (x >> a.ctb_log2)];
    [[maybe_unused]] const int dya = vertical ? -1 : 0;
    int up[10], mid[10], dn[10];
    load10<T>(row_at(y0 - 1), x, a.plane_w, up);
    load10<T>(row_at(y0), x, a.plane_w, mid);
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int y = y0 + r;
        load10<T>(row_at(y + 1), x, a.plane_w, dn);
        const bool rows_ok = !vertical || (y > 0 && y < a.plane_h - 1);
        int o[8];
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int rec = mid[1 + i];
            const int xa = x + i + dxa, xb = x + i - dxa;
            bool ok = rows_ok && xa >= 0 && xa < a.plane_w && xb >= 0 && xb < a.plane_w;
            if constexpr (NOX) { /* per sample: the CTB either neighbour lies in, against the byte */
                const int L2 = a.ctb_log2, cx = (x + i) >> L2, cy = y >> L2;
                ok = ok && !(nox & (sao_nox_bit((xa >> L2) - cx, ((y + dya) >> L2) - cy) | sao_nox_bit((xb >> L2) - cx, ((y - dya) >> L2) - cy)));
            }
            const int (&ra)[10] = vertical ? up : mid;
            const int (&rb)[10] = vertical ? dn : mid;
            const int na = dxa < 0 ? ra[i] : (dxa == 0 ? ra[1 + i] : ra[2 + i]);
            const int nb = dxa < 0 ? rb[2 + i] : (dxa == 0 ? rb[1 + i] : rb[i]);
            const int e = 2 + sgn(rec - na) + sgn(rec - nb);
            /* raw 0 -> SaoOffsetVal[1], 1 -> [2], 2 -> none, 3 -> [3], 4 -> [4] */
            const int off = e == 0 ? c.offset[0] : (e == 1 ? c.offset[1] : (e == 3 ? c.offset[2] : (e == 4 ? c.offset[3] : 0)));
            const int v = rec + (ok ? off : 0);
            o[i] = v < 0 ? 0 : (v > a.max_v ? a.max_v : v);
        }
        store8<T>(dst + (long long)y * a.pitch, x, o);
#pragma unroll
        for (int i = 0; i < 10; i++) { up[i] = mid[i]; mid[i] = dn[i]; }
    }
