/*
 * decoder_loop.c -- plain-C sketch of a decoder's in-loop stage on top of include/hevc_deblock.h: per picture, derive bS
 * from the prediction data on the GPU (H.265 8.7.2.4), then deblock + SAO all three planes of the picture into the output
 * picture in ONE launch (8.7.2 + 8.7.3).  Everything stays in HBM; the caller owns all buffers.  Two pictures:
 *   1920x1088  every plane a multiple of 8: hevcdbk_h265_derive_bs_device + hevc_deblock_sao_h265_device_planes;
 *   1920x1080  the picture of a 1080p stream coded with 8x8 minimum coding blocks.  Its 4:2:0 chroma planes are 960x540, and
 *              540 = 67 * 8 + 4: the _g4 entries (same signatures as the _cf / _sl entries, planes sized in multiples of 4).
 * Built by the CPU test-suite with `gcc -std=c99 -pedantic -Wall -Werror` to prove that the header is a C header; run it on a
 * machine with an MI355X:
 *
 *   gcc -std=c99 -Iinclude examples/decoder_loop.c -Lgpu_video_codec_amd -lhevcdbk -Wl,-rpath,$PWD/gpu_video_codec_amd -o decoder_loop
 *   ./decoder_loop [dump]     with a file name, what went in and what came out of the 1920x1080 picture is written there
 *                             (the test-suite recomputes the output from the input with its CPU statement of the standard)
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hevc_deblock.h"

#define CHECK(call)                                                                                      \
    do {                                                                                                 \
        int rc_ = (call);                                                                                \
        if (rc_ != HEVCDBK_OK) {                                                                         \
            fprintf(stderr, "%s -> %s (%s)\n", #call, hevcdbk_strerror(rc_), hevcdbk_last_error(ctx));  \
            return 1;                                                                                    \
        }                                                                                                \
    } while (0)

/* what a decoder's reconstruction would have left: 8x8 blocks of one level each with a little texture */
static void fill_plane(uint8_t *p, unsigned w, unsigned h, unsigned seed)
{
    unsigned x, y, s = seed * 2654435761u + 12345u;
    for (y = 0; y < h; y++)
        for (x = 0; x < w; x++) {
            const unsigned level = 64u + (((x / 8u) * 37u + (y / 8u) * 91u + seed * 13u) % 21u) * 6u;
            s = s * 1664525u + 1013904223u;
            p[(size_t)y * w + x] = (uint8_t)(level + ((s >> 24) % 7u));
        }
}

/* a device buffer holding `bytes` of host memory */
static int upload(hevcdbk_context *ctx, const void *host, size_t bytes, void **dev)
{
    CHECK(hevcdbk_device_malloc(ctx, bytes, dev));
    CHECK(hevcdbk_memcpy_h2d(ctx, *dev, host, bytes));
    return 0;
}

/* one W x H 4:2:0 picture through the in-loop stage; dump (may be NULL) receives the operands and the result */
static int picture(hevcdbk_context *ctx, unsigned W, unsigned H, FILE *dump)
{
    const unsigned CW = W / 2, CH = H / 2;
    const int g4 = CW % 8 != 0 || CH % 8 != 0; /* chroma planes sized in multiples of 4: the _g4 entries */
    const unsigned uw = W / 4, uh = H / 4;
    const size_t units = (size_t)uw * uh;
    /* one SAO entry per CTB and plane: 64-sample luma CTBs are 32-sample CTBs of the 4:2:0 chroma planes, same grid; the last row
     * of CTBs of the 1080-row picture is cut to 56 luma / 28 chroma rows */
    const unsigned ctbs_x = (W + 63) / 64, ctbs_y = (H + 63) / 64;
    const size_t n_ctbs = (size_t)ctbs_x * ctbs_y;
    /* QpY per 16x16 quantization group (cu_qp_delta): one map in luma units, read by all three planes */
    const unsigned qg_x = (W + 15) / 16, qg_y = (H + 15) / 16;
    const size_t plane_bytes[3] = {(size_t)W * H, (size_t)CW * CH, (size_t)CW * CH};
    const size_t n_bs[4] = {hevcdbk_h265_num_vert_bs(W, H), hevcdbk_h265_num_hor_bs(W, H), hevcdbk_h265_num_vert_bs(CW, CH),
                            hevcdbk_h265_num_hor_bs(CW, CH)};
    uint8_t *host[3], *qp_host;
    uint16_t *flags_host;
    hevcdbk_sao_ctb *sao_host[3];
    void *src[3], *dst[3], *sao[3], *flags, *mv0, *mv1, *ref0, *ref1, *bs[4], *qpy;
    size_t k;
    unsigned x, y;
    int i;

    /* the operands a decoder holds after reconstruction, made up here: planes, prediction data (every 8x8 block an intra coding
     * block with a transform edge on its left and top: bS 2 on the whole 8-sample grid), SAO parameters of every kind, a QP map */
    flags_host = (uint16_t *)malloc(units * 2);
    qp_host = (uint8_t *)malloc((size_t)qg_x * qg_y);
    if (!flags_host || !qp_host) return 1;
    for (y = 0; y < uh; y++)
        for (x = 0; x < uw; x++)
            flags_host[(size_t)y * uw + x] = (uint16_t)(HEVCDBK_U_INTRA | (x % 2 == 0 ? HEVCDBK_U_TU_LEFT | HEVCDBK_U_PU_LEFT : 0) |
                                                        (y % 2 == 0 ? HEVCDBK_U_TU_TOP | HEVCDBK_U_PU_TOP : 0));
    for (k = 0; k < (size_t)qg_x * qg_y; k++) qp_host[k] = (uint8_t)(30 + (k * 7) % 12);
    for (i = 0; i < 3; i++) {
        host[i] = (uint8_t *)malloc(plane_bytes[i]);
        sao_host[i] = (hevcdbk_sao_ctb *)calloc(n_ctbs, sizeof(hevcdbk_sao_ctb));
        if (!host[i] || !sao_host[i]) return 1;
        fill_plane(host[i], i ? CW : W, i ? CH : H, (unsigned)i + 1);
        for (k = 0; k < n_ctbs; k++) {
            hevcdbk_sao_ctb *c = &sao_host[i][k];
            const unsigned kind = (unsigned)(k + (size_t)i) % 6u; /* 0 off, 1 band, 2..5 edge class 0..3 */
            c->type = (uint8_t)(kind == 0 ? 0 : (kind == 1 ? 1 : 2));
            c->cls = (uint8_t)(kind == 1 ? (k % 32) : (kind >= 2 ? kind - 2 : 0));
            c->offset[0] = 3; c->offset[1] = 1; c->offset[2] = (int8_t)(kind == 1 ? 2 : -1); c->offset[3] = (int8_t)(kind == 1 ? -2 : -3);
        }
    }

    /* picture planes, the output picture's planes, prediction data, bS arrays, SAO parameters: all in HBM */
    for (i = 0; i < 3; i++) {
        if (upload(ctx, host[i], plane_bytes[i], &src[i])) return 1;
        if (upload(ctx, sao_host[i], n_ctbs * sizeof(hevcdbk_sao_ctb), &sao[i])) return 1;
        CHECK(hevcdbk_device_malloc(ctx, plane_bytes[i], &dst[i]));
    }
    if (upload(ctx, flags_host, units * 2, &flags) || upload(ctx, qp_host, (size_t)qg_x * qg_y, &qpy)) return 1;
    CHECK(hevcdbk_device_malloc(ctx, units * 4, &mv0));
    CHECK(hevcdbk_device_malloc(ctx, units * 4, &mv1));
    CHECK(hevcdbk_device_malloc(ctx, units * 4, &ref0));
    CHECK(hevcdbk_device_malloc(ctx, units * 4, &ref1));
    CHECK(hevcdbk_memset_d(ctx, mv0, 0, units * 4));
    CHECK(hevcdbk_memset_d(ctx, mv1, 0, units * 4));
    CHECK(hevcdbk_memset_d(ctx, ref0, 0, units * 4));
    CHECK(hevcdbk_memset_d(ctx, ref1, 0, units * 4));
    for (i = 0; i < 4; i++) CHECK(hevcdbk_device_malloc(ctx, n_bs[i], &bs[i]));

    /* 8.7.2.4: the luma arrays and, gathered from them, the chroma arrays (floor division: 121 x 135 and 68 x 240 entries for 960x540) */
    {
        hevcdbk_h265_units u;
        u.flags = (const uint16_t *)flags; u.mv0 = (const int16_t *)mv0; u.mv1 = (const int16_t *)mv1;
        u.ref0 = (const int32_t *)ref0; u.ref1 = (const int32_t *)ref1;
        if (g4)
            CHECK(hevcdbk_h265_derive_bs_device_g4(ctx, &u, W, H, HEVCDBK_CHROMA_420, (uint8_t *)bs[0], (uint8_t *)bs[1], (uint8_t *)bs[2],
                                                   (uint8_t *)bs[3], NULL));
        else
            CHECK(hevcdbk_h265_derive_bs_device(ctx, &u, W, H, (uint8_t *)bs[0], (uint8_t *)bs[1], (uint8_t *)bs[2], (uint8_t *)bs[3], NULL));
    }

    /* 8.7.2 + 8.7.3 of Y, Cb, Cr: reconstruction -> output picture in ONE launch (a workgroup deblocks a tile into LDS and
     * applies SAO from there: the deblocked picture never exists in memory; the planes' tiles follow each other in the grid) */
    {
        hevcdbk_h265_params prm;
        hevcdbk_device_planes p[3];
        memset(&prm, 0, sizeof(prm));
        memset(p, 0, sizeof(p));
        for (i = 0; i < 3; i++) {
            const unsigned pw = i ? CW : W, ph = i ? CH : H;
            p[i].n_frames = 1; p[i].bit_depth = 8; p[i].sample_bytes = 1; p[i].is_chroma = i != 0;
            p[i].src = src[i]; p[i].dst = dst[i]; p[i].pitch = pw; p[i].frame_stride = (size_t)pw * ph; p[i].plane_w = pw; p[i].plane_h = ph;
            p[i].vert_bs = (const uint8_t *)bs[i ? 2 : 0]; p[i].hor_bs = (const uint8_t *)bs[i ? 3 : 1];
            p[i].qp_map = (const uint8_t *)qpy; p[i].qp_map_stride = qg_x; p[i].ctu_log2 = 4; /* the map unit: 16 luma samples */
        }
        if (g4) {
            /* no slice / tile borders and no per-slice offsets in this picture: both operands NULL */
            hevcdbk_sao_plane_cf so[3];
            memset(so, 0, sizeof(so));
            for (i = 0; i < 3; i++) {
                so[i].params = (const hevcdbk_sao_ctb *)sao[i]; so[i].params_stride = ctbs_x;
                so[i].ctb_log2_w = so[i].ctb_log2_h = i ? 5 : 6;
            }
            CHECK(hevcdbk_h265_deblock_sao_device_planes_g4(ctx, p, 3, HEVCDBK_CHROMA_420, /* qp: unused with a map */ 0, &prm, so,
                                                            HEVCDBK_FUSED_AUTO, NULL, NULL, NULL));
        } else {
            hevcdbk_sao_plane so[3];
            memset(so, 0, sizeof(so));
            for (i = 0; i < 3; i++) {
                so[i].params = (const hevcdbk_sao_ctb *)sao[i]; so[i].params_stride = ctbs_x; so[i].ctb_log2 = i ? 5 : 6;
            }
            CHECK(hevc_deblock_sao_h265_device_planes(ctx, p, 3, /* qp: unused with a map */ 0, &prm, so, HEVCDBK_FUSED_AUTO, NULL));
        }
        /* a picture whose chroma SAO is switched off deblocks Cb / Cr in place instead:
         *   hevcdbk_h265_filter_device_g4(ctx, &chroma_plane, c_idx, HEVCDBK_CHROMA_420, qp, &prm, HEVCDBK_KERNEL_AUTO, NULL, NULL) */
    }
    CHECK(hevcdbk_synchronize(ctx));

    if (dump) {
        /* W, H, CTB columns and rows, QP map columns and rows; then the input planes, the unit flags, the QP map, the SAO parameters of
         * the three planes, the output planes */
        const unsigned head[6] = {W, H, ctbs_x, ctbs_y, qg_x, qg_y};
        fwrite(head, sizeof(head), 1, dump);
        for (i = 0; i < 3; i++) fwrite(host[i], 1, plane_bytes[i], dump);
        fwrite(flags_host, 2, units, dump);
        fwrite(qp_host, 1, (size_t)qg_x * qg_y, dump);
        for (i = 0; i < 3; i++) fwrite(sao_host[i], sizeof(hevcdbk_sao_ctb), n_ctbs, dump);
        for (i = 0; i < 3; i++) {
            CHECK(hevcdbk_memcpy_d2h(ctx, host[i], dst[i], plane_bytes[i]));
            fwrite(host[i], 1, plane_bytes[i], dump);
        }
    }
    printf("one %ux%u picture through bS derivation, deblocking and SAO on the GPU\n", W, H);

    for (i = 0; i < 3; i++) {
        hevcdbk_device_free(ctx, src[i]); hevcdbk_device_free(ctx, dst[i]); hevcdbk_device_free(ctx, sao[i]);
        free(host[i]); free(sao_host[i]);
    }
    for (i = 0; i < 4; i++) hevcdbk_device_free(ctx, bs[i]);
    hevcdbk_device_free(ctx, flags); hevcdbk_device_free(ctx, mv0); hevcdbk_device_free(ctx, mv1);
    hevcdbk_device_free(ctx, ref0); hevcdbk_device_free(ctx, ref1); hevcdbk_device_free(ctx, qpy);
    free(flags_host); free(qp_host);
    return 0;
}

int main(int argc, char **argv)
{
    hevcdbk_context *ctx = NULL;
    FILE *dump = NULL;
    int rc;
    if (hevcdbk_create(0, &ctx) != HEVCDBK_OK) {
        fprintf(stderr, "no HIP device: this library has no CPU path\n");
        return 2;
    }
    if (argc > 1 && !(dump = fopen(argv[1], "wb"))) {
        fprintf(stderr, "cannot write %s\n", argv[1]);
        hevcdbk_destroy(ctx);
        return 1;
    }
    rc = picture(ctx, 1920, 1088, NULL);
    if (rc == 0) rc = picture(ctx, 1920, 1080, dump);
    if (dump) fclose(dump);
    hevcdbk_destroy(ctx);
    return rc;
}
