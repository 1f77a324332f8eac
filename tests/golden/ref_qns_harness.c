/* ref_qns_harness.c -- calls the reference's own get_vissual_weight (libavcodec/mpegvideo_enc.c:1434-1455), dct_quantize_c
 * (:3647-3724) and dct_quantize_refine (:3271-3645) on a hand-filled MpegEncContext.  A tool of
 * tests/golden/make_ref_qns_golden.py, which compiles it inside a temporary build of the reference's ffmpeg and links it with
 * that build's libavcodec.a / libavutil.a; nothing of that build is kept.
 *
 * Two of the three functions are `static`, so this file takes the reference's mpegvideo_enc.c in by #include where it lies in
 * that build (the archive's own copy of the object is then never pulled in: everything it defines is defined here).  It holds
 * nothing of the file itself.
 *
 * The reference's command line cannot reach dct_quantize_refine for its amv encoder: intra_ac_vlc_length is NULL for MJPEG.
 * Here the context is what the amv encoder would have had, plus the tables it lacked:
 *   dsputil_init on a zeroed AVCodecContext (fdct = ff_jpeg_fdct_islow, try_8x8basis / add_8x8basis the C ones, the identity
 *   permutation), the zig-zag scan, q_intra_matrix as ff_convert_matrix makes it from ff_mpeg1_default_intra_matrix,
 *   y_dc_scale = c_dc_scale = 8, mb_intra = 1, out_format = FMT_MJPEG, lambda2, quantizer_noise_shaping,
 *   intra_ac_vlc_length = intra_ac_vlc_last_length = the caller's table (UNI_AC_ENC_INDEX layout).
 *
 *   ref_qns_harness IN OUT
 * IN (text): qscale lambda2 qns blocks, then 64 * 128 table entries, then blocks * 64 samples (0 .. 255, row-major).
 * OUT (text): first the 64 * 64 entries of the function's basis table, then per block 64 levels (row-major, position 0 the
 * DC) and the function's return value. */
#include "mpegvideo_enc.c"

#include <stdio.h>
#include <stdlib.h>
/* the reference's internal headers turn these into link errors for its own files; this is not one of them */
#undef fprintf
#undef printf
#undef malloc
#undef free

int main(int argc, char **argv)
{
    if (argc != 3) return fprintf(stderr, "usage: %s IN OUT\n", argv[0]), 2;
    FILE *in = fopen(argv[1], "r"), *out = fopen(argv[2], "w");
    if (!in || !out) return fprintf(stderr, "cannot open the files\n"), 2;
    int qscale, lambda2, qns, blocks;
    if (fscanf(in, "%d %d %d %d", &qscale, &lambda2, &qns, &blocks) != 4 || qscale < 1 || qscale > 31) return fprintf(stderr, "bad header\n"), 2;
    static uint8_t length[64 * 128];
    for (int i = 0; i < 64 * 128; i++) {
        int v;
        if (fscanf(in, "%d", &v) != 1) return fprintf(stderr, "short table\n"), 2;
        length[i] = (uint8_t)v;
    }

    avcodec_init();
    MpegEncContext *s = calloc(1, sizeof *s);
    AVCodecContext *avctx = calloc(1, sizeof *avctx);
    static int q_intra[32][64];
    s->avctx = avctx;
    avctx->quantizer_noise_shaping = qns;
    dsputil_init(&s->dsp, avctx);
    if (s->dsp.fdct != ff_jpeg_fdct_islow || s->dsp.idct_permutation_type != FF_NO_IDCT_PERM) return fprintf(stderr, "not the amv encoder's dsp\n"), 2;
    ff_init_scantable(s->dsp.idct_permutation, &s->intra_scantable, ff_zigzag_direct);
    for (int i = 0; i < 64; i++) s->intra_matrix[i] = ff_mpeg1_default_intra_matrix[i];
    s->q_intra_matrix = q_intra;
    ff_convert_matrix(&s->dsp, s->q_intra_matrix, NULL, s->intra_matrix, 0, qscale, qscale, 1);
    s->y_dc_scale = s->c_dc_scale = 8;
    s->mb_intra = 1;
    s->out_format = FMT_MJPEG;
    s->lambda2 = lambda2;
    s->intra_ac_vlc_length = s->intra_ac_vlc_last_length = length;
    s->dct_error_sum = NULL;
    s->max_qcoeff = 1023;

    int basis_written = 0;
    for (int b = 0; b < blocks; b++) {
        DECLARE_ALIGNED_16(DCTELEM, block[64]);
        DECLARE_ALIGNED_16(DCTELEM, orig[64]);
        DECLARE_ALIGNED_16(int16_t, weight[64]);
        uint8_t pixels[64];
        for (int i = 0; i < 64; i++) {
            int v;
            if (fscanf(in, "%d", &v) != 1) return fprintf(stderr, "short block %d\n", b), 2;
            pixels[i] = (uint8_t)v;
            block[i] = orig[i] = (DCTELEM)v;
        }
        int overflow = 0;
        get_vissual_weight(weight, pixels, 8);
        s->block_last_index[0] = dct_quantize_c(s, block, 0, qscale, &overflow);
        const int last = dct_quantize_refine(s, block, weight, orig, 0, qscale);
        if (!basis_written) {
            for (int i = 0; i < 64; i++) {
                for (int k = 0; k < 64; k++) fprintf(out, "%d ", basis[i][k]);
                fprintf(out, "\n");
            }
            basis_written = 1;
        }
        for (int i = 0; i < 64; i++) fprintf(out, "%d ", block[i]);
        fprintf(out, "%d\n", last);
    }
    fclose(out);
    return 0;
}
