/* ref_nr_trellis_harness.c -- calls the reference's own dct_quantize_trellis_c (libavcodec/mpegvideo_enc.c:2961-3247) with
 * noise reduction on: a hand-filled MpegEncContext whose dct_error_sum is set, so that the function calls denoise_dct right
 * behind its fdct (:2987-2990) and searches on what that leaves.  A tool of tests/golden/make_ref_nr_trellis_golden.py, which
 * compiles it against a build of the reference's ffmpeg (its headers, libavcodec.a, libavutil.a); nothing of that build is kept.
 *
 * The context is that of ref_trellis_harness.c (which says why the command line cannot reach this function for the amv
 * encoder), and: denoise_dct = the reference's denoise_dct_c, dct_error_sum / dct_offset = arrays of this program with row 1
 * (mb_intra = 1) filled from the input, dct_count[1] from the input.
 *
 *   ref_nr_trellis_harness IN OUT
 * IN (text): qscale lambda2 esc_length blocks, then 64 * 128 table entries, then 64 error sums, the count, 64 offsets, then
 * blocks * 64 samples (0 .. 255, row-major).
 * OUT (text): per block 64 levels (row-major, position 0 the DC) and the function's return value; then one line of the 64
 * error sums and the count as the calls left them. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "libavcodec/avcodec.h"
#include "libavcodec/dsputil.h"
#include "libavcodec/mpegvideo.h"

int dct_quantize_trellis_c(MpegEncContext *s, DCTELEM *block, int n, int qscale, int *overflow);
void denoise_dct_c(MpegEncContext *s, DCTELEM *block);
void ff_convert_matrix(DSPContext *dsp, int (*qmat)[64], uint16_t (*qmat16)[2][64], const uint16_t *quant_matrix, int bias, int qmin,
                       int qmax, int intra);

int main(int argc, char **argv)
{
    if (argc != 3) return fprintf(stderr, "usage: %s IN OUT\n", argv[0]), 2;
    FILE *in = fopen(argv[1], "r"), *out = fopen(argv[2], "w");
    if (!in || !out) return fprintf(stderr, "cannot open the files\n"), 2;
    int qscale, lambda2, esc_length, blocks;
    if (fscanf(in, "%d %d %d %d", &qscale, &lambda2, &esc_length, &blocks) != 4 || qscale < 1 || qscale > 31) return fprintf(stderr, "bad header\n"), 2;
    static uint8_t length[64 * 128];
    for (int i = 0; i < 64 * 128; i++) {
        int v;
        if (fscanf(in, "%d", &v) != 1) return fprintf(stderr, "short table\n"), 2;
        length[i] = (uint8_t)v;
    }
    static int error_sum[2][64];
    static uint16_t offset[2][64];
    int count;
    for (int i = 0; i < 64; i++)
        if (fscanf(in, "%d", &error_sum[1][i]) != 1) return fprintf(stderr, "short sums\n"), 2;
    if (fscanf(in, "%d", &count) != 1) return fprintf(stderr, "no count\n"), 2;
    for (int i = 0; i < 64; i++) {
        int v;
        if (fscanf(in, "%d", &v) != 1 || v < 0 || v > 65535) return fprintf(stderr, "bad offset %d\n", i), 2;
        offset[1][i] = (uint16_t)v;
    }

    MpegEncContext *s = calloc(1, sizeof *s);
    static int q_intra[32][64];
    s->dsp.fdct = ff_jpeg_fdct_islow;
    for (int i = 0; i < 64; i++) {
        s->dsp.idct_permutation[i] = (uint8_t)i;
        s->intra_scantable.permutated[i] = ff_zigzag_direct[i];
        s->intra_matrix[i] = ff_mpeg1_default_intra_matrix[i];
    }
    s->intra_scantable.scantable = ff_zigzag_direct;
    s->q_intra_matrix = q_intra;
    ff_convert_matrix(&s->dsp, s->q_intra_matrix, NULL, s->intra_matrix, 0, qscale, qscale, 1);
    s->y_dc_scale = s->c_dc_scale = 8;
    s->mb_intra = 1;
    s->out_format = FMT_MJPEG;
    s->lambda2 = lambda2;
    s->intra_ac_vlc_length = s->intra_ac_vlc_last_length = length;
    s->ac_esc_length = esc_length;
    s->max_qcoeff = 1023;
    s->denoise_dct = denoise_dct_c;
    s->dct_error_sum = error_sum;
    s->dct_offset = offset;
    s->dct_count[1] = count;

    for (int b = 0; b < blocks; b++) {
        DECLARE_ALIGNED_16(DCTELEM, block[64]);
        for (int i = 0; i < 64; i++) {
            int v;
            if (fscanf(in, "%d", &v) != 1) return fprintf(stderr, "short block %d\n", b), 2;
            block[i] = (DCTELEM)v;
        }
        int overflow = 0;
        const int last = dct_quantize_trellis_c(s, block, 0, qscale, &overflow);
        for (int i = 0; i < 64; i++) fprintf(out, "%d ", block[i]);
        fprintf(out, "%d\n", last);
    }
    for (int i = 0; i < 64; i++) fprintf(out, "%d ", s->dct_error_sum[1][i]);
    fprintf(out, "%d\n", s->dct_count[1]);
    fclose(out);
    return 0;
}
