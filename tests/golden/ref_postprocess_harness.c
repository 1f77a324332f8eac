/* ref_postprocess_harness.c -- calls the reference's own pp_get_mode_by_name_and_quality and pp_postprocess (libpostproc/
 * postprocess.c) on pictures a file gives it.  A tool of tests/golden/make_ref_postprocess_golden.py, which compiles it inside a
 * temporary build of the reference's ffmpeg (configured without MMX, so the C path is the only one) and links it with that
 * build's libavutil.a; nothing of that build is kept.  It takes postprocess.c in by #include where it lies in that build and
 * holds nothing of the file itself.
 *
 *   ref_postprocess_harness IN OUT
 * IN (text): one line per case, `width height quality mode file`: `file` holds the Y, U and V planes back to back, pitch = width.
 * OUT (text): per case `lumMode chromMode baseDcDiff flatnessThreshold forcedQuant same hy hu hv usec`: the parsed mode
 * (forcedQuant 0 unless FORCE_QUANT is set: the reference leaves it uninitialised), whether the three runs -- destination
 * pre-filled with 0x00, with 0xFF, and on a context that has processed another picture -- gave the same planes, the FNV-1a-64
 * of each output plane of the first run, and the microseconds of one pp_postprocess call.  A mode the reference refuses gives
 * `refused`. */
#include "libpostproc/postprocess.c"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#undef fprintf
#undef printf
#undef malloc
#undef free
#undef exit

static unsigned long long fnv(const uint8_t *p, size_t n)
{
    unsigned long long h = 0xcbf29ce484222325ULL;
    for (size_t i = 0; i < n; i++) h = (h ^ p[i]) * 0x100000001b3ULL;
    return h;
}

/* one line of slack in front of each destination plane: with fewer than 16 lines the loop copies the line above the plane
 * into tempDst (and never uses it) */
static void run(pp_context_t *c, pp_mode_t *m, uint8_t *in, uint8_t *out, int w, int h, int fill, double *usec)
{
    const size_t ysz = (size_t)w * h, csz = (size_t)(w / 2) * (h / 2);
    uint8_t *buf = malloc(ysz + 2 * csz + 3 * (size_t)w + 64);
    memset(buf, fill, ysz + 2 * csz + 3 * (size_t)w + 64);
    uint8_t *src[3] = {in, in + ysz, in + ysz + csz};
    uint8_t *dst[3] = {buf + w, buf + 2 * w + ysz, buf + 3 * w + ysz + csz};
    int stride[3] = {w, w / 2, w / 2};
    struct timespec a, b;
    clock_gettime(CLOCK_MONOTONIC, &a);
    pp_postprocess(src, stride, dst, stride, w, h, NULL, 0, m, c, 0);
    clock_gettime(CLOCK_MONOTONIC, &b);
    if (usec) *usec = (b.tv_sec - a.tv_sec) * 1e6 + (b.tv_nsec - a.tv_nsec) / 1e3;
    memcpy(out, dst[0], ysz);
    memcpy(out + ysz, dst[1], csz);
    memcpy(out + ysz + csz, dst[2], csz);
    free(buf);
}

int main(int argc, char **argv)
{
    if (argc != 3) return fprintf(stderr, "usage: %s IN OUT\n", argv[0]), 2;
    FILE *in = fopen(argv[1], "r"), *out = fopen(argv[2], "w");
    if (!in || !out) return fprintf(stderr, "cannot open the files\n"), 2;
    int w, h, quality;
    char mode[256], path[1024];
    while (fscanf(in, "%d %d %d %255s %1023s", &w, &h, &quality, mode, path) == 5) {
        const size_t ysz = (size_t)w * h, csz = (size_t)(w / 2) * (h / 2), all = ysz + 2 * csz;
        PPMode *m = pp_get_mode_by_name_and_quality(mode, quality);
        if (!m) {
            fprintf(out, "refused\n");
            continue;
        }
        uint8_t *pic = malloc(all), *other = malloc(all), *o0 = malloc(all), *o1 = malloc(all), *o2 = malloc(all);
        FILE *f = fopen(path, "rb");
        if (!f || fread(pic, 1, all, f) != all) return fprintf(stderr, "short picture %s\n", path), 2;
        fclose(f);
        for (size_t i = 0; i < all; i++) other[i] = (uint8_t)(i * 2654435761u >> 13);
        double usec = 0;
        pp_context_t *c = pp_get_context(w, h, PP_FORMAT_420);
        run(c, m, pic, o0, w, h, 0x00, NULL);
        pp_free_context(c);
        c = pp_get_context(w, h, PP_FORMAT_420);
        run(c, m, pic, o1, w, h, 0xFF, NULL);
        pp_free_context(c);
        c = pp_get_context(w, h, PP_FORMAT_420);
        run(c, m, other, o2, w, h, 0x55, NULL);
        run(c, m, pic, o2, w, h, 0xAA, &usec);
        pp_free_context(c);
        const int same = !memcmp(o0, o1, all) && !memcmp(o0, o2, all);
        fprintf(out, "%d %d %d %d %d %d %016llx %016llx %016llx %.1f\n", m->lumMode, m->chromMode, m->baseDcDiff, m->flatnessThreshold,
                (m->lumMode | m->chromMode) & FORCE_QUANT ? m->forcedQuant : 0, same, fnv(o0, ysz), fnv(o0 + ysz, csz), fnv(o0 + ysz + csz, csz), usec);
        free(pic); free(other); free(o0); free(o1); free(o2);
        pp_free_mode(m);
    }
    fclose(out);
    return 0;
}
