/* ref_harness_audio.c -- TEST INFRASTRUCTURE ONLY.  Entry points around the reference's audio resampler, compiled into
 * oracle/_ref/libarref.so next to the reference's own libavcodec/resample.c and resample2.c (see the Makefile): nothing
 * of the reference is restated here.  One call runs one stream: audio_resample_init, one audio_resample per packet on a
 * copy of the packet (an allocation of exactly the packet's size, and an output of exactly the `lenout` samples per
 * channel that resample.c:194 lets av_resample write), audio_resample_close.  tests/golden/make_ref_audio_resample_golden.py
 * is the only caller. */
#include <stdlib.h>
#include <string.h>

#define EXPORT __attribute__((visibility("default")))

struct ReSampleContext;
struct ReSampleContext *audio_resample_init(int output_channels, int input_channels, int output_rate, int input_rate);
int audio_resample(struct ReSampleContext *s, short *output, short *input, int nb_samples);
void audio_resample_close(struct ReSampleContext *s);

/* in: interleaved in_ch, the packets back to back; packets[i]: frames of call i; out: room for out_cap samples;
 * counts[i]: what call i returned.  Returns the output frames of all calls, -1: a refusal of the reference's init or a
 * call that cannot be made (a packet of no frames before the resampler holds any: the mirrored head's `% src_size` would
 * divide by zero), -2: out too small. */
EXPORT long ref_audio_resample_run(int out_ch, int in_ch, int out_rate, int in_rate, const short *in, const int *packets,
                                   int n_packets, short *out, long out_cap, int *counts)
{
    struct ReSampleContext *s;
    long total = 0, fed = 0, pos = 0;
    int i, rc = 0;
    const float ratio = (float)out_rate / (float)in_rate;

    if (in_ch < 1 || in_ch > 2 || out_ch < 1 || out_ch > 2)
        return -1;
    s = audio_resample_init(out_ch, in_ch, out_rate, in_rate);
    if (!s)
        return -1;
    for (i = 0; i < n_packets && rc == 0; i++) {
        const int nb = packets[i];
        const int lenout = (int)(4 * nb * ratio) + 16;
        short *pkt, *dst;
        int n;
        fed += nb;
        if (nb < 0 || fed == 0) {
            rc = -1;
            break;
        }
        pkt = malloc(nb ? (size_t)nb * in_ch * sizeof(short) : 1);
        dst = malloc((size_t)lenout * out_ch * sizeof(short));
        if (!pkt || !dst) {
            free(pkt);
            free(dst);
            rc = -1;
            break;
        }
        memcpy(pkt, in + pos * in_ch, (size_t)nb * in_ch * sizeof(short));
        pos += nb;
        n = audio_resample(s, dst, pkt, nb);
        counts[i] = n;
        if (n < 0 || n > lenout)
            rc = -1;
        else if ((total + n) * out_ch > out_cap)
            rc = -2;
        else {
            memcpy(out + total * out_ch, dst, (size_t)n * out_ch * sizeof(short));
            total += n;
        }
        free(pkt);
        free(dst);
    }
    audio_resample_close(s);
    return rc ? rc : total;
}
