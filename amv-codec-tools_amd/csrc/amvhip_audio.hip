// amvhip_audio.hip -- audio behind the C ABI: the resampler (batch and streaming) and the ADPCM codecs.
#include "amvhip_ctx.h"

using namespace amv;

static_assert(kBankPhases == kAudioPhases, "the bank the host builds has the kernel's phases");

namespace {

bool audio_args_ok(uint32_t in_ch, uint32_t in_rate, uint32_t out_ch, uint32_t out_rate) {
    return in_ch >= 1 && in_ch <= 2 && out_ch >= 1 && out_ch <= 2 && in_rate >= AMVHIP_AUDIO_RATE_MIN &&
           in_rate <= AMVHIP_AUDIO_RATE_MAX && out_rate >= AMVHIP_AUDIO_RATE_MIN && out_rate <= AMVHIP_AUDIO_RATE_MAX;
}

struct AudioPlan {
    uint32_t fl, fl_pad, tile;
    uint64_t D;
};

AudioPlan audio_plan(uint32_t in_rate, uint32_t out_rate) {
    AudioPlan p;
    p.fl = audio_filter_length(in_rate, out_rate);
    p.fl_pad = (p.fl + 7u) & ~7u;
    p.tile = audio_resample_tile(in_rate, out_rate, p.fl_pad);
    p.D = (uint64_t)in_rate * kAudioPhases;
    return p;
}

// the bank of (in_rate, out_rate): built and uploaded on first use, then kept for the context's life.  Caller holds c->mu.
int audio_bank(amvhip_ctx* c, uint32_t in_rate, uint32_t out_rate, const AudioPlan& p, const int16_t** out) {
    DevBuf& b = c->audio_banks[(uint64_t)in_rate << 32 | out_rate];
    if (!b.p) {
        std::vector<int16_t> h;
        build_audio_bank(h, in_rate, out_rate, p.fl, p.fl_pad);
        if (int r = ensure(c, b, h.size() * 2)) return r;
        HIP_TRY(c, hipMemcpy(b.p, h.data(), h.size() * 2, hipMemcpyHostToDevice));
    }
    *out = (const int16_t*)b.p;
    return AMVHIP_OK;
}

// the launch every form shares; caller holds c->mu
int audio_resample_core(amvhip_ctx* c, const int16_t* d_pcm, const uint64_t* d_pcm_offs, const uint64_t* d_nsamp, uint32_t n,
                        uint32_t in_ch, uint32_t in_rate, int16_t* d_out, const uint64_t* d_out_offs, uint32_t out_ch,
                        uint32_t out_rate, int64_t base, uint64_t frac0, uint64_t cap, hipStream_t st) {
    const AudioPlan p = audio_plan(in_rate, out_rate);
    AudioResampleArgs a{};
    if (int r = audio_bank(c, in_rate, out_rate, p, &a.bank)) return r;
    if (int r = ensure(c, c->audio_tiles, ((size_t)n + 1) * 4)) return r;
    a.pcm = d_pcm;
    a.pcm_offs = d_pcm_offs;
    a.nsamp = d_nsamp;
    a.out = d_out;
    a.out_offs = d_out_offs;
    a.tiles = (uint32_t*)c->audio_tiles.p;
    a.n = n;
    a.in_ch = in_ch;
    a.out_ch = out_ch;
    a.out_rate = out_rate;
    a.fl = p.fl;
    a.fl_pad = p.fl_pad;
    a.tile = p.tile;
    a.D = p.D;
    a.base = base;
    a.frac0 = frac0;
    a.cap = cap;
    Timed t(c, AMVHIP_K_AUDIO_RESAMPLE, st);
    launch_audio_resample(a, c->cus * 8u, st);
    return check_launch(c, "audio_resample");
}

}  // namespace

extern "C" uint64_t amvhip_audio_resample_out_samples(uint32_t in_rate, uint32_t out_rate, uint64_t in_samples) {
    if (!audio_args_ok(1, in_rate, 1, out_rate) || in_samples == 0 || (in_samples >> 32)) return 0;
    const AudioPlan p = audio_plan(in_rate, out_rate);
    return audio_out_count(in_samples, audio_index0(p.fl), 0, p.D, out_rate, p.fl);
}

extern "C" int amvhip_audio_resample_batch_dev(amvhip_ctx* c, const int16_t* d_pcm, const uint64_t* d_pcm_offs, const uint64_t* d_nsamp,
                                               uint32_t n, uint32_t in_channels, uint32_t in_rate, int16_t* d_out,
                                               const uint64_t* d_out_offs, uint32_t out_channels, uint32_t out_rate, void* stream) {
    if (!c) return AMVHIP_ERR_ARG;
    if (!audio_args_ok(in_channels, in_rate, out_channels, out_rate))
        return fail(c, AMVHIP_ERR_ARG, "audio_resample: channels 1 or 2 in and out, rates %d .. %d", AMVHIP_AUDIO_RATE_MIN,
                    AMVHIP_AUDIO_RATE_MAX);
    if (n && (!d_pcm || !d_pcm_offs || !d_nsamp || !d_out || !d_out_offs)) return fail(c, AMVHIP_ERR_ARG, "audio_resample: null argument");
    if (n == 0) return AMVHIP_OK;
    if (int r = use_device(c)) return r;
    std::lock_guard<std::mutex> lk(c->mu);
    const AudioPlan p = audio_plan(in_rate, out_rate);
    return audio_resample_core(c, d_pcm, d_pcm_offs, d_nsamp, n, in_channels, in_rate, d_out, d_out_offs, out_channels, out_rate,
                               audio_index0(p.fl), 0, ~0ull, (hipStream_t)stream);
}

extern "C" int amvhip_audio_resample_batch(amvhip_ctx* c, const int16_t* pcm, uint64_t pcm_samples, const uint64_t* pcm_offs,
                                           const uint64_t* nsamp, uint32_t n, uint32_t in_channels, uint32_t in_rate, int16_t* out,
                                           uint64_t out_samples, const uint64_t* out_offs, uint32_t out_channels, uint32_t out_rate) {
    if (!c) return AMVHIP_ERR_ARG;
    if (!audio_args_ok(in_channels, in_rate, out_channels, out_rate))
        return fail(c, AMVHIP_ERR_ARG, "audio_resample: channels 1 or 2 in and out, rates %d .. %d", AMVHIP_AUDIO_RATE_MIN,
                    AMVHIP_AUDIO_RATE_MAX);
    if (n && (!pcm || !pcm_offs || !nsamp || !out || !out_offs)) return fail(c, AMVHIP_ERR_ARG, "audio_resample: null argument");
    if (n == 0) return AMVHIP_OK;
    for (uint32_t i = 0; i < n; ++i) {
        if ((nsamp[i] >> 32) || pcm_offs[i] > pcm_samples || nsamp[i] * in_channels > pcm_samples - pcm_offs[i])
            return fail(c, AMVHIP_ERR_ARG, "audio_resample: stream %u reads past pcm", i);
        const uint64_t m = amvhip_audio_resample_out_samples(in_rate, out_rate, nsamp[i]) * out_channels;
        if (out_offs[i] > out_samples || m > out_samples - out_offs[i])
            return fail(c, AMVHIP_ERR_SPACE, "audio_resample: out too small for stream %u", i);
    }
    hipStream_t hs;
    if (int r = host_stream(c, &hs)) return r;
    std::lock_guard<std::mutex> hlk(c->hmu);   // the staging buffers: one host-buffer call at a time
    if (int r = stage(c, c->r_in, pcm_samples * 2 + 16, pcm, pcm_samples * 2, hs)) return r;
    if (int r = stage(c, c->r_out, out_samples * 2 + 16, out, out_samples * 2, hs)) return r;   // keep untouched gaps
    if (int r = ensure(c, c->r_tab, (size_t)n * 24)) return r;
    uint64_t* tab = (uint64_t*)c->r_tab.p;
    HIP_TRY(c, hipMemcpyAsync(tab, pcm_offs, (size_t)n * 8, hipMemcpyHostToDevice, hs));
    HIP_TRY(c, hipMemcpyAsync(tab + n, nsamp, (size_t)n * 8, hipMemcpyHostToDevice, hs));
    HIP_TRY(c, hipMemcpyAsync(tab + 2 * (size_t)n, out_offs, (size_t)n * 8, hipMemcpyHostToDevice, hs));
    if (int r = amvhip_audio_resample_batch_dev(c, (const int16_t*)c->r_in.p, tab, tab + n, n, in_channels, in_rate, (int16_t*)c->r_out.p,
                                                tab + 2 * (size_t)n, out_channels, out_rate, hs))
        return r;
    HIP_TRY(c, hipMemcpyAsync(out, c->r_out.p, out_samples * 2, hipMemcpyDeviceToHost, hs));
    HIP_TRY(c, hipStreamSynchronize(hs));
    return AMVHIP_OK;
}

// The streaming form: audio_resample_init / audio_resample / audio_resample_close of resample.c, the calls ffmpeg.c:1639-1641
// and :502 make.  The host keeps what ReSampleContext keeps -- index and frac of the AVResampleContext and the unconsumed
// tail `temp` (:186-226) -- and runs every packet through the batch kernel as one stream: the tail and the packet, from the
// kept position, at most lenout (:194) outputs.  The tail is kept as input frames as they came (2 -> 1 mixes down on the
// device; a frame (l, r) mixes to the value the reference keeps), so nothing is computed here but positions.
struct amvhip_audio_resampler {
    amvhip_ctx* c = nullptr;
    uint32_t in_ch = 0, out_ch = 0, in_rate = 0, out_rate = 0;
    float ratio = 0;
    int64_t index = 0;
    uint64_t frac = 0;
    std::vector<int16_t> temp;   // unconsumed input frames, interleaved in_ch
};

extern "C" amvhip_audio_resampler* amvhip_audio_resample_init(amvhip_ctx* c, int output_channels, int input_channels, int output_rate,
                                                              int input_rate) {
    if (!c) return nullptr;
    if (output_channels < 1 || input_channels < 1 || output_rate < 0 || input_rate < 0 ||
        !audio_args_ok((uint32_t)input_channels, (uint32_t)input_rate, (uint32_t)output_channels, (uint32_t)output_rate)) {
        fail(c, AMVHIP_ERR_ARG, "audio_resample_init: channels 1 or 2 in and out (no 5.1), rates %d .. %d", AMVHIP_AUDIO_RATE_MIN,
             AMVHIP_AUDIO_RATE_MAX);
        return nullptr;
    }
    if (use_device(c)) return nullptr;
    const AudioPlan p = audio_plan((uint32_t)input_rate, (uint32_t)output_rate);
    {
        std::lock_guard<std::mutex> lk(c->mu);
        const int16_t* bank;
        if (audio_bank(c, (uint32_t)input_rate, (uint32_t)output_rate, p, &bank)) return nullptr;
    }
    amvhip_audio_resampler* r = new amvhip_audio_resampler;
    r->c = c;
    r->in_ch = (uint32_t)input_channels;
    r->out_ch = (uint32_t)output_channels;
    r->in_rate = (uint32_t)input_rate;
    r->out_rate = (uint32_t)output_rate;
    r->ratio = (float)output_rate / (float)input_rate;   // s->ratio (:146)
    r->index = audio_index0(p.fl);                       // c->index of av_resample_init (:201)
    return r;
}

extern "C" int amvhip_audio_resample(amvhip_audio_resampler* r, short* output, short* input, int nb_samples) {
    if (!r) return AMVHIP_ERR_ARG;
    amvhip_ctx* c = r->c;
    if (nb_samples < 0 || nb_samples > (1 << 28) || !output || (nb_samples && !input))
        return fail(c, AMVHIP_ERR_ARG, "audio_resample: bad argument");
    const AudioPlan p = audio_plan(r->in_rate, r->out_rate);
    const int lenout = (int)(4 * nb_samples * r->ratio) + 16;                      // :194
    const size_t have = r->temp.size(), add = (size_t)nb_samples * r->in_ch;
    const uint64_t src = (have + add) / r->in_ch;                                   // nb_samples += s->temp_len (:218)
    if (src == 0) return 0;
    uint64_t count = audio_out_count(src, r->index, r->frac, p.D, r->out_rate, p.fl);
    if (count > (uint64_t)lenout) count = (uint64_t)lenout;
    if (count) {
            hipStream_t hs;
        if (int e = host_stream(c, &hs)) return e;
        std::lock_guard<std::mutex> hlk(c->hmu);
        if (int e = ensure(c, c->r_in, (have + add) * 2 + 16)) return e;
        if (int e = ensure(c, c->r_out, count * r->out_ch * 2 + 16)) return e;
        if (int e = ensure(c, c->r_tab, 24)) return e;
        const uint64_t tab[3] = {0, src, 0};   // pcm offset, frames, out offset of the one stream
        if (have) HIP_TRY(c, hipMemcpyAsync(c->r_in.p, r->temp.data(), have * 2, hipMemcpyHostToDevice, hs));
        if (add) HIP_TRY(c, hipMemcpyAsync((int16_t*)c->r_in.p + have, input, add * 2, hipMemcpyHostToDevice, hs));
        HIP_TRY(c, hipMemcpyAsync(c->r_tab.p, tab, sizeof tab, hipMemcpyHostToDevice, hs));
        {
            std::lock_guard<std::mutex> lk(c->mu);
            const uint64_t* d_tab = (const uint64_t*)c->r_tab.p;
            if (int e = audio_resample_core(c, (const int16_t*)c->r_in.p, d_tab, d_tab + 1, 1, r->in_ch, r->in_rate, (int16_t*)c->r_out.p,
                                            d_tab + 2, r->out_ch, r->out_rate, r->index, r->frac, count, hs))
                return e;
        }
        HIP_TRY(c, hipMemcpyAsync(output, c->r_out.p, count * r->out_ch * 2, hipMemcpyDeviceToHost, hs));
        HIP_TRY(c, hipStreamSynchronize(hs));
    }
    // the state av_resample leaves and the new tail (:222-225)
    const uint64_t consumed = audio_advance(r->index, r->frac, count, p.D, r->out_rate);
    std::vector<int16_t> rest;
    rest.reserve(have + add - consumed * r->in_ch);
    for (uint64_t i = consumed * r->in_ch; i < have + add; ++i) rest.push_back(i < have ? r->temp[i] : input[i - have]);
    r->temp.swap(rest);
    return (int)count;
}

extern "C" void amvhip_audio_resample_close(amvhip_audio_resampler* r) { delete r; }

// ---- ADPCM ------------------------------------------------------------------------------------------------------------

extern "C" int amvhip_adpcm_decode_batch_dev(amvhip_ctx* c, const uint8_t* d_blob, uint64_t blob_bytes, const uint64_t* d_offs,
                                             const uint32_t* d_lens, uint32_t n, int16_t* d_pcm, const uint64_t* d_pcm_offs,
                                             int32_t* d_final_state, void* stream) {
    if (!c) return AMVHIP_ERR_ARG;
    if (n && (!d_blob || !d_offs || !d_lens || !d_pcm || !d_pcm_offs)) return fail(c, AMVHIP_ERR_ARG, "adpcm_decode: null argument");
    if (int r = use_device(c)) return r;
    {
        Timed t(c, AMVHIP_K_ADPCM_DEC, (hipStream_t)stream);
        launch_adpcm_decode(d_blob, blob_bytes, d_offs, d_lens, n, d_pcm, d_pcm_offs, d_final_state, (hipStream_t)stream);
    }
    return check_launch(c, "adpcm_decode");
}

extern "C" int amvhip_adpcm_encode_batch_dev(amvhip_ctx* c, const int16_t* d_pcm, const uint64_t* d_pcm_offs, const uint32_t* d_nsamp,
                                             uint32_t n, const int32_t* d_step_in, uint8_t* d_blob, const uint64_t* d_offs, void* stream) {
    if (!c) return AMVHIP_ERR_ARG;
    if (n && (!d_pcm || !d_pcm_offs || !d_nsamp || !d_blob || !d_offs)) return fail(c, AMVHIP_ERR_ARG, "adpcm_encode: null argument");
    if (n == 0) return AMVHIP_OK;
    if (int r = use_device(c)) return r;
    std::lock_guard<std::mutex> lk(c->mu);
    Timed t(c, AMVHIP_K_ADPCM_ENC, (hipStream_t)stream);
    if (!d_step_in) {  // the reference's behaviour: step_index runs through the whole stream
        if (int r = ensure(c, c->chain, adpcm_plain_chain_plan(n).bytes)) return r;
        // guessed starts + sweeps, the exhaustive route behind them runs only if they do not settle (adpcm_sweeps < 0: it
        // runs at once).  (state, lists, counters and maps live in the context's `chain` buffer: chained encodes of ONE
        // context must be ordered on the device -- one stream at a time, as for every _dev entry point; see amvhip.h)
        const int sweeps = c->adpcm_sweeps_set ? c->adpcm_sweeps : (int)adpcm_default_sweeps(n);
        if (!launch_adpcm_stream(d_pcm, d_pcm_offs, d_nsamp, n, d_blob, d_offs, c->chain.p, sweeps, c->adpcm_settle, (hipStream_t)stream))
            return fail(c, AMVHIP_ERR_DEVICE, "adpcm_encode: clearing the chain counters failed");
        // chain_n != 0: `chain` holds the counters of a chained encode of chain_n chunks (amvhip_adpcm_chain_stats).  The
        // forced exhaustive route counts nothing and leaves it alone: its knob is fixed when the context is made, so such
        // a context never has statistics, as before
        if (sweeps >= 0) c->chain_n = n;
        return check_launch(c, "adpcm_encode");
    }
    launch_adpcm_encode(d_pcm, d_pcm_offs, d_nsamp, n, d_step_in, d_blob, d_offs, nullptr, (hipStream_t)stream);
    return check_launch(c, "adpcm_encode");
}

extern "C" void amvhip_adpcm_quotient_table(float out[89]) {
    if (out) adpcm_quotient_table(out);
}

// what both chains' statistics are: out[0] = the exhaustive route ran, out[1 + k] = the counter word first + k of the
// last call's plan p in buffer b.  Caller holds c->mu.
static int chain_stats(amvhip_ctx* c, const DevBuf& b, const ChainPlan& p, uint32_t first, uint32_t out[64]) {
    uint32_t w[kChainCounterWords];
    HIP_TRY(c, hipDeviceSynchronize());
    HIP_TRY(c, hipMemcpy(w, (const uint8_t*)b.p + p.counters, sizeof w, hipMemcpyDeviceToHost));
    out[0] = w[kChainWordNeed] ? 1u : 0u;
    for (uint32_t k = 0; k < 62u; ++k) out[k + 1u] = w[first + k];
    out[63] = 0;
    return AMVHIP_OK;
}

extern "C" int amvhip_adpcm_chain_stats(amvhip_ctx* c, uint32_t out[64]) {
    if (!c || !out) return AMVHIP_ERR_ARG;
    if (int r = use_device(c)) return r;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->chain_n) return fail(c, AMVHIP_ERR_ARG, "adpcm_chain_stats: no chained encode has run");
    return chain_stats(c, c->chain, adpcm_plain_chain_plan(c->chain_n), chain_word_list(0), out);
}

extern "C" int amvhip_adpcm_decode_batch_async(amvhip_ctx* c, const uint8_t* blob, uint64_t blob_bytes,
                                               const uint64_t* offs, const uint32_t* lens, uint32_t n, int16_t* pcm,
                                               uint64_t pcm_samples, const uint64_t* pcm_offs, int32_t* final_state) {
    if (!c) return AMVHIP_ERR_ARG;
    if (n && (!blob || !offs || !lens || !pcm || !pcm_offs)) return fail(c, AMVHIP_ERR_ARG, "adpcm_decode: null argument");
    if (n == 0) return AMVHIP_OK;
    for (uint32_t i = 0; i < n; ++i)
        if (lens[i] > 8 && pcm_offs[i] + 2ull * (lens[i] - 8) > pcm_samples) return fail(c, AMVHIP_ERR_SPACE, "adpcm_decode: pcm too small for chunk %u", i);
    hipStream_t st;
    if (int r = host_stream(c, &st)) return r;
    // audio staging sits behind the video staging of the same stream: separate buffers, so that a video batch and the
    // audio batch that travels with it can both be in flight
    std::lock_guard<std::mutex> hlk(c->hmu);   // the staging buffers: one host-buffer call at a time
    if (int r = stage(c, c->a_in, blob_bytes + 16, blob, blob_bytes, st)) return r;
    if (int r = ensure(c, c->a_tab, (size_t)n * 28)) return r;
    if (int r = stage(c, c->a_out, pcm_samples * 2, pcm, pcm_samples * 2, st)) return r;   // keep untouched gaps
    uint8_t* tab = (uint8_t*)c->a_tab.p;
    uint64_t* d_offs = (uint64_t*)tab;
    uint64_t* d_pcm_offs = (uint64_t*)(tab + (size_t)n * 8);
    int32_t* d_fin = (int32_t*)(tab + (size_t)n * 16);
    uint32_t* d_lens = (uint32_t*)(tab + (size_t)n * 24);
    HIP_TRY(c, hipMemcpyAsync(d_offs, offs, (size_t)n * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(d_lens, lens, (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(d_pcm_offs, pcm_offs, (size_t)n * 8, hipMemcpyHostToDevice, st));
    if (int r = amvhip_adpcm_decode_batch_dev(c, (const uint8_t*)c->a_in.p, blob_bytes, d_offs, d_lens, n, (int16_t*)c->a_out.p,
                                              d_pcm_offs, d_fin, st))
        return r;
    HIP_TRY(c, hipMemcpyAsync(pcm, c->a_out.p, pcm_samples * 2, hipMemcpyDeviceToHost, st));
    if (final_state) HIP_TRY(c, hipMemcpyAsync(final_state, d_fin, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    return AMVHIP_OK;
}

extern "C" int amvhip_adpcm_decode_batch(amvhip_ctx* c, const uint8_t* blob, uint64_t blob_bytes, const uint64_t* offs, const uint32_t* lens,
                                         uint32_t n, int16_t* pcm, uint64_t pcm_samples, const uint64_t* pcm_offs, int32_t* final_state) {
    if (int r = amvhip_adpcm_decode_batch_async(c, blob, blob_bytes, offs, lens, n, pcm, pcm_samples, pcm_offs, final_state)) return r;
    return amvhip_sync(c);
}

extern "C" int amvhip_adpcm_encode_batch(amvhip_ctx* c, const int16_t* pcm, uint64_t pcm_samples, const uint64_t* pcm_offs,
                                         const uint32_t* nsamp, uint32_t n, const int32_t* step_in, uint8_t* blob, uint64_t blob_bytes,
                                         const uint64_t* offs) {
    if (!c) return AMVHIP_ERR_ARG;
    if (n && (!pcm || !pcm_offs || !nsamp || !blob || !offs)) return fail(c, AMVHIP_ERR_ARG, "adpcm_encode: null argument");
    if (n == 0) return AMVHIP_OK;
    for (uint32_t i = 0; i < n; ++i) {
        if (pcm_offs[i] + nsamp[i] > pcm_samples) return fail(c, AMVHIP_ERR_ARG, "adpcm_encode: chunk %u reads past pcm", i);
        if (offs[i] + 8ull + (nsamp[i] >> 1) > blob_bytes) return fail(c, AMVHIP_ERR_SPACE, "adpcm_encode: blob too small for chunk %u", i);
    }
    hipStream_t hs;
    if (int r = host_stream(c, &hs)) return r;
    std::lock_guard<std::mutex> hlk(c->hmu);   // the staging buffers: one host-buffer call at a time
    if (int r = stage(c, c->h_in, pcm_samples * 2 + 16, pcm, pcm_samples * 2, hs)) return r;
    if (int r = stage(c, c->h_offs, (size_t)n * 8, offs, (size_t)n * 8, hs)) return r;
    if (int r = stage(c, c->h_lens, (size_t)n * 4, nsamp, (size_t)n * 4, hs)) return r;
    if (int r = stage(c, c->h_out, blob_bytes, blob, blob_bytes, hs)) return r;
    if (int r = stage(c, c->h_aux, (size_t)n * 8, pcm_offs, (size_t)n * 8, hs)) return r;
    if (int r = ensure(c, c->h_status, (size_t)n * 4)) return r;
    if (step_in) HIP_TRY(c, hipMemcpyAsync(c->h_status.p, step_in, (size_t)n * 4, hipMemcpyHostToDevice, hs));
    if (int r = amvhip_adpcm_encode_batch_dev(c, (const int16_t*)c->h_in.p, (const uint64_t*)c->h_aux.p,
                                              (const uint32_t*)c->h_lens.p, n,
                                              step_in ? (const int32_t*)c->h_status.p : nullptr,
                                              (uint8_t*)c->h_out.p, (const uint64_t*)c->h_offs.p, hs))
        return r;
    HIP_TRY(c, hipMemcpyAsync(blob, c->h_out.p, blob_bytes, hipMemcpyDeviceToHost, hs));
    HIP_TRY(c, hipStreamSynchronize(hs));
    return AMVHIP_OK;
}

// The reference's `-trellis N` quality mode (adpcm_compress_trellis, adpcm.c:287-443) for independent chunks: every chunk
// starts from d_step_in[i] and reports the index it ends on in d_step_out[i] (optional).
extern "C" int amvhip_adpcm_encode_trellis_batch_dev(amvhip_ctx* c, const int16_t* d_pcm, const uint64_t* d_pcm_offs,
                                                     const uint32_t* d_nsamp, uint32_t n, const int32_t* d_step_in, uint32_t trellis,
                                                     uint8_t* d_blob, const uint64_t* d_offs, int32_t* d_step_out, void* stream) {
    if (!c) return AMVHIP_ERR_ARG;
    if (trellis < 1 || trellis > 5 || (n && (!d_pcm || !d_pcm_offs || !d_nsamp || !d_step_in || !d_blob || !d_offs)))
        return fail(c, AMVHIP_ERR_ARG, "adpcm_encode_trellis: bad argument (trellis 1..5, start indices required)");
    if (n == 0) return AMVHIP_OK;
    if (int r = use_device(c)) return r;
    std::lock_guard<std::mutex> lk(c->mu);
    if (int r = ensure(c, c->trellis_ws, adpcm_trellis_workspace(n, trellis))) return r;
    Timed t(c, AMVHIP_K_ADPCM_ENC, (hipStream_t)stream);
    if (!launch_adpcm_trellis(d_pcm, d_pcm_offs, d_nsamp, n, d_step_in, trellis, d_blob, d_offs, d_step_out, (uint16_t*)c->trellis_ws.p,
                              (hipStream_t)stream))
        return fail(c, AMVHIP_ERR_DEVICE, "adpcm_encode_trellis: kernel attributes refused");
    return check_launch(c, "adpcm_trellis");
}

// ... and for a stream: the chunks of a call in order, chunk 0 from first_step_index, every other from the index its
// predecessor ends on (what a loop over amvhip_adpcm_encode_frame_trellis computes), resolved on the device.
extern "C" int amvhip_adpcm_encode_trellis_stream_dev(amvhip_ctx* c, const int16_t* d_pcm, const uint64_t* d_pcm_offs,
                                                      const uint32_t* d_nsamp, uint32_t n, int32_t first_step_index, uint32_t trellis,
                                                      uint8_t* d_blob, const uint64_t* d_offs, int32_t* d_step_out, void* stream) {
    if (!c) return AMVHIP_ERR_ARG;
    if (trellis < 1 || trellis > 5 || (n && (!d_pcm || !d_pcm_offs || !d_nsamp || !d_blob || !d_offs)))
        return fail(c, AMVHIP_ERR_ARG, "adpcm_encode_trellis_stream: bad argument (trellis 1..5)");
    if (n == 0) return AMVHIP_OK;
    if (int r = use_device(c)) return r;
    std::lock_guard<std::mutex> lk(c->mu);
    if (int r = ensure(c, c->trellis_ws, adpcm_trellis_workspace(n, trellis))) return r;
    if (int r = ensure(c, c->trellis_chain, adpcm_trellis_chain_plan(n).bytes)) return r;
    const uint32_t first = (uint32_t)(first_step_index < 0 ? 0 : (first_step_index > 88 ? 88 : first_step_index));
    Timed t(c, AMVHIP_K_ADPCM_ENC, (hipStream_t)stream);
    // (state, lists and counters live in the context's `trellis_chain` buffer: stream calls of ONE context must be ordered
    // on the device -- one stream at a time, as for every _dev entry point)
    if (!launch_adpcm_trellis_stream(d_pcm, d_pcm_offs, d_nsamp, n, first, trellis, d_blob, d_offs, d_step_out, (uint16_t*)c->trellis_ws.p,
                                     c->trellis_chain.p, c->trellis_sweeps, (hipStream_t)stream))
        return fail(c, AMVHIP_ERR_DEVICE, "adpcm_encode_trellis_stream: kernel attributes or the counters' memset refused");
    c->trellis_chain_n = n;
    return check_launch(c, "adpcm_trellis_stream");
}

extern "C" int amvhip_adpcm_trellis_chain_stats(amvhip_ctx* c, uint32_t out[64]) {
    if (!c || !out) return AMVHIP_ERR_ARG;
    if (int r = use_device(c)) return r;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->trellis_chain_n) return fail(c, AMVHIP_ERR_ARG, "adpcm_trellis_chain_stats: no trellis stream has been coded");
    return chain_stats(c, c->trellis_chain, adpcm_trellis_chain_plan(c->trellis_chain_n), chain_word_recoded(0), out);
}

extern "C" int amvhip_adpcm_encode_trellis_stream(amvhip_ctx* c, const int16_t* pcm, uint64_t pcm_samples, const uint64_t* pcm_offs,
                                                  const uint32_t* nsamp, uint32_t n, int32_t first_step_index, uint32_t trellis,
                                                  uint8_t* blob, uint64_t blob_bytes, const uint64_t* offs, int32_t* step_out) {
    if (!c) return AMVHIP_ERR_ARG;
    if (trellis < 1 || trellis > 5 || (n && (!pcm || !pcm_offs || !nsamp || !blob || !offs)))
        return fail(c, AMVHIP_ERR_ARG, "adpcm_encode_trellis_stream: bad argument (trellis 1..5)");
    if (n == 0) return AMVHIP_OK;
    for (uint32_t i = 0; i < n; ++i) {
        if (pcm_offs[i] > pcm_samples || nsamp[i] > pcm_samples - pcm_offs[i])
            return fail(c, AMVHIP_ERR_ARG, "adpcm_encode_trellis_stream: chunk %u reads past pcm", i);
        if (offs[i] > blob_bytes || 8ull + (nsamp[i] >> 1) > blob_bytes - offs[i])
            return fail(c, AMVHIP_ERR_SPACE, "adpcm_encode_trellis_stream: blob too small for chunk %u", i);
    }
    hipStream_t hs;
    if (int r = host_stream(c, &hs)) return r;
    std::lock_guard<std::mutex> hlk(c->hmu);   // the staging buffers: one host-buffer call at a time
    if (int r = stage(c, c->h_in, pcm_samples * 2 + 16, pcm, pcm_samples * 2, hs)) return r;
    if (int r = stage(c, c->h_offs, (size_t)n * 8, offs, (size_t)n * 8, hs)) return r;
    if (int r = stage(c, c->h_lens, (size_t)n * 4, nsamp, (size_t)n * 4, hs)) return r;
    if (int r = stage(c, c->h_out, blob_bytes, blob, blob_bytes, hs)) return r;   // keep untouched gaps
    if (int r = stage(c, c->h_aux, (size_t)n * 8, pcm_offs, (size_t)n * 8, hs)) return r;
    if (int r = ensure(c, c->h_status, (size_t)n * 4)) return r;
    if (int r = amvhip_adpcm_encode_trellis_stream_dev(c, (const int16_t*)c->h_in.p, (const uint64_t*)c->h_aux.p, (const uint32_t*)c->h_lens.p, n,
                                                       first_step_index, trellis, (uint8_t*)c->h_out.p, (const uint64_t*)c->h_offs.p,
                                                       step_out ? (int32_t*)c->h_status.p : nullptr, hs))
        return r;
    HIP_TRY(c, hipMemcpyAsync(blob, c->h_out.p, blob_bytes, hipMemcpyDeviceToHost, hs));
    if (step_out) HIP_TRY(c, hipMemcpyAsync(step_out, c->h_status.p, (size_t)n * 4, hipMemcpyDeviceToHost, hs));
    HIP_TRY(c, hipStreamSynchronize(hs));
    return AMVHIP_OK;
}

// One AMV audio chunk with the step index handed in and out: what adpcm_encode_frame (adpcm.c:461-498) does per
// call with the index it keeps in its context.  The end index is read off a decode of the fresh chunk (the decoder
// walks the same index chain), one synchronisation for both kernels.
static int adpcm_encode_frame_impl(amvhip_ctx* c, const int16_t* samples, uint32_t nsamp, int32_t* step_index, uint32_t trellis,
                                   uint8_t* chunk, uint32_t cap);

extern "C" int amvhip_adpcm_encode_frame(amvhip_ctx* c, const int16_t* samples, uint32_t nsamp, int32_t* step_index,
                                         uint8_t* chunk, uint32_t cap) {
    return adpcm_encode_frame_impl(c, samples, nsamp, step_index, 0u, chunk, cap);
}

extern "C" int amvhip_adpcm_encode_frame_trellis(amvhip_ctx* c, const int16_t* samples, uint32_t nsamp, int32_t* step_index,
                                                 uint32_t trellis, uint8_t* chunk, uint32_t cap) {
    if (trellis < 1 || trellis > 5) return c ? fail(c, AMVHIP_ERR_ARG, "adpcm_encode_frame_trellis: trellis 1..5") : AMVHIP_ERR_ARG;
    return adpcm_encode_frame_impl(c, samples, nsamp, step_index, trellis, chunk, cap);
}

static int adpcm_encode_frame_impl(amvhip_ctx* c, const int16_t* samples, uint32_t nsamp, int32_t* step_index, uint32_t trellis,
                                   uint8_t* chunk, uint32_t cap) {
    if (!c) return AMVHIP_ERR_ARG;
    const uint32_t len = 8u + (nsamp >> 1);
    if (!samples || !step_index || !chunk || (nsamp & 1u) || nsamp == 0 || *step_index < 0 || *step_index > 88)
        return fail(c, AMVHIP_ERR_ARG, "adpcm_encode_frame: bad argument (even, non-zero sample count; index 0..88)");
    if (cap < len) return fail(c, AMVHIP_ERR_SPACE, "adpcm_encode_frame: chunk needs %u bytes", len);
    hipStream_t hs;
    if (int r = host_stream(c, &hs)) return r;
    // staging: [pcm | chunk | scratch pcm] + small tables {pcm_off, chunk_off, nsamp, len, step, final[2]}
    std::lock_guard<std::mutex> hlk(c->hmu);   // the staging buffers: one host-buffer call at a time
    struct { uint64_t pcm_off, chunk_off; uint32_t nsamp, len; int32_t step; int32_t final_state[2]; } tab = {0, 0, nsamp, len, *step_index, {0, 0}};
    if (int r = stage(c, c->h_in, (size_t)nsamp * 2 + 16, samples, (size_t)nsamp * 2, hs)) return r;
    if (int r = ensure(c, c->h_out, (size_t)len + 16 + (size_t)nsamp * 2 + 16)) return r;
    if (int r = stage(c, c->h_aux, 64, &tab, sizeof tab, hs)) return r;
    uint8_t* aux = (uint8_t*)c->h_aux.p;
    uint8_t* d_chunk = (uint8_t*)c->h_out.p;
    int16_t* d_scratch = (int16_t*)(d_chunk + ((len + 15u) & ~15u));
    if (trellis) {
        if (int r = amvhip_adpcm_encode_trellis_batch_dev(c, (const int16_t*)c->h_in.p, (const uint64_t*)aux, (const uint32_t*)(aux + 16), 1,
                                                          (const int32_t*)(aux + 24), trellis, d_chunk, (const uint64_t*)(aux + 8), nullptr, hs))
            return r;
    } else if (int r = amvhip_adpcm_encode_batch_dev(c, (const int16_t*)c->h_in.p, (const uint64_t*)aux, (const uint32_t*)(aux + 16), 1,
                                                     (const int32_t*)(aux + 24), d_chunk, (const uint64_t*)(aux + 8), hs)) {
        return r;
    }
    if (int r = amvhip_adpcm_decode_batch_dev(c, d_chunk, len, (const uint64_t*)(aux + 8), (const uint32_t*)(aux + 20), 1, d_scratch,
                                              (const uint64_t*)aux, (int32_t*)(aux + 28), hs))
        return r;
    int32_t fin[2] = {0, 0};
    HIP_TRY(c, hipMemcpyAsync(chunk, d_chunk, len, hipMemcpyDeviceToHost, hs));
    HIP_TRY(c, hipMemcpyAsync(fin, aux + 28, 8, hipMemcpyDeviceToHost, hs));
    HIP_TRY(c, hipStreamSynchronize(hs));
    *step_index = fin[1];
    return (int)len;
}

// (amvhip_amv_audio_pairs / amvhip_amv_audio_frame_size, the AMV audio framing in host arithmetic, live in
// host/amv_container.c: plain C, no device -- they are part of every link of the host side, the FFmpeg one included)

extern "C" int amvhip_adpcm_wav_encode_frame(amvhip_ctx* c, const int16_t* samples, int frame_size,
                                             int32_t state[2], uint8_t* frame, int buf_size) {
    if (!c) return AMVHIP_ERR_ARG;
    const int groups = frame_size / 8;   // AdpcmIma.c:105
    if (!samples || !state || !frame || frame_size < 1 || buf_size < 4 + 4 * groups)
        return fail(c, AMVHIP_ERR_ARG, "adpcm_wav_encode: bad argument");
    hipStream_t hs;
    if (int r = host_stream(c, &hs)) return r;
    const size_t ns = (size_t)1 + 8 * (size_t)groups;
    std::lock_guard<std::mutex> hlk(c->hmu);   // the staging buffers: one host-buffer call at a time
    if (int r = stage(c, c->h_in, ns * 2, samples, ns * 2, hs)) return r;
    if (int r = ensure(c, c->h_out, 4 + 4 * (size_t)groups)) return r;
    if (int r = stage(c, c->h_status, 8, state, 8, hs)) return r;
    launch_adpcm_wav_encode((const int16_t*)c->h_in.p, groups, (int32_t*)c->h_status.p, (uint8_t*)c->h_out.p, hs);
    if (int r = check_launch(c, "adpcm_wav_encode")) return r;
    HIP_TRY(c, hipMemcpyAsync(frame, c->h_out.p, 4 + 4 * (size_t)groups, hipMemcpyDeviceToHost, hs));
    HIP_TRY(c, hipMemcpyAsync(state, c->h_status.p, 8, hipMemcpyDeviceToHost, hs));
    HIP_TRY(c, hipStreamSynchronize(hs));
    return 4 + 4 * groups;
}
