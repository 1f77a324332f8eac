// amvhip_context.hip -- the context of libamvhip.so: create / destroy, what every entry point begins and ends with
// (device selection, workspace growth, event-based kernel timing), the statistics readers and the synthetic sources.
//
// Nothing in the library computes codec results on the CPU: if the device is missing the calls fail.
#include <stdlib.h>

#include "amvhip_ctx.h"

using namespace amv;

namespace amv {

int fail(amvhip_ctx* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return code;
}

int ensure(amvhip_ctx* c, DevBuf& b, size_t bytes) {
    if (bytes <= b.cap) return AMVHIP_OK;
    if (c->front) {   // a submitted batch may still be using the buffer
        HIP_TRY(c, hipStreamSynchronize(c->front));
        HIP_TRY(c, hipStreamSynchronize(c->back));
    }
    if (b.p) HIP_TRY(c, hipFree(b.p));
    b.p = nullptr;
    b.cap = 0;
    size_t want = bytes + bytes / 8 + 256;
    HIP_TRY(c, hipMalloc(&b.p, want));
    b.cap = want;
    return AMVHIP_OK;
}

int stage(amvhip_ctx* c, DevBuf& b, size_t room, const void* src, size_t bytes, hipStream_t st) {
    if (int r = ensure(c, b, room)) return r;
    HIP_TRY(c, hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, st));
    return AMVHIP_OK;
}

void drain(amvhip_ctx* c) {
    for (ProfRec& r : c->recs) {
        float ms = 0;
        if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
            c->launches[r.kernel]++;
            c->total_ms[r.kernel] += ms;
        }
        c->pool.push_back(r.a);
        c->pool.push_back(r.b);
    }
    c->recs.clear();
}

int check_launch(amvhip_ctx* c, const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(c, AMVHIP_ERR_DEVICE, "%s launch: %s", what, hipGetErrorString(e));
    return AMVHIP_OK;
}

int select_device(amvhip_ctx* c) {
    HIP_TRY(c, hipSetDevice(c->device));
    return AMVHIP_OK;
}

int use_device(amvhip_ctx* c) {
    if (int r = select_device(c)) return r;
    if (c->front && c->submitted != 0) {
        HIP_TRY(c, hipStreamSynchronize(c->front));
        HIP_TRY(c, hipStreamSynchronize(c->back));
    }
    return AMVHIP_OK;
}

int host_stream(amvhip_ctx* c, hipStream_t* out) {
    if (int r = use_device(c)) return r;
    if (!c->hstream) HIP_TRY(c, hipStreamCreateWithFlags(&c->hstream, hipStreamNonBlocking));
    *out = c->hstream;
    return AMVHIP_OK;
}

}  // namespace amv

// the environment's tuning and test knobs
static void read_knobs(amvhip_ctx* c) {
    if (const char* e = getenv("AMVHIP_SYNC_LANES")) {   // tuning knob: lanes per frame of the entropy kernel
        const int v = atoi(e);
        if (v == 1 || v == 2 || v == 4 || v == 8 || v == 16 || v == 32 || v == 64) c->sync_lanes = v;
    }
    if (const char* e = getenv("AMVHIP_SPLIT")) {   // tuning / test knob: 0 = no split, a power of two = lanes per heavy frame
        const int v = atoi(e);
        c->split_heavy = v != 0;
        if (v == 2 || v == 4 || v == 8 || v == 16 || v == 32 || v == 64) c->heavy_lanes = (uint32_t)v;
        if (v == -1) c->heavy_lanes = 1;    // two lists, one lane per frame in both (measurements)
    }
    if (const char* e = getenv("AMVHIP_LAYOUT")) c->layout_large = strcmp(e, "large") == 0;   // test knob: the three-launch layout for small batches too
    if (const char* e = getenv("AMVHIP_ADPCM_SWEEPS")) {   // tuning / test knob: "map" = exhaustive route only, or a sweep count
        if (strcmp(e, "nosettle") == 0) {
            c->adpcm_settle = false;   // sweeps by stream length, then nothing: the chain's check sends the stream down the exhaustive route
        } else {
            c->adpcm_sweeps_set = true;
            c->adpcm_sweeps = strcmp(e, "map") == 0 ? -1 : (atoi(e) < 0 ? 0 : (atoi(e) > (int)kAdpcmSweepsMost ? (int)kAdpcmSweepsMost : atoi(e)));
        }
    }
    if (const char* e = getenv("AMVHIP_ADPCM_TRELLIS_SWEEPS"))   // test knob: "map" = the fall-back at once, or a sweep count (0: none)
        c->trellis_sweeps = strcmp(e, "map") == 0 ? -1 : (atoi(e) < 0 ? 0 : (atoi(e) > (int)kTrellisSweepsMost ? (int)kTrellisSweepsMost : atoi(e)));
}

extern "C" int amvhip_create(amvhip_ctx** out, int device) {
    if (!out) return AMVHIP_ERR_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count)
        return AMVHIP_ERR_DEVICE;
    amvhip_ctx* c = new amvhip_ctx;
    c->device = device;
    static HuffDecodeImage dec;
    static HuffEncodeImage enc;
    static std::once_flag once;
    std::call_once(once, [] { build_images(dec, enc); mark_big_ac(dec); });
    auto die = [&](int code) { amvhip_destroy(c); return code; };
    if (hipSetDevice(device) != hipSuccess) return die(AMVHIP_ERR_DEVICE);
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) c->cus = (uint32_t)cus;
    read_knobs(c);
    if (hipMalloc(&c->d_dec.p, sizeof dec) != hipSuccess) return die(AMVHIP_ERR_NOMEM);
    if (hipMalloc(&c->d_enc.p, sizeof enc) != hipSuccess) return die(AMVHIP_ERR_NOMEM);
    if (hipMemcpy(c->d_dec.p, &dec, sizeof dec, hipMemcpyHostToDevice) != hipSuccess) return die(AMVHIP_ERR_DEVICE);
    if (hipMemcpy(c->d_enc.p, &enc, sizeof enc, hipMemcpyHostToDevice) != hipSuccess) return die(AMVHIP_ERR_DEVICE);
    *out = c;
    return AMVHIP_OK;
}

extern "C" void amvhip_destroy(amvhip_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    drain(c);
    for (hipEvent_t e : c->pool) (void)hipEventDestroy(e);
    if (c->hstream) { (void)hipStreamSynchronize(c->hstream); (void)hipStreamDestroy(c->hstream); }
    if (c->dstream) { (void)hipStreamSynchronize(c->dstream); (void)hipStreamDestroy(c->dstream); }
    for (hipEvent_t e : {c->ev_decoded, c->ev_copied[0], c->ev_copied[1]})
        if (e) (void)hipEventDestroy(e);
    for (hipStream_t q : {c->front, c->back})
        if (q) { (void)hipStreamSynchronize(q); (void)hipStreamDestroy(q); }
    for (hipEvent_t e : {c->ev_in, c->ev_front, c->ev_done[0], c->ev_done[1]})
        if (e) (void)hipEventDestroy(e);
    delete c;   // (every stream is drained: the buffers go with the context)
}

extern "C" const char* amvhip_last_error(const amvhip_ctx* c) { return c ? c->err.c_str() : "null context"; }
extern "C" int amvhip_device(const amvhip_ctx* c) { return c ? c->device : -1; }

extern "C" uint32_t amvhip_stride(uint32_t w) { return (w * 24 + 31) / 32 * 4; }
extern "C" uint64_t amvhip_frame_bytes(uint32_t w, uint32_t h) { return (uint64_t)amvhip_stride(w) * h; }
extern "C" uint64_t amvhip_yuv420_frame_bytes(uint32_t w, uint32_t h) {
    return (uint64_t)w * h + 2ull * ((w + 1) / 2) * ((h + 1) / 2);
}
extern "C" uint32_t amvhip_encode_bound(uint32_t w, uint32_t h) {
    // per coefficient at most a 16-bit code + 11 magnitude bits (< 4 bytes), doubled by FF escaping
    return 4 + ((w + 15) / 16) * ((h + 15) / 16) * 6 * 64 * 4 * 2;
}

extern "C" int amvhip_sync(amvhip_ctx* c) {
    if (!c) return AMVHIP_ERR_ARG;
    if (int r = use_device(c)) return r;
    if (c->hstream) HIP_TRY(c, hipStreamSynchronize(c->hstream));
    if (c->dstream) HIP_TRY(c, hipStreamSynchronize(c->dstream));
    return AMVHIP_OK;
}

// page-locked host memory for the *_async entry points (pageable buffers work too, but their copies block)
extern "C" int amvhip_host_alloc(amvhip_ctx* c, void** p, size_t bytes) {
    if (!c || !p) return AMVHIP_ERR_ARG;
    *p = nullptr;
    if (int r = use_device(c)) return r;
    HIP_TRY(c, hipHostMalloc(p, bytes ? bytes : 1, hipHostMallocDefault));
    return AMVHIP_OK;
}

extern "C" void amvhip_host_free(amvhip_ctx* c, void* p) {
    if (!c || !p) return;
    (void)hipSetDevice(c->device);
    (void)hipHostFree(p);
}

extern "C" int amvhip_synth_frames_dev(amvhip_ctx* c, uint32_t seed, uint32_t first, uint32_t n, uint32_t w,
                                       uint32_t h, uint8_t* d_rgb, void* stream) {
    if (!c) return AMVHIP_ERR_ARG;
    if (!size_ok(w, h) || (n && !d_rgb)) return fail(c, AMVHIP_ERR_ARG, "synth: bad argument");
    if (int r = use_device(c)) return r;
    {
        Timed t(c, AMVHIP_K_SYNTH, (hipStream_t)stream);
        launch_synth_frames(seed, first, n, w, h, d_rgb, (hipStream_t)stream);
    }
    return check_launch(c, "synth_frames");
}

extern "C" int amvhip_synth_audio_dev(amvhip_ctx* c, uint32_t seed, uint64_t first, uint64_t n, int16_t* d_pcm, void* stream) {
    if (!c) return AMVHIP_ERR_ARG;
    if (n && !d_pcm) return fail(c, AMVHIP_ERR_ARG, "synth: bad argument");
    if (int r = use_device(c)) return r;
    launch_synth_audio(seed, first, n, d_pcm, (hipStream_t)stream);
    return check_launch(c, "synth_audio");
}

extern "C" int amvhip_set_entropy_mode(amvhip_ctx* c, int mode) {
    if (!c || (mode != AMVHIP_ENTROPY_AUTO && mode != AMVHIP_ENTROPY_SERIAL)) return AMVHIP_ERR_ARG;
    c->entropy_mode = mode;
    return AMVHIP_OK;
}

extern "C" int amvhip_entropy_stats(amvhip_ctx* c, int enable, uint64_t out[11]) {
    if (!c) return AMVHIP_ERR_ARG;
    if (int r = use_device(c)) return r;
    std::lock_guard<std::mutex> lk(c->mu);
    if (int r = ensure(c, c->stats, amv::kStatsBytes)) return r;
    HIP_TRY(c, hipDeviceSynchronize());
    if (out) {
        if (c->want_stats) HIP_TRY(c, hipMemcpy(out, c->stats.p, 88, hipMemcpyDeviceToHost));
        else memset(out, 0, 88);
        // frames of the LAST decode call that the synchronising kernel handed to the one-lane-per-frame kernel (chunk
        // over the workspace window, long FF run, more records than the record space holds: see blob_bytes in amvhip.h)
        uint32_t handed = 0;
        if (c->last_decode_retry && c->last_decode_retry->p) HIP_TRY(c, hipMemcpy(&handed, c->last_decode_retry->p, 4, hipMemcpyDeviceToHost));
        out[3] = handed;
    }
    // the counters always; the per-task lines too when gathering goes on, so that amvhip_entropy_trace finds zeros behind the
    // tasks of the launches that follow (a fresh allocation holds whatever the pool last kept there)
    HIP_TRY(c, hipMemset(c->stats.p, 0, enable ? amv::kStatsBytes : 128));
    c->want_stats = enable != 0;
    return AMVHIP_OK;
}

extern "C" int amvhip_entropy_trace(amvhip_ctx* c, uint64_t* out, uint32_t tasks) {
    if (!c || (tasks && !out)) return AMVHIP_ERR_ARG;
    if (int r = use_device(c)) return r;
    std::lock_guard<std::mutex> lk(c->mu);
    if (tasks > amv::kTraceTasks) tasks = amv::kTraceTasks;
    if (!c->stats.p || c->stats.cap < amv::kStatsBytes) return fail(c, AMVHIP_ERR_ARG, "entropy_trace: gathering was never switched on");
    HIP_TRY(c, hipDeviceSynchronize());
    HIP_TRY(c, hipMemcpy(out, (const uint64_t*)c->stats.p + amv::kTraceBase, (size_t)tasks * 64, hipMemcpyDeviceToHost));
    return (int)tasks;
}

extern "C" int amvhip_decode_split_stats(amvhip_ctx* c, uint32_t out[2]) {
    if (!c || !out) return AMVHIP_ERR_ARG;
    if (int r = use_device(c)) return r;
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(c, hipDeviceSynchronize());
    out[0] = out[1] = 0;
    if (c->last_split && c->split.p) HIP_TRY(c, hipMemcpy(out, c->split.p, 8, hipMemcpyDeviceToHost));
    return AMVHIP_OK;
}

extern "C" void amvhip_prof_enable(amvhip_ctx* c, int on) { if (c) c->prof = on != 0; }

extern "C" void amvhip_prof_reset(amvhip_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    drain(c);
    for (int k = 0; k < AMVHIP_K_COUNT; ++k) { c->launches[k] = 0; c->total_ms[k] = 0; }
}

extern "C" int amvhip_prof_read(amvhip_ctx* c, int kernel, uint64_t* launches, double* total_ms) {
    if (!c || kernel < 0 || kernel >= AMVHIP_K_COUNT) return AMVHIP_ERR_ARG;
    (void)hipSetDevice(c->device);
    drain(c);
    if (launches) *launches = c->launches[kernel];
    if (total_ms) *total_ms = c->total_ms[kernel];
    return AMVHIP_OK;
}

// The JPEG file header amvlib puts in front of a chunk's scan (AmvJpegPutHeader, AmvJpeg.c:315-414):
// SOI, JFIF APP0 (:282-313), two DQT segments with the fixed tables (:162-213), SOF0 4:2:0, the four
// K.3 Huffman tables (:245-279), SOS.  Host-only; the tables come from amv_tables.h.
extern "C" uint32_t amvhip_jpeg_header(uint16_t height, uint16_t width, uint8_t* out, uint32_t cap) {
    std::vector<uint8_t> b;
    auto put = [&](std::initializer_list<int> v) { for (int x : v) b.push_back((uint8_t)x); };
    put({0xff, 0xd8});                                                              // SOI
    put({0xff, 0xe0, 0x00, 0x10, 'J', 'F', 'I', 'F', 0x00, 0x01, 0x01, 0x01, 0x00, 0x60, 0x00, 0x60, 0x00, 0x00});
    for (int t = 0; t < 2; ++t) {                                                   // DQT, 8-bit, table t
        put({0xff, 0xdb, 0x00, 2 + 1 + 64, t});
        for (int i = 0; i < 64; ++i) b.push_back(t ? kQuantChroma[i] : kQuantLuma[i]);
    }
    put({0xff, 0xc0, 0, 17, 8, height >> 8, height & 0xff, width >> 8, width & 0xff, 3,
         1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1});                                      // SOF0
    const int order[4] = {0, 2, 1, 3};                                              // DC luma, AC luma, DC chroma, AC chroma (:247-278)
    for (int j = 0; j < 4; ++j) {
        const int t = order[j];
        int nsym = 0;
        for (int l = 0; l < 16; ++l) nsym += kHuffCount[t][l];
        const int len = 2 + 1 + 16 + nsym;                                          // 0x1F / 0xB5
        put({0xff, 0xc4, len >> 8, len & 0xff, ((t >= 2 ? 1 : 0) << 4) | (t & 1)});
        for (int l = 0; l < 16; ++l) b.push_back(kHuffCount[t][l]);
        const uint8_t* syms = symbols_of(t);
        for (int i = 0; i < nsym; ++i) b.push_back(syms[i]);
    }
    put({0xff, 0xda, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});               // SOS
    if (out && cap >= b.size()) memcpy(out, b.data(), b.size());
    return (uint32_t)b.size();
}

extern "C" const char* amvhip_kernel_name(int kernel) {
    switch (kernel) {
        case AMVHIP_K_HUFFMAN: return "amv_huffman_fast_kernel|sync2|sync";   // whichever the batch got (huffman_sync_lanes); a key of bench lines and profiles, kept as it was
        case AMVHIP_K_UNSTUFF: return "amv_unstuff_kernel";
        case AMVHIP_K_HUFFMAN_SERIAL: return "amv_huffman_kernel";
        case AMVHIP_K_RECON: return "amv_reconstruct_kernel";
        case AMVHIP_K_FDCT: return "amv_forward_kernel";
        case AMVHIP_K_PACK: return "amv_encode_frame_kernel";
        case AMVHIP_K_PACK_SERIAL: return "amv_pack_kernel";
        case AMVHIP_K_COMPACT: return "amv_scan_kernel+amv_gather_kernel";
        case AMVHIP_K_ADPCM_DEC: return "amv_adpcm_decode_kernel";
        case AMVHIP_K_ADPCM_ENC: return "amv_adpcm_guess_kernel+amv_adpcm_sweep_kernel*+front+settle+check (+map, chain, encode_mapped when the chain does not settle)";
        case AMVHIP_K_SYNTH: return "amv_synth_frames_kernel";
        case AMVHIP_K_AUDIO_RESAMPLE: return "amv_audio_tiles_kernel+amv_audio_resample_kernel";
        case AMVHIP_K_PIXFMT: return "amv_pix_*_kernel";
        default: return "";
    }
}
