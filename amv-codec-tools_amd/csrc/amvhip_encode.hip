// amvhip_encode.hip -- video encode behind the C ABI: pixels or planes to chunks, the picture rescaler in front of it.
#include "amvhip_ctx.h"

using namespace amv;

// The parts of a request (QuantRequest, amvhip_ctx.h): its -nr half -- nr and where the state's pointer is -- and its lambda
struct NrPart {
    uint32_t nr;
    int32_t** state;
};
static bool nr_part_of(QuantRequest& req, NrPart* p) {
    if (NrRequest* q = std::get_if<NrRequest>(&req)) { *p = NrPart{q->nr, &q->state}; return true; }
    if (NrTrellisRequest* q = std::get_if<NrTrellisRequest>(&req)) { *p = NrPart{q->nr, &q->state}; return true; }
    return false;
}
static bool lambda_of(const QuantRequest& req, uint32_t* lambda) {
    if (const TrellisArg* t = std::get_if<TrellisArg>(&req)) { *lambda = t->lambda; return true; }
    if (const NrTrellisRequest* q = std::get_if<NrTrellisRequest>(&req)) { *lambda = q->lambda; return true; }
    return false;
}

extern "C" uint32_t amvhip_encode_nr_max(uint32_t w, uint32_t h) {
    if (!encode_size_ok(w, h, 0u)) return 0u;
    return nr_max(make_geom(w, h).blocks);
}
extern "C" uint32_t amvhip_encode_trellis_lambda_max(void) { return trellis_lambda_max(); }
extern "C" uint32_t amvhip_encode_trellis_lambda(uint32_t qscale) { return trellis_lambda_of_qscale(qscale); }

// what a request asks beyond the plain entries' checks; 0 = go on
static int trellis_args_ok(amvhip_ctx* c, uint32_t lambda) {
    if (lambda > trellis_lambda_max())
        return fail(c, AMVHIP_ERR_ARG, "encode_trellis: lambda %u is more than amvhip_encode_trellis_lambda_max() = %u", lambda, trellis_lambda_max());
    return AMVHIP_OK;
}
int amv::quant_args_ok(amvhip_ctx* c, uint32_t n, uint32_t w, uint32_t h, const QuantRequest& req) {
    uint32_t lambda;
    if (lambda_of(req, &lambda))
        if (int r = trellis_args_ok(c, lambda)) return r;
    QuantRequest copy = req;
    NrPart q;
    if (!nr_part_of(copy, &q)) return AMVHIP_OK;
    if (q.nr > amvhip_encode_nr_max(w, h))
        return fail(c, AMVHIP_ERR_ARG, "encode_nr: nr %u is more than amvhip_encode_nr_max(%u, %u) = %u", q.nr, w, h, amvhip_encode_nr_max(w, h));
    if (n && q.nr && (!*q.state || ((uintptr_t)*q.state & 3u))) return fail(c, AMVHIP_ERR_ARG, "encode_nr: the state is null or not 4-byte aligned");
    return AMVHIP_OK;
}

int amv::quant_request_of(amvhip_ctx* c, const amvhip_quant* q, QuantRequest* req) {
    if (!q) return fail(c, AMVHIP_ERR_ARG, "encode_quant: the quantiser request is null");
    if (q->trellis > 1u) return fail(c, AMVHIP_ERR_ARG, "encode_quant: trellis is 0 or 1");
    *req = PlainQuant{};
    if (q->trellis) *req = NrTrellisRequest{q->nr, q->d_state, q->lambda};
    else if (q->nr) *req = NrRequest{q->nr, q->d_state};
    return AMVHIP_OK;
}
extern "C" uint32_t amvhip_encode_qns_lambda2_max(void) { return qns_lambda2_max(); }
extern "C" uint32_t amvhip_encode_qns_lambda2(uint32_t qscale) { return qns_lambda2_of_qscale(qscale); }
int amv::qns_args_ok(amvhip_ctx* c, const QnsArg& qns) {
    if (qns.qns > kQnsMost) return fail(c, AMVHIP_ERR_ARG, "encode_qns: qns is 0 .. %u", kQnsMost);
    if (qns.lambda2 > qns_lambda2_max())
        return fail(c, AMVHIP_ERR_ARG, "encode_qns: lambda2 %u is more than amvhip_encode_qns_lambda2_max() = %u", qns.lambda2, qns_lambda2_max());
    return AMVHIP_OK;
}
// the basis as amv_qns_refine_kernel reads it, on the device (the context is locked): made and uploaded on the first call
static int qns_basis_on_device(amvhip_ctx* c) {
    if (c->qns_basis.p) return AMVHIP_OK;
    static const std::vector<int16_t> table = [] {
        QnsBasis basis;
        qns_build_basis(basis);
        constexpr QnsScan scan = make_qns_scan();
        std::vector<int16_t> t(64 * 64);
        for (int k = 0; k < 64; ++k)
            for (int i = 0; i < 64; ++i) t[k * 64 + i] = basis.b[scan.natural[i]][k];
        return t;
    }();
    DevBuf fresh;
    if (int r = ensure(c, fresh, table.size() * 2)) return r;
    HIP_TRY(c, hipMemcpy(fresh.p, table.data(), table.size() * 2, hipMemcpyHostToDevice));   // (done before any stream reads it)
    std::swap(c->qns_basis.p, fresh.p);
    std::swap(c->qns_basis.cap, fresh.cap);
    return AMVHIP_OK;
}
int amv::error_sink_ok(amvhip_ctx* c, uint32_t n, const ErrorSink& err) {
    if (err.wanted && n && (!err.sse || ((uintptr_t)err.sse & 7u))) return fail(c, AMVHIP_ERR_ARG, "encode_psnr: d_sse is null or not 8-byte aligned");
    return AMVHIP_OK;
}

// amvhip_encode_coefs_dev and its trellis form: amv_forward_kernel's lines for the caller (no workspace, so no lock)
static int encode_coefs(amvhip_ctx* c, const uint8_t* d_pix, uint32_t pix_stride, int is_bgr, uint32_t n, uint32_t w, uint32_t h, uint32_t qbias,
                        const Quantiser& quant, int16_t* d_coef, void* stream, const char* what) {
    if (!c) return AMVHIP_ERR_ARG;
    if (!encode_size_ok(w, h, qbias) || pix_stride < w * 3 || (n && (!d_pix || !d_coef)))
        return fail(c, AMVHIP_ERR_ARG, "encode: bad argument (width/height must be even)");
    if ((uintptr_t)d_coef & 15u) return fail(c, AMVHIP_ERR_ARG, "encode: coef must be 16-byte aligned");
    if (const TrellisArg* t = std::get_if<TrellisArg>(&quant))
        if (int r = trellis_args_ok(c, t->lambda)) return r;
    if (int r = use_device(c)) return r;
    {
        Timed t(c, AMVHIP_K_FDCT, (hipStream_t)stream);
        launch_forward(rgb_source(d_pix, pix_stride, is_bgr), n, kAllFrames, n, make_geom(w, h), qbias, quant, d_coef, (hipStream_t)stream);
    }
    return check_launch(c, what);
}

extern "C" int amvhip_encode_coefs_dev(amvhip_ctx* c, const uint8_t* d_pix, uint32_t pix_stride, int is_bgr, uint32_t n, uint32_t w, uint32_t h,
                                       uint32_t qbias, int16_t* d_coef, void* stream) {
    return encode_coefs(c, d_pix, pix_stride, is_bgr, n, w, h, qbias, PlainQuant{}, d_coef, stream, "forward");
}

extern "C" int amvhip_encode_trellis_coefs_dev(amvhip_ctx* c, const uint8_t* d_pix, uint32_t pix_stride, int is_bgr, uint32_t n, uint32_t w,
                                               uint32_t h, uint32_t qbias, uint32_t lambda, int16_t* d_coef, void* stream) {
    return encode_coefs(c, d_pix, pix_stride, is_bgr, n, w, h, qbias, TrellisArg{lambda}, d_coef, stream, "forward (trellis)");
}

// Pixels -> chunks for n frames (the context is locked).  The one-kernel encoder takes the batch; what it hands back -- and
// the whole batch in AMVHIP_ENTROPY_SERIAL mode -- goes through amv_forward_kernel + amv_pack_kernel a round of dense lines
// at a time (with a list the count is on the device: the rounds past it find nothing to do and leave at once -- usually all
// of them).  Both routes run the instantiation of `quant`.
// d_sse (the _psnr entries; else nullptr): the frames' error, amv_encode_error.hip, off the dense lines of `quant`'s
// instantiation of amv_forward_kernel -- in AMVHIP_ENTROPY_SERIAL mode the lines the call packs, between the two launches;
// otherwise the one-kernel encoder keeps its levels on the chip, so the front half runs a second time for all frames, a
// round of the workspace at a time, as default launches over the round's part of the source.
static Source frames_from(const Source& in, uint32_t base, const FrameGeom& g) {
    Source s = in;
    if (s.planar) {
        s.yuv.y += (uint64_t)base * s.yuv.y_frame;
        s.yuv.cb += (uint64_t)base * s.yuv.c_frame;
        s.yuv.cr += (uint64_t)base * s.yuv.c_frame;
    } else {
        s.pix += (uint64_t)base * s.pix_stride * g.height;
    }
    return s;
}
static Quantiser frames_from(const Quantiser& quant, uint32_t base) {   // (the offsets are 64 per frame)
    if (const uint16_t* const* o = std::get_if<const uint16_t*>(&quant)) return Quantiser{*o + (uint64_t)base * 64u};
    if (const NrTrellisArg* t = std::get_if<NrTrellisArg>(&quant)) return Quantiser{NrTrellisArg{t->offsets + (uint64_t)base * 64u, t->lambda}};
    if (const TrellisFrames* t = std::get_if<TrellisFrames>(&quant)) return Quantiser{TrellisFrames{t->lambda + base}};   // (a lambda per frame)
    if (const NrTrellisFrames* t = std::get_if<NrTrellisFrames>(&quant))
        return Quantiser{NrTrellisFrames{t->offsets + (uint64_t)base * 64u, t->lambda + base}};
    return quant;
}
// qns (qns.qns > 0): every frame takes the two-stage route in both entropy modes, with the refinement (amv_encode_qns.hip)
// between amv_forward_kernel and what reads its lines -- the error kernel, where errors are wanted, and amv_pack_kernel.
static int encode_core(amvhip_ctx* c, const Source& in, uint32_t n, const FrameGeom& g, uint32_t qbias, const Quantiser& quant, const QnsArg& qns,
                       uint8_t* d_blob, uint64_t blob_cap, uint64_t* d_offs, uint32_t* d_lens, uint64_t* d_sse, hipStream_t stream) {
    const uint32_t bound = amvhip_encode_bound(g.width, g.height);
    const HuffEncodeImage* book = (const HuffEncodeImage*)c->d_enc.p;
    const uint32_t round = fallback_round(n, g, 1024u, 2u);
    if (int r = ensure(c, c->coef, (size_t)round * g.blocks * 128)) return r;
    if (int r = ensure(c, c->tmp, (size_t)n * bound)) return r;
    if (int r = ensure(c, c->flag, 16)) return r;
    if (qns.qns)
        if (int r = qns_basis_on_device(c)) return r;
    if (int r = ensure(c, c->enc_retry, ((size_t)n + 4) * 8)) return r;   // (the encoder's own: the decode path's counter is read by amvhip_entropy_stats)
    uint32_t* retry_count = (uint32_t*)c->enc_retry.p;
    uint32_t* retry_list = retry_count + 8;
    HIP_TRY(c, hipMemsetAsync(retry_count, 0, 32, stream));
    if (d_sse) HIP_TRY(c, hipMemsetAsync(d_sse, 0, (size_t)n * 24u, stream));
    const bool fused = c->entropy_mode != AMVHIP_ENTROPY_SERIAL && !qns.qns;
    if (fused) {
        Timed t(c, AMVHIP_K_PACK, stream);
        launch_encode_frames(in, n, g, qbias, quant, book, (uint8_t*)c->tmp.p, bound, d_lens, retry_list, retry_count, stream);
    }
    if (int r = check_launch(c, "encode_frames")) return r;
    for (uint32_t base = 0; base < n; base += round) {
        const uint32_t items = n - base < round ? n - base : round;
        const FrameSel sel{fused ? retry_list : nullptr, fused ? retry_count : nullptr, base, items};
        {
            Timed t(c, AMVHIP_K_FDCT, stream);
            launch_forward(in, n, sel, items, g, qbias, quant, (int16_t*)c->coef.p, stream);
            if (qns.qns)
                launch_qns_refine(in, n, sel, items, g, (int16_t*)c->coef.p, (const int16_t*)c->qns_basis.p, qns.qns, qns.lambda2, stream);
            if (d_sse && !fused) launch_encode_error(in, n, sel, items, g, (const int16_t*)c->coef.p, d_sse, stream);
        }
        {
            Timed t(c, AMVHIP_K_PACK_SERIAL, stream);
            launch_pack((const int16_t*)c->coef.p, n, sel, items, g, book, (uint8_t*)c->tmp.p, bound, d_lens, stream);
        }
        if (int r = check_launch(c, "forward + pack")) return r;
    }
    for (uint32_t base = 0; d_sse && fused && base < n; base += round) {
        const uint32_t items = n - base < round ? n - base : round;
        {
            Timed t(c, AMVHIP_K_FDCT, stream);
            const Source part = frames_from(in, base, g);
            launch_forward(part, items, kAllFrames, items, g, qbias, frames_from(quant, base), (int16_t*)c->coef.p, stream);
            launch_encode_error(part, items, kAllFrames, items, g, (const int16_t*)c->coef.p, d_sse + (uint64_t)base * 3u, stream);
        }
        if (int r = check_launch(c, "forward + error")) return r;
    }
    {
        Timed t(c, AMVHIP_K_COMPACT, stream);
        launch_compact((const uint8_t*)c->tmp.p, bound, d_lens, n, d_offs, d_blob, blob_cap, (int32_t*)c->flag.p, stream);
    }
    return check_launch(c, "compact");
}

// Passes A and B in front of encode_core (the context is locked; nr > 0): the frames' sums, the chain from d_state to
// d_state, and the encoder with the offsets the chain wrote -- rounding behind them, or, with a lambda, searching.  The sums
// are taken before the offsets are applied, so the state does not depend on which.
static int nr_quantiser(amvhip_ctx* c, const Source& in, uint32_t n, const FrameGeom& g, uint32_t nr, int32_t* d_state, const uint32_t* lambda,
                        Quantiser* quant, hipStream_t stream) {
    const NrPlan plan = nr_plan(n);
    if (int r = ensure(c, c->nr_ws, plan.bytes)) return r;
    uint32_t* sums = (uint32_t*)((uint8_t*)c->nr_ws.p + plan.sums);
    uint16_t* offsets = (uint16_t*)((uint8_t*)c->nr_ws.p + plan.offsets);
    launch_nr_sums(in, n, g, sums, stream);
    launch_nr_chain(sums, n, g.blocks, nr, d_state, offsets, stream);
    if (int r = check_launch(c, "nr sums + chain")) return r;
    *quant = lambda ? Quantiser{NrTrellisArg{offsets, *lambda}} : Quantiser{offsets};
    return AMVHIP_OK;
}
// the request's quantiser as the kernels take it (the context is locked; for nr > 0 passes A and B run, and the state moves on)
static int request_quantiser(amvhip_ctx* c, const Source& in, uint32_t n, const FrameGeom& g, QuantRequest req, Quantiser* quant,
                             hipStream_t stream) {
    uint32_t lambda;
    const bool trellis = lambda_of(req, &lambda);
    NrPart q;
    if (nr_part_of(req, &q) && q.nr) return nr_quantiser(c, in, n, g, q.nr, *q.state, trellis ? &lambda : nullptr, quant, stream);
    *quant = trellis ? Quantiser{TrellisArg{lambda}} : Quantiser{PlainQuant{}};
    return AMVHIP_OK;
}

// the request's core (the context is locked, the request checked, n > 0; req's state is on the device)
static int encode_request(amvhip_ctx* c, const Source& in, uint32_t n, const FrameGeom& g, uint32_t qbias, QuantRequest req, const QnsArg& qns,
                          uint8_t* d_blob, uint64_t blob_cap, uint64_t* d_offs, uint32_t* d_lens, uint64_t* d_sse, hipStream_t stream) {
    Quantiser quant;
    if (int r = request_quantiser(c, in, n, g, req, &quant, stream)) return r;
    return encode_core(c, in, n, g, qbias, quant, qns, d_blob, blob_cap, d_offs, d_lens, d_sse, stream);
}

// what every device-pointer encoder asks of the size, of the live half of `in` and of its outputs (no_out: one of them is null)
static int source_args_ok(amvhip_ctx* c, const Source& in, uint32_t n, uint32_t w, uint32_t h, uint32_t qbias, bool no_out) {
    if (in.planar) {
        if (!encode_size_ok(w, h, qbias) || in.yuv.y_stride < w || in.yuv.c_stride < w / 2 || (n && (!in.yuv.y || !in.yuv.cb || !in.yuv.cr)) || no_out)
            return fail(c, AMVHIP_ERR_ARG, "encode_yuv: bad argument (width/height must be even)");
    } else {
        if (!encode_size_ok(w, h, qbias) || in.pix_stride < w * 3 || (n && !in.pix))
            return fail(c, AMVHIP_ERR_ARG, "encode: bad argument (width/height must be even)");
        if (no_out) return fail(c, AMVHIP_ERR_ARG, "encode: null output");
    }
    return AMVHIP_OK;
}

// Every device-pointer encoder whole: the checks of the live half of `in`, of the outputs and of the request, n == 0, the
// device, the lock (held from the workspace's allocation to the last launch), the request's core.  req's state is on the device.
// err: where a _psnr entry wants the frames' error (kNoError: not asked for).
static int encode_dev(amvhip_ctx* c, const Source& in, uint32_t n, uint32_t w, uint32_t h, uint32_t qbias, const QuantRequest& req,
                      uint8_t* d_blob, uint64_t blob_cap, uint64_t* d_offs, uint32_t* d_lens, void* stream, const ErrorSink& err = kNoError,
                      const QnsArg& qns = kNoQns) {
    if (!c) return AMVHIP_ERR_ARG;
    if (int r = source_args_ok(c, in, n, w, h, qbias, n && (!d_blob || !d_offs || !d_lens))) return r;
    if (int r = quant_args_ok(c, n, w, h, req)) return r;
    if (int r = error_sink_ok(c, n, err)) return r;
    if (int r = qns_args_ok(c, qns)) return r;
    if (n == 0) return AMVHIP_OK;
    if (int r = use_device(c)) return r;
    std::lock_guard<std::mutex> lk(c->mu);
    return encode_request(c, in, n, make_geom(w, h), qbias, req, qns, d_blob, blob_cap, d_offs, d_lens, err.wanted ? err.sse : nullptr,
                          (hipStream_t)stream);
}

extern "C" int amvhip_encode_batch_dev(amvhip_ctx* c, const uint8_t* d_pix, uint32_t pix_stride, int is_bgr, uint32_t n, uint32_t w, uint32_t h,
                                       uint32_t qbias, uint8_t* d_blob, uint64_t blob_cap, uint64_t* d_offs, uint32_t* d_lens, void* stream) {
    return encode_dev(c, rgb_source(d_pix, pix_stride, is_bgr), n, w, h, qbias, PlainQuant{}, d_blob, blob_cap, d_offs, d_lens, stream);
}

extern "C" int amvhip_encode_nr_stream_dev(amvhip_ctx* c, const uint8_t* d_pix, uint32_t pix_stride, int is_bgr, uint32_t n, uint32_t w, uint32_t h,
                                           uint32_t qbias, uint32_t nr, int32_t* d_state, uint8_t* d_blob, uint64_t blob_cap, uint64_t* d_offs,
                                           uint32_t* d_lens, void* stream) {
    return encode_dev(c, rgb_source(d_pix, pix_stride, is_bgr), n, w, h, qbias, NrRequest{nr, d_state}, d_blob, blob_cap, d_offs, d_lens, stream);
}

extern "C" int amvhip_encode_trellis_batch_dev(amvhip_ctx* c, const uint8_t* d_pix, uint32_t pix_stride, int is_bgr, uint32_t n, uint32_t w,
                                               uint32_t h, uint32_t qbias, uint32_t lambda, uint8_t* d_blob, uint64_t blob_cap, uint64_t* d_offs,
                                               uint32_t* d_lens, void* stream) {
    return encode_dev(c, rgb_source(d_pix, pix_stride, is_bgr), n, w, h, qbias, TrellisArg{lambda}, d_blob, blob_cap, d_offs, d_lens, stream);
}

extern "C" int amvhip_encode_yuv420_batch_dev(amvhip_ctx* c, const uint8_t* d_y, const uint8_t* d_cb, const uint8_t* d_cr, uint32_t y_stride,
                                              uint32_t c_stride, uint64_t y_frame_stride, uint64_t c_frame_stride, uint32_t n, uint32_t w,
                                              uint32_t h, uint32_t qbias, uint8_t* d_blob, uint64_t blob_cap, uint64_t* d_offs, uint32_t* d_lens,
                                              void* stream) {
    return encode_dev(c, yuv_source({d_y, d_cb, d_cr, y_stride, c_stride, y_frame_stride, c_frame_stride, 0u}), n, w, h, qbias, PlainQuant{}, d_blob,
                      blob_cap, d_offs, d_lens, stream);
}

extern "C" int amvhip_encode_yuv422_batch_dev(amvhip_ctx* c, const uint8_t* d_y, const uint8_t* d_cb, const uint8_t* d_cr, uint32_t y_stride,
                                              uint32_t c_stride, uint64_t y_frame_stride, uint64_t c_frame_stride, uint32_t n, uint32_t w,
                                              uint32_t h, uint32_t qbias, uint8_t* d_blob, uint64_t blob_cap, uint64_t* d_offs, uint32_t* d_lens,
                                              void* stream) {
    return encode_dev(c, yuv_source({d_y, d_cb, d_cr, y_stride, c_stride, y_frame_stride, c_frame_stride, 1u}), n, w, h, qbias, PlainQuant{}, d_blob,
                      blob_cap, d_offs, d_lens, stream);
}

extern "C" int amvhip_encode_yuv420_nr_stream_dev(amvhip_ctx* c, const uint8_t* d_y, const uint8_t* d_cb, const uint8_t* d_cr, uint32_t y_stride,
                                                  uint32_t c_stride, uint64_t y_frame_stride, uint64_t c_frame_stride, uint32_t n, uint32_t w,
                                                  uint32_t h, uint32_t qbias, uint32_t nr, int32_t* d_state, uint8_t* d_blob, uint64_t blob_cap,
                                                  uint64_t* d_offs, uint32_t* d_lens, void* stream) {
    return encode_dev(c, yuv_source({d_y, d_cb, d_cr, y_stride, c_stride, y_frame_stride, c_frame_stride, 0u}), n, w, h, qbias, NrRequest{nr, d_state},
                      d_blob, blob_cap, d_offs, d_lens, stream);
}

extern "C" int amvhip_encode_yuv420_trellis_batch_dev(amvhip_ctx* c, const uint8_t* d_y, const uint8_t* d_cb, const uint8_t* d_cr,
                                                      uint32_t y_stride, uint32_t c_stride, uint64_t y_frame_stride, uint64_t c_frame_stride,
                                                      uint32_t n, uint32_t w, uint32_t h, uint32_t qbias, uint32_t lambda, uint8_t* d_blob,
                                                      uint64_t blob_cap, uint64_t* d_offs, uint32_t* d_lens, void* stream) {
    return encode_dev(c, yuv_source({d_y, d_cb, d_cr, y_stride, c_stride, y_frame_stride, c_frame_stride, 0u}), n, w, h, qbias, TrellisArg{lambda},
                      d_blob, blob_cap, d_offs, d_lens, stream);
}

extern "C" int amvhip_encode_nr_trellis_stream_dev(amvhip_ctx* c, const uint8_t* d_pix, uint32_t pix_stride, int is_bgr, uint32_t n, uint32_t w,
                                                   uint32_t h, uint32_t qbias, uint32_t nr, uint32_t lambda, int32_t* d_state, uint8_t* d_blob,
                                                   uint64_t blob_cap, uint64_t* d_offs, uint32_t* d_lens, void* stream) {
    return encode_dev(c, rgb_source(d_pix, pix_stride, is_bgr), n, w, h, qbias, NrTrellisRequest{nr, d_state, lambda}, d_blob, blob_cap, d_offs,
                      d_lens, stream);
}

extern "C" int amvhip_encode_yuv420_nr_trellis_stream_dev(amvhip_ctx* c, const uint8_t* d_y, const uint8_t* d_cb, const uint8_t* d_cr,
                                                          uint32_t y_stride, uint32_t c_stride, uint64_t y_frame_stride, uint64_t c_frame_stride,
                                                          uint32_t n, uint32_t w, uint32_t h, uint32_t qbias, uint32_t nr, uint32_t lambda,
                                                          int32_t* d_state, uint8_t* d_blob, uint64_t blob_cap, uint64_t* d_offs, uint32_t* d_lens,
                                                          void* stream) {
    return encode_dev(c, yuv_source({d_y, d_cb, d_cr, y_stride, c_stride, y_frame_stride, c_frame_stride, 0u}), n, w, h, qbias,
                      NrTrellisRequest{nr, d_state, lambda}, d_blob, blob_cap, d_offs, d_lens, stream);
}

// ---- the _psnr entries: a request (amvhip_quant) in the place of qbias, and the frames' error beside the chunks ---------
extern "C" int amvhip_encode_quant_psnr_stream_dev(amvhip_ctx* c, const uint8_t* d_pix, uint32_t pix_stride, int is_bgr, uint32_t n, uint32_t w,
                                                   uint32_t h, const amvhip_quant* q, uint8_t* d_blob, uint64_t blob_cap, uint64_t* d_offs,
                                                   uint32_t* d_lens, uint64_t* d_sse, void* stream) {
    if (!c) return AMVHIP_ERR_ARG;
    QuantRequest req;
    if (int r = quant_request_of(c, q, &req)) return r;
    return encode_dev(c, rgb_source(d_pix, pix_stride, is_bgr), n, w, h, q->qbias, req, d_blob, blob_cap, d_offs, d_lens, stream,
                      ErrorSink{d_sse, true});
}

extern "C" int amvhip_encode_yuv420_quant_psnr_stream_dev(amvhip_ctx* c, const uint8_t* d_y, const uint8_t* d_cb, const uint8_t* d_cr,
                                                          uint32_t y_stride, uint32_t c_stride, uint64_t y_frame_stride, uint64_t c_frame_stride,
                                                          uint32_t n, uint32_t w, uint32_t h, const amvhip_quant* q, uint8_t* d_blob,
                                                          uint64_t blob_cap, uint64_t* d_offs, uint32_t* d_lens, uint64_t* d_sse, void* stream) {
    if (!c) return AMVHIP_ERR_ARG;
    QuantRequest req;
    if (int r = quant_request_of(c, q, &req)) return r;
    return encode_dev(c, yuv_source({d_y, d_cb, d_cr, y_stride, c_stride, y_frame_stride, c_frame_stride, 0u}), n, w, h, q->qbias, req, d_blob,
                      blob_cap, d_offs, d_lens, stream, ErrorSink{d_sse, true});
}

// ---- the _qns entries: the request, then qns and lambda2 (amv_qns_plan.h); d_sse NULL = errors not wanted -----------------
extern "C" int amvhip_encode_qns_stream_dev(amvhip_ctx* c, const uint8_t* d_pix, uint32_t pix_stride, int is_bgr, uint32_t n, uint32_t w, uint32_t h,
                                            const amvhip_quant* q, uint32_t qns, uint32_t lambda2, uint8_t* d_blob, uint64_t blob_cap,
                                            uint64_t* d_offs, uint32_t* d_lens, uint64_t* d_sse, void* stream) {
    if (!c) return AMVHIP_ERR_ARG;
    QuantRequest req;
    if (int r = quant_request_of(c, q, &req)) return r;
    return encode_dev(c, rgb_source(d_pix, pix_stride, is_bgr), n, w, h, q->qbias, req, d_blob, blob_cap, d_offs, d_lens, stream,
                      ErrorSink{d_sse, d_sse != nullptr}, QnsArg{qns, lambda2});
}

extern "C" int amvhip_encode_yuv420_qns_stream_dev(amvhip_ctx* c, const uint8_t* d_y, const uint8_t* d_cb, const uint8_t* d_cr, uint32_t y_stride,
                                                   uint32_t c_stride, uint64_t y_frame_stride, uint64_t c_frame_stride, uint32_t n, uint32_t w,
                                                   uint32_t h, const amvhip_quant* q, uint32_t qns, uint32_t lambda2, uint8_t* d_blob,
                                                   uint64_t blob_cap, uint64_t* d_offs, uint32_t* d_lens, uint64_t* d_sse, void* stream) {
    if (!c) return AMVHIP_ERR_ARG;
    QuantRequest req;
    if (int r = quant_request_of(c, q, &req)) return r;
    return encode_dev(c, yuv_source({d_y, d_cb, d_cr, y_stride, c_stride, y_frame_stride, c_frame_stride, 0u}), n, w, h, q->qbias, req, d_blob,
                      blob_cap, d_offs, d_lens, stream, ErrorSink{d_sse, d_sse != nullptr}, QnsArg{qns, lambda2});
}

// the levels themselves, beside amvhip_encode_trellis_coefs_dev: the request's quantiser, then the refinement, into d_coef
extern "C" int amvhip_encode_qns_coefs_dev(amvhip_ctx* c, const uint8_t* d_pix, uint32_t pix_stride, int is_bgr, uint32_t n, uint32_t w, uint32_t h,
                                           const amvhip_quant* q, uint32_t qns, uint32_t lambda2, int16_t* d_coef, void* stream) {
    if (!c) return AMVHIP_ERR_ARG;
    QuantRequest req;
    if (int r = quant_request_of(c, q, &req)) return r;
    if (!encode_size_ok(w, h, q->qbias) || pix_stride < w * 3 || (n && (!d_pix || !d_coef)))
        return fail(c, AMVHIP_ERR_ARG, "encode_qns: bad argument (width/height must be even)");
    if ((uintptr_t)d_coef & 15u) return fail(c, AMVHIP_ERR_ARG, "encode_qns: coef must be 16-byte aligned");
    if (int r = quant_args_ok(c, n, w, h, req)) return r;
    if (int r = qns_args_ok(c, QnsArg{qns, lambda2})) return r;
    if (n == 0) return AMVHIP_OK;
    if (int r = use_device(c)) return r;
    std::lock_guard<std::mutex> lk(c->mu);       // (the -nr workspace and the basis are the context's)
    const Source in = rgb_source(d_pix, pix_stride, is_bgr);
    const FrameGeom g = make_geom(w, h);
    Quantiser quant;
    if (int r = request_quantiser(c, in, n, g, req, &quant, (hipStream_t)stream)) return r;
    if (qns)
        if (int r = qns_basis_on_device(c)) return r;
    {
        Timed t(c, AMVHIP_K_FDCT, (hipStream_t)stream);
        launch_forward(in, n, kAllFrames, n, g, q->qbias, quant, d_coef, (hipStream_t)stream);
        if (qns) launch_qns_refine(in, n, kAllFrames, n, g, d_coef, (const int16_t*)c->qns_basis.p, qns, lambda2, (hipStream_t)stream);
    }
    return check_launch(c, "forward + qns");
}

// ---- the rate entries: a byte budget per frame, met by a search over lambda (amv_rate_plan.h, amv_encode_rate.hip) --------
int amv::rate_request_of(amvhip_ctx* c, const amvhip_quant* q, const amvhip_rate* rate, QuantRequest* req, RateArg* arg) {
    if (int r = quant_request_of(c, q, req)) return r;
    if (q->trellis != 1u) return fail(c, AMVHIP_ERR_ARG, "encode_rate: the search is over the trellis quantiser's lambda: trellis must be 1");
    *req = NrTrellisRequest{q->nr, q->d_state, 0u};            // (q->lambda is not read)
    if (!rate || !rate->ladder) return fail(c, AMVHIP_ERR_ARG, "encode_rate: the rate request or its ladder is null");
    if (rate->rungs == 0u || rate->rungs > kRateRungsMax) return fail(c, AMVHIP_ERR_ARG, "encode_rate: a ladder has 1 .. %u rungs", kRateRungsMax);
    if ((uintptr_t)rate->d_budget & 3u) return fail(c, AMVHIP_ERR_ARG, "encode_rate: d_budget is not 4-byte aligned");
    *arg = RateArg{RateLadder{}, rate->budget, rate->d_budget};
    arg->ladder.rungs = rate->rungs;
    for (uint32_t r = 0; r < rate->rungs; ++r) {
        if (rate->ladder[r] > trellis_lambda_max())
            return fail(c, AMVHIP_ERR_ARG, "encode_rate: rung %u's lambda %u is more than amvhip_encode_trellis_lambda_max() = %u", r, rate->ladder[r],
                        trellis_lambda_max());
        arg->ladder.lambda[r] = rate->ladder[r];
    }
    return AMVHIP_OK;
}
int amv::rate_args_ok(amvhip_ctx* c, uint32_t n, uint32_t w, uint32_t h, const QuantRequest& req, const uint32_t* d_rung) {
    if (int r = quant_args_ok(c, n, w, h, req)) return r;
    if (!rate_blocks_ok(make_geom(w, h).blocks))
        return fail(c, AMVHIP_ERR_ARG, "encode_rate: a picture of more than %u blocks (a frame's bits need not fit 32)", kRateBlocksMost);
    if ((n && !d_rung) || ((uintptr_t)d_rung & 3u)) return fail(c, AMVHIP_ERR_ARG, "encode_rate: d_rung / d_bits is null or not 4-byte aligned");
    return AMVHIP_OK;
}

// The bits of n frames at every rung, ADDED to bits [n][rungs] (the context is locked, c->rate_ws holds the call's rate_plan):
// the probe's two launches, as many frames at a time as a grid takes.  offsets: the frames' -nr offsets, or nullptr.
static int rate_probe(amvhip_ctx* c, const Source& in, uint32_t n, const FrameGeom& g, uint32_t qbias, const uint16_t* offsets,
                      const RateLadder& ladder, uint32_t* bits, hipStream_t stream) {
    int16_t* const dc = (int16_t*)((uint8_t*)c->rate_ws.p + rate_plan(n, ladder.rungs, g.blocks).dc);
    const uint64_t segs = (uint64_t)g.mcu_rows * seg_split(g).nseg;
    const uint32_t most = (uint32_t)((1ull << 30) / segs);      // frames per launch: >= 1 (a picture has at most 2^20 MCUs)
    Timed t(c, AMVHIP_K_FDCT, stream);
    for (uint32_t base = 0; base < n; base += most) {
        const uint32_t items = n - base < most ? n - base : most;
        launch_rate_probe(frames_from(in, base, g), items, g, qbias, offsets ? offsets + (uint64_t)base * 64u : nullptr, ladder,
                          dc + (uint64_t)base * g.blocks, bits + (uint64_t)base * ladder.rungs, stream);
    }
    return check_launch(c, "rate probe");
}

// amvhip_encode_*_rate_probe_dev's core (the context is locked, the request checked, n > 0).  With nr > 0 the chain runs on a
// copy of the state in the workspace: the caller's stays as it was.
static int probe_core(amvhip_ctx* c, const Source& in, uint32_t n, const FrameGeom& g, uint32_t qbias, uint32_t nr, const int32_t* d_state,
                      const RateLadder& ladder, uint32_t* d_bits, hipStream_t stream) {
    const RatePlan plan = rate_plan(n, ladder.rungs, g.blocks);
    if (int r = ensure(c, c->rate_ws, plan.bytes)) return r;
    HIP_TRY(c, hipMemsetAsync(d_bits, 0, (size_t)n * ladder.rungs * 4u, stream));
    const uint16_t* offsets = nullptr;
    if (nr) {
        int32_t* const copy = (int32_t*)((uint8_t*)c->rate_ws.p + plan.state);
        HIP_TRY(c, hipMemcpyAsync(copy, d_state, kNrStateWords * 4u, hipMemcpyDeviceToDevice, stream));
        Quantiser quant;
        if (int r = nr_quantiser(c, in, n, g, nr, copy, nullptr, &quant, stream)) return r;
        offsets = std::get<const uint16_t*>(quant);
    }
    return rate_probe(c, in, n, g, qbias, offsets, ladder, d_bits, stream);
}

// The byte-budget flow, once, for the encoder's and the requant side's rate and clip entries (the context is locked).
// Everything is queued on `stream`, nothing is read back:
//   the workspaces: rate_ws, and clip_ws with a clip; the spans a call zeroes;
//   probe(bits) -> the bits table;
//   the choice: every frame's first floor-fit -> d_rung, the frame's lambda.  With a clip, in its place: the floor sums over
//   `frames`, and the start: the first clip rung whose floor sum fits, every frame's record and lambda there;
//   first_pass(lambda): every frame coded at its lambda, its length in d_lens; the check: a frame over its budget moves to its
//   next floor-fit and joins a list.  With a clip, behind every check the settle: with every frame inside its budget the
//   lengths are summed, and the clip is final or moves on and lists the frames it takes along;
//   up to rungs - 1 (with a clip: clip_passes_most - 1) redo passes over that list, redo_round(sel, items, lambda) a round of
//   the coefficient workspace at a time (FrameSel rounds: small launches, usually with nothing to do -- the host cannot know),
//   each pass with its check (and settle) behind it.
// The counters of the passes are the rate plan's without a clip, the clip plan's with one.  who: the entry, for check_launch.
int amv::budget_passes(amvhip_ctx* c, const RateArg& rate, const ClipArg* clip, const ClipFrames& frames, uint32_t n, uint32_t blocks,
                       uint32_t round, uint32_t* d_lens, uint32_t* d_rung, const char* who, hipStream_t stream, const BudgetProbe& probe,
                       const BudgetFirstPass& first_pass, const BudgetRedoRound& redo_round) {
    const RateLadder& lad = rate.ladder;
    const uint32_t rungs = lad.rungs;
    const RatePlan plan = rate_plan(n, rungs, blocks);
    const ClipPlan cplan = clip_plan();
    if (int r = ensure(c, c->rate_ws, plan.bytes)) return r;
    if (clip)
        if (int r = ensure(c, c->clip_ws, cplan.bytes)) return r;
    uint8_t* const ws = (uint8_t*)c->rate_ws.p;
    uint8_t* const cws = clip ? (uint8_t*)c->clip_ws.p : nullptr;
    uint32_t* const counters = clip ? (uint32_t*)(cws + cplan.counters) : (uint32_t*)(ws + plan.counters);
    uint64_t* const F = clip ? (uint64_t*)(cws + cplan.F) : nullptr;
    ClipState* const state = clip ? (ClipState*)(cws + cplan.state) : nullptr;
    uint32_t* const bits = (uint32_t*)(ws + plan.bits);
    uint32_t* const lambda = (uint32_t*)(ws + plan.lambda);
    uint32_t* const lists[2] = {(uint32_t*)(ws + plan.list[0]), (uint32_t*)(ws + plan.list[1])};
    HIP_TRY(c, hipMemsetAsync(ws + plan.zero, 0, plan.zero_bytes, stream));
    if (clip) HIP_TRY(c, hipMemsetAsync(cws, 0, cplan.bytes, stream));
    if (int r = probe(bits)) return r;
    if (clip) {
        launch_clip_floor(bits, rungs, rate.d_budget, rate.budget, n, frames, F, stream);
        launch_clip_start(bits, lad, rate.d_budget, rate.budget, n, frames, F, clip->total, state, d_rung, lambda, stream);
        if (int r = check_launch(c, (std::string(who) + ": floor + start").c_str())) return r;
    } else {
        launch_rate_choose(bits, lad, rate.d_budget, rate.budget, n, d_rung, lambda, stream);
    }
    if (int r = first_pass(lambda)) return r;
    // behind a pass over list[0 .. *count) (nullptr: over all n)
    const auto check = [&](const uint32_t* list, const uint32_t* count, uint32_t* next, uint32_t* next_count) {
        launch_rate_check(bits, lad, rate.d_budget, rate.budget, n, d_lens, list, count, d_rung, lambda, next, next_count, stream);
        if (clip)
            launch_clip_settle(bits, lad, rate.d_budget, rate.budget, n, frames, d_lens, F, clip->total, state, d_rung, lambda, next, next_count,
                               clip->d_clip, stream);
    };
    check(nullptr, nullptr, lists[0], counters + 1);
    const uint32_t passes = clip ? clip_passes_most(rungs) : rungs;
    for (uint32_t pass = 1; pass < passes; ++pass) {
        const uint32_t* const list = lists[(pass - 1u) & 1u];
        const uint32_t* const count = counters + pass;
        for (uint32_t base = 0; base < n; base += round) {
            const uint32_t items = n - base < round ? n - base : round;
            if (int r = redo_round(FrameSel{list, count, base, items}, items, lambda)) return r;
        }
        check(list, count, lists[pass & 1u], counters + pass + 1u);
        if (int r = check_launch(c, (std::string(who) + ": redo pass").c_str())) return r;
    }
    return AMVHIP_OK;
}

// amvhip_encode_*_rate_stream_dev's and (clip not null) amvhip_encode_*_clip_stream_dev's core (the context is locked, the
// request checked, n > 0): budget_passes over the pictures.  With nr > 0 passes A and B run once, in front of the probe (the
// state moves as in _nr_trellis_stream).  The first pass is amv_forward_kernel with the frames' lambdas + amv_pack_kernel over
// all frames, a round of the coefficient workspace at a time (default launches over the round's part of the source); a redo
// round is the same pair over a FrameSel; the compaction ends the call.
// The one-kernel encoder takes no part: it has no instantiation with a lambda per frame, so both entropy modes run this.
static int rate_core(amvhip_ctx* c, const Source& in, uint32_t n, const FrameGeom& g, uint32_t qbias, uint32_t nr, int32_t* d_state,
                     const RateArg& rate, const ClipArg* clip, uint8_t* d_blob, uint64_t blob_cap, uint64_t* d_offs, uint32_t* d_lens,
                     uint32_t* d_rung, hipStream_t stream) {
    const uint32_t bound = amvhip_encode_bound(g.width, g.height);
    const HuffEncodeImage* book = (const HuffEncodeImage*)c->d_enc.p;
    const uint32_t round = fallback_round(n, g, 1024u, 2u);
    if (int r = ensure(c, c->coef, (size_t)round * g.blocks * 128)) return r;
    if (int r = ensure(c, c->tmp, (size_t)n * bound)) return r;
    if (int r = ensure(c, c->flag, 16)) return r;
    const uint16_t* offsets = nullptr;
    const auto quant_of = [&](const uint32_t* lambda) { return offsets ? Quantiser{NrTrellisFrames{offsets, lambda}} : Quantiser{TrellisFrames{lambda}}; };
    // forward + pack of one launch: `frames` of src, their chunks and lengths from frame `base` on
    const auto code = [&](const Source& src, uint32_t frames, const FrameSel& sel, uint32_t items, const Quantiser& quant, uint32_t base) {
        {
            Timed t(c, AMVHIP_K_FDCT, stream);
            launch_forward(src, frames, sel, items, g, qbias, quant, (int16_t*)c->coef.p, stream);
        }
        Timed t(c, AMVHIP_K_PACK_SERIAL, stream);
        launch_pack((const int16_t*)c->coef.p, frames, sel, items, g, book, (uint8_t*)c->tmp.p + (uint64_t)base * bound, bound, d_lens + base,
                    stream);
    };
    if (int r = budget_passes(
            c, rate, clip, kClipAllFrames, n, g.blocks, round, d_lens, d_rung, clip ? "clip" : "rate", stream,
            [&](uint32_t* bits) {
                if (nr) {
                    Quantiser with_offsets;
                    if (int r = nr_quantiser(c, in, n, g, nr, d_state, nullptr, &with_offsets, stream)) return r;
                    offsets = std::get<const uint16_t*>(with_offsets);
                }
                return rate_probe(c, in, n, g, qbias, offsets, rate.ladder, bits, stream);
            },
            [&](const uint32_t* lambda) {
                const Quantiser quant = quant_of(lambda);
                for (uint32_t base = 0; base < n; base += round) {
                    const uint32_t items = n - base < round ? n - base : round;
                    code(frames_from(in, base, g), items, kAllFrames, items, frames_from(quant, base), base);
                    if (int r = check_launch(c, clip ? "clip: forward + pack" : "rate: forward + pack")) return r;
                }
                return (int)AMVHIP_OK;
            },
            [&](const FrameSel& sel, uint32_t items, const uint32_t* lambda) {
                code(in, n, sel, items, quant_of(lambda), 0u);
                return (int)AMVHIP_OK;
            }))
        return r;
    {
        Timed t(c, AMVHIP_K_COMPACT, stream);
        launch_compact((const uint8_t*)c->tmp.p, bound, d_lens, n, d_offs, d_blob, blob_cap, (int32_t*)c->flag.p, stream);
    }
    return check_launch(c, "compact");
}

static const NrTrellisRequest& rate_nr_of(const QuantRequest& req) { return std::get<NrTrellisRequest>(req); }

int amv::rate_scaled_tail(amvhip_ctx* c, uint32_t n, uint32_t w, uint32_t h, uint32_t qbias, const QuantRequest& req, const RateArg& rate,
                          uint8_t* d_blob, uint64_t blob_cap, uint64_t* d_offs, uint32_t* d_lens, uint32_t* d_rung, hipStream_t stream) {
    return rate_core(c, yuv_source(yuv_source_of(tight_420((uint8_t*)c->scaled.p, w, h))), n, make_geom(w, h), qbias, rate_nr_of(req).nr,
                     rate_nr_of(req).state, rate, nullptr, d_blob, blob_cap, d_offs, d_lens, d_rung, stream);
}

static int rate_probe_dev(amvhip_ctx* c, const Source& in, uint32_t n, uint32_t w, uint32_t h, const amvhip_quant* q, const uint32_t* ladder,
                          uint32_t rungs, uint32_t* d_bits, void* stream) {
    if (!c) return AMVHIP_ERR_ARG;
    const amvhip_rate as_rate{ladder, rungs, 0u, nullptr};
    QuantRequest req;
    RateArg rate;
    if (int r = rate_request_of(c, q, &as_rate, &req, &rate)) return r;
    if (int r = source_args_ok(c, in, n, w, h, q->qbias, false)) return r;
    if (int r = rate_args_ok(c, n, w, h, req, d_bits)) return r;
    if (n == 0) return AMVHIP_OK;
    if (int r = use_device(c)) return r;
    std::lock_guard<std::mutex> lk(c->mu);
    return probe_core(c, in, n, make_geom(w, h), q->qbias, rate_nr_of(req).nr, rate_nr_of(req).state, rate.ladder, d_bits, (hipStream_t)stream);
}

static int rate_stream_dev(amvhip_ctx* c, const Source& in, uint32_t n, uint32_t w, uint32_t h, const amvhip_quant* q, const amvhip_rate* rate_in,
                           uint8_t* d_blob, uint64_t blob_cap, uint64_t* d_offs, uint32_t* d_lens, uint32_t* d_rung, void* stream) {
    if (!c) return AMVHIP_ERR_ARG;
    QuantRequest req;
    RateArg rate;
    if (int r = rate_request_of(c, q, rate_in, &req, &rate)) return r;
    if (int r = source_args_ok(c, in, n, w, h, q->qbias, n && (!d_blob || !d_offs || !d_lens))) return r;
    if (int r = rate_args_ok(c, n, w, h, req, d_rung)) return r;
    if (n == 0) return AMVHIP_OK;
    if (int r = use_device(c)) return r;
    std::lock_guard<std::mutex> lk(c->mu);
    return rate_core(c, in, n, make_geom(w, h), q->qbias, rate_nr_of(req).nr, rate_nr_of(req).state, rate, nullptr, d_blob, blob_cap, d_offs, d_lens,
                     d_rung, (hipStream_t)stream);
}

extern "C" int amvhip_encode_rate_probe_dev(amvhip_ctx* c, const uint8_t* d_pix, uint32_t pix_stride, int is_bgr, uint32_t n, uint32_t w, uint32_t h,
                                            const amvhip_quant* q, const uint32_t* ladder, uint32_t rungs, uint32_t* d_bits, void* stream) {
    return rate_probe_dev(c, rgb_source(d_pix, pix_stride, is_bgr), n, w, h, q, ladder, rungs, d_bits, stream);
}

extern "C" int amvhip_encode_yuv420_rate_probe_dev(amvhip_ctx* c, const uint8_t* d_y, const uint8_t* d_cb, const uint8_t* d_cr, uint32_t y_stride,
                                                   uint32_t c_stride, uint64_t y_frame_stride, uint64_t c_frame_stride, uint32_t n, uint32_t w,
                                                   uint32_t h, const amvhip_quant* q, const uint32_t* ladder, uint32_t rungs, uint32_t* d_bits,
                                                   void* stream) {
    return rate_probe_dev(c, yuv_source({d_y, d_cb, d_cr, y_stride, c_stride, y_frame_stride, c_frame_stride, 0u}), n, w, h, q, ladder, rungs,
                          d_bits, stream);
}

extern "C" int amvhip_encode_rate_stream_dev(amvhip_ctx* c, const uint8_t* d_pix, uint32_t pix_stride, int is_bgr, uint32_t n, uint32_t w,
                                             uint32_t h, const amvhip_quant* q, const amvhip_rate* rate, uint8_t* d_blob, uint64_t blob_cap,
                                             uint64_t* d_offs, uint32_t* d_lens, uint32_t* d_rung, void* stream) {
    return rate_stream_dev(c, rgb_source(d_pix, pix_stride, is_bgr), n, w, h, q, rate, d_blob, blob_cap, d_offs, d_lens, d_rung, stream);
}

extern "C" int amvhip_encode_yuv420_rate_stream_dev(amvhip_ctx* c, const uint8_t* d_y, const uint8_t* d_cb, const uint8_t* d_cr,
                                                    uint32_t y_stride, uint32_t c_stride, uint64_t y_frame_stride, uint64_t c_frame_stride,
                                                    uint32_t n, uint32_t w, uint32_t h, const amvhip_quant* q, const amvhip_rate* rate,
                                                    uint8_t* d_blob, uint64_t blob_cap, uint64_t* d_offs, uint32_t* d_lens, uint32_t* d_rung,
                                                    void* stream) {
    return rate_stream_dev(c, yuv_source({d_y, d_cb, d_cr, y_stride, c_stride, y_frame_stride, c_frame_stride, 0u}), n, w, h, q, rate, d_blob,
                           blob_cap, d_offs, d_lens, d_rung, stream);
}

// ---- the clip entries: a byte budget for the whole call, above the one per frame (amv_clip_plan.h, amv_encode_clip.hip) ---
int amv::clip_args_ok(amvhip_ctx* c, uint32_t n, const uint64_t* d_clip) {
    if ((n && !d_clip) || ((uintptr_t)d_clip & 7u)) return fail(c, AMVHIP_ERR_ARG, "encode_clip: d_clip is null or not 8-byte aligned");
    return AMVHIP_OK;
}

int amv::clip_scaled_tail(amvhip_ctx* c, uint32_t n, uint32_t w, uint32_t h, uint32_t qbias, const QuantRequest& req, const RateArg& rate,
                          const ClipArg& clip, uint8_t* d_blob, uint64_t blob_cap, uint64_t* d_offs, uint32_t* d_lens, uint32_t* d_rung,
                          hipStream_t stream) {
    return rate_core(c, yuv_source(yuv_source_of(tight_420((uint8_t*)c->scaled.p, w, h))), n, make_geom(w, h), qbias, rate_nr_of(req).nr,
                     rate_nr_of(req).state, rate, &clip, d_blob, blob_cap, d_offs, d_lens, d_rung, stream);
}

static int clip_stream_dev(amvhip_ctx* c, const Source& in, uint32_t n, uint32_t w, uint32_t h, const amvhip_quant* q, const amvhip_rate* rate_in,
                           uint64_t total, uint8_t* d_blob, uint64_t blob_cap, uint64_t* d_offs, uint32_t* d_lens, uint32_t* d_rung,
                           uint64_t* d_clip, void* stream) {
    if (!c) return AMVHIP_ERR_ARG;
    QuantRequest req;
    RateArg rate;
    if (int r = rate_request_of(c, q, rate_in, &req, &rate)) return r;
    if (int r = source_args_ok(c, in, n, w, h, q->qbias, n && (!d_blob || !d_offs || !d_lens))) return r;
    if (int r = rate_args_ok(c, n, w, h, req, d_rung)) return r;
    if (int r = clip_args_ok(c, n, d_clip)) return r;
    if (n == 0) return AMVHIP_OK;
    if (int r = use_device(c)) return r;
    std::lock_guard<std::mutex> lk(c->mu);
    const ClipArg clip{total, d_clip};
    return rate_core(c, in, n, make_geom(w, h), q->qbias, rate_nr_of(req).nr, rate_nr_of(req).state, rate, &clip, d_blob, blob_cap, d_offs, d_lens,
                     d_rung, (hipStream_t)stream);
}

extern "C" int amvhip_encode_clip_stream_dev(amvhip_ctx* c, const uint8_t* d_pix, uint32_t pix_stride, int is_bgr, uint32_t n, uint32_t w,
                                             uint32_t h, const amvhip_quant* q, const amvhip_rate* rate, uint64_t total, uint8_t* d_blob,
                                             uint64_t blob_cap, uint64_t* d_offs, uint32_t* d_lens, uint32_t* d_rung, uint64_t* d_clip,
                                             void* stream) {
    return clip_stream_dev(c, rgb_source(d_pix, pix_stride, is_bgr), n, w, h, q, rate, total, d_blob, blob_cap, d_offs, d_lens, d_rung, d_clip,
                           stream);
}

extern "C" int amvhip_encode_yuv420_clip_stream_dev(amvhip_ctx* c, const uint8_t* d_y, const uint8_t* d_cb, const uint8_t* d_cr,
                                                    uint32_t y_stride, uint32_t c_stride, uint64_t y_frame_stride, uint64_t c_frame_stride,
                                                    uint32_t n, uint32_t w, uint32_t h, const amvhip_quant* q, const amvhip_rate* rate,
                                                    uint64_t total, uint8_t* d_blob, uint64_t blob_cap, uint64_t* d_offs, uint32_t* d_lens,
                                                    uint32_t* d_rung, uint64_t* d_clip, void* stream) {
    return clip_stream_dev(c, yuv_source({d_y, d_cb, d_cr, y_stride, c_stride, y_frame_stride, c_frame_stride, 0u}), n, w, h, q, rate, total,
                           d_blob, blob_cap, d_offs, d_lens, d_rung, d_clip, stream);
}

// the device-to-host half of the host-buffer encoders: offs/lens, then the chunks
static int encode_fetch(amvhip_ctx* c, hipStream_t hs, uint32_t n, uint8_t* blob, uint64_t blob_cap, uint64_t* offs, uint32_t* lens) {
    int32_t overflow = 0;
    HIP_TRY(c, hipMemcpyAsync(offs, c->h_offs.p, (size_t)n * 8, hipMemcpyDeviceToHost, hs));
    HIP_TRY(c, hipMemcpyAsync(lens, c->h_lens.p, (size_t)n * 4, hipMemcpyDeviceToHost, hs));
    HIP_TRY(c, hipMemcpyAsync(&overflow, c->flag.p, 4, hipMemcpyDeviceToHost, hs));
    HIP_TRY(c, hipStreamSynchronize(hs));
    const uint64_t total = offs[n - 1] + lens[n - 1];
    if (overflow || total > blob_cap)
        return fail(c, AMVHIP_ERR_SPACE, "encode: the chunks need more than the %llu bytes of blob", (unsigned long long)blob_cap);
    HIP_TRY(c, hipMemcpyAsync(blob, c->h_out.p, total, hipMemcpyDeviceToHost, hs));
    HIP_TRY(c, hipStreamSynchronize(hs));
    return AMVHIP_OK;
}

// The host-buffer forms behind their own checks of the pointers and strides: the request's checks and n == 0 before anything
// is staged; then, with c->hmu held round the staging buffers (one host-buffer call at a time), stage_in(hs, in) queues the
// pixels' way to c->h_in and says where they are, the state of a request with nr > 0 goes up to the device before the call
// and comes back after it, and the chunks follow.  req's state is the caller's, on the host.
template <class StageIn>
static int encode_host(amvhip_ctx* c, uint32_t n, uint32_t w, uint32_t h, uint32_t qbias, QuantRequest req, uint8_t* blob, uint64_t blob_cap,
                       uint64_t* offs, uint32_t* lens, StageIn&& stage_in) {
    if (int r = quant_args_ok(c, n, w, h, req)) return r;
    if (n == 0) return AMVHIP_OK;
    hipStream_t hs;
    if (int r = host_stream(c, &hs)) return r;
    std::lock_guard<std::mutex> hlk(c->hmu);
    if (int r = ensure(c, c->h_out, blob_cap + 16)) return r;   // (before a copy from the caller's memory is queued)
    if (int r = ensure(c, c->h_offs, (size_t)n * 8)) return r;
    if (int r = ensure(c, c->h_lens, (size_t)n * 4)) return r;
    Source in;
    if (int r = stage_in(hs, in)) return r;
    NrPart q;
    int32_t* const state = nr_part_of(req, &q) && q.nr ? *q.state : nullptr;
    if (state) {                               // req is this call's copy: from here on its state is the device's, as encode_dev wants it
        if (int r = stage(c, c->nr_state, kNrStateWords * 4u, state, kNrStateWords * 4u, hs)) return r;
        *q.state = (int32_t*)c->nr_state.p;
    }
    if (int r = encode_dev(c, in, n, w, h, qbias, req, (uint8_t*)c->h_out.p, blob_cap, (uint64_t*)c->h_offs.p, (uint32_t*)c->h_lens.p, hs)) return r;
    if (state) {                               // (the state has moved on even where the chunks do not fit the blob)
        HIP_TRY(c, hipMemcpyAsync(state, c->nr_state.p, kNrStateWords * 4u, hipMemcpyDeviceToHost, hs));
        HIP_TRY(c, hipStreamSynchronize(hs));
    }
    return encode_fetch(c, hs, n, blob, blob_cap, offs, lens);
}

static int encode_rgb_host(amvhip_ctx* c, const uint8_t* pix, uint32_t pix_stride, int is_bgr, uint32_t n, uint32_t w, uint32_t h,
                           uint32_t qbias, const QuantRequest& req, uint8_t* blob, uint64_t blob_cap, uint64_t* offs, uint32_t* lens) {
    if (!c) return AMVHIP_ERR_ARG;
    if (n && (!pix || !blob || !offs || !lens)) return fail(c, AMVHIP_ERR_ARG, "encode: null argument");
    return encode_host(c, n, w, h, qbias, req, blob, blob_cap, offs, lens, [&](hipStream_t hs, Source& in) -> int {
        const size_t in_bytes = (size_t)pix_stride * h * n;
        if (int r = stage(c, c->h_in, in_bytes, pix, in_bytes, hs)) return r;
        in = rgb_source((const uint8_t*)c->h_in.p, pix_stride, is_bgr);
        return AMVHIP_OK;
    });
}

extern "C" int amvhip_encode_batch(amvhip_ctx* c, const uint8_t* pix, uint32_t pix_stride, int is_bgr, uint32_t n, uint32_t w, uint32_t h,
                                   uint32_t qbias, uint8_t* blob, uint64_t blob_cap, uint64_t* offs, uint32_t* lens) {
    return encode_rgb_host(c, pix, pix_stride, is_bgr, n, w, h, qbias, PlainQuant{}, blob, blob_cap, offs, lens);
}

extern "C" int amvhip_encode_nr_stream(amvhip_ctx* c, const uint8_t* pix, uint32_t pix_stride, int is_bgr, uint32_t n, uint32_t w, uint32_t h,
                                       uint32_t qbias, uint32_t nr, int32_t* state, uint8_t* blob, uint64_t blob_cap, uint64_t* offs,
                                       uint32_t* lens) {
    return encode_rgb_host(c, pix, pix_stride, is_bgr, n, w, h, qbias, NrRequest{nr, state}, blob, blob_cap, offs, lens);
}

extern "C" int amvhip_encode_trellis_batch(amvhip_ctx* c, const uint8_t* pix, uint32_t pix_stride, int is_bgr, uint32_t n, uint32_t w, uint32_t h,
                                           uint32_t qbias, uint32_t lambda, uint8_t* blob, uint64_t blob_cap, uint64_t* offs, uint32_t* lens) {
    return encode_rgb_host(c, pix, pix_stride, is_bgr, n, w, h, qbias, TrellisArg{lambda}, blob, blob_cap, offs, lens);
}

extern "C" int amvhip_encode_nr_trellis_stream(amvhip_ctx* c, const uint8_t* pix, uint32_t pix_stride, int is_bgr, uint32_t n, uint32_t w,
                                               uint32_t h, uint32_t qbias, uint32_t nr, uint32_t lambda, int32_t* state, uint8_t* blob,
                                               uint64_t blob_cap, uint64_t* offs, uint32_t* lens) {
    return encode_rgb_host(c, pix, pix_stride, is_bgr, n, w, h, qbias, NrTrellisRequest{nr, state, lambda}, blob, blob_cap, offs, lens);
}

static int encode_yuv_host(amvhip_ctx* c, const uint8_t* y, const uint8_t* cb, const uint8_t* cr, uint32_t y_stride, uint32_t c_stride,
                           uint64_t y_frame_stride, uint64_t c_frame_stride, uint32_t rows422, uint32_t n, uint32_t w, uint32_t h, uint32_t qbias,
                           const QuantRequest& req, uint8_t* blob, uint64_t blob_cap, uint64_t* offs, uint32_t* lens) {
    if (!c) return AMVHIP_ERR_ARG;
    if (!size_ok(w, h) || (w & 1) || (h & 1) || y_stride < w || c_stride < w / 2 || (n && (!y || !cb || !cr || !blob || !offs || !lens)))
        return fail(c, AMVHIP_ERR_ARG, "encode_yuv420: bad argument");
    return encode_host(c, n, w, h, qbias, req, blob, blob_cap, offs, lens, [&](hipStream_t hs, Source& in) -> int {
        // staged tight: Y w*h, Cb, Cr (w/2 x h/2, or w/2 x h when the source is 4:2:2) per frame
        const uint32_t cw = w / 2, chh = rows422 ? h : h / 2;
        const uint64_t fb = (uint64_t)w * h + 2ull * cw * chh;
        if (int r = ensure(c, c->h_in, fb * n)) return r;
        uint8_t* d = (uint8_t*)c->h_in.p;
        for (uint32_t i = 0; i < n; ++i) {
            HIP_TRY(c, hipMemcpy2DAsync(d + i * fb, w, y + i * y_frame_stride, y_stride, w, h, hipMemcpyHostToDevice, hs));
            HIP_TRY(c, hipMemcpy2DAsync(d + i * fb + (uint64_t)w * h, cw, cb + i * c_frame_stride, c_stride, cw, chh, hipMemcpyHostToDevice, hs));
            HIP_TRY(c, hipMemcpy2DAsync(d + i * fb + (uint64_t)w * h + (uint64_t)cw * chh, cw, cr + i * c_frame_stride, c_stride, cw, chh, hipMemcpyHostToDevice, hs));
        }
        in = yuv_source({d, d + (uint64_t)w * h, d + (uint64_t)w * h + (uint64_t)cw * chh, w, cw, fb, fb, rows422});
        return AMVHIP_OK;
    });
}

extern "C" int amvhip_encode_yuv420_nr_stream(amvhip_ctx* c, const uint8_t* y, const uint8_t* cb, const uint8_t* cr, uint32_t y_stride,
                                              uint32_t c_stride, uint64_t y_frame_stride, uint64_t c_frame_stride, uint32_t n, uint32_t w,
                                              uint32_t h, uint32_t qbias, uint32_t nr, int32_t* state, uint8_t* blob, uint64_t blob_cap,
                                              uint64_t* offs, uint32_t* lens) {
    return encode_yuv_host(c, y, cb, cr, y_stride, c_stride, y_frame_stride, c_frame_stride, 0u, n, w, h, qbias, NrRequest{nr, state}, blob, blob_cap,
                           offs, lens);
}

extern "C" int amvhip_encode_yuv420_trellis_batch(amvhip_ctx* c, const uint8_t* y, const uint8_t* cb, const uint8_t* cr, uint32_t y_stride,
                                                  uint32_t c_stride, uint64_t y_frame_stride, uint64_t c_frame_stride, uint32_t n, uint32_t w,
                                                  uint32_t h, uint32_t qbias, uint32_t lambda, uint8_t* blob, uint64_t blob_cap, uint64_t* offs,
                                                  uint32_t* lens) {
    return encode_yuv_host(c, y, cb, cr, y_stride, c_stride, y_frame_stride, c_frame_stride, 0u, n, w, h, qbias, TrellisArg{lambda}, blob, blob_cap,
                           offs, lens);
}

extern "C" int amvhip_encode_yuv420_nr_trellis_stream(amvhip_ctx* c, const uint8_t* y, const uint8_t* cb, const uint8_t* cr, uint32_t y_stride,
                                                      uint32_t c_stride, uint64_t y_frame_stride, uint64_t c_frame_stride, uint32_t n, uint32_t w,
                                                      uint32_t h, uint32_t qbias, uint32_t nr, uint32_t lambda, int32_t* state, uint8_t* blob,
                                                      uint64_t blob_cap, uint64_t* offs, uint32_t* lens) {
    return encode_yuv_host(c, y, cb, cr, y_stride, c_stride, y_frame_stride, c_frame_stride, 0u, n, w, h, qbias,
                           NrTrellisRequest{nr, state, lambda}, blob, blob_cap, offs, lens);
}

extern "C" int amvhip_encode_yuv420_batch(amvhip_ctx* c, const uint8_t* y, const uint8_t* cb, const uint8_t* cr, uint32_t y_stride,
                                          uint32_t c_stride, uint64_t y_frame_stride, uint64_t c_frame_stride, uint32_t n, uint32_t w,
                                          uint32_t h, uint32_t qbias, uint8_t* blob, uint64_t blob_cap, uint64_t* offs, uint32_t* lens) {
    return encode_yuv_host(c, y, cb, cr, y_stride, c_stride, y_frame_stride, c_frame_stride, 0u, n, w, h, qbias, PlainQuant{}, blob, blob_cap, offs,
                           lens);
}

extern "C" int amvhip_encode_yuv422_batch(amvhip_ctx* c, const uint8_t* y, const uint8_t* cb, const uint8_t* cr, uint32_t y_stride,
                                          uint32_t c_stride, uint64_t y_frame_stride, uint64_t c_frame_stride, uint32_t n, uint32_t w,
                                          uint32_t h, uint32_t qbias, uint8_t* blob, uint64_t blob_cap, uint64_t* offs, uint32_t* lens) {
    return encode_yuv_host(c, y, cb, cr, y_stride, c_stride, y_frame_stride, c_frame_stride, 1u, n, w, h, qbias, PlainQuant{}, blob, blob_cap, offs,
                           lens);
}

// ---- picture rescale ------------------------------------------------------------------------------------------------

static ResamplePlanes resample_planes(const PixPicture& p, uint32_t w, uint32_t h) {
    return ResamplePlanes{p.p[0], p.p[1], p.p[2], p.stride[0], p.stride[1], p.frame[0], p.frame[1], w, h};
}

// img_resample_full_init (imgresample.c:425-472) for one pair of sizes
static ResampleFilters resample_filters(uint32_t src_w, uint32_t src_h, uint32_t dst_w, uint32_t dst_h) {
    ResampleFilters f;
    f.h_incr = resample_incr(src_w, dst_w);
    f.v_incr = resample_incr(src_h, dst_h);
    build_resample_filter(f.h, dst_w, src_w);
    build_resample_filter(f.v, dst_h, src_h);
    return f;
}

// n frames, 65535 (the launch's most) at a time
int amv::resample_launch(amvhip_ctx* c, const PixPicture& src, uint32_t src_w, uint32_t src_h, const PixPicture& dst, uint32_t dst_w,
                         uint32_t dst_h, uint32_t n, bool to_jpeg, hipStream_t st) {
    const ResampleFilters f = resample_filters(src_w, src_h, dst_w, dst_h);
    for (uint32_t base = 0; base < n; base += 65535u) {
        ResamplePlanes s = resample_planes(src, src_w, src_h), d = resample_planes(dst, dst_w, dst_h);
        s.y += base * s.y_frame; s.cb += base * s.c_frame; s.cr += base * s.c_frame;
        d.y += base * d.y_frame; d.cb += base * d.c_frame; d.cr += base * d.c_frame;
        launch_resample(s, d, f, n - base < 65535u ? n - base : 65535u, st, to_jpeg);
    }
    return check_launch(c, "resample");
}

extern "C" int amvhip_resample_yuv420_dev(amvhip_ctx* c, const uint8_t* d_src_y, const uint8_t* d_src_cb, const uint8_t* d_src_cr,
                                          uint32_t src_y_stride, uint32_t src_c_stride, uint64_t src_y_frame, uint64_t src_c_frame,
                                          uint32_t src_w, uint32_t src_h, uint8_t* d_dst_y, uint8_t* d_dst_cb, uint8_t* d_dst_cr,
                                          uint32_t dst_y_stride, uint32_t dst_c_stride, uint64_t dst_y_frame, uint64_t dst_c_frame,
                                          uint32_t dst_w, uint32_t dst_h, uint32_t n, void* stream) {
    if (!c) return AMVHIP_ERR_ARG;
    if (!size_ok(src_w, src_h) || !size_ok(dst_w, dst_h) || src_w < 2 || src_h < 2 || dst_w < 2 || dst_h < 2 ||
        src_y_stride < src_w || src_c_stride < src_w / 2 || dst_y_stride < dst_w || dst_c_stride < dst_w / 2 ||
        (n && (!d_src_y || !d_src_cb || !d_src_cr || !d_dst_y || !d_dst_cb || !d_dst_cr)))
        return fail(c, AMVHIP_ERR_ARG, "resample: bad argument");
    if (n == 0) return AMVHIP_OK;
    if (n > 65535u) return fail(c, AMVHIP_ERR_ARG, "resample: at most 65535 frames per call");
    if (int r = use_device(c)) return r;
    return resample_launch(c, make_picture(d_src_y, d_src_cb, d_src_cr, src_y_stride, src_c_stride, src_y_frame, src_c_frame), src_w, src_h,
                           make_picture(d_dst_y, d_dst_cb, d_dst_cr, dst_y_stride, dst_c_stride, dst_y_frame, dst_c_frame), dst_w, dst_h, n,
                           false, (hipStream_t)stream);
}

int amv::encode_scaled_tail(amvhip_ctx* c, uint32_t n, uint32_t w, uint32_t h, uint32_t qbias, const QuantRequest& req, uint8_t* d_blob,
                            uint64_t blob_cap, uint64_t* d_offs, uint32_t* d_lens, hipStream_t stream, uint64_t* d_sse, const QnsArg& qns) {
    return encode_request(c, yuv_source(yuv_source_of(tight_420((uint8_t*)c->scaled.p, w, h))), n, make_geom(w, h), qbias, req, qns, d_blob,
                          blob_cap, d_offs, d_lens, d_sse, stream);
}

// rescale + encode in one call: what ffmpeg.c:757-814 does per picture (sws_scale, then avcodec_encode_video) for a
// source that is not the target size.  The rescaled planes live in the context's workspace.
extern "C" int amvhip_encode_yuv420_scaled_batch_dev(amvhip_ctx* c, const uint8_t* d_y, const uint8_t* d_cb, const uint8_t* d_cr,
                                                     uint32_t y_stride, uint32_t c_stride, uint64_t y_frame_stride, uint64_t c_frame_stride,
                                                     uint32_t src_w, uint32_t src_h, uint32_t n, uint32_t w, uint32_t h, uint32_t qbias,
                                                     uint8_t* d_blob, uint64_t blob_cap, uint64_t* d_offs, uint32_t* d_lens, void* stream) {
    if (!c) return AMVHIP_ERR_ARG;
    if (!encode_size_ok(w, h, qbias) || !size_ok(src_w, src_h) || (n && (!d_blob || !d_offs || !d_lens)))
        return fail(c, AMVHIP_ERR_ARG, "encode_scaled: bad argument (width/height must be even)");
    if (n == 0) return AMVHIP_OK;
    if (int r = use_device(c)) return r;
    // the rescaled planes are the context's: the lock is held from their allocation to the last launch that reads them
    std::lock_guard<std::mutex> lk(c->mu);
    if (int r = ensure(c, c->scaled, amvhip_yuv420_frame_bytes(w, h) * n)) return r;
    const PixPicture dst = tight_420((uint8_t*)c->scaled.p, w, h);
    if (int r = amvhip_resample_yuv420_dev(c, d_y, d_cb, d_cr, y_stride, c_stride, y_frame_stride, c_frame_stride, src_w, src_h, dst.p[0],
                                           dst.p[1], dst.p[2], dst.stride[0], dst.stride[1], dst.frame[0], dst.frame[1], w, h, n, stream))
        return r;
    return encode_scaled_tail(c, n, w, h, qbias, PlainQuant{}, d_blob, blob_cap, d_offs, d_lens, (hipStream_t)stream);
}
