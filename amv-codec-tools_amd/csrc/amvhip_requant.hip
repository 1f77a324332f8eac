// amvhip_requant.hip -- AMV chunks requantised in the coefficient domain behind the C ABI: chunks in, chunks out, no pixel in
// between.  The decoder's entropy stage (amvhip_decode.hip: entropy_records, amv_huffman_kernel) in front, amv_requant.hip in
// the place of the encoder's front half, the encoder's coder, choice and compaction behind it.  The re-table entries are the
// same three cores with the call's tables in Front::rt (chunks written against foreign tables, made AMV's); the rate and the
// clip entries share one, the encoder's budget_passes (amvhip_encode.hip) over the chunks' levels.
#include "amvhip_ctx.h"

using namespace amv;

namespace {

// what the three entries ask of their inputs and shared outputs: the decode entries' words, the encoder entries' for the outputs
// (has_status false: the probe entry, which hands out no statuses)
int requant_args_ok(amvhip_ctx* c, const uint8_t* d_blob, const uint64_t* d_offs, const uint32_t* d_lens, uint32_t n, uint32_t w, uint32_t h,
                    const int32_t* d_status, bool has_status = true) {
    if (!size_ok(w, h)) return fail(c, AMVHIP_ERR_ARG, "requant: bad size %ux%u", w, h);
    if (n && (!d_blob || !d_offs || !d_lens || (has_status && !d_status))) return fail(c, AMVHIP_ERR_ARG, "requant: null argument");
    if (((uintptr_t)d_blob & 3u) || ((uintptr_t)d_status & 3u) || ((uintptr_t)d_lens & 3u) || ((uintptr_t)d_offs & 7u))
        return fail(c, AMVHIP_ERR_ARG, "requant: blob, lens and status must be 4-byte aligned, offs 8-byte");
    return AMVHIP_OK;
}
int requant_outputs_ok(amvhip_ctx* c, uint32_t n, const uint8_t* d_out, const uint64_t* d_out_offs, const uint32_t* d_out_lens) {
    if (n && (!d_out || !d_out_offs || !d_out_lens)) return fail(c, AMVHIP_ERR_ARG, "requant: null output");
    if (((uintptr_t)d_out_offs & 7u) || ((uintptr_t)d_out_lens & 3u)) return fail(c, AMVHIP_ERR_ARG, "requant: out_offs must be 8-byte, out_lens 4-byte aligned");
    return AMVHIP_OK;
}
int requant_lambda_ok(amvhip_ctx* c, uint32_t lambda) {
    if (lambda > trellis_lambda_max())
        return fail(c, AMVHIP_ERR_ARG, "requant: lambda %u is more than amvhip_encode_trellis_lambda_max() = %u", lambda, trellis_lambda_max());
    return AMVHIP_OK;
}
int requant_ladder_of(amvhip_ctx* c, const uint32_t* ladder, uint32_t rungs, RateLadder* out) {
    if (!ladder) return fail(c, AMVHIP_ERR_ARG, "requant_rate: the rate request or its ladder is null");
    if (rungs == 0u || rungs > kRateRungsMax) return fail(c, AMVHIP_ERR_ARG, "requant_rate: a ladder has 1 .. %u rungs", kRateRungsMax);
    *out = RateLadder{};
    out->rungs = rungs;
    for (uint32_t r = 0; r < rungs; ++r) {
        if (ladder[r] > trellis_lambda_max())
            return fail(c, AMVHIP_ERR_ARG, "requant_rate: rung %u's lambda %u is more than amvhip_encode_trellis_lambda_max() = %u", r, ladder[r],
                        trellis_lambda_max());
        out->lambda[r] = ladder[r];
    }
    return AMVHIP_OK;
}
int requant_rate_size_ok(amvhip_ctx* c, uint32_t n, uint32_t w, uint32_t h, const uint32_t* d_words) {
    if (!rate_blocks_ok(make_geom(w, h).blocks))
        return fail(c, AMVHIP_ERR_ARG, "requant_rate: a picture of more than %u blocks (a frame's bits need not fit 32)", kRateBlocksMost);
    if ((n && !d_words) || ((uintptr_t)d_words & 3u)) return fail(c, AMVHIP_ERR_ARG, "requant_rate: d_rung / d_bits is null or not 4-byte aligned");
    return AMVHIP_OK;
}

// A call's chunks, where the entropy stage left their levels, and the round of dense lines they pass through
struct Front {
    const uint8_t* blob;
    uint64_t blob_bytes;
    const uint64_t* offs;
    const uint32_t* lens;
    uint32_t n;
    FrameGeom g;
    int32_t* status;
    uint32_t* nmcu;
    uint32_t* flags;
    SyncSinks sinks;
    Fallback fb;
    uint32_t round;
    int16_t* coef;
    RetableTables rt;             // the re-table entries: the call's tables on the device (tables nullptr: a requant entry)
};

// The entries come in two forms, requant and re-table (amv_retable_plan.h): one core each, `rt` the re-table form's
// argument and nullptr for the requant form.  What the re-table form asks beyond its sibling:
struct Retable {
    const amvhip_retable* rt;
    bool wanted;
};
constexpr Retable kNoRetable{nullptr, false};
int retable_args_ok(amvhip_ctx* c, const Retable& t) {
    if (!t.wanted) return AMVHIP_OK;
    const amvhip_retable* rt = t.rt;
    if (!rt || !rt->tables) return fail(c, AMVHIP_ERR_ARG, "retable: the request or its tables are null");
    if (rt->count == 0u || rt->count > kRetableTablesMax) return fail(c, AMVHIP_ERR_ARG, "retable: a request has 1 .. %u tables", kRetableTablesMax);
    for (uint32_t i = 0; i < rt->count * kRetableTableBytes; ++i)
        if (rt->tables[i] == 0u)
            return fail(c, AMVHIP_ERR_ARG, "retable: table %u has a step of 0 (component %u, scan position %u)", i / kRetableTableBytes, i / 64u % 2u,
                        i % 64u);
    return AMVHIP_OK;
}

// The entropy stage of a call and its workspace (the context is locked).  A round is a multiple of a wave's 64 frames unless
// it is the whole batch: amv_huffman_kernel's last wave of a round takes whole waves of items.
int front_of(amvhip_ctx* c, const uint8_t* d_blob, uint64_t blob_bytes, const uint64_t* d_offs, const uint32_t* d_lens, uint32_t n,
             const FrameGeom& g, int32_t* d_status, hipStream_t st, const Retable& t, Front* f) {
    uint32_t round = fallback_round(n, g, 1024u, 2u);
    if (round < n) round = round >= 128u ? round & ~63u : 64u;
    if (int r = ensure(c, c->coef, (size_t)round * g.blocks * 128)) return r;
    if (int r = ensure(c, c->set[0].nmcu, (size_t)n * 4)) return r;
    if (int r = ensure(c, c->requant_flags, (size_t)n * 4)) return r;
    *f = Front{d_blob, blob_bytes, d_offs, d_lens, n, g, d_status, (uint32_t*)c->set[0].nmcu.p, (uint32_t*)c->requant_flags.p, SyncSinks{},
               Fallback{}, round, (int16_t*)c->coef.p, RetableTables{nullptr, 0u, nullptr}};
    if (t.wanted) {
        const size_t bytes = (size_t)t.rt->count * kRetableTableBytes;
        if (int r = stage(c, c->retable_tables, bytes, t.rt->tables, bytes, st)) return r;
        f->rt = RetableTables{(const uint8_t*)c->retable_tables.p, t.rt->count, t.rt->d_table_of};
    }
    HIP_TRY(c, hipMemsetAsync(f->flags, 0, (size_t)n * 4, st));
    return entropy_records(c, d_blob, blob_bytes, d_offs, d_lens, n, g, false, d_status, f->nmcu, c->set[0], st, f->sinks, f->fb);
}

// The serial kernel's lines of the items base .. base + items of (list, count) -- without a list: of the frames themselves --
// into the round
int serial_round(amvhip_ctx* c, const Front& f, const uint32_t* list, const uint32_t* count, uint32_t base, uint32_t items, hipStream_t st) {
    Timed t(c, AMVHIP_K_HUFFMAN_SERIAL, st);
    launch_huffman(f.blob, f.blob_bytes, f.offs, f.lens, f.n, f.g, (const HuffDecodeImage*)c->d_dec.p, f.coef, f.status, f.nmcu, list, count, base,
                   items, true, false, st);
    return check_launch(c, "requant: huffman");
}

// Every frame of the call once, a round of dense lines at a time: the frames in records form first (expanded a round of
// frames at a time: the sinks' per-frame arrays from `base` on -- a frame's records are found through them, and slot p of the
// round is frame base + p), then what the serial kernel decodes (with a list the count is on the device: rounds past it find
// nothing to do).  body(sel, items, src): the round's lines are in place.
template <class Body>
int each_round(amvhip_ctx* c, const Front& f, hipStream_t st, Body&& body) {
    const FrameGeom& g = f.g;
    if (f.fb.list) {
        const uint32_t segs = segs_per_row(g) * g.mcu_rows;
        for (uint32_t base = 0; base < f.n; base += f.round) {
            const uint32_t items = f.n - base < f.round ? f.n - base : f.round;
            SyncSinks part = f.sinks;
            part.rec_line += base;
            part.seg_start += (uint64_t)base * (segs + 1u) * 2u;
            part.lane_tab += (uint64_t)base * part.lanes * 4u;
            part.rec_count += base;
            launch_expand_records(part, f.nmcu + base, items, g, f.coef, st);
            if (int r = check_launch(c, "requant: expand_records")) return r;
            if (int r = body(FrameSel{nullptr, nullptr, base, items}, items, RequantSource{f.status, f.nmcu, f.sinks.rec_count})) return r;
        }
    }
    for (uint32_t base = 0; base < f.fb.items; base += f.round) {
        const uint32_t items = f.fb.items - base < f.round ? f.fb.items - base : f.round;
        if (int r = serial_round(c, f, f.fb.list, f.fb.count, base, items, st)) return r;
        if (int r = body(FrameSel{f.fb.list, f.fb.count, base, items}, items, RequantSource{f.status, f.nmcu, nullptr})) return r;
    }
    return AMVHIP_OK;
}

// requant + pack of one round whose lines are in place
int code_round(amvhip_ctx* c, const Front& f, const FrameSel& sel, uint32_t items, const RequantSource& src, uint32_t lambda,
               const uint32_t* lambdas, uint64_t* d_err, uint32_t bound, uint32_t* d_lens, hipStream_t st) {
    {
        Timed t(c, AMVHIP_K_FDCT, st);
        launch_requant(f.coef, f.n, sel, items, f.g, src, f.rt, lambda, lambdas, f.flags, d_err, st);
    }
    {
        Timed t(c, AMVHIP_K_PACK_SERIAL, st);
        launch_pack(f.coef, f.n, sel, items, f.g, (const HuffEncodeImage*)c->d_enc.p, (uint8_t*)c->tmp.p, bound, d_lens, st);
    }
    return check_launch(c, "requant: search + pack");
}

int compact(amvhip_ctx* c, uint32_t n, uint32_t bound, uint32_t* d_lens, uint64_t* d_offs, uint8_t* d_out, uint64_t out_cap, hipStream_t st) {
    Timed t(c, AMVHIP_K_COMPACT, st);
    launch_compact((const uint8_t*)c->tmp.p, bound, d_lens, n, d_offs, d_out, out_cap, (int32_t*)c->flag.p, st);
    return check_launch(c, "requant: compact");
}

// The bits of every frame at every rung into bits [n][rungs] (zeroed by the caller); rate_ws holds the call's rate_plan
int probe_pass(amvhip_ctx* c, const Front& f, const RateLadder& ladder, uint32_t* bits, hipStream_t st) {
    int16_t* const dc = (int16_t*)((uint8_t*)c->rate_ws.p + rate_plan(f.n, ladder.rungs, f.g.blocks).dc);
    if (int r = each_round(c, f, st, [&](const FrameSel& sel, uint32_t items, const RequantSource& src) {
            Timed t(c, AMVHIP_K_FDCT, st);
            launch_requant_probe(f.coef, f.n, sel, items, f.g, src, f.rt, ladder, f.flags, dc, bits, st);
            return check_launch(c, "requant: probe");
        }))
        return r;
    Timed t(c, AMVHIP_K_FDCT, st);
    launch_rate_dc(dc, f.n, f.g.blocks, ladder.rungs, bits, st);
    return check_launch(c, "requant: probe (dc)");
}

// what every entry ends its frames' records with (each pointer where the entry has it)
int finish(amvhip_ctx* c, const Front& f, uint32_t* d_lens, uint64_t* d_err, uint32_t* d_rung, uint32_t* d_bits, uint32_t rungs, hipStream_t st) {
    launch_requant_finish(f.n, f.g, f.status, f.nmcu, f.flags, d_lens, d_err, d_rung, d_bits, rungs, st);
    if (f.rt.tables) launch_retable_status(f.n, f.status, f.flags, st);
    return check_launch(c, "requant: finish");
}

int stream_core(amvhip_ctx* c, const uint8_t* d_blob, uint64_t blob_bytes, const uint64_t* d_offs, const uint32_t* d_lens,
                                         uint32_t n, uint32_t w, uint32_t h, uint32_t lambda, uint8_t* d_out, uint64_t out_cap,
                                         uint64_t* d_out_offs, uint32_t* d_out_lens, int32_t* d_status, uint64_t* d_err, void* stream, const Retable& t) {
    if (!c) return AMVHIP_ERR_ARG;
    if (int r = requant_args_ok(c, d_blob, d_offs, d_lens, n, w, h, d_status)) return r;
    if (int r = requant_outputs_ok(c, n, d_out, d_out_offs, d_out_lens)) return r;
    if ((uintptr_t)d_err & 7u) return fail(c, AMVHIP_ERR_ARG, "requant: d_err is not 8-byte aligned");
    if (int r = requant_lambda_ok(c, lambda)) return r;
    if (int r = retable_args_ok(c, t)) return r;
    if (n == 0) return AMVHIP_OK;
    if (int r = use_device(c)) return r;
    std::lock_guard<std::mutex> lk(c->mu);
    hipStream_t st = (hipStream_t)stream;
    const FrameGeom g = make_geom(w, h);
    const uint32_t bound = amvhip_encode_bound(w, h);
    if (int r = ensure(c, c->tmp, (size_t)n * bound)) return r;
    if (int r = ensure(c, c->flag, 16)) return r;
    Front f;
    if (int r = front_of(c, d_blob, blob_bytes, d_offs, d_lens, n, g, d_status, st, t, &f)) return r;
    if (d_err) HIP_TRY(c, hipMemsetAsync(d_err, 0, (size_t)n * 24u, st));
    if (int r = each_round(c, f, st, [&](const FrameSel& sel, uint32_t items, const RequantSource& src) {
            return code_round(c, f, sel, items, src, lambda, nullptr, d_err, bound, d_out_lens, st);
        }))
        return r;
    if (int r = finish(c, f, d_out_lens, d_err, nullptr, nullptr, 0u, st)) return r;
    return compact(c, n, bound, d_out_lens, d_out_offs, d_out, out_cap, st);
}

int probe_core(amvhip_ctx* c, const uint8_t* d_blob, uint64_t blob_bytes, const uint64_t* d_offs,
                                             const uint32_t* d_lens, uint32_t n, uint32_t w, uint32_t h, const uint32_t* ladder, uint32_t rungs,
                                             uint32_t* d_bits, void* stream, const Retable& t) {
    if (!c) return AMVHIP_ERR_ARG;
    RateLadder lad;
    if (int r = requant_ladder_of(c, ladder, rungs, &lad)) return r;
    if (int r = requant_args_ok(c, d_blob, d_offs, d_lens, n, w, h, nullptr, false)) return r;
    if (int r = requant_rate_size_ok(c, n, w, h, d_bits)) return r;
    if (int r = retable_args_ok(c, t)) return r;
    if (n == 0) return AMVHIP_OK;
    if (int r = use_device(c)) return r;
    std::lock_guard<std::mutex> lk(c->mu);
    hipStream_t st = (hipStream_t)stream;
    const FrameGeom g = make_geom(w, h);
    if (int r = ensure(c, c->rate_ws, rate_plan(n, rungs, g.blocks).bytes)) return r;
    if (int r = ensure(c, c->requant_status, (size_t)n * 4)) return r;    // the entry hands out no statuses: a zero row says `not coded`
    int32_t* const d_status = (int32_t*)c->requant_status.p;
    Front f;
    if (int r = front_of(c, d_blob, blob_bytes, d_offs, d_lens, n, g, d_status, st, t, &f)) return r;
    HIP_TRY(c, hipMemsetAsync(d_bits, 0, (size_t)n * rungs * 4u, st));
    if (int r = probe_pass(c, f, lad, d_bits, st)) return r;
    return finish(c, f, nullptr, nullptr, nullptr, d_bits, rungs, st);
}

// The rate entries' and (clip not null) the clip entries' core: the encoder's flow (amvhip_encode.hip: budget_passes) with the
// chunks' levels as the source.  The probe and the first pass go over every frame, a round at a time as the entropy stage left
// them.  A redo round takes its frames' lines from the serial kernel, whichever kernel decoded them first: it decodes any
// frame of the call into any slot, and a list names few.  With a clip (amv_clip_plan.h) the floor sums and the start go over
// the frames that are coded: a frame that is not coded adds nothing to a sum.
int rate_core(amvhip_ctx* c, const uint8_t* d_blob, uint64_t blob_bytes, const uint64_t* d_offs, const uint32_t* d_lens, uint32_t n, uint32_t w,
              uint32_t h, const amvhip_rate* rate, const ClipArg* clip, uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_offs, uint32_t* d_out_lens,
              int32_t* d_status, uint32_t* d_rung, void* stream, const Retable& t) {
    if (!c) return AMVHIP_ERR_ARG;
    if (!rate) return fail(c, AMVHIP_ERR_ARG, "requant_rate: the rate request or its ladder is null");
    RateArg arg{RateLadder{}, rate->budget, rate->d_budget};
    if (int r = requant_ladder_of(c, rate->ladder, rate->rungs, &arg.ladder)) return r;
    if ((uintptr_t)rate->d_budget & 3u) return fail(c, AMVHIP_ERR_ARG, "requant_rate: d_budget is not 4-byte aligned");
    if (int r = requant_args_ok(c, d_blob, d_offs, d_lens, n, w, h, d_status)) return r;
    if (int r = requant_outputs_ok(c, n, d_out, d_out_offs, d_out_lens)) return r;
    if (int r = requant_rate_size_ok(c, n, w, h, d_rung)) return r;
    if (clip)
        if (int r = clip_args_ok(c, n, clip->d_clip)) return r;
    if (int r = retable_args_ok(c, t)) return r;
    if (n == 0) return AMVHIP_OK;
    if (int r = use_device(c)) return r;
    std::lock_guard<std::mutex> lk(c->mu);
    hipStream_t st = (hipStream_t)stream;
    const FrameGeom g = make_geom(w, h);
    const uint32_t bound = amvhip_encode_bound(w, h);
    if (int r = ensure(c, c->tmp, (size_t)n * bound)) return r;
    if (int r = ensure(c, c->flag, 16)) return r;
    Front f;
    if (int r = front_of(c, d_blob, blob_bytes, d_offs, d_lens, n, g, d_status, st, t, &f)) return r;
    const ClipFrames coded{f.status, f.nmcu, f.flags, g.mcus};       // (read behind the probe, which sets the range flags)
    if (int r = budget_passes(
            c, arg, clip, coded, n, g.blocks, f.round, d_out_lens, d_rung, clip ? "requant_clip" : "requant_rate", st,
            [&](uint32_t* bits) { return probe_pass(c, f, arg.ladder, bits, st); },
            [&](const uint32_t* lambda) {
                return each_round(c, f, st, [&](const FrameSel& sel, uint32_t items, const RequantSource& src) {
                    return code_round(c, f, sel, items, src, 0u, lambda, nullptr, bound, d_out_lens, st);
                });
            },
            [&](const FrameSel& sel, uint32_t items, const uint32_t* lambda) {
                if (int r = serial_round(c, f, sel.list, sel.count, sel.base, items, st)) return r;
                return code_round(c, f, sel, items, RequantSource{f.status, f.nmcu, nullptr}, 0u, lambda, nullptr, bound, d_out_lens, st);
            }))
        return r;
    if (int r = finish(c, f, d_out_lens, nullptr, d_rung, nullptr, arg.ladder.rungs, st)) return r;
    return compact(c, n, bound, d_out_lens, d_out_offs, d_out, out_cap, st);
}

}  // namespace

extern "C" int amvhip_requant_stream_dev(amvhip_ctx* c, const uint8_t* d_blob, uint64_t blob_bytes, const uint64_t* d_offs, const uint32_t* d_lens,
                                         uint32_t n, uint32_t w, uint32_t h, uint32_t lambda, uint8_t* d_out, uint64_t out_cap,
                                         uint64_t* d_out_offs, uint32_t* d_out_lens, int32_t* d_status, uint64_t* d_err, void* stream) {
    return stream_core(c, d_blob, blob_bytes, d_offs, d_lens, n, w, h, lambda, d_out, out_cap, d_out_offs, d_out_lens, d_status, d_err, stream, kNoRetable);
}
extern "C" int amvhip_requant_rate_probe_dev(amvhip_ctx* c, const uint8_t* d_blob, uint64_t blob_bytes, const uint64_t* d_offs,
                                             const uint32_t* d_lens, uint32_t n, uint32_t w, uint32_t h, const uint32_t* ladder, uint32_t rungs,
                                             uint32_t* d_bits, void* stream) {
    return probe_core(c, d_blob, blob_bytes, d_offs, d_lens, n, w, h, ladder, rungs, d_bits, stream, kNoRetable);
}
extern "C" int amvhip_requant_rate_stream_dev(amvhip_ctx* c, const uint8_t* d_blob, uint64_t blob_bytes, const uint64_t* d_offs,
                                              const uint32_t* d_lens, uint32_t n, uint32_t w, uint32_t h, const amvhip_rate* rate, uint8_t* d_out,
                                              uint64_t out_cap, uint64_t* d_out_offs, uint32_t* d_out_lens, int32_t* d_status, uint32_t* d_rung,
                                              void* stream) {
    return rate_core(c, d_blob, blob_bytes, d_offs, d_lens, n, w, h, rate, nullptr, d_out, out_cap, d_out_offs, d_out_lens, d_status, d_rung, stream, kNoRetable);
}
extern "C" int amvhip_requant_clip_stream_dev(amvhip_ctx* c, const uint8_t* d_blob, uint64_t blob_bytes, const uint64_t* d_offs,
                                              const uint32_t* d_lens, uint32_t n, uint32_t w, uint32_t h, const amvhip_rate* rate, uint64_t total,
                                              uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_offs, uint32_t* d_out_lens, int32_t* d_status,
                                              uint32_t* d_rung, uint64_t* d_clip, void* stream) {
    const ClipArg clip{total, d_clip};
    return rate_core(c, d_blob, blob_bytes, d_offs, d_lens, n, w, h, rate, &clip, d_out, out_cap, d_out_offs, d_out_lens, d_status, d_rung, stream,
                     kNoRetable);
}

// ---- the re-table form: the siblings above with the tables the chunks were written against behind `height` ----------------------
extern "C" int amvhip_retable_stream_dev(amvhip_ctx* c, const uint8_t* d_blob, uint64_t blob_bytes, const uint64_t* d_offs, const uint32_t* d_lens,
                                         uint32_t n, uint32_t w, uint32_t h, const amvhip_retable* rt, uint32_t lambda, uint8_t* d_out,
                                         uint64_t out_cap, uint64_t* d_out_offs, uint32_t* d_out_lens, int32_t* d_status, uint64_t* d_err,
                                         void* stream) {
    return stream_core(c, d_blob, blob_bytes, d_offs, d_lens, n, w, h, lambda, d_out, out_cap, d_out_offs, d_out_lens, d_status, d_err, stream,
                       Retable{rt, true});
}
extern "C" int amvhip_retable_rate_probe_dev(amvhip_ctx* c, const uint8_t* d_blob, uint64_t blob_bytes, const uint64_t* d_offs,
                                             const uint32_t* d_lens, uint32_t n, uint32_t w, uint32_t h, const amvhip_retable* rt,
                                             const uint32_t* ladder, uint32_t rungs, uint32_t* d_bits, void* stream) {
    return probe_core(c, d_blob, blob_bytes, d_offs, d_lens, n, w, h, ladder, rungs, d_bits, stream, Retable{rt, true});
}
extern "C" int amvhip_retable_rate_stream_dev(amvhip_ctx* c, const uint8_t* d_blob, uint64_t blob_bytes, const uint64_t* d_offs,
                                              const uint32_t* d_lens, uint32_t n, uint32_t w, uint32_t h, const amvhip_retable* rt,
                                              const amvhip_rate* rate, uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_offs, uint32_t* d_out_lens,
                                              int32_t* d_status, uint32_t* d_rung, void* stream) {
    return rate_core(c, d_blob, blob_bytes, d_offs, d_lens, n, w, h, rate, nullptr, d_out, out_cap, d_out_offs, d_out_lens, d_status, d_rung, stream,
                     Retable{rt, true});
}
extern "C" int amvhip_retable_clip_stream_dev(amvhip_ctx* c, const uint8_t* d_blob, uint64_t blob_bytes, const uint64_t* d_offs,
                                              const uint32_t* d_lens, uint32_t n, uint32_t w, uint32_t h, const amvhip_retable* rt,
                                              const amvhip_rate* rate, uint64_t total, uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_offs,
                                              uint32_t* d_out_lens, int32_t* d_status, uint32_t* d_rung, uint64_t* d_clip, void* stream) {
    const ClipArg clip{total, d_clip};
    return rate_core(c, d_blob, blob_bytes, d_offs, d_lens, n, w, h, rate, &clip, d_out, out_cap, d_out_offs, d_out_lens, d_status, d_rung, stream,
                     Retable{rt, true});
}

extern "C" int amvhip_ffmpeg_amv_tables(uint32_t qscale, uint8_t tables[2][64]) {
    return retable_ffmpeg_amv_tables(qscale, tables) ? AMVHIP_OK : AMVHIP_ERR_ARG;
}
