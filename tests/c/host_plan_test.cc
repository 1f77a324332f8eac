// host_plan_test.cc -- the host side's arithmetic (amv-codec-tools_amd/csrc/amv_host_plan.h) walked on the CPU: the Huffman
// table images against codes derived a second way, the entropy stage's sizes and the fall-back rounds against their
// invariants, the two filter builders against their normalisation, the pixel-format routes against the list that
// include/amvhip.h states.  Arguments: (chunk length, blocks) pairs; for each the record space a frame gets is printed as
// "rec <len> <blocks> <words>" for the runner to compare with tests/scan_builder.py::record_space.  Built with g++ and the
// sanitizers by tests/test_abi_and_host.py; prints "ok <cases>" last, or the first failing case.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "amv_host_plan.h"

using namespace amv;

static unsigned cases = 0;

// ---- Huffman images ---------------------------------------------------------------------------------------------------

struct Code { uint32_t sym, len, pos, code; };

// JPEG Annex C: symbols sorted by (length, position in the symbol list), codes counted up, shifted at every length step
static std::vector<Code> codes_of(int t) {
    std::vector<Code> v;
    const uint8_t* syms = symbols_of(t);
    uint32_t pos = 0;
    for (uint32_t len = 1; len <= 16; ++len)
        for (int j = 0; j < kHuffCount[t][len - 1]; ++j, ++pos) v.push_back(Code{syms[pos], len, pos, 0});
    std::stable_sort(v.begin(), v.end(), [](const Code& a, const Code& b) { return a.len != b.len ? a.len < b.len : a.pos < b.pos; });
    uint32_t code = 0, si = v[0].len;
    for (size_t k = 0; k < v.size();) {
        while (k < v.size() && v[k].len == si) v[k++].code = code++;
        if (k == v.size()) break;
        do { code <<= 1; ++si; } while (v[k].len != si);
    }
    return v;
}

static int check_images() {
    static HuffDecodeImage dec;
    static HuffEncodeImage enc;
    build_images(dec, enc);
    std::vector<int> page_used(kLut2Pages, 0);
    for (int t = 0; t < 4; ++t) {
        const std::vector<Code> codes = codes_of(t);
        std::vector<uint8_t> reached(1u << kLut1Bits, 0);
        for (const Code& c : codes) {
            if (enc.code[t][c.sym] != (c.code | (c.len << 16))) return printf("enc t=%d sym=%02x\n", t, c.sym), 1;
            const uint32_t lo = c.code << (16 - c.len), hi = lo | ((1u << (16 - c.len)) - 1u);
            for (uint32_t w16 : {lo, hi}) {
                // the two-level look-up: 9 bits, then the 7 behind them
                uint16_t e = dec.l1[t][w16 >> (16 - kLut1Bits)];
                reached[w16 >> (16 - kLut1Bits)] = 1;
                if (e & 0x8000u) {
                    if ((e & 0xffu) >= (uint32_t)kLut2Pages) return printf("page t=%d sym=%02x\n", t, c.sym), 1;
                    page_used[e & 0xffu] = 1;
                    e = dec.l2[e & 0xffu][w16 & ((1u << kLut2Bits) - 1u)];
                }
                if ((e & 0xffu) != c.sym || ((e >> 8) & 31u) != c.len || (e & 0x8000u))
                    return printf("lut t=%d sym=%02x len=%u window=%04x: entry %04x\n", t, c.sym, c.len, w16, e), 1;
                // the one-lane walk's table, indexed as amv_tables.h documents: the two reads OR-ed
                const uint32_t f = dec.fast[t][w16 >> 7] | dec.fast[t][kFastM2Word + (std::max(w16, 0xfbffu) - 0xfbffu)];
                const bool dc = t < 2;
                const uint32_t size = c.sym & 15u;
                const uint32_t adv = dc ? 1u : (c.sym == 0 ? kFastEobAdvance : (c.sym >> 4) + 1u);
                const uint32_t want = size | ((dc || size) ? kFastEmit : 0u) | (adv << 16) | ((c.len + size) << 24);
                if (f != want) return printf("fast t=%d sym=%02x len=%u window=%04x: %08x, want %08x\n", t, c.sym, c.len, w16, f, want), 1;
                ++cases;
            }
            if (c.len <= (uint32_t)kLut1Bits)
                for (uint32_t s = lo >> 7; s <= hi >> 7; ++s) reached[s] = 1;
        }
        for (uint32_t s = 0; s < (1u << kLut1Bits); ++s) {
            if (reached[s]) continue;
            if (dec.l1[t][s] != 0) return printf("l1 t=%d slot=%u is %04x, no code reaches it\n", t, s, dec.l1[t][s]), 1;
            for (uint32_t w16 : {s << 7, (s << 7) | 0x7fu}) {
                const uint32_t f = dec.fast[t][w16 >> 7] | dec.fast[t][kFastM2Word + (std::max(w16, 0xfbffu) - 0xfbffu)];
                if (f != (kFastInvalid | (1u << 24))) return printf("fast t=%d prefix=%u without a code: %08x\n", t, s, f), 1;
            }
            ++cases;
        }
        if (dec.fast[t][kFastM2Word] != 0) return printf("fast t=%d word 512 is not 0\n", t), 1;
    }
    int pages = 0;
    for (int p = 0; p < kLut2Pages; ++p) {
        pages += page_used[p];
        if (!page_used[p])
            for (uint16_t e : dec.l2[p]) if (e) return printf("l2 page %d is unused and not empty\n", p), 1;
    }
    if (pages != 11) return printf("level-2 pages: %d, not 11\n", pages), 1;
    return 0;
}

// ---- entropy_plan, fallback_round -------------------------------------------------------------------------------------

static int check_plans() {
    const uint32_t dims[5][2] = {{16, 16}, {130, 98}, {160, 120}, {640, 480}, {AMVHIP_MAX_DIM, AMVHIP_MAX_DIM}};
    for (const auto& d : dims) {
        const FrameGeom g = make_geom(d[0], d[1]);
        for (uint32_t n : {1u, 63u, 64u, 16385u, 160000u}) {
            for (uint64_t blob : {(uint64_t)0, (uint64_t)n, (uint64_t)40 * n * g.blocks, (uint64_t)1 << 33}) {
                const EntropyPlan p = entropy_plan(n, blob, g);
                if (p.hi_rec % 32u) return printf("hi_rec %ux%u\n", d[0], d[1]), 1;
                if (p.cap_lines > (uint64_t)n * p.hi_rec / 32u || p.cap_lines > 0xffffffffull)
                    return printf("cap_lines %ux%u n=%u blob=%llu\n", d[0], d[1], n, (unsigned long long)blob), 1;
                if (p.ws_lines > 0xffffffffull || p.ws_lines * 16u < std::min<uint64_t>(blob + 48ull * n, 0xffffffffull * 16u))
                    return printf("ws_lines %ux%u n=%u blob=%llu\n", d[0], d[1], n, (unsigned long long)blob), 1;
                if (p.segs != (g.mcu_cols + 9u) / 10u * g.mcu_rows) return printf("segs %ux%u\n", d[0], d[1]), 1;
                ++cases;
            }
            for (const auto& mp : {std::pair<uint32_t, uint32_t>{16384u, 4u}, std::pair<uint32_t, uint32_t>{1024u, 2u}}) {
                const uint32_t round = fallback_round(n, g, mp.first, mp.second);
                const bool ok = round <= n && (round == n || round >= 64u) && (round <= 64u || (uint64_t)round * g.blocks * 128u <= (2ull << 30));
                if (!ok) return printf("fallback_round %ux%u n=%u most=%u: %u\n", d[0], d[1], n, mp.first, round), 1;
                ++cases;
            }
        }
    }
    return 0;
}

// ---- seg_split, seg_place (amv_segment.h): the encoder's segments ------------------------------------------------------

// every width up to the largest: a row's pieces are as many as the reconstruction's segments, no longer than one, in column
// order without gap or overlap; an empty piece (false, cnt 0) only behind the row's last column; past the last row: none
static int check_segments() {
    for (uint32_t cols = 1; cols <= (AMVHIP_MAX_DIM + 15u) / 16u; ++cols)
        for (uint32_t rows : {1u, 3u}) {
            FrameGeom g{};
            g.mcu_cols = cols;
            g.mcu_rows = rows;
            const SegSplit sp = seg_split(g);
            if (sp.nseg != segs_per_row(g) || sp.per_seg > kSegMcus || (uint64_t)sp.nseg * sp.per_seg < cols) return printf("split %u\n", cols), 1;
            for (uint32_t s = 0; s < (rows + 1u) * sp.nseg; ++s) {
                uint32_t my = ~0u, m0 = ~0u, cnt = ~0u;
                const bool has = seg_place(sp, g, s, my, m0, cnt);
                const uint32_t piece = s % sp.nseg, from = piece * sp.per_seg;
                const uint32_t want = s / sp.nseg < rows && from < cols ? std::min(sp.per_seg, cols - from) : 0u;
                if (has != (want != 0u) || cnt != want || (has && (my != s / sp.nseg || m0 != from)))
                    return printf("place cols=%u rows=%u s=%u: %d my %u m0 %u cnt %u\n", cols, rows, s, (int)has, my, m0, cnt), 1;
            }
            ++cases;
        }
    FrameGeom wide{};                                   // 11 columns: 6 + 5, not 10 + 1
    wide.mcu_cols = 11;
    wide.mcu_rows = 1;
    if (seg_split(wide).per_seg != 6) return printf("11 columns are not 6 + 5\n"), 1;
    return 0;
}

static void print_record_space(uint32_t len, uint32_t blocks) {
    FrameGeom g{};
    g.blocks = blocks;
    const EntropyPlan p = entropy_plan(1, len, g);
    const uint64_t want = std::min<uint64_t>(2ull * len + p.add_rec, p.hi_rec);
    printf("rec %u %u %llu\n", len, blocks, (unsigned long long)((want + 31u) / 32u * 32u));
}

// ---- filter builders ---------------------------------------------------------------------------------------------------

static int check_filters() {
    const uint32_t sizes[4][2] = {{160, 320}, {320, 160}, {128, 130}, {2, 4096}};   // (out, in)
    for (const auto& s : sizes) {
        int16_t f[64];
        build_resample_filter(f, s[0], s[1]);
        for (int ph = 0; ph < 16; ++ph) {
            int sum = 0;
            for (int i = 0; i < 4; ++i) sum += f[ph * 4 + i];
            if (abs(sum - 256) > 2) return printf("resample %u<-%u phase %d sums to %d\n", s[0], s[1], ph, sum), 1;   // lrintf: half a unit per tap
        }
        if (resample_incr(s[1], s[0]) != (int)(((uint64_t)s[1] << 16) / s[0])) return printf("incr %u<-%u\n", s[0], s[1]), 1;
        ++cases;
    }
    const uint32_t rates[4][2] = {{44100, 22050}, {22050, 44100}, {48000, 44100}, {1000, 192000}};   // (in, out)
    for (const auto& r : rates) {
        const uint32_t fl = audio_filter_length(r[0], r[1]), fl_pad = (fl + 7u) & ~7u;
        std::vector<int16_t> bank;
        build_audio_bank(bank, r[0], r[1], fl, fl_pad);
        if (bank.size() != (size_t)kBankPhases * fl_pad || fl < 16) return printf("bank %u->%u: size\n", r[0], r[1]), 1;
        for (uint32_t ph = 0; ph < kBankPhases; ++ph) {
            long sum = 0;
            for (uint32_t i = 0; i < fl; ++i) sum += bank[(size_t)ph * fl_pad + i];
            // half a unit per tap, and one more where a tap of 32768 was held at int16's 32767
            if (labs(sum - 32768) > (long)fl / 2 + 1) return printf("bank %u->%u phase %u sums to %ld\n", r[0], r[1], ph, sum), 1;
            for (uint32_t i = fl; i < fl_pad; ++i)
                if (bank[(size_t)ph * fl_pad + i]) return printf("bank %u->%u phase %u: tap %u of the padding is not 0\n", r[0], r[1], ph, i), 1;
        }
        if (audio_index0(fl) != -(int64_t)1024 * ((fl - 1) / 2)) return printf("index0 %u->%u\n", r[0], r[1]), 1;
        ++cases;
    }
    return 0;
}

// ---- pixel-format routes ----------------------------------------------------------------------------------------------

// the list of include/amvhip.h (amvhip_img_convert_supported); even: the route shrinks chroma or pairs pixels, odd sizes refused
struct Route { int src, dst; PixRoute route; bool even; };
static const int P0 = AMVHIP_PIX_YUV420P, PJ = AMVHIP_PIX_YUVJ420P;
static const Route kRoutes[] = {
    {AMVHIP_PIX_YUVJ420P, P0, kRoutePlanes, false}, {AMVHIP_PIX_YUV422P, P0, kRoutePlanes, true},  {AMVHIP_PIX_YUVJ422P, P0, kRoutePlanes, true},
    {AMVHIP_PIX_YUV444P, P0, kRoutePlanes, true},   {AMVHIP_PIX_YUVJ444P, P0, kRoutePlanes, true}, {AMVHIP_PIX_YUV420P, PJ, kRoutePlanes, false},
    {AMVHIP_PIX_YUV422P, PJ, kRoutePlanes, true},   {AMVHIP_PIX_YUVJ422P, PJ, kRoutePlanes, true}, {AMVHIP_PIX_YUV444P, PJ, kRoutePlanes, true},
    {AMVHIP_PIX_YUVJ444P, PJ, kRoutePlanes, true},  {AMVHIP_PIX_YUYV422, P0, kRoutePackedIn, true}, {AMVHIP_PIX_UYVY422, P0, kRoutePackedIn, true},
    {AMVHIP_PIX_RGB24, P0, kRouteRgbIn, true},      {AMVHIP_PIX_BGR24, P0, kRouteRgbIn, true},     {AMVHIP_PIX_RGB32, P0, kRouteRgbIn, true},
    {AMVHIP_PIX_RGB24, PJ, kRouteRgbIn, true},      {P0, AMVHIP_PIX_YUYV422, kRoutePackedOut, true}, {P0, AMVHIP_PIX_UYVY422, kRoutePackedOut, true},
    {P0, AMVHIP_PIX_RGB24, kRouteRgbOut, false},    {P0, AMVHIP_PIX_BGR24, kRouteRgbOut, false},   {P0, AMVHIP_PIX_RGB32, kRouteRgbOut, false},
    {P0, AMVHIP_PIX_RGB565, kRouteRgbOut, false},   {P0, AMVHIP_PIX_RGB555, kRouteRgbOut, false},  {P0, AMVHIP_PIX_GRAY8, kRouteGray, false},
    {PJ, AMVHIP_PIX_RGB24, kRouteRgbOut, false},    {PJ, AMVHIP_PIX_BGR24, kRouteRgbOut, false},   {PJ, AMVHIP_PIX_RGB32, kRouteRgbOut, false},
    {PJ, AMVHIP_PIX_RGB565, kRouteRgbOut, false},   {PJ, AMVHIP_PIX_RGB555, kRouteRgbOut, false},  {PJ, AMVHIP_PIX_GRAY8, kRouteGray, false}};

static int check_routes() {
    for (int s = -1; s <= AMVHIP_PIX_COUNT; ++s)
        for (int d = -1; d <= AMVHIP_PIX_COUNT; ++d) {
            const Route* want = nullptr;
            for (const Route& r : kRoutes) if (r.src == s && r.dst == d) want = &r;
            if (pix_route(s, d) != (want ? want->route : kRouteNone)) return printf("route %d -> %d: %d\n", s, d, (int)pix_route(s, d)), 1;
            if (!want) continue;
            const uint32_t wh[4][2] = {{16, 16}, {17, 16}, {16, 17}, {AMVHIP_MAX_DIM + 2, 16}};
            const int ok[4] = {1, !want->even, !want->even, 0};
            for (int k = 0; k < 4; ++k)
                if (pix_size_ok(s, d, wh[k][0], wh[k][1]) != ok[k]) return printf("size %d -> %d at %ux%u\n", s, d, wh[k][0], wh[k][1]), 1;
            ++cases;
        }
    // planes: 4:2:0 chroma rounds up, 4:2:2 halves the width alone, packed formats have plane 0 only
    uint32_t rb, rows;
    pix_plane_size(AMVHIP_PIX_YUVJ420P, 1, 17, 9, &rb, &rows);
    if (rb != 9 || rows != 5) return printf("plane size 4:2:0\n"), 1;
    pix_plane_size(AMVHIP_PIX_YUV422P, 2, 17, 9, &rb, &rows);
    if (rb != 9 || rows != 9) return printf("plane size 4:2:2\n"), 1;
    pix_plane_size(AMVHIP_PIX_RGB32, 1, 17, 9, &rb, &rows);
    if (rows != 0) return printf("plane size packed\n"), 1;
    pix_plane_size(AMVHIP_PIX_RGB565, 0, 17, 9, &rb, &rows);
    if (rb != 34 || rows != 9 || pix_bpp(AMVHIP_PIX_RGB24) != 3) return printf("plane 0 size\n"), 1;
    if (pix_frame_bytes(AMVHIP_PIX_YUV420P, 17, 9) != 17 * 9 + 2 * 9 * 5 || pix_frame_bytes(AMVHIP_PIX_YUVJ444P, 17, 9) != 3 * 17 * 9 ||
        pix_frame_bytes(AMVHIP_PIX_RGB24, 52, 9) != 52 * 9 || pix_frame_bytes(AMVHIP_PIX_COUNT, 52, 9) != 0)
        return printf("frame bytes\n"), 1;
    return 0;
}

int main(int argc, char** argv) {
    for (int i = 1; i + 1 < argc; i += 2) print_record_space((uint32_t)strtoul(argv[i], nullptr, 10), (uint32_t)strtoul(argv[i + 1], nullptr, 10));
    if (check_images() || check_plans() || check_segments() || check_filters() || check_routes()) return 1;
    printf("ok %u\n", cases);
    return 0;
}
