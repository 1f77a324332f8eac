/*
 * amvhip.h -- C ABI of libamvhip.so, the MI355X (gfx950) AMV codec hot path.
 *
 * Two surfaces, both plain C (no torch / C++ types in any signature):
 *
 *  1. The amvlib call surface of the reference (tomvanbraeckel/amv-codec-tools),
 *     same names, argument meaning, struct layouts and return codes, so that a host
 *     built against C-AMVDecoder/amvlib/{AMVDec.h,AmvJpeg.h,AdpcmIma.h} links against
 *     this library instead of AmvLib.dll / the amvlib objects.  Each declaration cites
 *     the reference interface it replaces (paths relative to the reference tree).
 *
 *  2. A batch surface (new): many independent chunks per call, device-resident
 *     inputs/outputs, asynchronous on a caller-supplied HIP stream.  This is what the
 *     AMVmuxer / a player loop should call when it has more than one frame in hand;
 *     INTEGRATION.md shows the binding.
 *
 * Every entry point runs on the GPU.  There is no CPU fallback: if no HIP device is
 * usable the calls fail (amvlib surface: -1 / NULL, batch surface: AMVHIP_ERR_DEVICE).
 */
#ifndef AMVHIP_H
#define AMVHIP_H

#include <stdint.h>
#include <stddef.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

/* =====================================================================================
 * 1. amvlib surface
 * =================================================================================== */

/* C-AMVDecoder/amvlib/AMVDec.h:29-47 */
typedef struct _amv_important_header_data {
    unsigned int dwMicroSecPerFrame;
    unsigned int dwWidth;
    unsigned int dwHeight;
    unsigned int dwSpeed;
    unsigned int dwTimeSec;
    unsigned int dwTimeMin;
    unsigned int dwTimeHour;
    unsigned short wFormatTag;
    unsigned short nChannels;
    unsigned int nSamplesPerSec;
    unsigned int nAvgBytesPerSec;
    unsigned short nBlockAlign;
    unsigned short wBitsPerSample;
    unsigned short cbSize;
    unsigned short wSamplesPerBlock;
} AMVInfo;

/* AMVDec.h:50-57 */
typedef struct _frame_buffer_struct {
    unsigned char *videobuff;
    unsigned char *audiobuff;
    unsigned int videobufflen;
    unsigned int audiobufflen;
    int framenum;
} FRAMEBUFF;

/* AMVDec.h:59-63 */
typedef struct _video_buffer_struct {
    unsigned char *fbmpdat;
    unsigned int len;
} VIDEOBUFF;

/* AMVDec.h:65-71 */
#define AUDIO_FILE_TYPE_PCM 0
#define AUDIO_FILE_TYPE_ADPCM_IMA 1
typedef struct _audio_buffer_struct {
    short *audiodata;
    unsigned int len;
} AUDIOBUFF;

/* AMVDec.h:74-91 */
typedef struct _amv_decode_struct {
    char *amvfilename;
    int opened;
    long dataseekpos;
    long fileseekpos;
    AMVInfo amvinfo;
    unsigned int currentframe;
    unsigned int totalframe;
    FRAMEBUFF framebuf;
    VIDEOBUFF videobuf;
    AUDIOBUFF audiobuf;
} AMVDecoder;

/* C-AMVDecoder/amvlib/AdpcmIma.h:11-25 */
typedef struct ADPCMChannelStatus {
    int predictor;
    short int step_index;
    int step;
    int prev_sample;
} ADPCMChannelStatus;

typedef struct ADPCMContext {
    int channel;
    ADPCMChannelStatus status[2];
    short sample_buffer[32];
} ADPCMContext;

/* AmvJpeg.h:95-96 (AmvJpeg.c:1396,1515).  PrepareForVideoDecode rebuilt constant tables per
 * frame in the reference; here the tables live in the code object and the call only
 * validates its argument.  AmvJpegDecode: video->fbmpdat must hold
 * ((dwWidth*24+31)/32)*4*dwHeight bytes; returns 0 ok, -1 on any decode error. */
void PrepareForVideoDecode(AMVInfo *info);
int AmvJpegDecode(AMVInfo *info, FRAMEBUFF *inbuff, VIDEOBUFF *video);

/* AdpcmIma.h:28-32 (AdpcmIma.c:206,92).  Decode: AMV nibble order (high nibble first); c->channel == 2 follows
 * the reference's stereo branch (of every 8 bytes, 4 are the left channel's and 4 the right's; samples leave
 * interleaved, each channel with the predictor and step index of c->status[ch]);
 * returns bytes consumed (>0) or -1.  Encode: the reference's IMA-WAV-layout routine, which
 * nothing in the reference calls; kept for ABI completeness. */
int AdpcmImaDecodeFrame(ADPCMContext *c, void *data, int *data_size, unsigned char *buf, int buf_size);
int AdpcmImaEncodeFrame(ADPCMContext *c, int channels, int frame_size, unsigned char *frame,
                        int buf_size, void *data);

/* AMVDec.h:94-109 (AMVDec.c:15,131,150,240,259,288,358,384).  The container reader is
 * restated LP64-safe (the reference's AMVHeader.h uses `unsigned long` DWORDs). */
AMVDecoder *AmvOpen(const char *amvname);
void AmvClose(AMVDecoder *amv);
int AmvReadNextFrame(AMVDecoder *amv);
int AmvRewindFrameStart(AMVDecoder *amv);
int AmvVideoDecode(AMVDecoder *amv);
int AmvAudioDecode(AMVDecoder *amv);

/* AMVDec.h:102-107 and AmvJpeg.h:93-94 (AMVDec.c:342-547, AmvJpeg.c:315-414,1289-1393): the export
 * helpers.  JPEG stills are the chunk's scan behind a standard JFIF header with amvlib's tables;
 * AmvConvertJpegFileToBmpFile reads back exactly such files (the reference's is a general baseline
 * JPEG reader; files with other tables or sampling factors return -1 here) and decodes on the GPU.
 * AmvCreateWavFileFromAmvFile: type AUDIO_FILE_TYPE_PCM decodes every chunk (GPU), AUDIO_FILE_TYPE_ADPCM_IMA
 * copies the nibbles.  0 on success, -1 on error, like the reference. */
void AmvJpegPutHeader(FILE *fp, unsigned short height, unsigned short width);
int AmvCreateJpegFileFromFrameBuffer(AMVDecoder *amv, const char *dirname);
int AmvCreateJpegFileFromBuffer(AMVInfo *amvinfo, FRAMEBUFF *framebuf, const char *filename);
int AmvConvertJpegFileToBmpFile(const char *jpgname, const char *bmpname);
int ConvertJpegFileToBmpFile(const char *jpgname, const char *bmpname);   /* AmvJpeg.h:94: the same function under its AmvJpeg.c name */
int AmvCreateWavFileFromAmvFile(AMVDecoder *amv, int type, const char *wavfile);

/* the names BASELINE.json's north_star uses; thin aliases of the single-frame paths.
 * decode: chunk -> BGR24 (amvlib layout); encode: RGB24/BGR24 top-down -> chunk, returns length. */
int decode_amv_frame(const unsigned char *chunk, unsigned int len, unsigned int width,
                     unsigned int height, unsigned char *bgr_out);
int encode_amv_frame(const unsigned char *pixels, unsigned int stride, unsigned int width,
                     unsigned int height, int is_bgr, unsigned char *chunk_out, unsigned int cap);

/* =====================================================================================
 * 2. batch surface
 * =================================================================================== */

typedef struct amvhip_ctx amvhip_ctx;

#define AMVHIP_MAX_DIM 16384 /* widest / tallest picture the batch ABI takes (AMVHIP_ERR_ARG beyond; the amvlib surface: -1) */
#define AMVHIP_OK 0
#define AMVHIP_ERR_ARG -1     /* null pointer, zero/odd size, ... */
#define AMVHIP_ERR_DEVICE -2  /* no usable HIP device / HIP call failed (see amvhip_last_error) */
#define AMVHIP_ERR_NOMEM -3
#define AMVHIP_ERR_SPACE -4   /* output capacity too small */

/* per-frame decode status bits written to status[i] (0 = frame ok) */
#define AMVHIP_ST_FORMAT 1u    /* invalid Huffman code (amvlib: FUNC_FORMAT_ERROR, AmvJpeg.c:887) */
#define AMVHIP_ST_OVERRUN 2u   /* coefficient index ran past 63 (amvlib writes out of bounds there) */
#define AMVHIP_ST_TRUNCATED 4u /* scan needs more bits than the chunk holds */

/* decode flags */
#define AMVHIP_FLAG_ZIGZAG_FIXED 1u /* standard zig-zag instead of amvlib's table (AmvJpeg.c:138) */
/* FFmpeg-compat mode: the output of the patched FFmpeg's amv_decoder instead of amvlib's -- sp5x "Q60" quantiser
 * tables (libavcodec/sp5xdec.c:40,60-61, sp5x.h:187-194), standard zig-zag (dsputil.c:50-59), last_dc = 1024 on
 * dequantised DC (mjpegdec.c:805,388-390), simple_idct_put (simple_idct.c:390-398) and planar YUVJ420P output
 * flipped with the formula of mjpegdec.c:672-677.  d_out then holds n * amvhip_yuv420_frame_bytes(w,h) bytes:
 * per frame the Y plane (w*h), then Cb and Cr ((w+1)/2 x (h+1)/2 each), rows tight.  The two reference decoders
 * do NOT agree with each other; amvlib's output is the default and the headline target. */
#define AMVHIP_FLAG_FFMPEG 2u
/* ... and, with it, what the patched FFmpeg leaves in the picture when a chunk is damaged: mjpeg_decode_scan returns at
 * the block whose decode_block fails (mjpegdec.c:699-706) with every block before it already put into the picture
 * (:708-716) and everything else as the picture buffer was.  So: every whole block before the frame's first error is
 * written -- the blocks of the failing MCU in front of the failing one included -- and every other byte of the frame in
 * d_out stays as the caller had it (no plane row is cleared either, not even for an undamaged frame: a host that wants
 * FFmpeg's "shows what it has" hands in the picture before).  Without this flag AMVHIP_FLAG_FFMPEG zero-fills from the
 * failing MCU on, as amvlib does (AMVDec.c:283).  WHERE a chunk fails is this library's strict decoder's verdict
 * (status bits above) in both modes -- mjpegdec.c's own (:384 "error dc", :420 "error count", no truncation check: it
 * reads what lies behind the chunk) is not a function of the chunk alone.  AMVHIP_ERR_ARG without AMVHIP_FLAG_FFMPEG. */
#define AMVHIP_FLAG_FFMPEG_KEEP 4u

/* encode quantiser bias in 1/256 of a step: 0 = the reference's AMV setting
 * (mpegvideo_enc.c:492-496), 128 = its MJPEG setting (round to nearest, :488-490). */
#define AMVHIP_QBIAS_AMV 0
#define AMVHIP_QBIAS_MJPEG 128

int amvhip_create(amvhip_ctx **ctx, int device);
void amvhip_destroy(amvhip_ctx *ctx);
const char *amvhip_last_error(const amvhip_ctx *ctx);
int amvhip_device(const amvhip_ctx *ctx);

/* geometry helpers (AmvJpeg.c:420,1524: stride; :1276-1284: MCU grid) */
uint32_t amvhip_stride(uint32_t width);
uint64_t amvhip_frame_bytes(uint32_t width, uint32_t height);
uint64_t amvhip_yuv420_frame_bytes(uint32_t width, uint32_t height);   /* YUVJ420P frame, tight planes (mjpegdec.c:312) */
uint32_t amvhip_encode_bound(uint32_t width, uint32_t height);
/* the bytes AmvJpegPutHeader writes (SOI ... SOS) for a picture size; returns their number (623) and
 * copies them to out when cap allows.  Host only. */
uint32_t amvhip_jpeg_header(uint16_t height, uint16_t width, uint8_t *out, uint32_t cap);

/*
 * Video decode, device-resident.  Replaces a loop of AmvVideoDecode/AmvJpegDecode calls
 * (AMVDec.c:259-286, AmvJpeg.c:1515-1539) over n independent chunks.
 *   d_blob     : all chunks back to back (each "FF D8" scan "FF D9"); the pointer must be 4-byte aligned (AMVHIP_ERR_ARG
 *                otherwise; chunks themselves may start at any byte)
 *   blob_bytes : the bytes of d_blob the chunks OCCUPY (the end of the last chunk), not the capacity of a larger
 *                buffer: chunks are bounds-checked against it, and the two workspaces between the decode stages -- the
 *                unstuffed scans, the coefficient records -- are laid out per frame from d_lens[i] (on the device) inside a
 *                total sized from blob_bytes here: 1x + 48 bytes per frame for the scans, 8x + (8 per block + 380) bytes per
 *                frame for the records.  Chunks that OVERLAP in the blob (their lengths add up to more than blob_bytes) are
 *                legal and decode correctly, but the layout runs out and the frames behind that point are decoded by the
 *                one-lane-per-frame kernel: same bytes, slower; so is a frame with more than two records per chunk byte
 *                (amvhip_entropy_stats reports how many frames of the last call took that route)
 *   d_offs[i]  : byte offset of chunk i in d_blob;  d_lens[i]: its length
 *   d_out      : n * amvhip_frame_bytes(w,h), 4-byte aligned; frame i is BGR24, row 0 = top, rows padded to
 *                amvhip_stride(w); pixels of MCUs after a failing one are zero (AMVDec.c:283)
 *   d_status   : n int32, AMVHIP_ST_* bits
 *   stream     : hipStream_t (NULL = default stream).  Asynchronous: returns after enqueue.
 * Workspace is owned by ctx and grown on demand (a hipMalloc on first use of a larger
 * batch; none in steady state).  Calls on one context reuse that workspace, so they must be
 * ordered on the device: keep a context on one stream at a time (the lock inside only orders the
 * enqueueing) and create one context per stream for work that is meant to overlap.
 */
int amvhip_decode_batch_dev(amvhip_ctx *ctx, const uint8_t *d_blob, uint64_t blob_bytes,
                            const uint64_t *d_offs, const uint32_t *d_lens, uint32_t n,
                            uint32_t width, uint32_t height, uint32_t flags,
                            uint8_t *d_out, int32_t *d_status, void *stream);

/*
 * The same decode in two halves, for a caller that has the next batch in hand before it needs the last one's pixels
 * (a player or transcoder working through windows of frames): the entropy stage of batch k+1 then runs beside the
 * reconstruction of batch k -- the first waits on memory, the second on the vector ALUs.
 *   amvhip_decode_submit_dev : arguments as amvhip_decode_batch_dev.  The inputs must be ready where `stream` stands
 *       at the call (that point is recorded); the work is queued on streams the context owns and `stream` is NOT made
 *       to wait.  d_blob/d_offs/d_lens must stay untouched and d_out/d_status belong to the batch until it has been
 *       collected and `stream` has passed that point: a batch submitted meanwhile needs buffers of its own.
 *   amvhip_decode_collect_dev: `stream` waits for the oldest batch submitted and not yet collected; work queued on
 *       `stream` afterwards sees its d_out and d_status.
 * At most two batches between submit and collect (a third submit returns AMVHIP_ERR_ARG): what the entropy stage hands
 * to the reconstruction exists twice in the context.  Any other entry point of the context first waits for the batches
 * submitted so far.  Results are those of amvhip_decode_batch_dev, byte for byte.
 */
int amvhip_decode_submit_dev(amvhip_ctx *ctx, const uint8_t *d_blob, uint64_t blob_bytes,
                             const uint64_t *d_offs, const uint32_t *d_lens, uint32_t n,
                             uint32_t width, uint32_t height, uint32_t flags,
                             uint8_t *d_out, int32_t *d_status, void *stream);
int amvhip_decode_collect_dev(amvhip_ctx *ctx, void *stream);

/* device workspace the context held for the last amvhip_decode_batch_dev call, in bytes per frame of that call */
double amvhip_decode_workspace_per_frame(const amvhip_ctx *ctx);

/* Same with host buffers: H2D, decode, D2H, synchronous. */
int amvhip_decode_batch(amvhip_ctx *ctx, const uint8_t *blob, uint64_t blob_bytes,
                        const uint64_t *offs, const uint32_t *lens, uint32_t n,
                        uint32_t width, uint32_t height, uint32_t flags,
                        uint8_t *out, int32_t *status);

/*
 * Asynchronous host-buffer forms, for a host that wants the GPU working while it does something else (the
 * read-ahead behind AmvReadNextFrame uses them): copies and kernels are queued on a stream the context owns and
 * the call returns; amvhip_sync waits for everything queued so far.  blob/offs/lens must stay untouched, and
 * out/status unread, until then.  Page-locked buffers (amvhip_host_alloc) make the copies truly asynchronous;
 * pageable ones work but block.  The host-buffer entry points of one context queue their uploads and kernels on that
 * one stream, in order; the decoded frames of amvhip_decode_batch_async come back on a second stream of the context
 * (so that the copy of one call runs beside the upload and the kernels of the next).  The results of an *_async call
 * are therefore complete only after amvhip_sync, which waits for both streams -- not after some other blocking
 * host-buffer call (the blocking encode and ADPCM entry points synchronise the first stream alone).
 */
int amvhip_decode_batch_async(amvhip_ctx *ctx, const uint8_t *blob, uint64_t blob_bytes,
                              const uint64_t *offs, const uint32_t *lens, uint32_t n,
                              uint32_t width, uint32_t height, uint32_t flags,
                              uint8_t *out, int32_t *status);
int amvhip_sync(amvhip_ctx *ctx);
int amvhip_host_alloc(amvhip_ctx *ctx, void **p, size_t bytes);
void amvhip_host_free(amvhip_ctx *ctx, void *p);

/* Entropy-stage kernel choice.  AUTO: several lanes per frame (self-synchronising parallel Huffman
 * decode); frames whose chunk does not fit its workspace window fall to the one-lane-per-frame kernel.
 * SERIAL: always the one-lane-per-frame kernel.  Results are identical; the switch exists so the
 * parity tests cover both kernels. */
#define AMVHIP_ENTROPY_AUTO 0
#define AMVHIP_ENTROPY_SERIAL 1
int amvhip_set_entropy_mode(amvhip_ctx *ctx, int mode);
/* Diagnostics of the synchronising entropy kernel: synchronises the device, returns the counters
 * gathered since the last call in out[] = {frames, sum of synchronisation rounds, max rounds, frames the LAST decode
 * call handed to the one-lane-per-frame kernel (always reported, whether gathering is on or not),
 * then shader clocks summed over waves for: coefficient zeroing, first walk, synchronisation
 * rounds, writing pass, DC pass, the number of waves, and the frames that left the entropy stage marked as carrying an
 * AC coefficient of ten magnitude bits or more (the reconstruction takes its general row pass for those)}, clears them
 * and switches gathering on or off (off by default; costs a few atomics per frame). */
int amvhip_entropy_stats(amvhip_ctx *ctx, int enable, uint64_t out[11]);
/* ... and, per task (wave) of the last launch of the several-lanes-per-frame kernel while gathering was on, a line of
 * eight words: {constant-rate clock (100 MHz) at the task's begin, at its end, shader clocks of the first walk, the
 * synchronisation rounds, the strict pass, the DC pass, rounds of the wave's worst frame | share length in bits << 32,
 * workgroup << 32 | wave << 16 | lanes per frame}.  out: 8 * tasks words; returns the lines copied (< 0: error).  Lines behind
 * the launch's tasks are zero when no launch since gathering went on had more (amvhip_entropy_stats clears them then).
 * The one-lane-per-frame kernel writes the same line per task of 64 frames, with {shader clocks of the task, strides of its
 * longest frame, 0, HW_ID | XCC_ID << 32 (the SIMD the wave ran on is bits 4-5), 0} in words 2 - 6 and 1 as its lanes per frame.
 * What a launch one generation of waves deep lasts as long as: its slowest task (tools/time_kernels.py --trace). */
int amvhip_entropy_trace(amvhip_ctx *ctx, uint64_t *out, uint32_t tasks);
/* A batch large enough to give every frame ONE entropy lane (a wave's 64 frames then finish together) gives the frames
 * whose chunk is over twice the batch's mean chunk several lanes each instead -- the split is made on the device, from
 * d_lens.  out[] = {frames of the LAST decode call that went the several-lanes way, frames that went one lane per frame};
 * {0, 0} when the call made no split (a smaller batch: every frame has several lanes anyway).  Synchronises the device.
 * No analogue in the reference (its decoder takes one frame at a time, AMVDec.c:259). */
int amvhip_decode_split_stats(amvhip_ctx *ctx, uint32_t out[2]);

/* Stage access for parity tests: entropy stage only, the same kernels amvhip_decode_batch_dev runs.  d_coef: n * nmcu*6*64
 * int16, DC-predicted quantised coefficients in bitstream order (amvlib MCUBuffer, AmvJpeg.c:1200-1223); d_nmcu_ok: MCUs
 * decoded before the first error.  Every line of every frame is written.  Lines of MCUs before d_nmcu_ok[i] are the
 * decoder's; lines at or after it are unspecified (frames that go through the serial kernel keep the failing block's
 * partial values there, the others zeros).  Nothing reads them: amvhip_reconstruct_dev stops at d_nmcu_ok[i]. */
int amvhip_huffman_decode_dev(amvhip_ctx *ctx, const uint8_t *d_blob, uint64_t blob_bytes,
                              const uint64_t *d_offs, const uint32_t *d_lens, uint32_t n,
                              uint32_t width, uint32_t height,
                              int16_t *d_coef, int32_t *d_status, uint32_t *d_nmcu_ok, void *stream);
/* Stage access: dequantise + IDCT + colour + store from coefficients
 * (IQtIZzBlock/Fast_IDCT/GetYUV/StoreBuffer, AmvJpeg.c:1010-1059,754-840).
 * For which coefficients the frame is the reference's, byte for byte:
 *   - AMVHIP_FLAG_FFMPEG: every int16 value at every place (the reference's int16 stores wrap, and so do the kernel's);
 *   - the amvlib modes (flags 0, AMVHIP_FLAG_ZIGZAG_FIXED): the DC any int16 and every AC coefficient c at scan position s
 *     with |c * step[s]| <= 100 000 (step: the amvlib quantiser tables, AmvJpeg.c:30-61).  That holds everything a scan
 *     can carry (|AC| <= 1023, steps <= 61), so everything amvhip_huffman_decode_dev hands out.  Beyond it the reference's
 *     all-AC-zero IDCT shortcuts (AmvJpeg.c:1087-1092, 1134-1140) keep 32-bit values where the kernel's general formula
 *     wraps, and the pixels of such a BLOCK (its 8x8 luma samples, or the 16x16 pixels under a chroma block) may differ
 *     from the reference's.  Every byte of the frame is written all the same, every pixel is a clamped 0..255 value, and
 *     no other block, frame or byte outside the frame's rows is affected. */
int amvhip_reconstruct_dev(amvhip_ctx *ctx, const int16_t *d_coef, const uint32_t *d_nmcu_ok,
                           uint32_t n, uint32_t width, uint32_t height, uint32_t flags,
                           uint8_t *d_out, void *stream);

/*
 * Video encode, device-resident.  Replaces amv_encode_picture + the RGB front end
 * (mjpegenc.c:454-472, imgconvert_template.h:654, mpegvideo_enc.c:3647, mjpegenc.c:379-450,
 * :282-355) over n frames.
 *   d_pix      : n frames, RGB24 (is_bgr=0) or BGR24 (is_bgr=1), top-down, pix_stride bytes/row,
 *                frame i at d_pix + i*pix_stride*height; width and height must be even
 *   d_blob     : output of blob_cap bytes; chunks are written back to back in frame order.
 *                n * amvhip_encode_bound(w,h) always suffices (real streams run at ~0.2 byte per pixel).
 *                A chunk that would end past blob_cap is NOT written and its d_lens entry is 0 (d_offs still
 *                says where it would have started): a consumer checks d_lens[i] != 0.  The host-buffer forms
 *                return AMVHIP_ERR_SPACE instead.
 *   d_offs/d_lens : n entries written
 */
int amvhip_encode_batch_dev(amvhip_ctx *ctx, const uint8_t *d_pix, uint32_t pix_stride, int is_bgr,
                            uint32_t n, uint32_t width, uint32_t height, uint32_t qbias,
                            uint8_t *d_blob, uint64_t blob_cap, uint64_t *d_offs, uint32_t *d_lens,
                            void *stream);
int amvhip_encode_batch(amvhip_ctx *ctx, const uint8_t *pix, uint32_t pix_stride, int is_bgr,
                        uint32_t n, uint32_t width, uint32_t height, uint32_t qbias,
                        uint8_t *blob, uint64_t blob_cap, uint64_t *offs, uint32_t *lens);
/*
 * The same from planar YUVJ420P, the pixel format the reference's amv_encoder declares and takes
 * (mjpegenc.c:485-494 pix_fmts; amv_encode_picture :454-472 flips it by negative linesize; get_pixels
 * mpegvideo_enc.c:1539-1549): no colour conversion, otherwise the path above.  Frame i's planes start at
 * d_y + i*y_frame_stride and d_cb/d_cr + i*c_frame_stride (bytes), rows y_stride / c_stride apart; chroma planes
 * are (w/2) x (h/2).  rgb24_to_yuvj420p followed by this entry equals amvhip_encode_batch_dev bit for bit.
 */
int amvhip_encode_yuv420_batch_dev(amvhip_ctx *ctx, const uint8_t *d_y, const uint8_t *d_cb, const uint8_t *d_cr,
                                   uint32_t y_stride, uint32_t c_stride, uint64_t y_frame_stride,
                                   uint64_t c_frame_stride, uint32_t n, uint32_t width, uint32_t height,
                                   uint32_t qbias, uint8_t *d_blob, uint64_t blob_cap, uint64_t *d_offs,
                                   uint32_t *d_lens, void *stream);
int amvhip_encode_yuv420_batch(amvhip_ctx *ctx, const uint8_t *y, const uint8_t *cb, const uint8_t *cr,
                               uint32_t y_stride, uint32_t c_stride, uint64_t y_frame_stride,
                               uint64_t c_frame_stride, uint32_t n, uint32_t width, uint32_t height,
                               uint32_t qbias, uint8_t *blob, uint64_t blob_cap, uint64_t *offs, uint32_t *lens);
/*
 * Trellis quantisation, the video side of the reference's -trellis / -flags trell (dct_quantize_trellis_c,
 * mpegvideo_enc.c:2961-3247): per 8x8 block, the AC levels that minimise distortion + lambda * bits, where the bits are
 * those of AMV's fixed AC code itself (run/size code, magnitude bits, ZRL, and the end-of-block code when one is written)
 * and the distortion is measured against what every AMV decoder reconstructs (level * Q).  The candidates per
 * coefficient are the plain quantiser's level and the one below it (the level 1 for a coefficient under the threshold
 * that lies below the block's last one above it).  The DC is quantised as ever; entropy coding is unchanged, so every
 * decoder of the plain entries' chunks decodes these.  Arguments and the blob-capacity rule are those of
 * amvhip_encode_batch(_dev) / amvhip_encode_yuv420_batch(_dev), and:
 *   lambda : the weight of a bit against squared error in the fdct's scale (8 x the sample's).  0 is legal (distortion
 *            alone decides; not the plain quantiser: it still may code a 1 under the threshold, or the level below).
 *            amvhip_encode_trellis_lambda(qscale) is the reference's value for a -qscale (3481 at 8, the scale AMV's
 *            tables correspond to; 0 where that is above the bound).  More than amvhip_encode_trellis_lambda_max() is
 *            refused (AMVHIP_ERR_ARG): beyond it the search's int scores could wrap.
 * Both entropy modes give the same bytes.
 */
uint32_t amvhip_encode_trellis_lambda_max(void);
uint32_t amvhip_encode_trellis_lambda(uint32_t qscale);
int amvhip_encode_trellis_batch_dev(amvhip_ctx *ctx, const uint8_t *d_pix, uint32_t pix_stride, int is_bgr,
                                    uint32_t n, uint32_t width, uint32_t height, uint32_t qbias, uint32_t lambda,
                                    uint8_t *d_blob, uint64_t blob_cap, uint64_t *d_offs, uint32_t *d_lens, void *stream);
int amvhip_encode_trellis_batch(amvhip_ctx *ctx, const uint8_t *pix, uint32_t pix_stride, int is_bgr,
                                uint32_t n, uint32_t width, uint32_t height, uint32_t qbias, uint32_t lambda,
                                uint8_t *blob, uint64_t blob_cap, uint64_t *offs, uint32_t *lens);
int amvhip_encode_yuv420_trellis_batch_dev(amvhip_ctx *ctx, const uint8_t *d_y, const uint8_t *d_cb, const uint8_t *d_cr,
                                           uint32_t y_stride, uint32_t c_stride, uint64_t y_frame_stride,
                                           uint64_t c_frame_stride, uint32_t n, uint32_t width, uint32_t height,
                                           uint32_t qbias, uint32_t lambda, uint8_t *d_blob, uint64_t blob_cap,
                                           uint64_t *d_offs, uint32_t *d_lens, void *stream);
int amvhip_encode_yuv420_trellis_batch(amvhip_ctx *ctx, const uint8_t *y, const uint8_t *cb, const uint8_t *cr,
                                       uint32_t y_stride, uint32_t c_stride, uint64_t y_frame_stride,
                                       uint64_t c_frame_stride, uint32_t n, uint32_t width, uint32_t height,
                                       uint32_t qbias, uint32_t lambda, uint8_t *blob, uint64_t blob_cap, uint64_t *offs,
                                       uint32_t *lens);
/*
 * The reference's -nr N noise reduction (denoise_dct_c, mpegvideo_enc.c:2937-2959; update_noise_reduction,
 * mpegvideo.c:861-876) for a stream coded in calls of any size: a dead zone in the DCT domain, between fdct and
 * quantiser, whose width adapts per coefficient position to the running mean magnitude of the stream.  The one lever
 * on size against detail that works with AMV's fixed quantiser tables.  Arguments as amvhip_encode_yuv420_batch(_dev) /
 * amvhip_encode_batch(_dev), and:
 *   nr       : the reference's avctx->noise_reduction.  0: the bytes of the plain entry, the state left as it was (the
 *              reference allocates nothing then, mpegvideo.c:318, :520).  More than amvhip_encode_nr_max(width, height)
 *              is refused (AMVHIP_ERR_ARG): beyond it the reference's int arithmetic would wrap.
 *   d_state  : int32[65] on the device (state: the same in host memory), 4-byte aligned: dct_error_sum[64] in the
 *              reference's index order (the fdct output's row-major order; the six blocks of an MCU share the array), then
 *              dct_count.  Read at entry, written at exit; all zeros starts a stream.  The layout is part of the contract:
 *              a caller may save and restore it.  n frames in one call equal the same frames in any number of calls with
 *              the state carried, byte for byte.  A state the caller made up (negative sums, a count no stream of this
 *              frame size reaches) gives unspecified bytes and state, but no access out of range.
 * The blob-capacity rule is the plain entries'.  The arithmetic is the reference's bit for bit, the offset's truncation to
 * 16 bits included; this encoder's fdct runs on samples - 128, so the DC enters the sums and the dead zone as DC + 8192,
 * which is the reference's DC exactly.
 */
uint32_t amvhip_encode_nr_max(uint32_t width, uint32_t height);   /* 0: no nr but 0 at this size (the frame is too large) */
int amvhip_encode_yuv420_nr_stream_dev(amvhip_ctx *ctx, const uint8_t *d_y, const uint8_t *d_cb, const uint8_t *d_cr,
                                       uint32_t y_stride, uint32_t c_stride, uint64_t y_frame_stride,
                                       uint64_t c_frame_stride, uint32_t n, uint32_t width, uint32_t height,
                                       uint32_t qbias, uint32_t nr, int32_t *d_state, uint8_t *d_blob, uint64_t blob_cap,
                                       uint64_t *d_offs, uint32_t *d_lens, void *stream);
int amvhip_encode_yuv420_nr_stream(amvhip_ctx *ctx, const uint8_t *y, const uint8_t *cb, const uint8_t *cr,
                                   uint32_t y_stride, uint32_t c_stride, uint64_t y_frame_stride,
                                   uint64_t c_frame_stride, uint32_t n, uint32_t width, uint32_t height,
                                   uint32_t qbias, uint32_t nr, int32_t *state, uint8_t *blob, uint64_t blob_cap,
                                   uint64_t *offs, uint32_t *lens);
int amvhip_encode_nr_stream_dev(amvhip_ctx *ctx, const uint8_t *d_pix, uint32_t pix_stride, int is_bgr,
                                uint32_t n, uint32_t width, uint32_t height, uint32_t qbias, uint32_t nr,
                                int32_t *d_state, uint8_t *d_blob, uint64_t blob_cap, uint64_t *d_offs,
                                uint32_t *d_lens, void *stream);
int amvhip_encode_nr_stream(amvhip_ctx *ctx, const uint8_t *pix, uint32_t pix_stride, int is_bgr,
                            uint32_t n, uint32_t width, uint32_t height, uint32_t qbias, uint32_t nr,
                            int32_t *state, uint8_t *blob, uint64_t blob_cap, uint64_t *offs, uint32_t *lens);
/*
 * Both levers in one call, `ffmpeg -nr N -trellis 1`: dct_quantize_trellis_c calls denoise_dct right behind the fdct
 * (mpegvideo_enc.c:2987-2990) and searches on what comes out.  Here too: the sums are taken of the fdct's outputs, the dead
 * zone is applied, the DC is quantised as ever, and the trellis search of the entries above runs on the denoised AC outputs.
 * Arguments are those of the -nr stream entries with `lambda` directly behind `nr`, each with its own entry's meaning and
 * bound:
 *   nr      : more than amvhip_encode_nr_max(width, height) is refused.  0: the bytes of the trellis entry, the state left
 *             as it was (and not looked at: it may be NULL).
 *   lambda  : more than amvhip_encode_trellis_lambda_max() is refused (denoising only shrinks magnitudes, so the bound
 *             stands).  0 is the trellis at lambda 0, not the plain quantiser.
 *   d_state : as in the -nr entries, and the same state: the sums do not depend on the quantiser behind them, so a stream
 *             may change between the -nr entries and these from call to call.  n frames in one call equal the same frames
 *             in any number of calls with the state carried, byte for byte.
 * The blob-capacity rule is the plain entries'.  Both entropy modes give the same bytes.
 */
int amvhip_encode_yuv420_nr_trellis_stream_dev(amvhip_ctx *ctx, const uint8_t *d_y, const uint8_t *d_cb, const uint8_t *d_cr,
                                               uint32_t y_stride, uint32_t c_stride, uint64_t y_frame_stride,
                                               uint64_t c_frame_stride, uint32_t n, uint32_t width, uint32_t height,
                                               uint32_t qbias, uint32_t nr, uint32_t lambda, int32_t *d_state, uint8_t *d_blob,
                                               uint64_t blob_cap, uint64_t *d_offs, uint32_t *d_lens, void *stream);
int amvhip_encode_yuv420_nr_trellis_stream(amvhip_ctx *ctx, const uint8_t *y, const uint8_t *cb, const uint8_t *cr,
                                           uint32_t y_stride, uint32_t c_stride, uint64_t y_frame_stride,
                                           uint64_t c_frame_stride, uint32_t n, uint32_t width, uint32_t height,
                                           uint32_t qbias, uint32_t nr, uint32_t lambda, int32_t *state, uint8_t *blob,
                                           uint64_t blob_cap, uint64_t *offs, uint32_t *lens);
int amvhip_encode_nr_trellis_stream_dev(amvhip_ctx *ctx, const uint8_t *d_pix, uint32_t pix_stride, int is_bgr,
                                        uint32_t n, uint32_t width, uint32_t height, uint32_t qbias, uint32_t nr,
                                        uint32_t lambda, int32_t *d_state, uint8_t *d_blob, uint64_t blob_cap,
                                        uint64_t *d_offs, uint32_t *d_lens, void *stream);
int amvhip_encode_nr_trellis_stream(amvhip_ctx *ctx, const uint8_t *pix, uint32_t pix_stride, int is_bgr,
                                    uint32_t n, uint32_t width, uint32_t height, uint32_t qbias, uint32_t nr,
                                    uint32_t lambda, int32_t *state, uint8_t *blob, uint64_t blob_cap, uint64_t *offs,
                                    uint32_t *lens);
/*
 * ... and from planar YUVJ422P, the other pixel format amv_encoder declares (mjpegenc.c:493; chroma planes (w/2) x h,
 * mpegvideo_enc.c:534-543 h/v sampling 2x2 : 1x2).  The reference would code such a picture as MCUs of eight blocks
 * (ff_mjpeg_encode_mb, mjpegenc.c:437-450, the CHROMA_420 test failing) -- a scan no AMV decoder can read: the container
 * has no frame header, and both amvlib (AmvJpeg.c:1406-1420) and the reference's own amv decoder (sp5xdec.c:51-91, a
 * fixed 4:2:0 SOF) take six blocks per MCU.  Here the two chroma rows over every 4:2:0 sample are averaged ((a + b + 1)
 * >> 1) and the picture is coded as above: a valid AMV chunk.  Arguments as amvhip_encode_yuv420_batch(_dev).
 */
int amvhip_encode_yuv422_batch_dev(amvhip_ctx *ctx, const uint8_t *d_y, const uint8_t *d_cb, const uint8_t *d_cr,
                                   uint32_t y_stride, uint32_t c_stride, uint64_t y_frame_stride,
                                   uint64_t c_frame_stride, uint32_t n, uint32_t width, uint32_t height,
                                   uint32_t qbias, uint8_t *d_blob, uint64_t blob_cap, uint64_t *d_offs,
                                   uint32_t *d_lens, void *stream);
int amvhip_encode_yuv422_batch(amvhip_ctx *ctx, const uint8_t *y, const uint8_t *cb, const uint8_t *cr,
                               uint32_t y_stride, uint32_t c_stride, uint64_t y_frame_stride,
                               uint64_t c_frame_stride, uint32_t n, uint32_t width, uint32_t height,
                               uint32_t qbias, uint8_t *blob, uint64_t blob_cap, uint64_t *offs, uint32_t *lens);
/*
 * The picture rescaler in front of the encoder: img_resample (libavcodec/imgresample.c:474-495), the arithmetic of
 * the sws_scale shim (:599) ffmpeg.c:757 runs when the source is not the target size (AMVmuxer/Makefile:15-17 asks for
 * -s 160x120): four-tap, 16-phase polyphase filter built as av_build_filter does (resample2.c:93-140), horizontal pass
 * into bytes, vertical pass over four such lines, edges repeated; the luma increments and filters also serve the
 * chroma planes, which are (w >> 1) x (h >> 1).  YUV420P frames in, YUV420P frames out, plane layout as in
 * amvhip_encode_yuv420_batch_dev; at most 65535 frames per call.  Byte-identical to the reference's routine.
 * A source from 2 x 2 on is taken.  For a source plane narrower than the four taps (source width below 4, chroma below 8)
 * the reference's h_resample is undefined at imgresample.c:339-341 (its count of fast columns goes negative and steps
 * the destination back), and the library repeats the edge sample, there as at every other edge.
 */
int amvhip_resample_yuv420_dev(amvhip_ctx *ctx, const uint8_t *d_src_y, const uint8_t *d_src_cb, const uint8_t *d_src_cr,
                               uint32_t src_y_stride, uint32_t src_c_stride, uint64_t src_y_frame_stride,
                               uint64_t src_c_frame_stride, uint32_t src_width, uint32_t src_height,
                               uint8_t *d_dst_y, uint8_t *d_dst_cb, uint8_t *d_dst_cr,
                               uint32_t dst_y_stride, uint32_t dst_c_stride, uint64_t dst_y_frame_stride,
                               uint64_t dst_c_frame_stride, uint32_t dst_width, uint32_t dst_height, uint32_t n, void *stream);
/* rescale to width x height, then encode: one call for ffmpeg.c's sws_scale + avcodec_encode_video pair (:757-814).  Of the
 * shim this is the case without a conversion on either side: the bytes of the YUV420P source go rescaled to the encoder as
 * they are.  amvhip_encode_fmt_scaled_batch_dev runs the whole shim, the conversions in front and the range step behind. */
int amvhip_encode_yuv420_scaled_batch_dev(amvhip_ctx *ctx, const uint8_t *d_y, const uint8_t *d_cb, const uint8_t *d_cr,
                                          uint32_t y_stride, uint32_t c_stride, uint64_t y_frame_stride,
                                          uint64_t c_frame_stride, uint32_t src_width, uint32_t src_height, uint32_t n,
                                          uint32_t width, uint32_t height, uint32_t qbias, uint8_t *d_blob,
                                          uint64_t blob_cap, uint64_t *d_offs, uint32_t *d_lens, void *stream);
/*
 * Pixel formats on both sides of the codec: img_convert (libavcodec/imgconvert.c:2329-2571) for the formats that meet the
 * AMV codec, as the sws_scale shim (imgresample.c:599-690) runs it in front of img_resample (a decoder's format ->
 * YUV420P, :619-643) and behind it (YUV420P -> the encoder's YUVJ420P, :671-680), and as `ffmpeg -i x.amv -pix_fmt ...`
 * runs it behind the AMV decoder.  Byte for byte the reference's arithmetic: the 10-bit FIX() constants of
 * colorspace.h:30-109, the cm clamp, the 2x2 sums and shifts of imgconvert_template.h, the four 256-entry range tables
 * (imgconvert.c:1216-1233) applied to the destination.
 *
 * AMVHIP_PIX_RGB32 is the reference's native-endian 32-bit word (a << 24 | r << 16 | g << 8 | b): B G R A in memory here;
 * RGB565 / RGB555 are native 16-bit words.  Planar formats use three planes, every other format plane 0 alone (pass NULL,
 * 0, 0 for the rest).  A picture is handed over flat, as in amvhip_resample_yuv420_dev: plane pointers, the row pitch of
 * plane 0 and of the chroma planes, the frame pitch of plane 0 and of the chroma planes (bytes); frame i's planes start
 * i frame pitches on.  Plane pointers must be 4-byte aligned.  No byte beyond a row's bytes and no row beyond the
 * picture's height is written: pictures may be strided.  Deinterlacing (avpicture_deinterlace), cropping (av_picture_crop,
 * ffmpeg.c:730-738) and padding (av_picture_pad) are amvhip_video_frontend_dev's, further down.  The -r frame duplication /
 * dropping of ffmpeg.c:705-728 is not offered.
 *
 * A (src, dst) pair is supported when the reference reaches it in ONE step -- a routine of convert_table
 * (imgconvert.c:1940-2190), the planar route (:2415-2513: luma copied, chroma through ff_img_copy_plane / shrink12 /
 * ff_shrink22, then the range tables) or the gray route (:2399-2413):
 *   towards the encoder   YUVJ420P, YUV422P, YUVJ422P, YUV444P, YUVJ444P -> YUV420P and -> YUVJ420P;  YUV420P -> YUVJ420P;
 *                         YUYV422, UYVY422, RGB24, BGR24, RGB32 -> YUV420P;  RGB24 -> YUVJ420P (the routine the encoder
 *                         fuses: this entry followed by amvhip_encode_yuv420_batch_dev equals amvhip_encode_batch_dev)
 *   from the decoder      YUVJ420P, YUV420P -> RGB24, BGR24, RGB32, RGB565, RGB555, GRAY8;  YUVJ420P -> YUV420P;
 *                         YUV420P -> YUYV422, UYVY422
 * Every other pair -- the same format twice; anything the reference reaches only through an intermediate picture
 * (:2514-2571), such as YUYV422 / UYVY422 / BGR24 / RGB32 -> YUVJ420P, YUVJ420P -> YUYV422 / UYVY422, RGB <-> RGB, any
 * source that is RGB565 / RGB555 / GRAY8, any 4:2:2 or 4:4:4 destination -- returns AMVHIP_ERR_ARG
 * (amvhip_img_convert_supported tells, for a picture size, without a context or a device: 1 = the pair is offered at that size).
 * Sizes: the routes into 4:2:0 from another sampling or from a packed / RGB format, and YUV420P -> YUYV422 / UYVY422, want
 * even width and height (AMVHIP_ERR_ARG otherwise, as the encoder demands).  The routes out of 4:2:0 planes into RGB / GRAY8
 * and between the two 4:2:0 formats take every size the decoder takes: chroma planes (w + 1) / 2 x (h + 1) / 2, the last
 * column and row serving one pixel (the routines' tail code).  Between the two 4:2:0 formats the whole chroma planes are
 * converted; the reference's planar route stops at w >> 1 x h >> 1 and leaves an odd picture's last chroma column and row
 * as the destination had them.
 *
 * amvhip_img_convert_dev   n frames, device-resident, asynchronous on `stream`
 * amvhip_img_convert       the same with host buffers (rows staged tight, converted, copied back row by row; synchronous)
 * amvhip_pix_frame_bytes   bytes of one frame whose planes lie back to back with rows `stride` apart (chroma rows
 *                          (stride + 1) / 2 apart, or `stride` for 4:4:4): the layout amvhip_decode_fmt_batch_dev writes
 */
#define AMVHIP_PIX_YUV420P 0
#define AMVHIP_PIX_YUVJ420P 1
#define AMVHIP_PIX_YUV422P 2
#define AMVHIP_PIX_YUVJ422P 3
#define AMVHIP_PIX_YUV444P 4
#define AMVHIP_PIX_YUVJ444P 5
#define AMVHIP_PIX_YUYV422 6
#define AMVHIP_PIX_UYVY422 7
#define AMVHIP_PIX_RGB24 8
#define AMVHIP_PIX_BGR24 9
#define AMVHIP_PIX_RGB32 10
#define AMVHIP_PIX_RGB565 11
#define AMVHIP_PIX_RGB555 12
#define AMVHIP_PIX_GRAY8 13
#define AMVHIP_PIX_COUNT 14
int amvhip_img_convert_supported(int src_fmt, int dst_fmt, uint32_t width, uint32_t height);
uint64_t amvhip_pix_frame_bytes(int fmt, uint32_t stride, uint32_t height);
int amvhip_img_convert_dev(amvhip_ctx *ctx, int src_fmt, const uint8_t *d_src0, const uint8_t *d_src1, const uint8_t *d_src2,
                           uint32_t src_stride, uint32_t src_c_stride, uint64_t src_frame_stride, uint64_t src_c_frame_stride,
                           int dst_fmt, uint8_t *d_dst0, uint8_t *d_dst1, uint8_t *d_dst2,
                           uint32_t dst_stride, uint32_t dst_c_stride, uint64_t dst_frame_stride, uint64_t dst_c_frame_stride,
                           uint32_t width, uint32_t height, uint32_t n, void *stream);
int amvhip_img_convert(amvhip_ctx *ctx, int src_fmt, const uint8_t *src0, const uint8_t *src1, const uint8_t *src2,
                       uint32_t src_stride, uint32_t src_c_stride, uint64_t src_frame_stride, uint64_t src_c_frame_stride,
                       int dst_fmt, uint8_t *dst0, uint8_t *dst1, uint8_t *dst2,
                       uint32_t dst_stride, uint32_t dst_c_stride, uint64_t dst_frame_stride, uint64_t dst_c_frame_stride,
                       uint32_t width, uint32_t height, uint32_t n);
/*
 * The shim as one call: sws_scale (imgresample.c:599-690).  Sizes differ: img_convert to YUV420P when the source is not
 * YUV420P (:619-643), img_resample (amvhip_resample_yuv420_dev's kernel), img_convert to dst_fmt when that is not YUV420P
 * (:671-680; towards YUVJ420P the range tables are applied where the rescaler stores its bytes).  Sizes equal: one
 * img_convert, or a plane copy when the formats are equal too (av_picture_copy, :681-684).  Each conversion must be a
 * supported pair at its size (AMVHIP_ERR_ARG otherwise); a rescaled picture is at least 2 x 2.  The pictures in between
 * live in the context's workspace, grown on demand.  An odd destination size behind the rescaler: img_resample writes
 * (w >> 1) x (h >> 1) chroma samples.  Into YUV420P / YUVJ420P the last chroma column and row of the caller's planes are
 * then left as they were (undefined in the reference too); towards the RGB formats the routine reads
 * those samples, which the reference leaves undefined and which are 128 here: the picture's last column and row come out
 * without colour (GRAY8 reads no chroma; YUYV422 / UYVY422 want even sizes).  A narrow source: for a source plane narrower
 * than the four taps (source width below 4, chroma below 8) the reference's h_resample is undefined at
 * imgresample.c:339-341, and the library repeats the edge sample (see amvhip_resample_yuv420_dev).
 */
int amvhip_sws_scale_dev(amvhip_ctx *ctx, int src_fmt, const uint8_t *d_src0, const uint8_t *d_src1, const uint8_t *d_src2,
                         uint32_t src_stride, uint32_t src_c_stride, uint64_t src_frame_stride, uint64_t src_c_frame_stride,
                         uint32_t src_width, uint32_t src_height,
                         int dst_fmt, uint8_t *d_dst0, uint8_t *d_dst1, uint8_t *d_dst2,
                         uint32_t dst_stride, uint32_t dst_c_stride, uint64_t dst_frame_stride, uint64_t dst_c_frame_stride,
                         uint32_t dst_width, uint32_t dst_height, uint32_t n, void *stream);
/*
 * Front end + encoder in one call: ffmpeg.c:757-814 for any supported source -- the shim to YUVJ420P at width x height, then
 * the encoder (arguments as amvhip_encode_yuv420_scaled_batch_dev).  At another size the range step is part of the
 * rescaler's store, not a pass over memory.  At the target size RGB24 and BGR24 (frames back to back) take
 * amvhip_encode_batch_dev's path and YUVJ420P takes amvhip_encode_yuv420_batch_dev's, byte for byte; the other sources
 * need a one-step route to YUVJ420P there.
 */
int amvhip_encode_fmt_scaled_batch_dev(amvhip_ctx *ctx, int src_fmt, const uint8_t *d_src0, const uint8_t *d_src1, const uint8_t *d_src2,
                                       uint32_t src_stride, uint32_t src_c_stride, uint64_t src_frame_stride,
                                       uint64_t src_c_frame_stride, uint32_t src_width, uint32_t src_height, uint32_t n,
                                       uint32_t width, uint32_t height, uint32_t qbias, uint8_t *d_blob, uint64_t blob_cap,
                                       uint64_t *d_offs, uint32_t *d_lens, void *stream);
/*
 * The rest of ffmpeg's video front end: -deinterlace (pre_process_video_frame, ffmpeg.c:579-623), -crop*, -pad* and
 * -padcolor (do_video_out, :730-765), around the shim above.  The stages run in the reference's order, each byte for byte
 * its own: deinterlace at the source size and format, crop, sws_scale into the window of the padded picture, the bands.
 *
 * Deinterlace (avpicture_deinterlace, imgconvert.c:2673-2864, the C branch): per plane, even rows copied, odd row 2k + 1 =
 * clamp((-r[2k-1] + 4 r[2k] + 2 r[2k+1] + 4 r[2k+2] - r[2k+3] + 4) >> 3) with r[-1] = r[0] and, for the last row, both rows
 * below it the row itself.  Accepted for YUV420P, YUV422P, YUV444P and GRAY8 with width and height multiples of 4
 * (amvhip_deinterlace_supported; no context or device needed) -- the YUVJ formats are not in the reference's list.
 * amvhip_deinterlace_dev / amvhip_deinterlace (host buffers, synchronous) are the stage alone: one format for both
 * sides, pictures flat as in amvhip_img_convert_dev; anything else than the list returns AMVHIP_ERR_ARG, and so do source
 * and destination that overlap (the reference's in-place form, :2794-2817, gives the same bytes as its out-of-place one, so
 * nothing is lost).  ffmpeg.c:602-608 goes on without deinterlacing when the routine refuses: amvhip_video_frontend_dev
 * does the same, a caller of the stage alone asks amvhip_deinterlace_supported first.
 *
 * Crop (av_picture_crop, :2224-2244): planar YUV sources only (AMVHIP_ERR_ARG otherwise), plane origins moved by
 * top, left (chroma: >> the format's shifts).  Behind a deinterlace only the kept rows and columns are computed.
 * Pad (av_picture_pad, :2246-2304): the encoder's picture is width x height, the rescaler's target the window
 * (width - pad_left - pad_right) x (height - pad_top - pad_bottom) inside it; the bands of plane i are the byte pad_color[i]
 * written unconverted into the YUVJ420P planes ({16, 128, 128} is ffmpeg's default; amvhip_pad_color_from_rgb is
 * -padcolor RRGGBB's arithmetic, ffmpeg.c:2246-2271).  The result is defined for every combination: the window is the
 * rescaled (or, sizes and format equal, copied) picture, every other byte the colour.  The reference is that too, except with
 * crop + pad and no rescale, where its row copy takes the uncropped pitch and runs past the window (and, without a bottom or
 * right band, past the buffer): there it is not a function of its input, and the clean result is ours.
 *
 * All bands are even (AMVHIP_ERR_ARG), leave at least 2 x 2 of the source and of the window, and the shim must have a
 * route from src_fmt at the cropped size to YUVJ420P at the window's size.  fe == NULL: every field zero.
 *
 * amvhip_video_frontend_dev         n YUVJ420P pictures of width x height (even) into the caller's planes
 * amvhip_encode_frontend_batch_dev  the same into the context's workspace, then the encoder; with fe NULL or all zero it IS
 *                                   amvhip_encode_fmt_scaled_batch_dev (its fused RGB24 / BGR24 and direct YUVJ420P routes too);
 *                                   a blob too small is reported as there: the chunks that do not fit have length 0
 */
typedef struct amvhip_frontend {
    uint32_t deinterlace;                                    /* 0 / 1 */
    uint32_t crop_top, crop_bottom, crop_left, crop_right;   /* source pixels, even */
    uint32_t pad_top, pad_bottom, pad_left, pad_right;       /* encoder pixels, even */
    uint8_t pad_color[3];                                    /* Y, Cb, Cr as written; {16,128,128} is ffmpeg's default */
} amvhip_frontend;
void amvhip_pad_color_from_rgb(uint32_t rrggbb, uint8_t out[3]);
int amvhip_deinterlace_supported(int fmt, uint32_t width, uint32_t height);
int amvhip_deinterlace_dev(amvhip_ctx *ctx, int fmt, const uint8_t *d_src0, const uint8_t *d_src1, const uint8_t *d_src2,
                           uint32_t src_stride, uint32_t src_c_stride, uint64_t src_frame_stride, uint64_t src_c_frame_stride,
                           uint8_t *d_dst0, uint8_t *d_dst1, uint8_t *d_dst2,
                           uint32_t dst_stride, uint32_t dst_c_stride, uint64_t dst_frame_stride, uint64_t dst_c_frame_stride,
                           uint32_t width, uint32_t height, uint32_t n, void *stream);
int amvhip_deinterlace(amvhip_ctx *ctx, int fmt, const uint8_t *src0, const uint8_t *src1, const uint8_t *src2,
                       uint32_t src_stride, uint32_t src_c_stride, uint64_t src_frame_stride, uint64_t src_c_frame_stride,
                       uint8_t *dst0, uint8_t *dst1, uint8_t *dst2,
                       uint32_t dst_stride, uint32_t dst_c_stride, uint64_t dst_frame_stride, uint64_t dst_c_frame_stride,
                       uint32_t width, uint32_t height, uint32_t n);
int amvhip_video_frontend_dev(amvhip_ctx *ctx, int src_fmt, const uint8_t *d_src0, const uint8_t *d_src1, const uint8_t *d_src2,
                              uint32_t src_stride, uint32_t src_c_stride, uint64_t src_frame_stride, uint64_t src_c_frame_stride,
                              uint32_t src_width, uint32_t src_height, uint32_t n, const amvhip_frontend *fe,
                              uint8_t *d_y, uint8_t *d_cb, uint8_t *d_cr, uint32_t y_stride, uint32_t c_stride,
                              uint64_t y_frame_stride, uint64_t c_frame_stride, uint32_t width, uint32_t height, void *stream);
int amvhip_encode_frontend_batch_dev(amvhip_ctx *ctx, int src_fmt, const uint8_t *d_src0, const uint8_t *d_src1, const uint8_t *d_src2,
                                     uint32_t src_stride, uint32_t src_c_stride, uint64_t src_frame_stride,
                                     uint64_t src_c_frame_stride, uint32_t src_width, uint32_t src_height, uint32_t n,
                                     const amvhip_frontend *fe, uint32_t width, uint32_t height, uint32_t qbias, uint8_t *d_blob,
                                     uint64_t blob_cap, uint64_t *d_offs, uint32_t *d_lens, void *stream);
/*
 * The front end with a quantiser behind it, `ffmpeg -deinterlace -s 160x120 -nr N -trellis 1` in one call:
 * amvhip_encode_frontend_batch_dev with the request *q in the place of qbias.  The pictures are made in the context's
 * workspace (with every front end, the all-zero one included: then the shim's conversion or copy alone) and the encoder
 * behind them takes the request, so chunks and state are those of amvhip_video_frontend_dev into tight planes followed
 * by the YUV420 entry of the request -- amvhip_encode_yuv420_batch_dev, _nr_stream_dev, _trellis_batch_dev or
 * _nr_trellis_stream_dev -- byte for byte.  nr == 0 and trellis == 0 give the bytes of amvhip_encode_frontend_batch_dev.
 * q == NULL, a trellis other than 0 / 1, and what those entries refuse of nr, lambda and d_state are AMVHIP_ERR_ARG.
 */
typedef struct amvhip_quant {
    uint32_t qbias;
    uint32_t nr;        /* 0: no noise reduction */
    uint32_t trellis;   /* 0 / 1 */
    uint32_t lambda;    /* read when trellis is 1 */
    int32_t *d_state;   /* int32[65] on the device; required when nr > 0, not touched otherwise */
} amvhip_quant;
int amvhip_encode_frontend_quant_stream_dev(amvhip_ctx *ctx, int src_fmt, const uint8_t *d_src0, const uint8_t *d_src1,
                                            const uint8_t *d_src2, uint32_t src_stride, uint32_t src_c_stride,
                                            uint64_t src_frame_stride, uint64_t src_c_frame_stride, uint32_t src_width,
                                            uint32_t src_height, uint32_t n, const amvhip_frontend *fe, uint32_t width,
                                            uint32_t height, const amvhip_quant *q, uint8_t *d_blob, uint64_t blob_cap,
                                            uint64_t *d_offs, uint32_t *d_lens, void *stream);
/*
 * `ffmpeg -psnr`: what a lever did to the picture, beside what it did to the size.
 *
 * Host arithmetic (no context, no device):
 *   amvhip_psnr_db      psnr() of ffmpeg.c:849-852 on sse / (samples * 255^2), in dB; INFINITY for sse == 0, NaN for
 *                       samples == 0.  The -vstats figure of a frame (:873-877) is amvhip_psnr_db(sse[i][0], width * height).
 *   amvhip_psnr_report  the last-report line (:953-972) over n frames whose errors are sse[n][3]: out = Y, U, V and `*`.
 *                       The luma scale is width * height * 255^2 * n, a chroma scale a quarter of it, `*` is the summed
 *                       errors over the summed scales.
 *   amvhip_picture_sse_supported   1: amvhip_picture_sse_dev takes the format at that size.
 *
 * Picture against picture, amvhip_picture_sse_dev (asynchronous on `stream`, no workspace) and amvhip_picture_sse (host
 * buffers, synchronous): two batches of n pictures of one format and size, each handed over flat as in
 * amvhip_img_convert_dev (plane pointers need no alignment here).  d_sse is uint64_t [n][3], 8-byte aligned; entries a
 * format has no use for are written as 0.  The six planar YUV formats: entry k is plane k (4:2:0 chroma (w + 1) / 2 x
 * (h + 1) / 2, every size the decoder takes; 4:2:2 chroma (w + 1) / 2 x h); GRAY8: entry 0; RGB24 and BGR24: entry k is
 * byte k of the pixel.  Every other format returns AMVHIP_ERR_ARG.  Only a row's own bytes count, never those between a
 * row's end and the pitch.  This is the general tool: a source against what amvhip_decode_batch_dev or
 * amvhip_decode_fmt_batch_dev shows for it, in either decoder's domain.
 *
 * The encoder's own error, in the coding call (device-pointer forms only):
 *   amvhip_encode_quant_psnr_stream_dev           RGB24 / BGR24 source, arguments as amvhip_encode_batch_dev with the
 *                                                 request *q (amvhip_quant, d_state on the device) in the place of qbias
 *   amvhip_encode_yuv420_quant_psnr_stream_dev    planes as amvhip_encode_yuv420_batch_dev, then q
 *   amvhip_encode_frontend_quant_psnr_stream_dev  amvhip_encode_frontend_quant_stream_dev with d_sse in front of stream
 * Chunks, d_offs, d_lens and the -nr state are byte for byte those of the entry of the request without _psnr -- the plain
 * one, _nr_stream, _trellis_batch or _nr_trellis_stream -- in both entropy modes; the state advances once per call; what
 * those entries refuse of q is refused here (and q == NULL, a trellis other than 0 / 1, a null or misaligned d_sse).
 * d_sse[i][p], uint64_t [n][3], 8-byte aligned, is written for every frame, a frame whose chunk did not fit the blob
 * included: the squared error, summed over the visible samples of plane p (w x h luma, w/2 x h/2 chroma), between the
 * picture the encoder was handed and the reconstruction of the levels it coded.  The handed picture: for RGB / BGR sources
 * the planes of the fused rgb24_to_yuvj420p, for the front-end entry the workspace pictures, with -nr the picture before
 * the dead zone (the reference compares new_picture, mpegvideo_enc.c:2590-2606).  The reconstruction is the FFmpeg-compat
 * decoder's block arithmetic with the encoder's own tables in the place of Q60: v[natural] = (int16)(level[scan] *
 * Q[scan]) with amvlib's luma / chroma tables and the standard scan the encoder writes, + 1024 on the DC, simple_idct_put
 * (the reference encoder's idct_put) and its 0..255 clip, placed as the encoder places its blocks (bottom-up); rows and
 * columns an edge MCU replicates beyond the picture do not count.  This is the pixel-domain form of the trellis search's
 * own distortion model ("level * Q").
 *   It is NOT the reference's number: the reference's MPV_decode_mb unquantises with the MPEG-1 intra rule and the MPEG
 *   matrix, a rule that fits neither AMV decoder.
 *   It is not amvlib's picture either: amvlib differs by its IDCT's rounding, its one scan quirk and the colour step.
 *   amvhip_picture_sse_dev measures against amvlib's picture (or the FFmpeg-compat decoder's planes).
 * No entropy decode, no host synchronisation, no launch per frame: the levels are made a second time by the two-stage
 * route's front half (in AMVHIP_ENTROPY_SERIAL mode they are the ones the call packs) a round of the context's
 * coefficient workspace at a time, and one kernel per round reconstructs and compares.
 * For users of amvhip_prof_read: no kernel id was added.  amv_picture_sse_kernel is counted under AMVHIP_K_PIXFMT; the
 * error kernel shares a timed span with the forward launch in front of it, so under AMVHIP_K_FDCT (which
 * amvhip_kernel_name calls amv_forward_kernel) a _psnr call's figure is the second front half and the error kernel together.
 */
double amvhip_psnr_db(uint64_t sse, uint64_t samples);
void amvhip_psnr_report(const uint64_t *sse /* [n][3] */, uint32_t n, uint32_t width, uint32_t height, double out[4]);
int amvhip_picture_sse_supported(int fmt, uint32_t width, uint32_t height);
int amvhip_picture_sse_dev(amvhip_ctx *ctx, int fmt, const uint8_t *d_a0, const uint8_t *d_a1, const uint8_t *d_a2,
                           uint32_t a_stride, uint32_t a_c_stride, uint64_t a_frame_stride, uint64_t a_c_frame_stride,
                           const uint8_t *d_b0, const uint8_t *d_b1, const uint8_t *d_b2,
                           uint32_t b_stride, uint32_t b_c_stride, uint64_t b_frame_stride, uint64_t b_c_frame_stride,
                           uint32_t width, uint32_t height, uint32_t n, uint64_t *d_sse, void *stream);
int amvhip_picture_sse(amvhip_ctx *ctx, int fmt, const uint8_t *a0, const uint8_t *a1, const uint8_t *a2,
                       uint32_t a_stride, uint32_t a_c_stride, uint64_t a_frame_stride, uint64_t a_c_frame_stride,
                       const uint8_t *b0, const uint8_t *b1, const uint8_t *b2,
                       uint32_t b_stride, uint32_t b_c_stride, uint64_t b_frame_stride, uint64_t b_c_frame_stride,
                       uint32_t width, uint32_t height, uint32_t n, uint64_t *sse);
int amvhip_encode_quant_psnr_stream_dev(amvhip_ctx *ctx, const uint8_t *d_pix, uint32_t pix_stride, int is_bgr,
                                        uint32_t n, uint32_t width, uint32_t height, const amvhip_quant *q,
                                        uint8_t *d_blob, uint64_t blob_cap, uint64_t *d_offs, uint32_t *d_lens,
                                        uint64_t *d_sse, void *stream);
int amvhip_encode_yuv420_quant_psnr_stream_dev(amvhip_ctx *ctx, const uint8_t *d_y, const uint8_t *d_cb, const uint8_t *d_cr,
                                               uint32_t y_stride, uint32_t c_stride, uint64_t y_frame_stride,
                                               uint64_t c_frame_stride, uint32_t n, uint32_t width, uint32_t height,
                                               const amvhip_quant *q, uint8_t *d_blob, uint64_t blob_cap,
                                               uint64_t *d_offs, uint32_t *d_lens, uint64_t *d_sse, void *stream);
int amvhip_encode_frontend_quant_psnr_stream_dev(amvhip_ctx *ctx, int src_fmt, const uint8_t *d_src0, const uint8_t *d_src1,
                                                 const uint8_t *d_src2, uint32_t src_stride, uint32_t src_c_stride,
                                                 uint64_t src_frame_stride, uint64_t src_c_frame_stride, uint32_t src_width,
                                                 uint32_t src_height, uint32_t n, const amvhip_frontend *fe, uint32_t width,
                                                 uint32_t height, const amvhip_quant *q, uint8_t *d_blob, uint64_t blob_cap,
                                                 uint64_t *d_offs, uint32_t *d_lens, uint64_t *d_sse, void *stream);
/*
 * `ffmpeg -qns N`: quantizer noise shaping (avctx->quantizer_noise_shaping), the reference encoder's one perceptual lever,
 * behind any of the request's quantisers (device-pointer forms only).
 *
 * The reference (encode_mb_internal, mpegvideo_enc.c:1637-1671) takes a visual weight per sample from the local variance of
 * the source block (get_vissual_weight), quantises with the installed quantiser, and then refines each block's levels one
 * +-1 change at a time (dct_quantize_refine, :3271-3645), each change the one that lowers the weighted error of the
 * reconstruction in the pixel domain plus lambda * bits the most: error in busy texture is cheap, error in flat areas dear.
 * The walk, its roundings and the weights are the reference's.  The reference's own ffmpeg cannot run the function for its
 * amv encoder (it unquantises by the H.263 rule and reads a length table MJPEG does not set), so -- as for the trellis --
 * the reconstruction is the one every AMV decoder applies, level * Q, and the rate is the length of AMV's fixed AC code
 * itself, ZRLs and the EOB included.  Its numbers are therefore neither the reference's own nor those of amvlib's picture
 * (amvlib differs by its IDCT's rounding, its one scan quirk and the colour step); tests/golden/ref_qns.json pins the walk
 * to the reference's real function.
 *   qns      0: nothing -- the bytes, state and errors of the corresponding _psnr (d_sse != NULL) or plain entry.
 *            1: only changes that lower a level's magnitude, up to one position behind the last non-zero one.
 *            2: changes that raise a magnitude too.  3: every position, and the gradient rule for every block.
 *   lambda2  the reference's lambda2; amvhip_encode_qns_lambda2(qscale) = ((118 * qscale)^2 + 64) >> 7 is its value for a
 *            -qscale (6962 at 8), 0 where that is above amvhip_encode_qns_lambda2_max(); 0 shapes the noise with no regard
 *            for size.
 * With qns > 0 every frame takes the two-stage route in both entropy modes (equal bytes): per round of the coefficient
 * workspace amv_forward_kernel with the request's quantiser, amv_qns_refine_kernel, the error kernel where d_sse is given,
 * amv_pack_kernel.  The -nr sums and state are as ever: the refinement works towards the undenoised samples, as the
 * reference's does.  d_sse NULL: errors not wanted; otherwise as in the _psnr entries, measured on the refined levels.
 * AMVHIP_ERR_ARG: qns > 3, lambda2 above the bound, a misaligned d_sse, whatever the entries of q refuse.  No kernel id was
 * added: the refinement is counted under AMVHIP_K_FDCT.  There are no host-buffer forms.
 *   amvhip_encode_qns_stream_dev            RGB24 / BGR24 source, as amvhip_encode_quant_psnr_stream_dev with qns, lambda2
 *                                           behind q
 *   amvhip_encode_yuv420_qns_stream_dev     planes as amvhip_encode_yuv420_quant_psnr_stream_dev
 *   amvhip_encode_frontend_qns_stream_dev   as amvhip_encode_frontend_quant_psnr_stream_dev
 *   amvhip_encode_qns_coefs_dev             the levels themselves, beside amvhip_encode_trellis_coefs_dev: d_coef
 *                                           [n][blocks][64] int16, scan order, 16-byte aligned, the DC not predicted
 */
uint32_t amvhip_encode_qns_lambda2(uint32_t qscale);
uint32_t amvhip_encode_qns_lambda2_max(void);
int amvhip_encode_qns_stream_dev(amvhip_ctx *ctx, const uint8_t *d_pix, uint32_t pix_stride, int is_bgr, uint32_t n,
                                 uint32_t width, uint32_t height, const amvhip_quant *q, uint32_t qns, uint32_t lambda2,
                                 uint8_t *d_blob, uint64_t blob_cap, uint64_t *d_offs, uint32_t *d_lens, uint64_t *d_sse,
                                 void *stream);
int amvhip_encode_yuv420_qns_stream_dev(amvhip_ctx *ctx, const uint8_t *d_y, const uint8_t *d_cb, const uint8_t *d_cr,
                                        uint32_t y_stride, uint32_t c_stride, uint64_t y_frame_stride, uint64_t c_frame_stride,
                                        uint32_t n, uint32_t width, uint32_t height, const amvhip_quant *q, uint32_t qns,
                                        uint32_t lambda2, uint8_t *d_blob, uint64_t blob_cap, uint64_t *d_offs,
                                        uint32_t *d_lens, uint64_t *d_sse, void *stream);
int amvhip_encode_frontend_qns_stream_dev(amvhip_ctx *ctx, int src_fmt, const uint8_t *d_src0, const uint8_t *d_src1,
                                          const uint8_t *d_src2, uint32_t src_stride, uint32_t src_c_stride,
                                          uint64_t src_frame_stride, uint64_t src_c_frame_stride, uint32_t src_width,
                                          uint32_t src_height, uint32_t n, const amvhip_frontend *fe, uint32_t width,
                                          uint32_t height, const amvhip_quant *q, uint32_t qns, uint32_t lambda2,
                                          uint8_t *d_blob, uint64_t blob_cap, uint64_t *d_offs, uint32_t *d_lens,
                                          uint64_t *d_sse, void *stream);
int amvhip_encode_qns_coefs_dev(amvhip_ctx *ctx, const uint8_t *d_pix, uint32_t pix_stride, int is_bgr, uint32_t n,
                                uint32_t width, uint32_t height, const amvhip_quant *q, uint32_t qns, uint32_t lambda2,
                                int16_t *d_coef, void *stream);
/*
 * A byte budget per frame, met by a search over the trellis quantiser's lambda on the device (device-pointer forms only).
 *
 * AMV's quantiser tables are fixed and the reference fixes the qscale of its amv encoder (mpegvideo_enc.c:492-496), so `-b`
 * does nothing there.  Of this encoder's levers the trellis lambda is the one that can differ from frame to frame: -nr is a
 * stream state, and its offsets do not depend on lambda, so a request with nr > 0 keeps its one nr and the search runs
 * behind it.
 *
 * A ladder is a host array of `rungs` lambdas, 1 <= rungs <= AMVHIP_RATE_RUNGS_MAX, each <= amvhip_encode_trellis_lambda_max(),
 * in the caller's order of preference (ascending is usual; duplicates and descending orders are legal).  len_r(i) is the
 * length (d_lens: SOI, EOI, padding and FF escapes included) of the chunk the request's trellis entry -- _trellis_batch for
 * nr == 0, _nr_trellis_stream otherwise, same stream and state -- writes for frame i at lambda = ladder[r].  The budget B(i)
 * is d_budget[i] (uint32 [n] on the device) when d_budget is not NULL, `budget` otherwise.  The chosen rung r(i) is the FIRST
 * r, in ladder order, with len_r(i) <= B(i); if none fits it is the last rung and AMVHIP_RATE_OVER is set in d_rung[i].
 * (Sizes are not monotone in lambda, so the definition says "first" and nothing bisects.)  The chunk written for frame i is
 * byte for byte that entry's chunk at ladder[r(i)], in both entropy modes; d_offs, d_lens and the blob-capacity rule are the
 * plain entries'.  With nr > 0 the state advances once per call: n frames in one call equal the same frames in any number
 * of calls with the state carried, the rungs included.
 *
 * How: one front half per block and the trellis walk per rung on the same fdct outputs give, without packing a byte, the
 * bits of the frame's scan at every rung; 4 + ceil(bits / 8) is a floor of the chunk's length (escapes come on top), so a
 * frame starts at its first rung whose floor fits, is coded (amv_forward_kernel with the frame's own lambda, amv_pack_kernel:
 * the two-stage route for every frame, as with qns), and moves on to its next floor-fit only where escapes pushed it over
 * -- up to rungs - 1 small launches that usually find nothing.  No host synchronisation.
 *
 *   amvhip_encode_rate_probe_dev, amvhip_encode_yuv420_rate_probe_dev
 *       the arguments of amvhip_encode_quant_psnr_stream_dev / amvhip_encode_yuv420_quant_psnr_stream_dev up to q, then the
 *       ladder and d_bits, uint32 [n][rungs], 4-byte aligned: d_bits[i][r] = the bits the entropy coder writes for frame i's
 *       scan at ladder[r] (DC codes and magnitudes, AC run/size codes, magnitudes, ZRLs, EOBs; before padding and escaping).
 *       No chunk is written, q->d_state is read and never written: R(lambda) per frame, for a caller who allocates a total
 *       over the frames themselves and hands the result back as d_budget.
 *   amvhip_encode_rate_stream_dev (RGB24 / BGR24), amvhip_encode_yuv420_rate_stream_dev, amvhip_encode_frontend_rate_stream_dev
 *       the _quant_psnr_stream_dev entries with `rate` behind q and d_rung, uint32 [n], 4-byte aligned, in the place of
 *       d_sse: d_rung[i] = r(i), AMVHIP_RATE_OVER or-ed in where no rung fit.  It is written for every frame, a frame whose
 *       chunk did not fit the blob included.
 * In q, trellis must be 1 and lambda is not read; qbias, nr and d_state mean what they mean everywhere.  AMVHIP_ERR_ARG, with
 * nothing queued and the state untouched: rate or ladder NULL, rungs 0 or above the maximum, a lambda above the bound,
 * q->trellis != 1, a NULL or misaligned d_rung or d_bits, a misaligned d_budget, whatever the trellis entries refuse of q,
 * and a picture of more than 349 525 MCUs (beyond it a frame's bits need not fit 32).  Not here: qns or d_sse in a rate call,
 * 4:2:2 sources, host-buffer forms, the plain quantiser as a rung, a carry of unused bytes from frame to frame.  No kernel
 * id was added: the probe is counted under AMVHIP_K_FDCT.
 */
#define AMVHIP_RATE_RUNGS_MAX 16
#define AMVHIP_RATE_OVER 0x80000000u          /* in d_rung[i]: no rung met the budget; the chunk is the last rung's */
typedef struct amvhip_rate {
    const uint32_t *ladder;     /* host, `rungs` lambdas */
    uint32_t rungs;
    uint32_t budget;            /* bytes per chunk, read when d_budget is NULL */
    const uint32_t *d_budget;   /* device, uint32[n], or NULL */
} amvhip_rate;
int amvhip_encode_rate_probe_dev(amvhip_ctx *ctx, const uint8_t *d_pix, uint32_t pix_stride, int is_bgr, uint32_t n,
                                 uint32_t width, uint32_t height, const amvhip_quant *q, const uint32_t *ladder, uint32_t rungs,
                                 uint32_t *d_bits, void *stream);
int amvhip_encode_yuv420_rate_probe_dev(amvhip_ctx *ctx, const uint8_t *d_y, const uint8_t *d_cb, const uint8_t *d_cr,
                                        uint32_t y_stride, uint32_t c_stride, uint64_t y_frame_stride, uint64_t c_frame_stride,
                                        uint32_t n, uint32_t width, uint32_t height, const amvhip_quant *q,
                                        const uint32_t *ladder, uint32_t rungs, uint32_t *d_bits, void *stream);
int amvhip_encode_rate_stream_dev(amvhip_ctx *ctx, const uint8_t *d_pix, uint32_t pix_stride, int is_bgr, uint32_t n,
                                  uint32_t width, uint32_t height, const amvhip_quant *q, const amvhip_rate *rate,
                                  uint8_t *d_blob, uint64_t blob_cap, uint64_t *d_offs, uint32_t *d_lens, uint32_t *d_rung,
                                  void *stream);
int amvhip_encode_yuv420_rate_stream_dev(amvhip_ctx *ctx, const uint8_t *d_y, const uint8_t *d_cb, const uint8_t *d_cr,
                                         uint32_t y_stride, uint32_t c_stride, uint64_t y_frame_stride, uint64_t c_frame_stride,
                                         uint32_t n, uint32_t width, uint32_t height, const amvhip_quant *q,
                                         const amvhip_rate *rate, uint8_t *d_blob, uint64_t blob_cap, uint64_t *d_offs,
                                         uint32_t *d_lens, uint32_t *d_rung, void *stream);
int amvhip_encode_frontend_rate_stream_dev(amvhip_ctx *ctx, int src_fmt, const uint8_t *d_src0, const uint8_t *d_src1,
                                           const uint8_t *d_src2, uint32_t src_stride, uint32_t src_c_stride,
                                           uint64_t src_frame_stride, uint64_t src_c_frame_stride, uint32_t src_width,
                                           uint32_t src_height, uint32_t n, const amvhip_frontend *fe, uint32_t width,
                                           uint32_t height, const amvhip_quant *q, const amvhip_rate *rate, uint8_t *d_blob,
                                           uint64_t blob_cap, uint64_t *d_offs, uint32_t *d_lens, uint32_t *d_rung,
                                           void *stream);
/*
 * AMV chunks requantised in the coefficient domain, at one lambda or under a byte budget per frame (device-pointer forms
 * only): chunks in, chunks out, and no pixel in between.
 *
 * AMV's quantiser tables are fixed, so a chunk's levels already are the coefficients the trellis quantiser searches on,
 * level * Q.  The rule (csrc/amv_requant_plan.h), per frame whose entropy decode is clean, over its 6 * nmcu lines of levels
 * in scan order as amvhip_huffman_decode_dev hands them out:
 *   1. the DC level is carried unchanged;
 *   2. the AC levels are searched as amvhip_encode_trellis_batch_dev searches fdct outputs, on c = level * 8 Q, with the
 *      caller's lambda and the rounding term one half (the levels are rounded already: there is no qbias here).  A coded
 *      position's first candidate is the chunk's own level; lambda = 0 returns the levels unchanged;
 *   3. the lines are coded by the entropy coder of every encoder entry: SOI, the escaped scan, padding, EOI.  lambda = 0 is the
 *      canonical re-coding of the chunk (a chunk this library's encoders wrote comes back byte for byte).
 * A frame is coded only if its entropy decode reports nothing, reaches the last MCU, and every block is in range:
 * |level| * 8 Q <= 8681 per AC coefficient, the sum of (level * 8 Q)^2 over a block's AC coefficients <= 2^30, |DC level| <=
 * 1023 (every chunk an encoder of 8-bit samples writes with AMV's tables is inside; beyond, the search's int scores could wrap
 * or the DC difference would have no code).  Otherwise d_status[i] is not zero -- the decode's AMVHIP_ST_* bits, or
 * AMVHIP_ST_RANGE -- d_out_lens[i] is 0 and nothing is written for the frame: the caller keeps its own chunk.
 *
 * The input arguments are amvhip_decode_batch_dev's up to height (any width and height that entry takes: there are no pixels
 * here and no evenness rule); chunks are written back to back into d_out as the encoder entries write them (d_out_offs,
 * d_out_lens; a chunk that would end past out_cap is not written and its length is 0).  Asynchronous on `stream`, no host
 * synchronisation, no launch per frame; both entropy modes give the same bytes.
 *
 *   amvhip_requant_stream_dev       the rule at `lambda` (<= amvhip_encode_trellis_lambda_max()).  d_err: NULL, or uint64 [n][3],
 *       8-byte aligned: entry p of frame i = the sum of ((new - old) * Q)^2 over the AC positions of the blocks of plane p (Y:
 *       blocks 0-3 of an MCU, Cb: block 4, Cr: block 5) -- by Parseval the unclipped pixel error between the two decodes.
 *       Written for every frame, 0 for a frame that is not coded.
 *   amvhip_requant_rate_probe_dev   d_bits [n][rungs] as amvhip_encode_rate_probe_dev's: the bits of the frame's scan at
 *       ladder[r], before padding and escapes.  The row of a frame that is not coded is 0.  No chunk is written.
 *   amvhip_requant_rate_stream_dev  the rate entries' definition above word for word, with amvhip_requant_stream_dev in the
 *       place of the trellis entry: the first rung in ladder order whose chunk fits B(i), that rung's chunk byte for byte as
 *       amvhip_requant_stream_dev writes it at that lambda, AMVHIP_RATE_OVER with the last rung where none fits.  A frame that
 *       is not coded gets AMVHIP_RATE_OVER | (rungs - 1): d_status tells the two cases apart.  A ladder whose first rung is 0
 *       leaves a frame that already fits as it is (re-coded canonically).
 * AMVHIP_ERR_ARG with nothing queued: null or misaligned pointers (d_blob, d_lens, d_status, d_out_lens, d_rung, d_bits,
 * d_budget: 4 bytes; d_offs, d_out_offs, d_err: 8), a lambda above the bound, rate or ladder NULL, rungs 0 or above
 * AMVHIP_RATE_RUNGS_MAX, and for the two rate entries a picture of more than 349 525 MCUs.  n == 0 succeeds and queues nothing.
 * Not here: -nr and -qns behind a coefficient source, host-buffer forms, writing the frames that are not coded through to
 * d_out.  No kernel id was added: the search is counted under AMVHIP_K_FDCT, as the probe is.
 */
#define AMVHIP_ST_RANGE 8u     /* requant: a block's levels are outside the range the search is proved for */
int amvhip_requant_stream_dev(amvhip_ctx *ctx, const uint8_t *d_blob, uint64_t blob_bytes, const uint64_t *d_offs,
                              const uint32_t *d_lens, uint32_t n, uint32_t width, uint32_t height, uint32_t lambda,
                              uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_offs, uint32_t *d_out_lens, int32_t *d_status,
                              uint64_t *d_err, void *stream);
int amvhip_requant_rate_probe_dev(amvhip_ctx *ctx, const uint8_t *d_blob, uint64_t blob_bytes, const uint64_t *d_offs,
                                  const uint32_t *d_lens, uint32_t n, uint32_t width, uint32_t height, const uint32_t *ladder,
                                  uint32_t rungs, uint32_t *d_bits, void *stream);
int amvhip_requant_rate_stream_dev(amvhip_ctx *ctx, const uint8_t *d_blob, uint64_t blob_bytes, const uint64_t *d_offs,
                                   const uint32_t *d_lens, uint32_t n, uint32_t width, uint32_t height, const amvhip_rate *rate,
                                   uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_offs, uint32_t *d_out_lens,
                                   int32_t *d_status, uint32_t *d_rung, void *stream);
/*
 * A byte budget per CLIP -- "these n frames in at most `total` bytes" -- settled on the device (device-pointer forms only).
 *
 * The terms are the rate section's: the ladder, len_r(i), B(i) (d_budget[i], or `budget`; a caller who wants no cap per frame
 * passes budget = 0xffffffff) and AMVHIP_RATE_OVER.
 *   Per frame.  For a clip rung c in 0 .. rungs - 1, frame i is coded at r_c(i): the FIRST r >= c, in ladder order, with
 *               len_r(i) <= B(i); if none fits, the last rung, flagged AMVHIP_RATE_OVER.
 *   The sum.    S(c) = the sum over i of len_{r_c(i)}(i), a uint64.
 *   The clip.   The chosen clip rung c* is the FIRST c with S(c) <= total; if none fits, c* = rungs - 1 and AMVHIP_RATE_OVER
 *               is or-ed into the clip record.  (S is not monotone in c, and duplicate and descending ladders have a meaning
 *               too: "first", and nothing bisects.)
 *   Chunks.     Byte for byte those of the rate sibling called with ladder + c* and rungs - c*: that trellis or requant
 *               entry's chunks at ladder[r(i)], in both entropy modes; d_offs, d_lens and the blob-capacity rule as there.
 *   d_rung[i]   indexes the caller's full ladder: c* + that call's rung, AMVHIP_RATE_OVER as in that call.
 *   d_clip      uint64 [2] on the device, 8-byte aligned: [0] = c*, AMVHIP_RATE_OVER or-ed in when no clip rung fit;
 *               [1] = S(c*).  S is taken over the lengths the coder produced, before the blob-capacity rule drops a chunk: a
 *               blob that is too small changes neither c*, d_rung nor d_clip.
 *   -nr         the state advances once per call, as in the rate entries.
 * One lambda for the whole clip is the equal-slope allocation of a total (the trellis walk minimises distortion + lambda *
 * bits per block); the first fit per frame on top of it is the guard against a chunk a player stalls on.
 *
 * How: the probe's bits give, without packing a byte, a lower bound F(c) of S(c) (csrc/amv_clip_plan.h), so the clip starts
 * at the first c whose bound fits and passes every later c whose bound does not; at a clip rung the frames are coded and
 * moved along their floor-fits as in a rate call, the lengths are summed on the device, and the clip is final or moves to
 * the next c, taking along only the frames that stand below it.  The passes are queued without knowing their counts, at
 * most rungs * (rungs + 1) / 2 of them, nearly all of which find nothing to do.  No host synchronisation.
 *
 *   amvhip_encode_clip_stream_dev (RGB24 / BGR24), amvhip_encode_yuv420_clip_stream_dev, amvhip_encode_frontend_clip_stream_dev
 *       the arguments of the _rate_stream_dev sibling with `total` behind rate and d_clip behind d_rung.
 *   amvhip_requant_clip_stream_dev
 *       amvhip_requant_rate_stream_dev's likewise.  A frame that is not coded contributes 0 to S, keeps AMVHIP_RATE_OVER |
 *       (rungs - 1) and d_out_lens 0: its bytes are the caller's, who subtracts them from `total`.
 * AMVHIP_ERR_ARG with nothing queued and the state untouched: whatever the rate sibling refuses (the picture of more than
 * 349 525 MCUs included), and a NULL or misaligned d_clip.  n == 0 succeeds and queues nothing (d_clip is not written).
 * Not here: spending the slack between S(c*) and total on single frames, a carry of unused bytes from frame to frame, a
 * total split over several calls, host-buffer forms, 4:2:2 sources, qns in a clip call.
 *
 * From a file size to `total` and back: amvhip_mux_file_bytes / amvhip_mux_video_total beside the muxer below.
 */
int amvhip_encode_clip_stream_dev(amvhip_ctx *ctx, const uint8_t *d_pix, uint32_t pix_stride, int is_bgr, uint32_t n,
                                  uint32_t width, uint32_t height, const amvhip_quant *q, const amvhip_rate *rate,
                                  uint64_t total, uint8_t *d_blob, uint64_t blob_cap, uint64_t *d_offs, uint32_t *d_lens,
                                  uint32_t *d_rung, uint64_t *d_clip, void *stream);
int amvhip_encode_yuv420_clip_stream_dev(amvhip_ctx *ctx, const uint8_t *d_y, const uint8_t *d_cb, const uint8_t *d_cr,
                                         uint32_t y_stride, uint32_t c_stride, uint64_t y_frame_stride, uint64_t c_frame_stride,
                                         uint32_t n, uint32_t width, uint32_t height, const amvhip_quant *q,
                                         const amvhip_rate *rate, uint64_t total, uint8_t *d_blob, uint64_t blob_cap,
                                         uint64_t *d_offs, uint32_t *d_lens, uint32_t *d_rung, uint64_t *d_clip, void *stream);
int amvhip_encode_frontend_clip_stream_dev(amvhip_ctx *ctx, int src_fmt, const uint8_t *d_src0, const uint8_t *d_src1,
                                           const uint8_t *d_src2, uint32_t src_stride, uint32_t src_c_stride,
                                           uint64_t src_frame_stride, uint64_t src_c_frame_stride, uint32_t src_width,
                                           uint32_t src_height, uint32_t n, const amvhip_frontend *fe, uint32_t width,
                                           uint32_t height, const amvhip_quant *q, const amvhip_rate *rate, uint64_t total,
                                           uint8_t *d_blob, uint64_t blob_cap, uint64_t *d_offs, uint32_t *d_lens,
                                           uint32_t *d_rung, uint64_t *d_clip, void *stream);
int amvhip_requant_clip_stream_dev(amvhip_ctx *ctx, const uint8_t *d_blob, uint64_t blob_bytes, const uint64_t *d_offs,
                                   const uint32_t *d_lens, uint32_t n, uint32_t width, uint32_t height, const amvhip_rate *rate,
                                   uint64_t total, uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_offs, uint32_t *d_out_lens,
                                   int32_t *d_status, uint32_t *d_rung, uint64_t *d_clip, void *stream);
/*
 * Re-table: chunks whose levels were written against quantiser tables that are not AMV's, made AMV's (device-pointer forms
 * only): chunks in, chunks out, and no pixel in between.
 *
 * Every AMV decoder dequantises with AMV's fixed tables Qd.  The reference's own amv encoder quantises with
 * clip8(ff_mpeg1_default_intra_matrix[i] * qscale >> 3), entry 0 = 8, one matrix for luma and chroma
 * (mpegvideo_enc.c:2866-2877): its files MEAN level * Qs and are READ as level * Qd.  The rule (csrc/amv_retable_plan.h), per
 * frame whose entropy decode is clean, over its lines of levels in scan order as amvhip_huffman_decode_dev hands them out,
 * with Qs the frame's source table:
 *   1. DC: the new level is level * Qs[0] / Qd[0], rounded to nearest, halves away from zero (Qs[0] 9 against 8: level 4 is
 *      36 / 8 and comes out as 5); with Qs[0] == Qd[0] the level is carried unchanged;
 *   2. AC: c[k] = level[k] * 8 Qs[k] is searched as amvhip_requant_stream_dev searches level * 8 Qd: against AMV's tables, the
 *      rounding term one half, the caller's lambda.  At lambda = 0 every position comes back within half an AMV step of what
 *      the chunk meant: |new * 8 Qd - c| <= 4 Qd + 1;
 *   3. the lines are coded by the entropy coder of every encoder entry.
 * With source tables equal to AMV's the entries are their requant siblings (but for the range rule's cap, below).
 * A frame is coded only if its entropy decode reports nothing, reaches the last MCU, its table index names a table, and every
 * block is in range: |level| * 8 Qs <= 8193 per AC coefficient (what the search's fits are proved for with arbitrary
 * coefficients; requant's 8681 rests on multiples of 8 Qd), the sum of (level * 8 Qs)^2 over a block's AC coefficients <= 2^30,
 * |NEW DC level| <= 1023.  Otherwise d_status[i] is not zero -- the decode's AMVHIP_ST_* bits, AMVHIP_ST_RANGE, or
 * AMVHIP_ST_TABLE -- d_out_lens[i] is 0 and nothing is written for the frame.
 *
 * amvhip_retable: tables = HOST memory, uint8 [count][2][64], luma then chroma, scan order, every entry 1 .. 255; copied
 * during the call by a hipMemcpyAsync queued on `stream` into the context's workspace (that call's rules say when the memory
 * is the caller's again: pageable memory at return, pinned memory once the stream has reached the copy).  count 1 ..
 * AMVHIP_RETABLE_TABLES_MAX.  d_table_of: NULL = table 0 for every frame, else uint8 [n] on the device, frame i's table (the
 * reference's default rate-controlled runs vary qscale per frame: the q= column of its -vstats log).
 *
 * The four entries are amvhip_requant_stream_dev, _rate_probe_dev, _rate_stream_dev and _clip_stream_dev with `rt` behind
 * height; every other argument, the definitions of rate and clip, d_bits, d_rung and d_clip are the siblings' word for word,
 * with amvhip_retable_stream_dev in amvhip_requant_stream_dev's place.  d_err: entry p of frame i = the sum over ALL 64
 * positions (the DC included) of the blocks of plane p of (new * Qd - old * Qs)^2 -- by Parseval the unclipped pixel error
 * between what the chunk meant and what the new chunk decodes to.
 * AMVHIP_ERR_ARG with nothing queued: whatever the sibling refuses; rt or rt->tables NULL; count 0 or above the maximum; a
 * table entry of 0.
 *
 * amvhip_ffmpeg_amv_tables: the reference encoder's tables at -qscale `qscale` (1 .. 31) in scan order, host arithmetic, no
 * context.  Returns AMVHIP_OK, or AMVHIP_ERR_ARG for a qscale outside 1 .. 31, for which nothing is written.
 * Not here: decoding WITH a caller's tables, the 4:2:2 scans of the reference's encoder, MJPEG (unflipped) sources, host-buffer
 * forms, the plugin.
 */
#define AMVHIP_RETABLE_TABLES_MAX 64
#define AMVHIP_ST_TABLE 0x10u  /* 16: retable: d_table_of[i] >= count, the frame is not coded */
typedef struct amvhip_retable {
    const uint8_t *tables;      /* host: [count][2][64], luma then chroma, scan order, entries 1..255 */
    uint32_t count;             /* 1 .. AMVHIP_RETABLE_TABLES_MAX */
    const uint8_t *d_table_of;  /* device: NULL = table 0 for every frame, else uint8 [n] */
} amvhip_retable;
int amvhip_retable_stream_dev(amvhip_ctx *ctx, const uint8_t *d_blob, uint64_t blob_bytes, const uint64_t *d_offs,
                              const uint32_t *d_lens, uint32_t n, uint32_t width, uint32_t height, const amvhip_retable *rt,
                              uint32_t lambda, uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_offs, uint32_t *d_out_lens,
                              int32_t *d_status, uint64_t *d_err, void *stream);
int amvhip_retable_rate_probe_dev(amvhip_ctx *ctx, const uint8_t *d_blob, uint64_t blob_bytes, const uint64_t *d_offs,
                                  const uint32_t *d_lens, uint32_t n, uint32_t width, uint32_t height, const amvhip_retable *rt,
                                  const uint32_t *ladder, uint32_t rungs, uint32_t *d_bits, void *stream);
int amvhip_retable_rate_stream_dev(amvhip_ctx *ctx, const uint8_t *d_blob, uint64_t blob_bytes, const uint64_t *d_offs,
                                   const uint32_t *d_lens, uint32_t n, uint32_t width, uint32_t height, const amvhip_retable *rt,
                                   const amvhip_rate *rate, uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_offs,
                                   uint32_t *d_out_lens, int32_t *d_status, uint32_t *d_rung, void *stream);
int amvhip_retable_clip_stream_dev(amvhip_ctx *ctx, const uint8_t *d_blob, uint64_t blob_bytes, const uint64_t *d_offs,
                                   const uint32_t *d_lens, uint32_t n, uint32_t width, uint32_t height, const amvhip_retable *rt,
                                   const amvhip_rate *rate, uint64_t total, uint8_t *d_out, uint64_t out_cap,
                                   uint64_t *d_out_offs, uint32_t *d_out_lens, int32_t *d_status, uint32_t *d_rung,
                                   uint64_t *d_clip, void *stream);
int amvhip_ffmpeg_amv_tables(uint32_t qscale, uint8_t tables[2][64]);
/*
 * Decoder + back end in one call: the patched FFmpeg's amv decoder (AMVHIP_FLAG_FFMPEG, required: AMVHIP_ERR_ARG without)
 * into workspace planes, then img_convert YUVJ420P -> dst_fmt (yuvj420p_to_*, imgconvert.c:1977-1993; the planar route for
 * YUV420P; the gray route for GRAY8): what `ffmpeg -i x.amv [-pix_fmt rgb24|bgr24|rgb32|rgb565] out` hands its next stage
 * (README:10-18).  Other arguments as amvhip_decode_batch_dev.  d_out: n frames of amvhip_pix_frame_bytes(dst_fmt,
 * out_stride, height) bytes, rows out_stride apart (for YUV420P: the Y plane, then Cb and Cr with rows (out_stride + 1) / 2
 * apart); bytes between a row's end and out_stride stay as they were.  AMVHIP_FLAG_FFMPEG_KEEP is refused (the caller's
 * buffer is not in plane form); damaged frames convert what the plain compat mode leaves, zeros behind the failing MCU.
 */
int amvhip_decode_fmt_batch_dev(amvhip_ctx *ctx, const uint8_t *d_blob, uint64_t blob_bytes,
                                const uint64_t *d_offs, const uint32_t *d_lens, uint32_t n,
                                uint32_t width, uint32_t height, uint32_t flags, int dst_fmt,
                                uint8_t *d_out, uint32_t out_stride, int32_t *d_status, void *stream);
/*
 * Reduced-size decode: pictures of 1/2, 1/4 or 1/8 the size (lowres = 1, 2, 3) straight from the entropy stage, for
 * contact sheets, scrub bars and preview strips -- the full-size reconstruction is neither run nor written.
 *
 * The block arithmetic is the reference's `-lowres` (libavcodec/utils.c:707, dsputil.c:3870-3889, mjpegdec.c:711), byte
 * for byte: decode_block's dequantisation (sp5x Q60 tables, +1024 on the DC), then j_rev_dct4 / j_rev_dct2 /
 * j_rev_dct1 (jrevdct.c:952-1156) over the top-left 4x4 / 2x2 / 1x1 coefficients of each block, every store into
 * the block wrapped to int16 as DCTELEM is, and put_pixels_clamped4_c / 2_c / ff_jref_idct1_put (dsputil.c:461-493,
 * 3774-3801) with the 0..255 clamp of ff_cropTbl.
 *
 * The placement is this library's: the full-size placement of AMVHIP_FLAG_FFMPEG scaled down.  The reference's own
 * cannot serve for AMV: its flip takes the start row from the full-size 8 * mb_height and does not shift it
 * (mjpegdec.c:675), aiming the first block far below a picture that avcodec_set_dimensions (utils.c:141-142) has
 * already shrunk, and ffmpeg.c:2699 sets CODEC_FLAG_EMU_EDGE whenever lowres is set, which that flip asserts
 * against (mjpegdec.c:674).  The rule, with bs = 8 >> lowres and `start` the full-size start row of the component
 * (v * (8 * mcu_rows - ((height / 2) & 7)) - 1 with v = 2 for luma and 1 for chroma: mjpegdec.c:675):
 *     start_L = ((start + 1 + (1 << lowres) - 1) >> lowres) - 1;
 *     row i of a block at canvas row sy, column sx (full-size units) lands at plane row start_L - ((sy >> lowres) + i),
 *     column sx >> lowres; rows and columns outside the plane are dropped.
 * Luma is W_L x H_L with W_L = amvhip_lowres_dim(width, lowres), H_L likewise; Cb and Cr are (W_L + 1) / 2 x
 * (H_L + 1) / 2; the planes are tight, Y then Cb then Cr: amvhip_lowres_frame_bytes per frame.  For height % 16 of 0 or
 * 8 this is the exact vertical flip of the reduced canvas; for other heights it keeps the full-size picture's row shift,
 * so a thumbnail is a downscale of what the full-size mode shows.  Every byte of every plane is written by every call
 * (plane rows no canvas row reaches -- height % 16 above 8 -- are zero); MCUs at or after a frame's first error are
 * zero, as in the plain compat mode.
 *
 * amvhip_decode_lowres_batch_dev: arguments as amvhip_decode_fmt_batch_dev.  flags must be exactly AMVHIP_FLAG_FFMPEG
 * (amvlib has no such mode; AMVHIP_FLAG_FFMPEG_KEEP is refused); lowres 1..3 (0 is refused: the full-size entry points
 * stay the only way to their output).  dst_fmt AMVHIP_PIX_YUVJ420P writes the planes into d_out, and out_stride must
 * equal W_L; every other format amvhip_decode_fmt_batch_dev takes goes through workspace planes and img_convert at
 * W_L x H_L (d_out: n frames of amvhip_pix_frame_bytes(dst_fmt, out_stride, H_L)).  amvhip_decode_lowres_batch: the same
 * from and to host buffers, synchronous.  amvhip_reconstruct_lowres_dev: the back half alone on dense coefficient lines,
 * as amvhip_reconstruct_dev with AMVHIP_FLAG_FFMPEG (any int16 anywhere).
 */
uint32_t amvhip_lowres_dim(uint32_t full, uint32_t lowres);              /* ceil(full / 2^lowres); 0 for lowres > 3 */
uint64_t amvhip_lowres_frame_bytes(uint32_t width, uint32_t height, uint32_t lowres);   /* the three tight planes */
int amvhip_decode_lowres_batch_dev(amvhip_ctx *ctx, const uint8_t *d_blob, uint64_t blob_bytes,
                                   const uint64_t *d_offs, const uint32_t *d_lens, uint32_t n,
                                   uint32_t width, uint32_t height, uint32_t flags, uint32_t lowres, int dst_fmt,
                                   uint8_t *d_out, uint32_t out_stride, int32_t *d_status, void *stream);
int amvhip_decode_lowres_batch(amvhip_ctx *ctx, const uint8_t *blob, uint64_t blob_bytes,
                               const uint64_t *offs, const uint32_t *lens, uint32_t n,
                               uint32_t width, uint32_t height, uint32_t flags, uint32_t lowres, int dst_fmt,
                               uint8_t *out, uint32_t out_stride, int32_t *status);
int amvhip_reconstruct_lowres_dev(amvhip_ctx *ctx, const int16_t *d_coef, const uint32_t *d_nmcu_ok, uint32_t n,
                                  uint32_t width, uint32_t height, uint32_t lowres, uint8_t *d_out, void *stream);
/*
 * Decode-side postprocessing: the reference's libpostproc (AMVmuxer/ffmpeg/libpostproc, pp_postprocess) for its horizontal
 * and vertical deblocking filters and its deringing filter (`hb`, `vb`, `dr`; the preset `de`), byte for byte the C path of
 * that library with a forced or absent quantiser table (`fq`; QP 1 without it, as the reference with a NULL QP_store).
 *
 * amvhip_pp_mode_parse restates pp_get_mode_by_name_and_quality for hb / hdeblock and vb / vdeblock with their `:diff:flat`
 * numeric options, dr / dering, fq / forcequant, the option letters a, c, y, n, the `-` prefix, `,` and `/` between filters
 * and the preset de / default.  Every other filter or preset the reference knows (h1 v1 ha va al lb li ci md fd l5 tn, the
 * presets fa / fast and ac) and whatever the reference refuses returns AMVHIP_ERR_ARG with *out untouched: nothing is dropped
 * silently.  No context or device needed.  lum_mode / chrom_mode carry the reference's own bit values; forced_quant is 0
 * unless AMVHIP_PP_FORCE_QUANT is set.  base_dc_diff is parsed and kept, but with a forced or absent QP table the reference's
 * classification never sees it (its nonBQP table stays zero: dcOffset = 1 whatever the option says), and so it is here.
 *
 * amvhip_postprocess_dev: n pictures, planes and pitches as in amvhip_deinterlace_dev, fmt AMVHIP_PIX_YUV420P or
 * AMVHIP_PIX_YUVJ420P (chroma planes width / 2 x height / 2, the same QP, as PP_FORMAT_420).  AMVHIP_ERR_ARG, with nothing
 * launched:
 *   - a row pitch other than `width` (luma) and `width / 2` (chroma), on either side.  The reference's dering window of a
 *     row's last block reads and writes one column behind the row: on a tight pitch that column is the next row's first, on
 *     a wider one it is padding, and the output would depend on what the padding held.  The feature is defined on tight
 *     pitches: the layout amvhip_decode_fmt_batch_dev writes.
 *   - planes or frame pitches that are not 4-byte aligned; source and destination that overlap;
 *   - mode bits outside AMVHIP_PP_V_DEBLOCK | AMVHIP_PP_H_DEBLOCK | AMVHIP_PP_DERING (| AMVHIP_PP_FORCE_QUANT in lum_mode),
 *     and AMVHIP_PP_DERING without AMVHIP_PP_V_DEBLOCK in a plane's mode: the reference then copies one line ahead only and
 *     its row-end window reads a destination pixel nobody has written -- its output depends on what the destination held;
 *   - forced_quant above 63 or below 0 (with AMVHIP_PP_FORCE_QUANT);
 *   - sizes amvhip_postprocess_supported refuses: it takes widths that are multiples of 16 and even heights, 16 x 16 up to
 *     1024 x 1024.
 * d_qp: NULL, or uint8 [n] on the device, a QP per frame (a batch may mix clips; entries above 63 count as 63); else
 * mode->forced_quant for all frames with AMVHIP_PP_FORCE_QUANT, else 1.  With chrom_mode == 0 the chroma planes are copied.
 * Asynchronous on `stream`, no host synchronisation; the source is never written.  amvhip_postprocess: the same from and to
 * host buffers (any pitch >= the row there: the planes are staged tight), synchronous.
 *
 * amvhip_decode_pp_batch_dev: arguments as amvhip_decode_fmt_batch_dev, then mode and d_qp.  The frames are decoded into
 * workspace planes, postprocessed, and written to d_out: straight out for AMVHIP_PIX_YUVJ420P (out_stride must equal width),
 * through img_convert for every other format the decode entry writes -- the route amvhip_decode_lowres_batch_dev takes.  A
 * frame with a non-zero status is postprocessed like any other; d_status is the decode's.
 *
 * For users of amvhip_prof_read: no kernel id was added.  amv_postprocess_kernel is counted under AMVHIP_K_PIXFMT, as
 * amv_picture_sse_kernel is.
 */
#define AMVHIP_PP_V_DEBLOCK 0x01
#define AMVHIP_PP_H_DEBLOCK 0x02
#define AMVHIP_PP_DERING 0x04
#define AMVHIP_PP_FORCE_QUANT 0x200000
typedef struct amvhip_pp_mode {
    int32_t lum_mode, chrom_mode;       /* AMVHIP_PP_* */
    int32_t base_dc_diff;               /* hb / vb option 1; default 32 */
    int32_t flatness_threshold;         /* hb / vb option 2; default 39 */
    int32_t forced_quant;               /* fq's QP (default 15); 0 without AMVHIP_PP_FORCE_QUANT */
} amvhip_pp_mode;
int amvhip_pp_mode_parse(const char *name, int quality, amvhip_pp_mode *out);
int amvhip_postprocess_supported(uint32_t width, uint32_t height);
int amvhip_postprocess_dev(amvhip_ctx *ctx, int fmt, const amvhip_pp_mode *mode,
                           const uint8_t *d_src0, const uint8_t *d_src1, const uint8_t *d_src2,
                           uint32_t src_stride, uint32_t src_c_stride, uint64_t src_frame_stride, uint64_t src_c_frame_stride,
                           uint8_t *d_dst0, uint8_t *d_dst1, uint8_t *d_dst2,
                           uint32_t dst_stride, uint32_t dst_c_stride, uint64_t dst_frame_stride, uint64_t dst_c_frame_stride,
                           uint32_t width, uint32_t height, uint32_t n, const uint8_t *d_qp, void *stream);
int amvhip_postprocess(amvhip_ctx *ctx, int fmt, const amvhip_pp_mode *mode,
                       const uint8_t *src0, const uint8_t *src1, const uint8_t *src2,
                       uint32_t src_stride, uint32_t src_c_stride, uint64_t src_frame_stride, uint64_t src_c_frame_stride,
                       uint8_t *dst0, uint8_t *dst1, uint8_t *dst2,
                       uint32_t dst_stride, uint32_t dst_c_stride, uint64_t dst_frame_stride, uint64_t dst_c_frame_stride,
                       uint32_t width, uint32_t height, uint32_t n, const uint8_t *qp);
int amvhip_decode_pp_batch_dev(amvhip_ctx *ctx, const uint8_t *d_blob, uint64_t blob_bytes,
                               const uint64_t *d_offs, const uint32_t *d_lens, uint32_t n,
                               uint32_t width, uint32_t height, uint32_t flags, int dst_fmt,
                               uint8_t *d_out, uint32_t out_stride, int32_t *d_status,
                               const amvhip_pp_mode *mode, const uint8_t *d_qp, void *stream);
/*
 * The audio resampler in front of the ADPCM encoder: audio_resample (libavcodec/resample.c:129-242) over av_resample
 * (resample2.c:182-324), what ffmpeg.c:1639-1641 / :502 run for `-ac 1 -ar 22050` (AMVmuxer/Makefile:16).  16-tap (at
 * 0.8 of the lower rate's Nyquist: 40 taps at 44.1 kHz -> 22.05 kHz, 44 at 48 kHz, 88 at 96 kHz), 1024-phase, Kaiser-windowed
 * polyphase filter in int16 with 32-bit wrapping sums, bit-exact with the reference.  Channels: 1 or 2 in, 1 or 2 out
 * (2 -> 1 mixes down (l + r) >> 1 first, 1 -> 2 duplicates; the reference's 5.1 output is not offered); rates
 * AMVHIP_AUDIO_RATE_MIN .. AMVHIP_AUDIO_RATE_MAX (AMVHIP_ERR_ARG beyond).  Samples int16, channels interleaved; offsets in
 * int16 elements, lengths in frames (one sample per channel).
 *
 * amvhip_audio_resample_out_samples  frames one audio_resample call makes of in_samples frames (host arithmetic, no device):
 *                                    the filter needs its whole span, so the last ~fl/2 input frames make no output and
 *                                    nothing flushes them (ffmpeg.c never does).  0 outside the rate range, for 0 frames and
 *                                    for 2^32 frames or more.
 * amvhip_audio_resample_batch_dev    n independent streams of one format; stream i = d_nsamp[i] frames at d_pcm + d_pcm_offs[i],
 *                                    its output (out_samples(d_nsamp[i]) frames) at d_out + d_out_offs[i]: equal to one
 *                                    audio_resample call on the whole stream.  Asynchronous on `stream`.
 * amvhip_audio_resample_batch        the same with host buffers (H2D, kernels, D2H, synchronous); pcm_samples / out_samples are
 *                                    the sizes in int16 of the whole arrays the offsets index into.
 * amvhip_audio_resample_init / amvhip_audio_resample / amvhip_audio_resample_close
 *                                    the reference's streaming calls with their argument order (output first): every packet of
 *                                    nb_samples frames goes to the device and returns the reference's count, the unconsumed tail
 *                                    and the filter position kept between calls (also the reference's lenout cap of
 *                                    4 * nb_samples * ratio + 16 outputs per call).  init: NULL for bad arguments (input or output
 *                                    channels beyond 2, as resample.c:134-138 refuses) or without a device; resample: the count,
 *                                    or a negative AMVHIP_ERR_*.
 */
#define AMVHIP_AUDIO_RATE_MIN 1000
#define AMVHIP_AUDIO_RATE_MAX 192000
uint64_t amvhip_audio_resample_out_samples(uint32_t in_rate, uint32_t out_rate, uint64_t in_samples);
int amvhip_audio_resample_batch_dev(amvhip_ctx *ctx, const int16_t *d_pcm, const uint64_t *d_pcm_offs, const uint64_t *d_nsamp,
                                    uint32_t n, uint32_t in_channels, uint32_t in_rate, int16_t *d_out,
                                    const uint64_t *d_out_offs, uint32_t out_channels, uint32_t out_rate, void *stream);
int amvhip_audio_resample_batch(amvhip_ctx *ctx, const int16_t *pcm, uint64_t pcm_samples, const uint64_t *pcm_offs,
                                const uint64_t *nsamp, uint32_t n, uint32_t in_channels, uint32_t in_rate, int16_t *out,
                                uint64_t out_samples, const uint64_t *out_offs, uint32_t out_channels, uint32_t out_rate);
typedef struct amvhip_audio_resampler amvhip_audio_resampler;
amvhip_audio_resampler *amvhip_audio_resample_init(amvhip_ctx *ctx, int output_channels, int input_channels, int output_rate,
                                                   int input_rate);
int amvhip_audio_resample(amvhip_audio_resampler *r, short *output, short *input, int nb_samples);
void amvhip_audio_resample_close(amvhip_audio_resampler *r);
/* Stage access: quantised coefficients (zig-zag order, not predicted), n*nmcu*6*64 int16 */
int amvhip_encode_coefs_dev(amvhip_ctx *ctx, const uint8_t *d_pix, uint32_t pix_stride, int is_bgr,
                            uint32_t n, uint32_t width, uint32_t height, uint32_t qbias,
                            int16_t *d_coef, void *stream);
/* ... and what the trellis quantiser makes of them (see amvhip_encode_trellis_batch_dev) */
int amvhip_encode_trellis_coefs_dev(amvhip_ctx *ctx, const uint8_t *d_pix, uint32_t pix_stride, int is_bgr,
                                    uint32_t n, uint32_t width, uint32_t height, uint32_t qbias, uint32_t lambda,
                                    int16_t *d_coef, void *stream);

/*
 * IMA ADPCM, AMV chunk layout (AMVDec.c:312-320 + AdpcmIma.c:206-242; adpcm.c:461-498).
 * decode: chunk i = {s16 predictor, u8 step_index, u8 0, u32 nsamples, nibbles}; writes
 *         2*(len-8) samples at d_pcm + d_pcm_offs[i] (offsets in samples).
 * encode: chunk i takes d_nsamp[i] (even) samples from d_pcm + d_pcm_offs[i] and writes
 *         8 + nsamp/2 bytes at d_blob + d_offs[i].  step_index handling:
 *         d_step_in != NULL : chunk i starts from d_step_in[i] (independent chunks);
 *         d_step_in == NULL : the reference's behaviour, step_index carried from chunk i-1
 *                             (chunk 0 starts at 0); chunks of one call form one stream.  The chain is
 *                             resolved on the device (guessed starts, chunks that guessed wrong coded
 *                             again; a stream that does not settle takes an exhaustive 89-start map
 *                             instead), never by a serial pass and never by waiting for the stream.
 */
int amvhip_adpcm_decode_batch_dev(amvhip_ctx *ctx, const uint8_t *d_blob, uint64_t blob_bytes,
                                  const uint64_t *d_offs, const uint32_t *d_lens, uint32_t n,
                                  int16_t *d_pcm, const uint64_t *d_pcm_offs,
                                  int32_t *d_final_state /* optional: n x {predictor, step_index} */,
                                  void *stream);
int amvhip_adpcm_encode_batch_dev(amvhip_ctx *ctx, const int16_t *d_pcm, const uint64_t *d_pcm_offs,
                                  const uint32_t *d_nsamp, uint32_t n, const int32_t *d_step_in,
                                  uint8_t *d_blob, const uint64_t *d_offs, void *stream);
/* The 89 factors r[i] with which the encode kernels take min(7, |delta| * 4 / step[i]) as trunc((float)|delta| * r[i])
 * (host arithmetic, no device needed): published so that the exactness of that shortcut can be checked off the device. */
void amvhip_adpcm_quotient_table(float out[89]);
/* Diagnostic of the last amvhip_adpcm_encode_batch_dev call with d_step_in == NULL (waits for the device):
 * out[0] = 1 if the stream took the exhaustive route, out[1..] = chunks coded again in sweep 1, 2, ... (0-terminated,
 * at most 60).  Returns AMVHIP_OK, or AMVHIP_ERR_ARG when no such call has been made. */
int amvhip_adpcm_chain_stats(amvhip_ctx *ctx, uint32_t out[64]);
/* host-buffer forms (H2D, kernel, D2H, synchronous).  pcm_samples / blob_bytes are the sizes of
 * the whole pcm / blob arrays the offsets index into. */
int amvhip_adpcm_decode_batch(amvhip_ctx *ctx, const uint8_t *blob, uint64_t blob_bytes,
                              const uint64_t *offs, const uint32_t *lens, uint32_t n,
                              int16_t *pcm, uint64_t pcm_samples, const uint64_t *pcm_offs,
                              int32_t *final_state);
int amvhip_adpcm_decode_batch_async(amvhip_ctx *ctx, const uint8_t *blob, uint64_t blob_bytes,
                                    const uint64_t *offs, const uint32_t *lens, uint32_t n,
                                    int16_t *pcm, uint64_t pcm_samples, const uint64_t *pcm_offs,
                                    int32_t *final_state);   /* see amvhip_decode_batch_async */
int amvhip_adpcm_encode_batch(amvhip_ctx *ctx, const int16_t *pcm, uint64_t pcm_samples,
                              const uint64_t *pcm_offs, const uint32_t *nsamp, uint32_t n,
                              const int32_t *step_in, uint8_t *blob, uint64_t blob_bytes,
                              const uint64_t *offs);
/* One AMV audio chunk, host buffers, the step index handed in and out (what adpcm_encode_frame keeps in its
 * context between calls, adpcm.c:461-498).  nsamp even and > 0; writes 8 + nsamp/2 bytes, returns that count. */
int amvhip_adpcm_encode_frame(amvhip_ctx *ctx, const int16_t *samples, uint32_t nsamp, int32_t *step_index,
                              uint8_t *chunk, uint32_t cap);
/* The reference's `-trellis N` quality mode (adpcm_compress_trellis, adpcm.c:287-443, as the AMV case calls it :482-487):
 * a beam search over the 2^N best decoder states instead of the plain quantiser, 1 <= N <= 5; same chunk layout, lower
 * error.  The batch form takes independent chunks (d_step_in required, d_step_out optional: the index each chunk ends
 * on); the frame form hands the index in and out like amvhip_adpcm_encode_frame. */
int amvhip_adpcm_encode_trellis_batch_dev(amvhip_ctx *ctx, const int16_t *d_pcm, const uint64_t *d_pcm_offs,
                                          const uint32_t *d_nsamp, uint32_t n, const int32_t *d_step_in, uint32_t trellis,
                                          uint8_t *d_blob, const uint64_t *d_offs, int32_t *d_step_out, void *stream);
int amvhip_adpcm_encode_frame_trellis(amvhip_ctx *ctx, const int16_t *samples, uint32_t nsamp, int32_t *step_index,
                                      uint32_t trellis, uint8_t *chunk, uint32_t cap);
/* `-trellis N` for a whole stream: the chunks of one call are one stream, in order.  Chunk 0 starts from
 * first_step_index (clipped to 0..88; 0 is a fresh encoder context, a track coded in windows hands in the previous
 * call's last end index), chunk i > 0 from the index chunk i - 1 ends on: byte for byte and index for index what a loop
 * over amvhip_adpcm_encode_frame_trellis gives.  Chunk layout, the nsamp & ~1 rule and the nsamp == 0 chunk (eight header
 * bytes, its end is its start) as in amvhip_adpcm_encode_trellis_batch_dev; no byte of d_blob outside the chunks'
 * 8 + nsamp/2 bytes is written.  d_step_out (optional) receives the n end indices.  The chain is resolved on the device
 * (guessed starts, a fixed number of sweeps that code again whoever guessed wrong, a check, and an 89-start map behind
 * it for a stream that does not settle): the device form only enqueues on `stream` -- no host synchronisation, no launch
 * per chunk, the same launches whatever n and the samples.  Calls of one context are ordered on the device by the
 * caller (one stream at a time), as for every _dev entry point. */
int amvhip_adpcm_encode_trellis_stream_dev(amvhip_ctx *ctx, const int16_t *d_pcm, const uint64_t *d_pcm_offs,
                                           const uint32_t *d_nsamp, uint32_t n, int32_t first_step_index, uint32_t trellis,
                                           uint8_t *d_blob, const uint64_t *d_offs, int32_t *d_step_out, void *stream);
/* host-buffer form (H2D, kernels, D2H, synchronous) */
int amvhip_adpcm_encode_trellis_stream(amvhip_ctx *ctx, const int16_t *pcm, uint64_t pcm_samples, const uint64_t *pcm_offs,
                                       const uint32_t *nsamp, uint32_t n, int32_t first_step_index, uint32_t trellis,
                                       uint8_t *blob, uint64_t blob_bytes, const uint64_t *offs, int32_t *step_out);
/* Diagnostic of the last trellis stream call (waits for the device), laid out as amvhip_adpcm_chain_stats: out[0] = 1 if
 * the stream took the fall-back route, out[1..] = chunks coded again in sweep 1, 2, ... (0-terminated).  Returns
 * AMVHIP_OK, or AMVHIP_ERR_ARG when no such call has been made. */
int amvhip_adpcm_trellis_chain_stats(amvhip_ctx *ctx, uint32_t out[64]);
/* The framing the reference's AMV audio encoder and muxer apply around the kernel (host arithmetic only):
 * amvhip_amv_audio_pairs      adpcm.c:469-477,497: sample pairs of the next chunk for a nominal frame_size (odd sizes
 *                             alternate, a chunk that would straddle a whole second is stretched to end on it);
 *                             *extra (0/1) and *samples_written are the stream state, both start at 0.
 * amvhip_amv_audio_frame_size amvenc.c:276-281: frame_size = sample_rate * time_base (22050/16 -> 1378). */
uint32_t amvhip_amv_audio_pairs(uint32_t frame_size, uint32_t sample_rate, uint32_t *extra, uint64_t *samples_written);
uint32_t amvhip_amv_audio_frame_size(uint32_t sample_rate, uint32_t tb_num, uint32_t tb_den);
/* amvlib's IMA-WAV-layout encoder (AdpcmIma.c:43-160), one mono frame, host buffers; backs
 * AdpcmImaEncodeFrame.  state = {prev_sample (out), step_index (in/out)}; returns bytes written. */
int amvhip_adpcm_wav_encode_frame(amvhip_ctx *ctx, const int16_t *samples, int frame_size,
                                  int32_t state[2], uint8_t *frame, int buf_size);

/* Seeded synthetic sources of BASELINE.md section 4, generated on the device
 * (integer-only; byte-identical to the CPU generator used by the parity tests). */
int amvhip_synth_frames_dev(amvhip_ctx *ctx, uint32_t seed, uint32_t first_frame, uint32_t n,
                            uint32_t width, uint32_t height, uint8_t *d_rgb, void *stream);
int amvhip_synth_audio_dev(amvhip_ctx *ctx, uint32_t seed, uint64_t first_sample, uint64_t n,
                           int16_t *d_pcm, void *stream);

/*
 * AMV container writer (host C, no device work): the muxer half of the path, with the layout
 * AMVmuxer/ffmpeg/libavformat/amvenc.c writes -- 304-byte header (amvh :128-177, two strl lists
 * :181-262), "movi" at 0x138, unpadded 00dc/01wb chunks (:317-321) in strict video/audio alternation
 * (:378-406), counters and duration patched at close (:72-114), "AMV_END_" trailer (:332).  The reader
 * half is AmvOpen / AmvReadNextFrame above.  bit rates: what FFmpeg's codec contexts would hold
 * (its defaults are 200000 and 64000); they only fill the two byte-rate fields.
 * open: NULL on error; write_frame / close: 0 or -1.
 */
typedef struct amvhip_muxer amvhip_muxer;
amvhip_muxer *amvhip_mux_open(const char *path, uint32_t width, uint32_t height, uint32_t fps,
                              uint32_t sample_rate, uint32_t video_bit_rate, uint32_t audio_bit_rate);
int amvhip_mux_write_frame(amvhip_muxer *m, const uint8_t *video, uint32_t video_len, const uint8_t *audio,
                           uint32_t audio_len);
int amvhip_mux_close(amvhip_muxer *m);
/*
 * amvhip_mux_file_bytes: exactly the size of the file open / write_frame x n / close leave for payloads of video_bytes and
 * audio_bytes in all -- the header, "movi", a tag and a size per chunk, the unpadded payloads, the trailer.
 * amvhip_mux_video_total: its inverse, the largest video_bytes with amvhip_mux_file_bytes(n, video_bytes, audio_bytes) <=
 * file_bytes, or 0 if there is none: the `total` of a clip entry for a caller whose card has file_bytes left.
 */
uint64_t amvhip_mux_file_bytes(uint32_t n, uint64_t video_bytes, uint64_t audio_bytes);
uint64_t amvhip_mux_video_total(uint64_t file_bytes, uint32_t n, uint64_t audio_bytes);

/*
 * Kernel timing with HIP events recorded on the launch stream around every kernel
 * launch (bench.py's roofline leg).  Off by default.  amvhip_prof_read synchronises the
 * events recorded since the last reset and returns launches / summed milliseconds.
 */
#define AMVHIP_K_HUFFMAN 0
#define AMVHIP_K_RECON 1
#define AMVHIP_K_FDCT 2
#define AMVHIP_K_PACK 3
#define AMVHIP_K_ADPCM_DEC 4
#define AMVHIP_K_ADPCM_ENC 5       /* map + chain + encode kernels, timed as one (the map dominates) */
#define AMVHIP_K_SYNTH 6
#define AMVHIP_K_HUFFMAN_SERIAL 7
#define AMVHIP_K_UNSTUFF 8
#define AMVHIP_K_PACK_SERIAL 9
#define AMVHIP_K_COMPACT 10   /* amv_scan_kernel + amv_gather_kernel, timed as one */
#define AMVHIP_K_AUDIO_RESAMPLE 11   /* amv_audio_tiles_kernel + amv_audio_resample_kernel, timed as one */
#define AMVHIP_K_PIXFMT 12   /* the amv_pix_*_kernel family (amvhip_img_convert_dev and the entries built on it) */
#define AMVHIP_K_COUNT 13
void amvhip_prof_enable(amvhip_ctx *ctx, int on);
void amvhip_prof_reset(amvhip_ctx *ctx);
int amvhip_prof_read(amvhip_ctx *ctx, int kernel, uint64_t *launches, double *total_ms);
const char *amvhip_kernel_name(int kernel);

#ifdef __cplusplus
}
#endif
#endif /* AMVHIP_H */
