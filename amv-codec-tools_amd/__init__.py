"""amv-codec-tools_amd -- MI355X-native AMV codec hot path (video decode/encode, IMA ADPCM).

The product is libamvhip.so (HIP kernels for gfx950 behind a C ABI, include/amvhip.h).  This
module is the thin ctypes binding tests and bench.py use; it contains no codec arithmetic and
no CPU fallback: importing it without the built library raises.

The directory name is not a Python identifier; load it with `__graft_entry__.load_package()`.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AMVHIP_LIB") or os.path.join(_HERE, "libamvhip.so")   # override: kernel experiments

OK, ERR_ARG, ERR_DEVICE, ERR_NOMEM, ERR_SPACE = 0, -1, -2, -3, -4
ST_FORMAT, ST_OVERRUN, ST_TRUNCATED = 1, 2, 4
ST_RANGE = 8            # requant: a block outside the range the search is proved for
ST_TABLE = 16           # retable: the frame's table index names no table
RETABLE_TABLES_MAX = 64
FLAG_ZIGZAG_FIXED = 1
FLAG_FFMPEG = 2
FLAG_FFMPEG_KEEP = 4
QBIAS_AMV, QBIAS_MJPEG = 0, 128
K_HUFFMAN, K_RECON, K_FDCT, K_PACK, K_ADPCM_DEC, K_ADPCM_ENC, K_SYNTH, K_HUFFMAN_SERIAL, K_UNSTUFF, K_PACK_SERIAL, K_COMPACT = range(11)
K_AUDIO_RESAMPLE = 11
K_PIXFMT = 12
(PIX_YUV420P, PIX_YUVJ420P, PIX_YUV422P, PIX_YUVJ422P, PIX_YUV444P, PIX_YUVJ444P, PIX_YUYV422, PIX_UYVY422, PIX_RGB24, PIX_BGR24,
 PIX_RGB32, PIX_RGB565, PIX_RGB555, PIX_GRAY8) = range(14)
PIX_COUNT = 14
AUDIO_RATE_MIN, AUDIO_RATE_MAX = 1000, 192000
ENTROPY_AUTO, ENTROPY_SERIAL = 0, 1
RATE_RUNGS_MAX, RATE_OVER = 16, 0x80000000

_vp, _u8p = ctypes.c_void_p, ctypes.c_void_p
_u32, _u64, _i32, _int = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int32, ctypes.c_int


class AMVInfo(ctypes.Structure):  # include/amvhip.h, reference AMVDec.h:29-47
    _fields_ = [("dwMicroSecPerFrame", ctypes.c_uint), ("dwWidth", ctypes.c_uint), ("dwHeight", ctypes.c_uint),
                ("dwSpeed", ctypes.c_uint), ("dwTimeSec", ctypes.c_uint), ("dwTimeMin", ctypes.c_uint),
                ("dwTimeHour", ctypes.c_uint), ("wFormatTag", ctypes.c_ushort), ("nChannels", ctypes.c_ushort),
                ("nSamplesPerSec", ctypes.c_uint), ("nAvgBytesPerSec", ctypes.c_uint),
                ("nBlockAlign", ctypes.c_ushort), ("wBitsPerSample", ctypes.c_ushort),
                ("cbSize", ctypes.c_ushort), ("wSamplesPerBlock", ctypes.c_ushort)]


class FRAMEBUFF(ctypes.Structure):  # AMVDec.h:50-57
    _fields_ = [("videobuff", ctypes.POINTER(ctypes.c_ubyte)), ("audiobuff", ctypes.POINTER(ctypes.c_ubyte)),
                ("videobufflen", ctypes.c_uint), ("audiobufflen", ctypes.c_uint), ("framenum", ctypes.c_int)]


class VIDEOBUFF(ctypes.Structure):  # AMVDec.h:59-63
    _fields_ = [("fbmpdat", ctypes.POINTER(ctypes.c_ubyte)), ("len", ctypes.c_uint)]


class AUDIOBUFF(ctypes.Structure):  # AMVDec.h:67-71
    _fields_ = [("audiodata", ctypes.POINTER(ctypes.c_short)), ("len", ctypes.c_uint)]


class AMVDecoder(ctypes.Structure):  # AMVDec.h:74-91
    _fields_ = [("amvfilename", ctypes.c_char_p), ("opened", ctypes.c_int), ("dataseekpos", ctypes.c_long),
                ("fileseekpos", ctypes.c_long), ("amvinfo", AMVInfo), ("currentframe", ctypes.c_uint),
                ("totalframe", ctypes.c_uint), ("framebuf", FRAMEBUFF), ("videobuf", VIDEOBUFF),
                ("audiobuf", AUDIOBUFF)]


class ADPCMChannelStatus(ctypes.Structure):  # AdpcmIma.h:11-18
    _fields_ = [("predictor", ctypes.c_int), ("step_index", ctypes.c_short), ("step", ctypes.c_int),
                ("prev_sample", ctypes.c_int)]


class ADPCMContext(ctypes.Structure):  # AdpcmIma.h:20-25
    _fields_ = [("channel", ctypes.c_int), ("status", ADPCMChannelStatus * 2), ("sample_buffer", ctypes.c_short * 32)]


# every symbol include/amvhip.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "PrepareForVideoDecode": (None, [ctypes.POINTER(AMVInfo)]),
    "AmvJpegDecode": (_int, [ctypes.POINTER(AMVInfo), ctypes.POINTER(FRAMEBUFF), ctypes.POINTER(VIDEOBUFF)]),
    "AdpcmImaDecodeFrame": (_int, [ctypes.POINTER(ADPCMContext), _vp, ctypes.POINTER(_int), _vp, _int]),
    "AdpcmImaEncodeFrame": (_int, [ctypes.POINTER(ADPCMContext), _int, _int, _vp, _int, _vp]),
    "AmvOpen": (ctypes.POINTER(AMVDecoder), [ctypes.c_char_p]),
    "AmvClose": (None, [ctypes.POINTER(AMVDecoder)]),
    "AmvReadNextFrame": (_int, [ctypes.POINTER(AMVDecoder)]),
    "AmvRewindFrameStart": (_int, [ctypes.POINTER(AMVDecoder)]),
    "AmvVideoDecode": (_int, [ctypes.POINTER(AMVDecoder)]),
    "AmvAudioDecode": (_int, [ctypes.POINTER(AMVDecoder)]),
    "AmvJpegPutHeader": (None, [_vp, ctypes.c_ushort, ctypes.c_ushort]),
    "AmvCreateJpegFileFromFrameBuffer": (_int, [ctypes.POINTER(AMVDecoder), ctypes.c_char_p]),
    "AmvCreateJpegFileFromBuffer": (_int, [ctypes.POINTER(AMVInfo), ctypes.POINTER(FRAMEBUFF), ctypes.c_char_p]),
    "AmvConvertJpegFileToBmpFile": (_int, [ctypes.c_char_p, ctypes.c_char_p]),
    "ConvertJpegFileToBmpFile": (_int, [ctypes.c_char_p, ctypes.c_char_p]),
    "AmvCreateWavFileFromAmvFile": (_int, [ctypes.POINTER(AMVDecoder), _int, ctypes.c_char_p]),
    "decode_amv_frame": (_int, [_vp, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, _vp]),
    "encode_amv_frame": (_int, [_vp, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, _int, _vp, ctypes.c_uint]),
    "amvhip_create": (_int, [ctypes.POINTER(_vp), _int]),
    "amvhip_destroy": (None, [_vp]),
    "amvhip_last_error": (ctypes.c_char_p, [_vp]),
    "amvhip_device": (_int, [_vp]),
    "amvhip_stride": (_u32, [_u32]),
    "amvhip_frame_bytes": (_u64, [_u32, _u32]),
    "amvhip_yuv420_frame_bytes": (_u64, [_u32, _u32]),
    "amvhip_encode_bound": (_u32, [_u32, _u32]),
    "amvhip_jpeg_header": (_u32, [ctypes.c_ushort, ctypes.c_ushort, _vp, _u32]),
    "amvhip_decode_batch_dev": (_int, [_vp, _vp, _u64, _vp, _vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp]),
    "amvhip_decode_submit_dev": (_int, [_vp, _vp, _u64, _vp, _vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp]),
    "amvhip_decode_collect_dev": (_int, [_vp, _vp]),
    "amvhip_decode_workspace_per_frame": (ctypes.c_double, [_vp]),
    "amvhip_decode_batch": (_int, [_vp, _vp, _u64, _vp, _vp, _u32, _u32, _u32, _u32, _vp, _vp]),
    "amvhip_decode_batch_async": (_int, [_vp, _vp, _u64, _vp, _vp, _u32, _u32, _u32, _u32, _vp, _vp]),
    "amvhip_sync": (_int, [_vp]),
    "amvhip_host_alloc": (_int, [_vp, ctypes.POINTER(_vp), ctypes.c_size_t]),
    "amvhip_host_free": (None, [_vp, _vp]),
    "amvhip_huffman_decode_dev": (_int, [_vp, _vp, _u64, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp, _vp]),
    "amvhip_reconstruct_dev": (_int, [_vp, _vp, _vp, _u32, _u32, _u32, _u32, _vp, _vp]),
    "amvhip_encode_batch_dev": (_int, [_vp, _vp, _u32, _int, _u32, _u32, _u32, _u32, _vp, _u64, _vp, _vp, _vp]),
    "amvhip_encode_batch": (_int, [_vp, _vp, _u32, _int, _u32, _u32, _u32, _u32, _vp, _u64, _vp, _vp]),
    "amvhip_encode_yuv420_batch_dev": (_int, [_vp, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _u32, _u32, _u32, _u32, _vp, _u64, _vp, _vp, _vp]),
    "amvhip_encode_yuv422_batch_dev": (_int, [_vp, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _u32, _u32, _u32, _u32, _vp, _u64, _vp, _vp, _vp]),
    "amvhip_encode_yuv420_batch": (_int, [_vp, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _u32, _u32, _u32, _u32, _vp, _u64, _vp, _vp]),
    "amvhip_encode_yuv422_batch": (_int, [_vp, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _u32, _u32, _u32, _u32, _vp, _u64, _vp, _vp]),
    "amvhip_encode_nr_max": (_u32, [_u32, _u32]),
    "amvhip_encode_yuv420_nr_stream_dev": (_int, [_vp, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _u64, _vp, _vp, _vp]),
    "amvhip_encode_yuv420_nr_stream": (_int, [_vp, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _u64, _vp, _vp]),
    "amvhip_encode_nr_stream_dev": (_int, [_vp, _vp, _u32, _int, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _u64, _vp, _vp, _vp]),
    "amvhip_encode_nr_stream": (_int, [_vp, _vp, _u32, _int, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _u64, _vp, _vp]),
    "amvhip_encode_trellis_lambda_max": (_u32, []),
    "amvhip_encode_trellis_lambda": (_u32, [_u32]),
    "amvhip_encode_trellis_batch_dev": (_int, [_vp, _vp, _u32, _int, _u32, _u32, _u32, _u32, _u32, _vp, _u64, _vp, _vp, _vp]),
    "amvhip_encode_trellis_batch": (_int, [_vp, _vp, _u32, _int, _u32, _u32, _u32, _u32, _u32, _vp, _u64, _vp, _vp]),
    "amvhip_encode_yuv420_trellis_batch_dev": (_int, [_vp, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _u32, _u32, _u32, _u32, _u32, _vp, _u64, _vp, _vp, _vp]),
    "amvhip_encode_yuv420_trellis_batch": (_int, [_vp, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _u32, _u32, _u32, _u32, _u32, _vp, _u64, _vp, _vp]),
    "amvhip_encode_yuv420_nr_trellis_stream_dev": (_int, [_vp, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _u64, _vp, _vp, _vp]),
    "amvhip_encode_yuv420_nr_trellis_stream": (_int, [_vp, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _u64, _vp, _vp]),
    "amvhip_encode_nr_trellis_stream_dev": (_int, [_vp, _vp, _u32, _int, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _u64, _vp, _vp, _vp]),
    "amvhip_encode_nr_trellis_stream": (_int, [_vp, _vp, _u32, _int, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _u64, _vp, _vp]),
    "amvhip_resample_yuv420_dev": (_int, [_vp, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _u32, _u32, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _u32, _u32, _u32, _vp]),
    "amvhip_encode_yuv420_scaled_batch_dev": (_int, [_vp, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _u64, _vp, _vp, _vp]),
    "amvhip_img_convert_supported": (_int, [_int, _int, _u32, _u32]),
    "amvhip_pix_frame_bytes": (_u64, [_int, _u32, _u32]),
    "amvhip_img_convert_dev": (_int, [_vp, _int, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _int, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _u32, _u32, _u32, _vp]),
    "amvhip_img_convert": (_int, [_vp, _int, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _int, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _u32, _u32, _u32]),
    "amvhip_sws_scale_dev": (_int, [_vp, _int, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _u32, _u32, _int, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _u32, _u32, _u32, _vp]),
    "amvhip_encode_fmt_scaled_batch_dev": (_int, [_vp, _int, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _u64, _vp, _vp, _vp]),
    "amvhip_pad_color_from_rgb": (None, [_u32, _vp]),
    "amvhip_deinterlace_supported": (_int, [_int, _u32, _u32]),
    "amvhip_deinterlace_dev": (_int, [_vp, _int, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _u32, _u32, _u32, _vp]),
    "amvhip_deinterlace": (_int, [_vp, _int, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _u32, _u32, _u32]),
    "amvhip_video_frontend_dev": (_int, [_vp, _int, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _u32, _u32, _vp]),
    "amvhip_encode_frontend_batch_dev": (_int, [_vp, _int, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _u32, _u32, _u32, _vp, _u32, _u32, _u32, _vp, _u64, _vp, _vp, _vp]),
    "amvhip_encode_frontend_quant_stream_dev": (_int, [_vp, _int, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _u32, _u32, _u32, _vp, _u32, _u32, _vp, _vp, _u64, _vp, _vp, _vp]),
    "amvhip_psnr_db": (ctypes.c_double, [_u64, _u64]),
    "amvhip_psnr_report": (None, [_vp, _u32, _u32, _u32, _vp]),
    "amvhip_picture_sse_supported": (_int, [_int, _u32, _u32]),
    "amvhip_picture_sse_dev": (_int, [_vp, _int, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _u32, _u32, _u32, _vp, _vp]),
    "amvhip_picture_sse": (_int, [_vp, _int, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _u32, _u32, _u32, _vp]),
    "amvhip_encode_quant_psnr_stream_dev": (_int, [_vp, _vp, _u32, _int, _u32, _u32, _u32, _vp, _vp, _u64, _vp, _vp, _vp, _vp]),
    "amvhip_encode_yuv420_quant_psnr_stream_dev": (_int, [_vp, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _u32, _u32, _u32, _vp, _vp, _u64, _vp, _vp, _vp, _vp]),
    "amvhip_encode_frontend_quant_psnr_stream_dev": (_int, [_vp, _int, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _u32, _u32, _u32, _vp, _u32, _u32, _vp, _vp, _u64, _vp, _vp, _vp, _vp]),
    "amvhip_encode_qns_lambda2_max": (_u32, []),
    "amvhip_encode_qns_lambda2": (_u32, [_u32]),
    "amvhip_encode_qns_stream_dev": (_int, [_vp, _vp, _u32, _int, _u32, _u32, _u32, _vp, _u32, _u32, _vp, _u64, _vp, _vp, _vp, _vp]),
    "amvhip_encode_yuv420_qns_stream_dev": (_int, [_vp, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _u32, _u32, _u32, _vp, _u32, _u32, _vp, _u64, _vp, _vp, _vp, _vp]),
    "amvhip_encode_frontend_qns_stream_dev": (_int, [_vp, _int, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _u32, _u32, _u32, _vp, _u32, _u32, _vp, _u32, _u32, _vp, _u64, _vp, _vp, _vp, _vp]),
    "amvhip_encode_qns_coefs_dev": (_int, [_vp, _vp, _u32, _int, _u32, _u32, _u32, _vp, _u32, _u32, _vp, _vp]),
    "amvhip_encode_rate_probe_dev": (_int, [_vp, _vp, _u32, _int, _u32, _u32, _u32, _vp, _vp, _u32, _vp, _vp]),
    "amvhip_encode_yuv420_rate_probe_dev": (_int, [_vp, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _u32, _u32, _u32, _vp, _vp, _u32, _vp, _vp]),
    "amvhip_encode_rate_stream_dev": (_int, [_vp, _vp, _u32, _int, _u32, _u32, _u32, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp]),
    "amvhip_encode_yuv420_rate_stream_dev": (_int, [_vp, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _u32, _u32, _u32, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp]),
    "amvhip_encode_frontend_rate_stream_dev": (_int, [_vp, _int, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _u32, _u32, _u32, _vp, _u32, _u32, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp]),
    "amvhip_requant_stream_dev": (_int, [_vp, _vp, _u64, _vp, _vp, _u32, _u32, _u32, _u32, _vp, _u64, _vp, _vp, _vp, _vp, _vp]),
    "amvhip_requant_rate_probe_dev": (_int, [_vp, _vp, _u64, _vp, _vp, _u32, _u32, _u32, _vp, _u32, _vp, _vp]),
    "amvhip_requant_rate_stream_dev": (_int, [_vp, _vp, _u64, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp]),
    "amvhip_encode_clip_stream_dev": (_int, [_vp, _vp, _u32, _int, _u32, _u32, _u32, _vp, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _vp, _vp]),
    "amvhip_encode_yuv420_clip_stream_dev": (_int, [_vp, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _u32, _u32, _u32, _vp, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _vp, _vp]),
    "amvhip_encode_frontend_clip_stream_dev": (_int, [_vp, _int, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _u32, _u32, _u32, _vp, _u32, _u32, _vp, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _vp, _vp]),
    "amvhip_requant_clip_stream_dev": (_int, [_vp, _vp, _u64, _vp, _vp, _u32, _u32, _u32, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "amvhip_retable_stream_dev": (_int, [_vp, _vp, _u64, _vp, _vp, _u32, _u32, _u32, _vp, _u32, _vp, _u64, _vp, _vp, _vp, _vp, _vp]),
    "amvhip_retable_rate_probe_dev": (_int, [_vp, _vp, _u64, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _u32, _vp, _vp]),
    "amvhip_retable_rate_stream_dev": (_int, [_vp, _vp, _u64, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp]),
    "amvhip_retable_clip_stream_dev": (_int, [_vp, _vp, _u64, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "amvhip_ffmpeg_amv_tables": (_int, [_u32, _vp]),
    "amvhip_decode_fmt_batch_dev": (_int, [_vp, _vp, _u64, _vp, _vp, _u32, _u32, _u32, _u32, _int, _vp, _u32, _vp, _vp]),
    "amvhip_lowres_dim": (_u32, [_u32, _u32]),
    "amvhip_lowres_frame_bytes": (_u64, [_u32, _u32, _u32]),
    "amvhip_decode_lowres_batch_dev": (_int, [_vp, _vp, _u64, _vp, _vp, _u32, _u32, _u32, _u32, _u32, _int, _vp, _u32, _vp, _vp]),
    "amvhip_decode_lowres_batch": (_int, [_vp, _vp, _u64, _vp, _vp, _u32, _u32, _u32, _u32, _u32, _int, _vp, _u32, _vp]),
    "amvhip_reconstruct_lowres_dev": (_int, [_vp, _vp, _vp, _u32, _u32, _u32, _u32, _vp, _vp]),
    "amvhip_pp_mode_parse": (_int, [ctypes.c_char_p, _int, _vp]),
    "amvhip_postprocess_supported": (_int, [_u32, _u32]),
    "amvhip_postprocess_dev": (_int, [_vp, _int, _vp, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _u32, _u32, _u32, _vp, _vp]),
    "amvhip_postprocess": (_int, [_vp, _int, _vp, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _u32, _u32, _u32, _vp]),
    "amvhip_decode_pp_batch_dev": (_int, [_vp, _vp, _u64, _vp, _vp, _u32, _u32, _u32, _u32, _int, _vp, _u32, _vp, _vp, _vp, _vp]),
    "amvhip_audio_resample_out_samples": (_u64, [_u32, _u32, _u64]),
    "amvhip_audio_resample_batch_dev": (_int, [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _u32, _u32, _vp]),
    "amvhip_audio_resample_batch": (_int, [_vp, _vp, _u64, _vp, _vp, _u32, _u32, _u32, _vp, _u64, _vp, _u32, _u32]),
    "amvhip_audio_resample_init": (_vp, [_vp, _int, _int, _int, _int]),
    "amvhip_audio_resample": (_int, [_vp, _vp, _vp, _int]),
    "amvhip_audio_resample_close": (None, [_vp]),
    "amvhip_encode_coefs_dev": (_int, [_vp, _vp, _u32, _int, _u32, _u32, _u32, _u32, _vp, _vp]),
    "amvhip_encode_trellis_coefs_dev": (_int, [_vp, _vp, _u32, _int, _u32, _u32, _u32, _u32, _u32, _vp, _vp]),
    "amvhip_adpcm_decode_batch_dev": (_int, [_vp, _vp, _u64, _vp, _vp, _u32, _vp, _vp, _vp, _vp]),
    "amvhip_adpcm_encode_batch_dev": (_int, [_vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp]),
    "amvhip_adpcm_decode_batch": (_int, [_vp, _vp, _u64, _vp, _vp, _u32, _vp, _u64, _vp, _vp]),
    "amvhip_adpcm_decode_batch_async": (_int, [_vp, _vp, _u64, _vp, _vp, _u32, _vp, _u64, _vp, _vp]),
    "amvhip_adpcm_encode_batch": (_int, [_vp, _vp, _u64, _vp, _vp, _u32, _vp, _vp, _u64, _vp]),
    "amvhip_adpcm_encode_frame": (_int, [_vp, _vp, _u32, ctypes.POINTER(_i32), _vp, _u32]),
    "amvhip_adpcm_encode_trellis_batch_dev": (_int, [_vp, _vp, _vp, _vp, _u32, _vp, _u32, _vp, _vp, _vp, _vp]),
    "amvhip_adpcm_encode_frame_trellis": (_int, [_vp, _vp, _u32, ctypes.POINTER(_i32), _u32, _vp, _u32]),
    "amvhip_adpcm_encode_trellis_stream_dev": (_int, [_vp, _vp, _vp, _vp, _u32, _i32, _u32, _vp, _vp, _vp, _vp]),
    "amvhip_adpcm_encode_trellis_stream": (_int, [_vp, _vp, _u64, _vp, _vp, _u32, _i32, _u32, _vp, _u64, _vp, _vp]),
    "amvhip_adpcm_trellis_chain_stats": (_int, [_vp, _vp]),
    "amvhip_amv_audio_pairs": (_u32, [_u32, _u32, ctypes.POINTER(_u32), ctypes.POINTER(_u64)]),
    "amvhip_amv_audio_frame_size": (_u32, [_u32, _u32, _u32]),
    "amvhip_adpcm_wav_encode_frame": (_int, [_vp, _vp, _int, _vp, _vp, _int]),
    "amvhip_synth_frames_dev": (_int, [_vp, _u32, _u32, _u32, _u32, _u32, _vp, _vp]),
    "amvhip_synth_audio_dev": (_int, [_vp, _u32, _u64, _u64, _vp, _vp]),
    "amvhip_set_entropy_mode": (_int, [_vp, _int]),
    "amvhip_entropy_stats": (_int, [_vp, _int, _vp]),
    "amvhip_entropy_trace": (_int, [_vp, _vp, _u32]),
    "amvhip_decode_split_stats": (_int, [_vp, _vp]),
    "amvhip_adpcm_chain_stats": (_int, [_vp, _vp]),
    "amvhip_adpcm_quotient_table": (None, [_vp]),
    "amvhip_prof_enable": (None, [_vp, _int]),
    "amvhip_prof_reset": (None, [_vp]),
    "amvhip_prof_read": (_int, [_vp, _int, ctypes.POINTER(_u64), ctypes.POINTER(ctypes.c_double)]),
    "amvhip_kernel_name": (ctypes.c_char_p, [_int]),
    # container writer (host C)
    "amvhip_mux_open": (_vp, [ctypes.c_char_p, _u32, _u32, _u32, _u32, _u32, _u32]),
    "amvhip_mux_write_frame": (_int, [_vp, _u8p, _u32, _u8p, _u32]),
    "amvhip_mux_close": (_int, [_vp]),
    "amvhip_mux_file_bytes": (_u64, [_u32, _u64, _u64]),
    "amvhip_mux_video_total": (_u64, [_u64, _u32, _u64]),
}

_lib = None


def load_library():
    """dlopen libamvhip.so and type every entry point.  Raises if the library is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libamvhip.so is not built (%s). Run `python amv-codec-tools_amd/build.py`; there is no CPU fallback."
                % LIB_PATH)
        # One HIP runtime per process: PyTorch ships its own libamdhip64 and the tensors this binding is
        # handed live in it.  If libamvhip.so were loaded first it would bring in the system runtime, and
        # the second runtime to initialise finds no usable device.  So torch (when present) goes first.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(lib, name)  # AttributeError if the ABI lost a symbol
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


class AmvHipError(RuntimeError):
    pass


PP_V_DEBLOCK, PP_H_DEBLOCK, PP_DERING, PP_FORCE_QUANT = 0x01, 0x02, 0x04, 0x200000


class PpMode(ctypes.Structure):
    """amvhip_pp_mode of include/amvhip.h: what amvhip_pp_mode_parse makes of a libpostproc mode string"""
    _fields_ = [("lum_mode", ctypes.c_int32), ("chrom_mode", ctypes.c_int32), ("base_dc_diff", ctypes.c_int32),
                ("flatness_threshold", ctypes.c_int32), ("forced_quant", ctypes.c_int32)]

    def __init__(self, lum_mode=0, chrom_mode=0, base_dc_diff=32, flatness_threshold=39, forced_quant=0):
        super().__init__(lum_mode, chrom_mode, base_dc_diff, flatness_threshold, forced_quant)


def pp_mode_parse(name, quality=6):
    """a libpostproc mode string (hb, vb, dr, fq, de and their options) -> PpMode; AmvHipError for anything else"""
    mode = PpMode()
    if load_library().amvhip_pp_mode_parse(name.encode(), quality, ctypes.byref(mode)) != OK:
        raise AmvHipError("pp_mode_parse: %r is not a mode of hb, vb, dr, fq, de" % name)
    return mode


class Frontend(ctypes.Structure):
    """amvhip_frontend of include/amvhip.h: the stages around the shim (all zero: none)"""
    _fields_ = [("deinterlace", _u32), ("crop_top", _u32), ("crop_bottom", _u32), ("crop_left", _u32), ("crop_right", _u32),
                ("pad_top", _u32), ("pad_bottom", _u32), ("pad_left", _u32), ("pad_right", _u32), ("pad_color", ctypes.c_uint8 * 3)]

    def __init__(self, deinterlace=0, crop=(0, 0, 0, 0), pad=(0, 0, 0, 0), pad_color=(16, 128, 128)):
        """crop and pad as (top, bottom, left, right)"""
        super().__init__(int(deinterlace), *crop, *pad, (ctypes.c_uint8 * 3)(*pad_color))


class Quant(ctypes.Structure):
    """amvhip_quant of include/amvhip.h: what amvhip_encode_frontend_quant_stream_dev asks of the quantiser"""
    _fields_ = [("qbias", _u32), ("nr", _u32), ("trellis", _u32), ("lambda_", _u32), ("d_state", _vp)]

    def __init__(self, qbias=0, nr=0, trellis=0, lam=0, state=None):
        """state: int32[65] on the device (a tensor or an address), required when nr > 0; the caller keeps it alive"""
        super().__init__(int(qbias), int(nr), int(trellis), int(lam), _ptr(state))


class Rate(ctypes.Structure):
    """amvhip_rate of include/amvhip.h: a ladder of lambdas (host) and a byte budget per frame, uniform or uint32 [n] on the device"""
    _fields_ = [("ladder", _vp), ("rungs", _u32), ("budget", _u32), ("d_budget", _vp)]

    def __init__(self, ladder, budget=0, d_budget=None, rungs=None):
        """ladder: a sequence of lambdas (kept alive here as a C array), or None for NULL; rungs: the count handed over where
        it is not the ladder's own; d_budget: a tensor or an address the caller keeps alive"""
        self._ladder = None if ladder is None else (_u32 * max(len(ladder), 1))(*[int(x) for x in ladder])
        at = None if self._ladder is None else ctypes.addressof(self._ladder)
        own = 0 if ladder is None else len(ladder)
        super().__init__(at, int(own if rungs is None else rungs), int(budget), _ptr(d_budget))


class Retable(ctypes.Structure):
    """amvhip_retable of include/amvhip.h: the tables the chunks were written against (host) and the frames' table indices
    (uint8 [n] on the device, or None: table 0 for every frame)"""
    _fields_ = [("tables", _vp), ("count", _u32), ("d_table_of", _vp)]

    def __init__(self, tables, d_table_of=None, count=None):
        """tables: uint8 [count][2][64] (anything numpy takes; kept alive here as a C array), or None for NULL; count: the
        count handed over where it is not the tables' own; d_table_of: a tensor or an address the caller keeps alive"""
        flat = None if tables is None else [int(x) for t in tables for comp in t for x in comp]
        self._tables = None if flat is None else (ctypes.c_uint8 * max(len(flat), 1))(*flat)
        at = None if self._tables is None else ctypes.addressof(self._tables)
        own = 0 if flat is None else len(flat) // 128
        super().__init__(at, int(own if count is None else count), _ptr(d_table_of))


def ffmpeg_amv_tables(qscale):
    """the reference encoder's tables at -qscale 1 .. 31 -> [2][64] lists, scan order (None outside); needs no device"""
    out = (ctypes.c_uint8 * 128)()
    if load_library().amvhip_ffmpeg_amv_tables(int(qscale), ctypes.cast(out, ctypes.c_void_p)) != OK:
        return None
    return [list(out[:64]), list(out[64:])]


def pad_color_from_rgb(rrggbb):
    """-padcolor RRGGBB -> (Y, Cb, Cr) as the pad bands are written; needs no device"""
    out = (ctypes.c_uint8 * 3)()
    load_library().amvhip_pad_color_from_rgb(rrggbb, ctypes.cast(out, ctypes.c_void_p))
    return tuple(out)


def _ptr(x):
    """device/host address of a torch tensor, numpy array, bytes object or int; None -> NULL.  The caller keeps x alive
    for the duration of the call; other buffer types (bytearray, memoryview ...) are refused: wrap them in numpy
    (np.frombuffer) so that the address is that of the caller's own memory, never of a temporary copy."""
    if x is None:
        return None
    if isinstance(x, int):
        return x
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    if hasattr(x, "ctypes"):
        return x.ctypes.data
    if isinstance(x, bytes):      # immutable, owned by the caller: input arguments only
        return ctypes.cast(ctypes.c_char_p(x), ctypes.c_void_p).value
    raise TypeError("pass a torch tensor, numpy array, bytes or int address, not %s" % type(x).__name__)


class Context:
    """One amvhip_ctx.  Methods mirror the batch entry points of include/amvhip.h one to one;
    arguments are torch tensors / numpy arrays (their addresses are passed through)."""

    def __init__(self, device=0):
        self.lib = load_library()
        h = ctypes.c_void_p()
        rc = self.lib.amvhip_create(ctypes.byref(h), int(device))
        if rc != OK:
            raise AmvHipError("amvhip_create(device=%d) failed with %d: no usable HIP device" % (device, rc))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.amvhip_destroy(self.h)
            self.h = None

    __del__ = close

    def _check(self, rc, what):
        if rc < 0:
            raise AmvHipError("%s failed (%d): %s" % (what, rc, self.lib.amvhip_last_error(self.h).decode()))
        return rc

    # geometry
    def stride(self, w):
        return self.lib.amvhip_stride(w)

    def frame_bytes(self, w, h):
        return self.lib.amvhip_frame_bytes(w, h)

    def yuv420_frame_bytes(self, w, h):
        return self.lib.amvhip_yuv420_frame_bytes(w, h)

    def encode_bound(self, w, h):
        return self.lib.amvhip_encode_bound(w, h)

    # device-resident
    def decode_batch_dev(self, blob, blob_bytes, offs, lens, n, w, h, flags, out, status, stream=None):
        return self._check(self.lib.amvhip_decode_batch_dev(self.h, _ptr(blob), blob_bytes, _ptr(offs), _ptr(lens), n,
                                                            w, h, flags, _ptr(out), _ptr(status), stream), "decode_batch_dev")

    def decode_submit_dev(self, blob, blob_bytes, offs, lens, n, w, h, flags, out, status, stream=None):
        """queue a batch on the context's own streams; `stream` marks where the inputs are ready and does not wait"""
        return self._check(self.lib.amvhip_decode_submit_dev(self.h, _ptr(blob), blob_bytes, _ptr(offs), _ptr(lens), n,
                                                             w, h, flags, _ptr(out), _ptr(status), stream), "decode_submit_dev")

    def decode_collect_dev(self, stream=None):
        """`stream` waits for the oldest submitted batch"""
        return self._check(self.lib.amvhip_decode_collect_dev(self.h, stream), "decode_collect_dev")

    def decode_workspace_per_frame(self):
        return self.lib.amvhip_decode_workspace_per_frame(self.h)

    def huffman_decode_dev(self, blob, blob_bytes, offs, lens, n, w, h, coef, status, nmcu_ok, stream=None):
        return self._check(self.lib.amvhip_huffman_decode_dev(self.h, _ptr(blob), blob_bytes, _ptr(offs), _ptr(lens), n,
                                                              w, h, _ptr(coef), _ptr(status), _ptr(nmcu_ok), stream),
                           "huffman_decode_dev")

    def reconstruct_dev(self, coef, nmcu_ok, n, w, h, flags, out, stream=None):
        return self._check(self.lib.amvhip_reconstruct_dev(self.h, _ptr(coef), _ptr(nmcu_ok), n, w, h, flags,
                                                           _ptr(out), stream), "reconstruct_dev")

    def encode_batch_dev(self, pix, pix_stride, is_bgr, n, w, h, qbias, blob, blob_cap, offs, lens, stream=None):
        return self._check(self.lib.amvhip_encode_batch_dev(self.h, _ptr(pix), pix_stride, is_bgr, n, w, h, qbias,
                                                            _ptr(blob), blob_cap, _ptr(offs), _ptr(lens), stream),
                           "encode_batch_dev")

    def encode_yuv420_batch_dev(self, y, cb, cr, y_stride, c_stride, y_frame, c_frame, n, w, h, qbias, blob, blob_cap, offs,
                                lens, stream=None):
        return self._check(self.lib.amvhip_encode_yuv420_batch_dev(self.h, _ptr(y), _ptr(cb), _ptr(cr), y_stride, c_stride,
                                                                   y_frame, c_frame, n, w, h, qbias, _ptr(blob), blob_cap,
                                                                   _ptr(offs), _ptr(lens), stream), "encode_yuv420_batch_dev")

    def encode_nr_max(self, w, h):
        """the largest `nr` the -nr entries take at this frame size (0: none but 0)"""
        return self.lib.amvhip_encode_nr_max(w, h)

    def encode_yuv420_nr_stream_dev(self, y, cb, cr, y_stride, c_stride, y_frame, c_frame, n, w, h, qbias, nr, state, blob, blob_cap,
                                    offs, lens, stream=None):
        """the reference's -nr over a stream coded in calls of any size; state: int32[65] on the device (64 sums, the
        count), read at entry and written at exit, all zeros at the start of a stream"""
        return self._check(self.lib.amvhip_encode_yuv420_nr_stream_dev(self.h, _ptr(y), _ptr(cb), _ptr(cr), y_stride, c_stride,
                                                                       y_frame, c_frame, n, w, h, qbias, nr, _ptr(state), _ptr(blob),
                                                                       blob_cap, _ptr(offs), _ptr(lens), stream),
                           "encode_yuv420_nr_stream_dev")

    def encode_yuv420_nr_stream(self, y, cb, cr, y_stride, c_stride, y_frame, c_frame, n, w, h, qbias, nr, state, blob, blob_cap, offs,
                                lens):
        return self._check(self.lib.amvhip_encode_yuv420_nr_stream(self.h, _ptr(y), _ptr(cb), _ptr(cr), y_stride, c_stride,
                                                                   y_frame, c_frame, n, w, h, qbias, nr, _ptr(state), _ptr(blob),
                                                                   blob_cap, _ptr(offs), _ptr(lens)), "encode_yuv420_nr_stream")

    def encode_nr_stream_dev(self, pix, pix_stride, is_bgr, n, w, h, qbias, nr, state, blob, blob_cap, offs, lens, stream=None):
        return self._check(self.lib.amvhip_encode_nr_stream_dev(self.h, _ptr(pix), pix_stride, is_bgr, n, w, h, qbias, nr,
                                                                _ptr(state), _ptr(blob), blob_cap, _ptr(offs), _ptr(lens), stream),
                           "encode_nr_stream_dev")

    def encode_nr_stream(self, pix, pix_stride, is_bgr, n, w, h, qbias, nr, state, blob, blob_cap, offs, lens):
        return self._check(self.lib.amvhip_encode_nr_stream(self.h, _ptr(pix), pix_stride, is_bgr, n, w, h, qbias, nr,
                                                            _ptr(state), _ptr(blob), blob_cap, _ptr(offs), _ptr(lens)),
                           "encode_nr_stream")

    def encode_yuv420_nr_trellis_stream_dev(self, y, cb, cr, y_stride, c_stride, y_frame, c_frame, n, w, h, qbias, nr, lam, state, blob,
                                            blob_cap, offs, lens, stream=None):
        """-nr and the trellis quantiser in one call: the search runs on the denoised outputs; state as in the -nr entries"""
        return self._check(self.lib.amvhip_encode_yuv420_nr_trellis_stream_dev(self.h, _ptr(y), _ptr(cb), _ptr(cr), y_stride, c_stride,
                                                                               y_frame, c_frame, n, w, h, qbias, nr, lam, _ptr(state),
                                                                               _ptr(blob), blob_cap, _ptr(offs), _ptr(lens), stream),
                           "encode_yuv420_nr_trellis_stream_dev")

    def encode_yuv420_nr_trellis_stream(self, y, cb, cr, y_stride, c_stride, y_frame, c_frame, n, w, h, qbias, nr, lam, state, blob,
                                        blob_cap, offs, lens):
        return self._check(self.lib.amvhip_encode_yuv420_nr_trellis_stream(self.h, _ptr(y), _ptr(cb), _ptr(cr), y_stride, c_stride,
                                                                           y_frame, c_frame, n, w, h, qbias, nr, lam, _ptr(state),
                                                                           _ptr(blob), blob_cap, _ptr(offs), _ptr(lens)),
                           "encode_yuv420_nr_trellis_stream")

    def encode_nr_trellis_stream_dev(self, pix, pix_stride, is_bgr, n, w, h, qbias, nr, lam, state, blob, blob_cap, offs, lens, stream=None):
        return self._check(self.lib.amvhip_encode_nr_trellis_stream_dev(self.h, _ptr(pix), pix_stride, is_bgr, n, w, h, qbias, nr, lam,
                                                                        _ptr(state), _ptr(blob), blob_cap, _ptr(offs), _ptr(lens), stream),
                           "encode_nr_trellis_stream_dev")

    def encode_nr_trellis_stream(self, pix, pix_stride, is_bgr, n, w, h, qbias, nr, lam, state, blob, blob_cap, offs, lens):
        return self._check(self.lib.amvhip_encode_nr_trellis_stream(self.h, _ptr(pix), pix_stride, is_bgr, n, w, h, qbias, nr, lam,
                                                                    _ptr(state), _ptr(blob), blob_cap, _ptr(offs), _ptr(lens)),
                           "encode_nr_trellis_stream")

    def encode_trellis_lambda_max(self):
        """the largest `lambda` the trellis entries take"""
        return self.lib.amvhip_encode_trellis_lambda_max()

    def encode_trellis_lambda(self, qscale):
        """the reference's trellis lambda for a -qscale (3481 at 8); 0 where it is above encode_trellis_lambda_max()"""
        return self.lib.amvhip_encode_trellis_lambda(qscale)

    def encode_trellis_batch_dev(self, pix, pix_stride, is_bgr, n, w, h, qbias, lam, blob, blob_cap, offs, lens, stream=None):
        """encode_batch_dev with the trellis quantiser: per block the AC levels of least distortion + lam * bits"""
        return self._check(self.lib.amvhip_encode_trellis_batch_dev(self.h, _ptr(pix), pix_stride, is_bgr, n, w, h, qbias, lam,
                                                                    _ptr(blob), blob_cap, _ptr(offs), _ptr(lens), stream),
                           "encode_trellis_batch_dev")

    def encode_trellis_batch(self, pix, pix_stride, is_bgr, n, w, h, qbias, lam, blob, blob_cap, offs, lens):
        return self._check(self.lib.amvhip_encode_trellis_batch(self.h, _ptr(pix), pix_stride, is_bgr, n, w, h, qbias, lam,
                                                                _ptr(blob), blob_cap, _ptr(offs), _ptr(lens)), "encode_trellis_batch")

    def encode_yuv420_trellis_batch_dev(self, y, cb, cr, y_stride, c_stride, y_frame, c_frame, n, w, h, qbias, lam, blob, blob_cap,
                                        offs, lens, stream=None):
        return self._check(self.lib.amvhip_encode_yuv420_trellis_batch_dev(self.h, _ptr(y), _ptr(cb), _ptr(cr), y_stride, c_stride,
                                                                           y_frame, c_frame, n, w, h, qbias, lam, _ptr(blob),
                                                                           blob_cap, _ptr(offs), _ptr(lens), stream),
                           "encode_yuv420_trellis_batch_dev")

    def encode_yuv420_trellis_batch(self, y, cb, cr, y_stride, c_stride, y_frame, c_frame, n, w, h, qbias, lam, blob, blob_cap, offs,
                                    lens):
        return self._check(self.lib.amvhip_encode_yuv420_trellis_batch(self.h, _ptr(y), _ptr(cb), _ptr(cr), y_stride, c_stride,
                                                                       y_frame, c_frame, n, w, h, qbias, lam, _ptr(blob),
                                                                       blob_cap, _ptr(offs), _ptr(lens)), "encode_yuv420_trellis_batch")

    def encode_yuv422_batch_dev(self, y, cb, cr, y_stride, c_stride, y_frame, c_frame, n, w, h, qbias, blob, blob_cap, offs,
                                lens, stream=None):
        return self._check(self.lib.amvhip_encode_yuv422_batch_dev(self.h, _ptr(y), _ptr(cb), _ptr(cr), y_stride, c_stride,
                                                                   y_frame, c_frame, n, w, h, qbias, _ptr(blob), blob_cap,
                                                                   _ptr(offs), _ptr(lens), stream), "encode_yuv422_batch_dev")

    def encode_yuv420_batch(self, y, cb, cr, y_stride, c_stride, y_frame, c_frame, n, w, h, qbias, blob, blob_cap, offs, lens):
        return self._check(self.lib.amvhip_encode_yuv420_batch(self.h, _ptr(y), _ptr(cb), _ptr(cr), y_stride, c_stride,
                                                               y_frame, c_frame, n, w, h, qbias, _ptr(blob), blob_cap,
                                                               _ptr(offs), _ptr(lens)), "encode_yuv420_batch")

    def encode_yuv422_batch(self, y, cb, cr, y_stride, c_stride, y_frame, c_frame, n, w, h, qbias, blob, blob_cap, offs, lens):
        return self._check(self.lib.amvhip_encode_yuv422_batch(self.h, _ptr(y), _ptr(cb), _ptr(cr), y_stride, c_stride,
                                                               y_frame, c_frame, n, w, h, qbias, _ptr(blob), blob_cap,
                                                               _ptr(offs), _ptr(lens)), "encode_yuv422_batch")

    def encode_coefs_dev(self, pix, pix_stride, is_bgr, n, w, h, qbias, coef, stream=None):
        return self._check(self.lib.amvhip_encode_coefs_dev(self.h, _ptr(pix), pix_stride, is_bgr, n, w, h, qbias,
                                                            _ptr(coef), stream), "encode_coefs_dev")

    def encode_trellis_coefs_dev(self, pix, pix_stride, is_bgr, n, w, h, qbias, lam, coef, stream=None):
        return self._check(self.lib.amvhip_encode_trellis_coefs_dev(self.h, _ptr(pix), pix_stride, is_bgr, n, w, h, qbias, lam,
                                                                    _ptr(coef), stream), "encode_trellis_coefs_dev")

    def adpcm_decode_batch_dev(self, blob, blob_bytes, offs, lens, n, pcm, pcm_offs, final_state=None, stream=None):
        return self._check(self.lib.amvhip_adpcm_decode_batch_dev(self.h, _ptr(blob), blob_bytes, _ptr(offs), _ptr(lens),
                                                                  n, _ptr(pcm), _ptr(pcm_offs), _ptr(final_state), stream),
                           "adpcm_decode_batch_dev")

    def adpcm_encode_batch_dev(self, pcm, pcm_offs, nsamp, n, step_in, blob, offs, stream=None):
        return self._check(self.lib.amvhip_adpcm_encode_batch_dev(self.h, _ptr(pcm), _ptr(pcm_offs), _ptr(nsamp), n,
                                                                  _ptr(step_in), _ptr(blob), _ptr(offs), stream),
                           "adpcm_encode_batch_dev")

    def adpcm_encode_trellis_stream_dev(self, pcm, pcm_offs, nsamp, n, first_step_index, trellis, blob, offs, step_out=None,
                                        stream=None):
        """`-trellis N` over the chunks of the call as one stream, the step index carried on the device"""
        return self._check(self.lib.amvhip_adpcm_encode_trellis_stream_dev(self.h, _ptr(pcm), _ptr(pcm_offs), _ptr(nsamp), n,
                                                                           first_step_index, trellis, _ptr(blob), _ptr(offs),
                                                                           _ptr(step_out), stream),
                           "adpcm_encode_trellis_stream_dev")

    # pixel formats.  A picture is (planes, stride, c_stride, frame_stride, c_frame_stride) with planes a sequence of up to
    # three tensors / arrays / addresses (packed formats and GRAY8: one)
    @staticmethod
    def _pic(pic):
        planes, stride, c_stride, frame, c_frame = pic
        planes = list(planes) + [None] * (3 - len(planes))
        return [_ptr(planes[0]), _ptr(planes[1]), _ptr(planes[2]), stride, c_stride, frame, c_frame]

    def img_convert_dev(self, src_fmt, src, dst_fmt, dst, w, h, n, stream=None):
        return self._check(self.lib.amvhip_img_convert_dev(self.h, src_fmt, *self._pic(src), dst_fmt, *self._pic(dst), w, h, n, stream),
                           "img_convert_dev")

    def img_convert(self, src_fmt, src, dst_fmt, dst, w, h, n):
        return self._check(self.lib.amvhip_img_convert(self.h, src_fmt, *self._pic(src), dst_fmt, *self._pic(dst), w, h, n), "img_convert")

    def sws_scale_dev(self, src_fmt, src, src_w, src_h, dst_fmt, dst, dst_w, dst_h, n, stream=None):
        return self._check(self.lib.amvhip_sws_scale_dev(self.h, src_fmt, *self._pic(src), src_w, src_h, dst_fmt, *self._pic(dst),
                                                         dst_w, dst_h, n, stream), "sws_scale_dev")

    def encode_fmt_scaled_batch_dev(self, src_fmt, src, src_w, src_h, n, w, h, qbias, blob, blob_cap, offs, lens, stream=None):
        return self._check(self.lib.amvhip_encode_fmt_scaled_batch_dev(self.h, src_fmt, *self._pic(src), src_w, src_h, n, w, h, qbias,
                                                                       _ptr(blob), blob_cap, _ptr(offs), _ptr(lens), stream),
                           "encode_fmt_scaled_batch_dev")

    # the video front end (deinterlace, crop, rescale / convert, pad).  fe: a Frontend, or None for all zero
    @staticmethod
    def _fe(fe):
        return None if fe is None else ctypes.addressof(fe)

    def pad_color_from_rgb(self, rrggbb):
        return pad_color_from_rgb(rrggbb)

    def deinterlace_supported(self, fmt, w, h):
        return self.lib.amvhip_deinterlace_supported(fmt, w, h)

    def deinterlace_dev(self, fmt, src, dst, w, h, n, stream=None):
        return self._check(self.lib.amvhip_deinterlace_dev(self.h, fmt, *self._pic(src), *self._pic(dst), w, h, n, stream), "deinterlace_dev")

    def deinterlace(self, fmt, src, dst, w, h, n):
        return self._check(self.lib.amvhip_deinterlace(self.h, fmt, *self._pic(src), *self._pic(dst), w, h, n), "deinterlace")

    def video_frontend_dev(self, src_fmt, src, src_w, src_h, n, fe, dst, w, h, stream=None):
        return self._check(self.lib.amvhip_video_frontend_dev(self.h, src_fmt, *self._pic(src), src_w, src_h, n, self._fe(fe), *self._pic(dst),
                                                              w, h, stream), "video_frontend_dev")

    def encode_frontend_batch_dev(self, src_fmt, src, src_w, src_h, n, fe, w, h, qbias, blob, blob_cap, offs, lens, stream=None):
        return self._check(self.lib.amvhip_encode_frontend_batch_dev(self.h, src_fmt, *self._pic(src), src_w, src_h, n, self._fe(fe), w, h,
                                                                     qbias, _ptr(blob), blob_cap, _ptr(offs), _ptr(lens), stream),
                           "encode_frontend_batch_dev")

    def encode_frontend_quant_stream_dev(self, src_fmt, src, src_w, src_h, n, fe, w, h, quant, blob, blob_cap, offs, lens, stream=None):
        """encode_frontend_batch_dev with a Quant (qbias, nr, trellis, lambda, state) in the place of qbias; None -> NULL"""
        q = None if quant is None else ctypes.addressof(quant)
        return self._check(self.lib.amvhip_encode_frontend_quant_stream_dev(self.h, src_fmt, *self._pic(src), src_w, src_h, n, self._fe(fe),
                                                                            w, h, q, _ptr(blob), blob_cap, _ptr(offs), _ptr(lens), stream),
                           "encode_frontend_quant_stream_dev")

    # `-psnr`: the encoder's own error beside the chunks (sse: uint64 [n][3] on the device), and picture against picture
    def encode_quant_psnr_stream_dev(self, pix, pix_stride, is_bgr, n, w, h, quant, blob, blob_cap, offs, lens, sse, stream=None):
        """encode_batch_dev / _nr_stream_dev / _trellis_batch_dev / _nr_trellis_stream_dev by the Quant, and per frame and plane
        the squared error between the handed picture and the reconstruction of the coded levels"""
        q = None if quant is None else ctypes.addressof(quant)
        return self._check(self.lib.amvhip_encode_quant_psnr_stream_dev(self.h, _ptr(pix), pix_stride, is_bgr, n, w, h, q, _ptr(blob),
                                                                        blob_cap, _ptr(offs), _ptr(lens), _ptr(sse), stream),
                           "encode_quant_psnr_stream_dev")

    def encode_yuv420_quant_psnr_stream_dev(self, y, cb, cr, y_stride, c_stride, y_frame, c_frame, n, w, h, quant, blob, blob_cap, offs,
                                            lens, sse, stream=None):
        q = None if quant is None else ctypes.addressof(quant)
        return self._check(self.lib.amvhip_encode_yuv420_quant_psnr_stream_dev(self.h, _ptr(y), _ptr(cb), _ptr(cr), y_stride, c_stride,
                                                                               y_frame, c_frame, n, w, h, q, _ptr(blob), blob_cap,
                                                                               _ptr(offs), _ptr(lens), _ptr(sse), stream),
                           "encode_yuv420_quant_psnr_stream_dev")

    def encode_frontend_quant_psnr_stream_dev(self, src_fmt, src, src_w, src_h, n, fe, w, h, quant, blob, blob_cap, offs, lens, sse,
                                              stream=None):
        q = None if quant is None else ctypes.addressof(quant)
        return self._check(self.lib.amvhip_encode_frontend_quant_psnr_stream_dev(self.h, src_fmt, *self._pic(src), src_w, src_h, n,
                                                                                 self._fe(fe), w, h, q, _ptr(blob), blob_cap, _ptr(offs),
                                                                                 _ptr(lens), _ptr(sse), stream),
                           "encode_frontend_quant_psnr_stream_dev")

    # `-qns`: quantizer noise shaping behind the Quant's quantiser (qns 0 .. 3, lambda2); sse None: errors not wanted
    def encode_qns_lambda2_max(self):
        return self.lib.amvhip_encode_qns_lambda2_max()

    def encode_qns_lambda2(self, qscale):
        """the reference's lambda2 for a -qscale (6962 at 8); 0 where it is above encode_qns_lambda2_max()"""
        return self.lib.amvhip_encode_qns_lambda2(qscale)

    def encode_qns_stream_dev(self, pix, pix_stride, is_bgr, n, w, h, quant, qns, lambda2, blob, blob_cap, offs, lens, sse=None, stream=None):
        q = None if quant is None else ctypes.addressof(quant)
        return self._check(self.lib.amvhip_encode_qns_stream_dev(self.h, _ptr(pix), pix_stride, is_bgr, n, w, h, q, qns, lambda2, _ptr(blob),
                                                                 blob_cap, _ptr(offs), _ptr(lens), None if sse is None else _ptr(sse), stream),
                           "encode_qns_stream_dev")

    def encode_yuv420_qns_stream_dev(self, y, cb, cr, y_stride, c_stride, y_frame, c_frame, n, w, h, quant, qns, lambda2, blob, blob_cap, offs,
                                     lens, sse=None, stream=None):
        q = None if quant is None else ctypes.addressof(quant)
        return self._check(self.lib.amvhip_encode_yuv420_qns_stream_dev(self.h, _ptr(y), _ptr(cb), _ptr(cr), y_stride, c_stride, y_frame,
                                                                        c_frame, n, w, h, q, qns, lambda2, _ptr(blob), blob_cap, _ptr(offs),
                                                                        _ptr(lens), None if sse is None else _ptr(sse), stream),
                           "encode_yuv420_qns_stream_dev")

    def encode_frontend_qns_stream_dev(self, src_fmt, src, src_w, src_h, n, fe, w, h, quant, qns, lambda2, blob, blob_cap, offs, lens, sse=None,
                                       stream=None):
        q = None if quant is None else ctypes.addressof(quant)
        return self._check(self.lib.amvhip_encode_frontend_qns_stream_dev(self.h, src_fmt, *self._pic(src), src_w, src_h, n, self._fe(fe), w,
                                                                          h, q, qns, lambda2, _ptr(blob), blob_cap, _ptr(offs), _ptr(lens),
                                                                          None if sse is None else _ptr(sse), stream),
                           "encode_frontend_qns_stream_dev")

    def encode_qns_coefs_dev(self, pix, pix_stride, is_bgr, n, w, h, quant, qns, lambda2, coef, stream=None):
        q = None if quant is None else ctypes.addressof(quant)
        return self._check(self.lib.amvhip_encode_qns_coefs_dev(self.h, _ptr(pix), pix_stride, is_bgr, n, w, h, q, qns, lambda2, _ptr(coef),
                                                                stream), "encode_qns_coefs_dev")

    # a byte budget per frame: the Quant (trellis 1; its lambda is not read), then a ladder of lambdas / a Rate
    def encode_rate_probe_dev(self, pix, pix_stride, is_bgr, n, w, h, quant, ladder, bits, stream=None, rungs=None):
        """bits uint32 [n][rungs] on the device: the bits of every frame's scan at every lambda of `ladder` (a sequence; None -> NULL)"""
        q = None if quant is None else ctypes.addressof(quant)
        rate = Rate(ladder, rungs=rungs)
        return self._check(self.lib.amvhip_encode_rate_probe_dev(self.h, _ptr(pix), pix_stride, is_bgr, n, w, h, q, rate.ladder, rate.rungs,
                                                                 _ptr(bits), stream), "encode_rate_probe_dev")

    def encode_yuv420_rate_probe_dev(self, y, cb, cr, y_stride, c_stride, y_frame, c_frame, n, w, h, quant, ladder, bits, stream=None,
                                     rungs=None):
        q = None if quant is None else ctypes.addressof(quant)
        rate = Rate(ladder, rungs=rungs)
        return self._check(self.lib.amvhip_encode_yuv420_rate_probe_dev(self.h, _ptr(y), _ptr(cb), _ptr(cr), y_stride, c_stride, y_frame,
                                                                        c_frame, n, w, h, q, rate.ladder, rate.rungs, _ptr(bits), stream),
                           "encode_yuv420_rate_probe_dev")

    def encode_rate_stream_dev(self, pix, pix_stride, is_bgr, n, w, h, quant, rate, blob, blob_cap, offs, lens, rung, stream=None):
        """every frame at the first rung of the Rate's ladder whose chunk fits its budget; rung uint32 [n] on the device says
        which (RATE_OVER or-ed in where none did)"""
        q = None if quant is None else ctypes.addressof(quant)
        r = None if rate is None else ctypes.addressof(rate)
        return self._check(self.lib.amvhip_encode_rate_stream_dev(self.h, _ptr(pix), pix_stride, is_bgr, n, w, h, q, r, _ptr(blob), blob_cap,
                                                                  _ptr(offs), _ptr(lens), _ptr(rung), stream), "encode_rate_stream_dev")

    def encode_yuv420_rate_stream_dev(self, y, cb, cr, y_stride, c_stride, y_frame, c_frame, n, w, h, quant, rate, blob, blob_cap, offs, lens,
                                      rung, stream=None):
        q = None if quant is None else ctypes.addressof(quant)
        r = None if rate is None else ctypes.addressof(rate)
        return self._check(self.lib.amvhip_encode_yuv420_rate_stream_dev(self.h, _ptr(y), _ptr(cb), _ptr(cr), y_stride, c_stride, y_frame,
                                                                         c_frame, n, w, h, q, r, _ptr(blob), blob_cap, _ptr(offs), _ptr(lens),
                                                                         _ptr(rung), stream), "encode_yuv420_rate_stream_dev")

    # chunks requantised in the coefficient domain: the decode entries' inputs up to h, then lambda / a ladder / a Rate
    def requant_stream_dev(self, blob, blob_bytes, offs, lens, n, w, h, lam, out, out_cap, out_offs, out_lens, status, err=None, stream=None):
        """the AC levels of every clean, in-range chunk searched at lam; err: None or uint64 [n][3] on the device"""
        return self._check(self.lib.amvhip_requant_stream_dev(self.h, _ptr(blob), blob_bytes, _ptr(offs), _ptr(lens), n, w, h, lam, _ptr(out),
                                                              out_cap, _ptr(out_offs), _ptr(out_lens), _ptr(status), _ptr(err), stream),
                           "requant_stream_dev")

    def requant_rate_probe_dev(self, blob, blob_bytes, offs, lens, n, w, h, ladder, bits, stream=None, rungs=None):
        rate = Rate(ladder, rungs=rungs)
        return self._check(self.lib.amvhip_requant_rate_probe_dev(self.h, _ptr(blob), blob_bytes, _ptr(offs), _ptr(lens), n, w, h, rate.ladder,
                                                                  rate.rungs, _ptr(bits), stream), "requant_rate_probe_dev")

    def requant_rate_stream_dev(self, blob, blob_bytes, offs, lens, n, w, h, rate, out, out_cap, out_offs, out_lens, status, rung, stream=None):
        r = None if rate is None else ctypes.addressof(rate)
        return self._check(self.lib.amvhip_requant_rate_stream_dev(self.h, _ptr(blob), blob_bytes, _ptr(offs), _ptr(lens), n, w, h, r, _ptr(out),
                                                                   out_cap, _ptr(out_offs), _ptr(out_lens), _ptr(status), _ptr(rung), stream),
                           "requant_rate_stream_dev")

    def encode_frontend_rate_stream_dev(self, src_fmt, src, src_w, src_h, n, fe, w, h, quant, rate, blob, blob_cap, offs, lens, rung,
                                        stream=None):
        q = None if quant is None else ctypes.addressof(quant)
        r = None if rate is None else ctypes.addressof(rate)
        return self._check(self.lib.amvhip_encode_frontend_rate_stream_dev(self.h, src_fmt, *self._pic(src), src_w, src_h, n, self._fe(fe), w,
                                                                           h, q, r, _ptr(blob), blob_cap, _ptr(offs), _ptr(lens), _ptr(rung),
                                                                           stream), "encode_frontend_rate_stream_dev")

    # a byte budget per clip: the rate siblings' arguments with `total` behind rate and clip, uint64 [2] on the device, behind rung
    def encode_clip_stream_dev(self, pix, pix_stride, is_bgr, n, w, h, quant, rate, total, blob, blob_cap, offs, lens, rung, clip, stream=None):
        """the n frames in at most `total` bytes: clip[0] = the clip rung (RATE_OVER or-ed in where none fit), clip[1] = the sum"""
        q = None if quant is None else ctypes.addressof(quant)
        r = None if rate is None else ctypes.addressof(rate)
        return self._check(self.lib.amvhip_encode_clip_stream_dev(self.h, _ptr(pix), pix_stride, is_bgr, n, w, h, q, r, total, _ptr(blob),
                                                                  blob_cap, _ptr(offs), _ptr(lens), _ptr(rung), _ptr(clip), stream),
                           "encode_clip_stream_dev")

    def encode_yuv420_clip_stream_dev(self, y, cb, cr, y_stride, c_stride, y_frame, c_frame, n, w, h, quant, rate, total, blob, blob_cap, offs,
                                      lens, rung, clip, stream=None):
        q = None if quant is None else ctypes.addressof(quant)
        r = None if rate is None else ctypes.addressof(rate)
        return self._check(self.lib.amvhip_encode_yuv420_clip_stream_dev(self.h, _ptr(y), _ptr(cb), _ptr(cr), y_stride, c_stride, y_frame,
                                                                         c_frame, n, w, h, q, r, total, _ptr(blob), blob_cap, _ptr(offs),
                                                                         _ptr(lens), _ptr(rung), _ptr(clip), stream),
                           "encode_yuv420_clip_stream_dev")

    def encode_frontend_clip_stream_dev(self, src_fmt, src, src_w, src_h, n, fe, w, h, quant, rate, total, blob, blob_cap, offs, lens, rung,
                                        clip, stream=None):
        q = None if quant is None else ctypes.addressof(quant)
        r = None if rate is None else ctypes.addressof(rate)
        return self._check(self.lib.amvhip_encode_frontend_clip_stream_dev(self.h, src_fmt, *self._pic(src), src_w, src_h, n, self._fe(fe), w,
                                                                           h, q, r, total, _ptr(blob), blob_cap, _ptr(offs), _ptr(lens),
                                                                           _ptr(rung), _ptr(clip), stream), "encode_frontend_clip_stream_dev")

    def requant_clip_stream_dev(self, blob, blob_bytes, offs, lens, n, w, h, rate, total, out, out_cap, out_offs, out_lens, status, rung, clip,
                                stream=None):
        r = None if rate is None else ctypes.addressof(rate)
        return self._check(self.lib.amvhip_requant_clip_stream_dev(self.h, _ptr(blob), blob_bytes, _ptr(offs), _ptr(lens), n, w, h, r, total,
                                                                   _ptr(out), out_cap, _ptr(out_offs), _ptr(out_lens), _ptr(status), _ptr(rung),
                                                                   _ptr(clip), stream), "requant_clip_stream_dev")

    # re-table: the requant entries with a Retable (the tables the chunks were written against) behind h
    def retable_stream_dev(self, blob, blob_bytes, offs, lens, n, w, h, rt, lam, out, out_cap, out_offs, out_lens, status, err=None, stream=None):
        t = None if rt is None else ctypes.addressof(rt)
        return self._check(self.lib.amvhip_retable_stream_dev(self.h, _ptr(blob), blob_bytes, _ptr(offs), _ptr(lens), n, w, h, t, lam, _ptr(out),
                                                              out_cap, _ptr(out_offs), _ptr(out_lens), _ptr(status), _ptr(err), stream),
                           "retable_stream_dev")

    def retable_rate_probe_dev(self, blob, blob_bytes, offs, lens, n, w, h, rt, ladder, bits, stream=None, rungs=None):
        t = None if rt is None else ctypes.addressof(rt)
        rate = Rate(ladder, rungs=rungs)
        return self._check(self.lib.amvhip_retable_rate_probe_dev(self.h, _ptr(blob), blob_bytes, _ptr(offs), _ptr(lens), n, w, h, t, rate.ladder,
                                                                  rate.rungs, _ptr(bits), stream), "retable_rate_probe_dev")

    def retable_rate_stream_dev(self, blob, blob_bytes, offs, lens, n, w, h, rt, rate, out, out_cap, out_offs, out_lens, status, rung, stream=None):
        t = None if rt is None else ctypes.addressof(rt)
        r = None if rate is None else ctypes.addressof(rate)
        return self._check(self.lib.amvhip_retable_rate_stream_dev(self.h, _ptr(blob), blob_bytes, _ptr(offs), _ptr(lens), n, w, h, t, r, _ptr(out),
                                                                   out_cap, _ptr(out_offs), _ptr(out_lens), _ptr(status), _ptr(rung), stream),
                           "retable_rate_stream_dev")

    def retable_clip_stream_dev(self, blob, blob_bytes, offs, lens, n, w, h, rt, rate, total, out, out_cap, out_offs, out_lens, status, rung,
                                clip, stream=None):
        t = None if rt is None else ctypes.addressof(rt)
        r = None if rate is None else ctypes.addressof(rate)
        return self._check(self.lib.amvhip_retable_clip_stream_dev(self.h, _ptr(blob), blob_bytes, _ptr(offs), _ptr(lens), n, w, h, t, r, total,
                                                                   _ptr(out), out_cap, _ptr(out_offs), _ptr(out_lens), _ptr(status), _ptr(rung),
                                                                   _ptr(clip), stream), "retable_clip_stream_dev")

    def picture_sse_supported(self, fmt, w, h):
        return picture_sse_supported(fmt, w, h)

    def picture_sse_dev(self, fmt, a, b, w, h, n, sse, stream=None):
        """two batches of n pictures of one format (each as in img_convert_dev) -> sse uint64 [n][3] on the device"""
        return self._check(self.lib.amvhip_picture_sse_dev(self.h, fmt, *self._pic(a), *self._pic(b), w, h, n, _ptr(sse), stream),
                           "picture_sse_dev")

    def picture_sse(self, fmt, a, b, w, h, n, sse):
        return self._check(self.lib.amvhip_picture_sse(self.h, fmt, *self._pic(a), *self._pic(b), w, h, n, _ptr(sse)), "picture_sse")

    def decode_fmt_batch_dev(self, blob, blob_bytes, offs, lens, n, w, h, flags, dst_fmt, out, out_stride, status, stream=None):
        return self._check(self.lib.amvhip_decode_fmt_batch_dev(self.h, _ptr(blob), blob_bytes, _ptr(offs), _ptr(lens), n, w, h, flags,
                                                                dst_fmt, _ptr(out), out_stride, _ptr(status), stream),
                           "decode_fmt_batch_dev")

    # reduced-size decode (lowres 1..3: 1/2, 1/4, 1/8 size)
    def lowres_dim(self, full, lowres):
        return self.lib.amvhip_lowres_dim(full, lowres)

    def lowres_frame_bytes(self, w, h, lowres):
        return self.lib.amvhip_lowres_frame_bytes(w, h, lowres)

    # decode-side postprocessing (the reference's libpostproc: hb, vb, dr).  mode: a PpMode; src / dst: pictures as in deinterlace_dev
    def postprocess_supported(self, w, h):
        return self.lib.amvhip_postprocess_supported(w, h)

    def postprocess_dev(self, fmt, mode, src, dst, w, h, n, qp=None, stream=None):
        return self._check(self.lib.amvhip_postprocess_dev(self.h, fmt, ctypes.byref(mode), *self._pic(src), *self._pic(dst), w, h, n, _ptr(qp), stream),
                           "postprocess_dev")

    def postprocess(self, fmt, mode, src, dst, w, h, n, qp=None):
        return self._check(self.lib.amvhip_postprocess(self.h, fmt, ctypes.byref(mode), *self._pic(src), *self._pic(dst), w, h, n, _ptr(qp)), "postprocess")

    def decode_pp_batch_dev(self, blob, blob_bytes, offs, lens, n, w, h, flags, dst_fmt, out, out_stride, status, mode, qp=None, stream=None):
        return self._check(self.lib.amvhip_decode_pp_batch_dev(self.h, _ptr(blob), blob_bytes, _ptr(offs), _ptr(lens), n, w, h, flags, dst_fmt,
                                                               _ptr(out), out_stride, _ptr(status), ctypes.byref(mode), _ptr(qp), stream),
                           "decode_pp_batch_dev")

    def decode_lowres_batch_dev(self, blob, blob_bytes, offs, lens, n, w, h, flags, lowres, dst_fmt, out, out_stride, status, stream=None):
        return self._check(self.lib.amvhip_decode_lowres_batch_dev(self.h, _ptr(blob), blob_bytes, _ptr(offs), _ptr(lens), n, w, h, flags,
                                                                   lowres, dst_fmt, _ptr(out), out_stride, _ptr(status), stream),
                           "decode_lowres_batch_dev")

    def decode_lowres_batch(self, blob, blob_bytes, offs, lens, n, w, h, flags, lowres, dst_fmt, out, out_stride, status):
        return self._check(self.lib.amvhip_decode_lowres_batch(self.h, _ptr(blob), blob_bytes, _ptr(offs), _ptr(lens), n, w, h, flags,
                                                               lowres, dst_fmt, _ptr(out), out_stride, _ptr(status)), "decode_lowres_batch")

    def reconstruct_lowres_dev(self, coef, nmcu_ok, n, w, h, lowres, out, stream=None):
        return self._check(self.lib.amvhip_reconstruct_lowres_dev(self.h, _ptr(coef), _ptr(nmcu_ok), n, w, h, lowres, _ptr(out), stream),
                           "reconstruct_lowres_dev")

    def audio_resample_out_samples(self, in_rate, out_rate, in_samples):
        return audio_resample_out_samples(in_rate, out_rate, in_samples)

    def audio_resample_batch_dev(self, pcm, pcm_offs, nsamp, n, in_channels, in_rate, out, out_offs, out_channels, out_rate,
                                 stream=None):
        return self._check(self.lib.amvhip_audio_resample_batch_dev(self.h, _ptr(pcm), _ptr(pcm_offs), _ptr(nsamp), n,
                                                                    in_channels, in_rate, _ptr(out), _ptr(out_offs),
                                                                    out_channels, out_rate, stream), "audio_resample_batch_dev")

    def audio_resampler(self, output_channels, input_channels, output_rate, input_rate):
        """the streaming form (amvhip_audio_resample_init): an AudioResampler bound to this context"""
        return AudioResampler(self, output_channels, input_channels, output_rate, input_rate)

    def synth_frames_dev(self, seed, first, n, w, h, rgb, stream=None):
        return self._check(self.lib.amvhip_synth_frames_dev(self.h, seed, first, n, w, h, _ptr(rgb), stream), "synth_frames_dev")

    def synth_audio_dev(self, seed, first, n, pcm, stream=None):
        return self._check(self.lib.amvhip_synth_audio_dev(self.h, seed, first, n, _ptr(pcm), stream), "synth_audio_dev")

    # host buffers
    def decode_batch(self, blob, blob_bytes, offs, lens, n, w, h, flags, out, status):
        return self._check(self.lib.amvhip_decode_batch(self.h, _ptr(blob), blob_bytes, _ptr(offs), _ptr(lens), n, w, h,
                                                        flags, _ptr(out), _ptr(status)), "decode_batch")

    def encode_batch(self, pix, pix_stride, is_bgr, n, w, h, qbias, blob, blob_cap, offs, lens):
        return self._check(self.lib.amvhip_encode_batch(self.h, _ptr(pix), pix_stride, is_bgr, n, w, h, qbias, _ptr(blob),
                                                        blob_cap, _ptr(offs), _ptr(lens)), "encode_batch")

    def adpcm_decode_batch(self, blob, blob_bytes, offs, lens, n, pcm, pcm_samples, pcm_offs, final_state=None):
        return self._check(self.lib.amvhip_adpcm_decode_batch(self.h, _ptr(blob), blob_bytes, _ptr(offs), _ptr(lens), n,
                                                              _ptr(pcm), pcm_samples, _ptr(pcm_offs), _ptr(final_state)),
                           "adpcm_decode_batch")

    def adpcm_encode_batch(self, pcm, pcm_samples, pcm_offs, nsamp, n, step_in, blob, blob_bytes, offs):
        return self._check(self.lib.amvhip_adpcm_encode_batch(self.h, _ptr(pcm), pcm_samples, _ptr(pcm_offs), _ptr(nsamp),
                                                              n, _ptr(step_in), _ptr(blob), blob_bytes, _ptr(offs)),
                           "adpcm_encode_batch")

    def adpcm_encode_trellis_stream(self, pcm, pcm_samples, pcm_offs, nsamp, n, first_step_index, trellis, blob, blob_bytes, offs,
                                    step_out=None):
        return self._check(self.lib.amvhip_adpcm_encode_trellis_stream(self.h, _ptr(pcm), pcm_samples, _ptr(pcm_offs), _ptr(nsamp),
                                                                       n, first_step_index, trellis, _ptr(blob), blob_bytes,
                                                                       _ptr(offs), _ptr(step_out)),
                           "adpcm_encode_trellis_stream")

    def audio_resample_batch(self, pcm, pcm_samples, pcm_offs, nsamp, n, in_channels, in_rate, out, out_samples, out_offs,
                             out_channels, out_rate):
        return self._check(self.lib.amvhip_audio_resample_batch(self.h, _ptr(pcm), pcm_samples, _ptr(pcm_offs), _ptr(nsamp), n,
                                                                in_channels, in_rate, _ptr(out), out_samples, _ptr(out_offs),
                                                                out_channels, out_rate), "audio_resample_batch")

    def set_entropy_mode(self, mode):
        return self._check(self.lib.amvhip_set_entropy_mode(self.h, mode), "set_entropy_mode")

    def entropy_stats(self, enable=True):
        out = (ctypes.c_uint64 * 11)()
        self._check(self.lib.amvhip_entropy_stats(self.h, 1 if enable else 0, out), "entropy_stats")
        waves = max(out[9], 1)
        return {"frames": out[0], "rounds": out[1], "max_rounds": out[2], "handed_to_serial": out[3], "waves": out[9],
                "big_ac_frames": out[10],
                "clocks_per_wave": {"zero": out[4] / waves, "first_walk": out[5] / waves, "sync_rounds": out[6] / waves,
                                    "write": out[7] / waves, "dc": out[8] / waves}}

    def entropy_trace(self, tasks):
        """per task (wave) of the last several-lanes-per-frame launch with gathering on: [tasks, 8] uint64 (include/amvhip.h)"""
        import numpy as np
        out = np.zeros((tasks, 8), np.uint64)
        got = self.lib.amvhip_entropy_trace(self.h, out.ctypes.data, tasks)
        if got < 0:
            self._check(got, "entropy_trace")
        return out[:got]

    def decode_split_stats(self):
        """last decode call: {"heavy": frames that got several entropy lanes, "light": frames that got one} (0, 0: no split)"""
        out = (ctypes.c_uint32 * 2)()
        self._check(self.lib.amvhip_decode_split_stats(self.h, out), "decode_split_stats")
        return {"heavy": int(out[0]), "light": int(out[1])}

    def adpcm_chain_stats(self):
        """last chained ADPCM encode: {"exhaustive": bool, "recoded": [chunks coded again in sweep 1, 2, ...]}"""
        out = (ctypes.c_uint32 * 64)()
        self._check(self.lib.amvhip_adpcm_chain_stats(self.h, out), "adpcm_chain_stats")
        rec = list(out[1:63])
        while rec and rec[-1] == 0:
            rec.pop()
        return {"exhaustive": bool(out[0]), "recoded": rec}

    def adpcm_trellis_chain_stats(self):
        """last trellis stream call: {"exhaustive": bool (the fall-back route), "recoded": [chunks coded again in sweep 1, 2, ...]}"""
        out = (ctypes.c_uint32 * 64)()
        self._check(self.lib.amvhip_adpcm_trellis_chain_stats(self.h, out), "adpcm_trellis_chain_stats")
        rec = list(out[1:63])
        while rec and rec[-1] == 0:
            rec.pop()
        return {"exhaustive": bool(out[0]), "recoded": rec}

    # timing
    def prof_enable(self, on=True):
        self.lib.amvhip_prof_enable(self.h, 1 if on else 0)

    def prof_reset(self):
        self.lib.amvhip_prof_reset(self.h)

    def prof_read(self, kernel):
        n, ms = ctypes.c_uint64(), ctypes.c_double()
        self.lib.amvhip_prof_read(self.h, kernel, ctypes.byref(n), ctypes.byref(ms))
        return n.value, ms.value

    def kernel_name(self, kernel):
        return self.lib.amvhip_kernel_name(kernel).decode()


def psnr_db(sse, samples):
    """ffmpeg's psnr() on sse / (samples * 255^2), dB: inf at sse == 0, nan at samples == 0 (host arithmetic, no device)"""
    return load_library().amvhip_psnr_db(int(sse), int(samples))


def psnr_report(sse, w, h):
    """the last-report PSNR line over the frames of sse (uint64 [n][3], numpy) -> (Y, U, V, *) in dB"""
    import numpy as np
    sse = np.ascontiguousarray(sse, np.uint64).reshape(-1, 3)
    out = (ctypes.c_double * 4)()
    load_library().amvhip_psnr_report(sse.ctypes.data, sse.shape[0], w, h, ctypes.cast(out, ctypes.c_void_p))
    return tuple(out)


def picture_sse_supported(fmt, w, h):
    return load_library().amvhip_picture_sse_supported(fmt, w, h)


def audio_resample_out_samples(in_rate, out_rate, in_samples):
    """frames one audio_resample call makes of in_samples frames (host arithmetic, no device)"""
    return load_library().amvhip_audio_resample_out_samples(in_rate, out_rate, in_samples)


class AudioResampler:
    """amvhip_audio_resample_init / _resample / _close: the reference's audio_resample, one packet per call"""

    def __init__(self, ctx, output_channels, input_channels, output_rate, input_rate):
        self.ctx, self.out_ch, self.in_ch = ctx, output_channels, input_channels
        self.ratio = ctypes.c_float(ctypes.c_float(output_rate).value / ctypes.c_float(input_rate).value).value
        self.h = ctx.lib.amvhip_audio_resample_init(ctx.h, output_channels, input_channels, output_rate, input_rate)
        if not self.h:
            raise AmvHipError("amvhip_audio_resample_init failed: %s" % ctx.lib.amvhip_last_error(ctx.h).decode())

    def resample(self, pcm):
        """one packet (numpy int16, interleaved input channels) -> its output (numpy int16, interleaved output channels)"""
        import numpy as np
        pcm = np.ascontiguousarray(pcm, np.int16)
        nb = pcm.size // self.in_ch
        out = np.zeros((int(4 * nb * self.ratio) + 18) * self.out_ch, np.int16)    # the reference's lenout bound (+2: float vs double)
        got = self.ctx._check(self.ctx.lib.amvhip_audio_resample(self.h, out.ctypes.data, pcm.ctypes.data, nb), "audio_resample")
        return out[:got * self.out_ch]

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.amvhip_audio_resample_close(self.h)
            self.h = None

    __del__ = close
