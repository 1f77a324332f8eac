"""Build libamvhip.so (HIP kernels + C ABI + amvlib call surface) in-tree for gfx950.  The FFmpeg `AVCodec` plugin
surface (host/amvhip_lavc.c) is compiled against the reference's own libavcodec/avcodec.h, so its recipe lives with the
other reference-built files in oracle/Makefile (`make lavc`, into oracle/_ref/).

    python amv-codec-tools_amd/build.py [--force]

hipcc cross-compiles without a GPU.  Objects go to amv-codec-tools_amd/build/, the library to
amv-codec-tools_amd/libamvhip.so (git-ignored).
"""
import concurrent.futures
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "libamvhip.so")
OBJ = os.path.join(HERE, "build")
ARCH = "gfx950"

HIP_SOURCES = ["csrc/amv_decode.hip", "csrc/amv_decode_sync.hip", "csrc/amv_reconstruct.hip", "csrc/amv_reconstruct_ff.hip", "csrc/amv_reconstruct_lowres.hip", "csrc/amv_encode.hip", "csrc/amv_encode_par.hip", "csrc/amv_encode_nr.hip", "csrc/amv_encode_error.hip", "csrc/amv_encode_qns.hip", "csrc/amv_encode_rate.hip", "csrc/amv_encode_clip.hip", "csrc/amv_requant.hip", "csrc/amv_resample.hip", "csrc/amv_pixfmt.hip", "csrc/amv_picture_sse.hip", "csrc/amv_frontend.hip", "csrc/amv_postprocess.hip", "csrc/amv_audio_resample.hip", "csrc/amv_adpcm.hip", "csrc/amv_adpcm_trellis.hip", "csrc/amv_synth.hip",
               "csrc/amvhip_context.hip", "csrc/amvhip_decode.hip", "csrc/amvhip_encode.hip", "csrc/amvhip_requant.hip", "csrc/amvhip_pixfmt.hip", "csrc/amvhip_audio.hip"]
C_SOURCES = ["host/amvlib_compat.c", "host/amv_container.c", "host/amvhip_pp_mode.c"]
HEADERS = ["csrc/amv_tables.h", "csrc/amv_kernels.h", "csrc/amv_block_load.h", "csrc/amv_piece_map.h", "csrc/amv_segment.h", "csrc/amv_ff_dequant.h", "csrc/amv_simple_idct.h", "csrc/amv_wave.h", "csrc/amv_encode_common.h", "csrc/amv_host_plan.h", "csrc/amv_nr_plan.h", "csrc/amv_trellis_plan.h", "csrc/amv_qns_plan.h", "csrc/amv_rate_plan.h", "csrc/amv_clip_plan.h", "csrc/amv_requant_plan.h", "csrc/amv_retable_plan.h", "csrc/amv_pp_plan.h", "csrc/amv_adpcm_chain.h",
           "csrc/amvhip_ctx.h", "../include/amvhip.h"]

# -fwrapv: the codec's integer pipeline is defined on two's-complement wrap (see amv_decode.hip)
HIPFLAGS = ["-O3", "-std=c++17", "-fPIC", "-fwrapv", "-fno-strict-aliasing", f"--offload-arch={ARCH}",
            "-Wall", "-Wno-unused-function"]
CFLAGS = ["-O2", "-fPIC", "-Wall", "-Wextra", "-std=gnu11"]


def _hipcc():
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: libamvhip.so cannot be built (there is no CPU fallback)")


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _run(cmd):
    p = subprocess.run(cmd, cwd=HERE, capture_output=True, text=True)
    if p.returncode != 0:
        raise RuntimeError("command failed: %s\n%s\n%s" % (" ".join(cmd), p.stdout, p.stderr))
    return p.stderr


def build(force=False, verbose=False):
    os.makedirs(OBJ, exist_ok=True)
    hipcc = _hipcc()
    hdrs = [os.path.join(HERE, h) for h in HEADERS] + [os.path.abspath(__file__)]
    jobs = []
    objs = []
    for src in HIP_SOURCES:
        o = os.path.join(OBJ, os.path.basename(src) + ".o")
        objs.append(o)
        if force or _stale(o, [os.path.join(HERE, src)] + hdrs):
            jobs.append([hipcc] + HIPFLAGS + ["-c", src, "-o", o])
    for src in C_SOURCES:
        o = os.path.join(OBJ, os.path.basename(src) + ".o")
        objs.append(o)
        if force or _stale(o, [os.path.join(HERE, src)] + hdrs):
            jobs.append(["gcc"] + CFLAGS + ["-c", src, "-o", o])
    if jobs:
        with concurrent.futures.ThreadPoolExecutor(max_workers=4) as ex:
            for warn in ex.map(_run, jobs):
                if verbose and warn:
                    sys.stderr.write(warn)
    if jobs or force or _stale(OUT, objs):
        _run([hipcc, "-shared", "-fPIC", f"--offload-arch={ARCH}", "-o", OUT] + objs + ["-lpthread"])
    return OUT


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
