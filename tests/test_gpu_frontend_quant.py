"""The front end with a quantiser behind it (amvhip_encode_frontend_quant_stream_dev) on a real MI355X: chunks, offsets,
lengths and state are those of amvhip_video_frontend_dev into tight planes followed by the YUV420 entry of the same request
-- for -nr alone, the trellis alone, both and neither, behind a front end with every stage and behind the identity one --
and, for both levers behind the deinterlace case, those of the CPU models (frontend_ref.py, then nr_trellis_ref.py)."""
import numpy as np
import pytest

import frontend_ref as F
import img_convert_ref as R
import nr_ref as N
import nr_trellis_ref as NT
from test_gpu_frontend import Pictures, chunks_of, encode_dev, stream

pytestmark = pytest.mark.gpu

W, H, N_FRAMES = 48, 32, 4
NR, LAM, QBIAS = 1200, 3481, 5
REQUESTS = {"nr": (NR, 0, 0), "trellis": (0, 1, LAM), "both": (NR, 1, LAM), "neither": (0, 0, 0)}
# deinterlace + crop + rescale + pad: 64x48 -> crop to 56x44 -> 44x28 inside 48x32; and RGB24 at the target size, no stage
STAGES = {"stages": (R.YUV420P, 64, 48, (1, (2, 2, 4, 4), (2, 2, 2, 2), (16, 128, 128))), "identity": (R.RGB24, W, H, None)}


def _source(name):
    src, sw, sh, fe = STAGES[name]
    frames = [R.make_picture(src, sw, sh, k, 31 + 7 * i) for i, k in enumerate(("ramp", "noise", "ramp", "noise"))]
    return src, sw, sh, fe, frames


def _state():
    import torch
    return torch.zeros(65, dtype=torch.int32, device="cuda:0")


def _two_calls(ctx, pkg, src, s, sw, sh, fe, request):
    """amvhip_video_frontend_dev into tight planes, then the YUV420 entry of the request -> ((blob, offs, lens), state)"""
    import torch
    nr, trellis, lam = REQUESTS[request]
    d = Pictures(R.YUVJ420P, W, H, N_FRAMES).to_dev()
    ctx.video_frontend_dev(src, s.pic(), sw, sh, N_FRAMES, fe, d.pic(), W, H, stream())
    torch.cuda.synchronize()
    state = _state()
    planes = (d.dev[0], d.dev[1], d.dev[2], d.stride[0], d.stride[1], d.frame[0], d.frame[1], N_FRAMES, W, H, QBIAS)
    if request == "nr":
        call = lambda b, c, o, l: ctx.encode_yuv420_nr_stream_dev(*planes, nr, state, b, c, o, l, stream())
    elif request == "trellis":
        call = lambda b, c, o, l: ctx.encode_yuv420_trellis_batch_dev(*planes, lam, b, c, o, l, stream())
    elif request == "both":
        call = lambda b, c, o, l: ctx.encode_yuv420_nr_trellis_stream_dev(*planes, nr, lam, state, b, c, o, l, stream())
    else:
        call = lambda b, c, o, l: ctx.encode_yuv420_batch_dev(*planes, b, c, o, l, stream())
    return encode_dev(ctx, call, N_FRAMES, W, H), state.cpu().numpy()


def _one_call(ctx, pkg, src, s, sw, sh, fe, request):
    nr, trellis, lam = REQUESTS[request]
    state = _state()
    q = pkg.Quant(QBIAS, nr, trellis, lam, state if nr else None)
    call = lambda b, c, o, l: ctx.encode_frontend_quant_stream_dev(src, s.pic(), sw, sh, N_FRAMES, fe, W, H, q, b, c, o, l, stream())
    return encode_dev(ctx, call, N_FRAMES, W, H), state.cpu().numpy()


@pytest.mark.parametrize("request_name", list(REQUESTS))
@pytest.mark.parametrize("stages", list(STAGES))
def test_front_end_and_encoder_equal_two_calls(ctx, pkg, stages, request_name):
    src, sw, sh, fe_args, frames = _source(stages)
    fe = pkg.Frontend(*fe_args) if fe_args else None
    s = Pictures(src, sw, sh, N_FRAMES).fill(frames).to_dev()
    (want, want_state), (got, got_state) = _two_calls(ctx, pkg, src, s, sw, sh, fe, request_name), _one_call(ctx, pkg, src, s, sw, sh, fe, request_name)
    assert all(int(x) > 4 for x in want[2])
    for a, b, what in zip(want, got, ("bytes", "offsets", "lengths")):
        assert (a == b).all(), "%s, %s: %s differ at %s" % (stages, request_name, what, np.flatnonzero(a != b)[:8])
    assert (want_state == got_state).all() and (got_state[64] == (N_FRAMES * 36 if REQUESTS[request_name][0] else 0))
    if request_name == "neither":                                      # ... which is amvhip_encode_frontend_batch_dev
        old = encode_dev(ctx, lambda b, c, o, l: ctx.encode_frontend_batch_dev(src, s.pic(), sw, sh, N_FRAMES, fe, W, H, QBIAS, b, c, o, l, stream()),
                         N_FRAMES, W, H)
        assert all((a == b).all() for a, b in zip(old, got)), stages


def test_both_levers_behind_the_deinterlace_case_against_the_models(ctx, pkg, orc):
    src, sw, sh, fe_args, frames = _source("stages")
    deint, crop, pad, color = fe_args
    planes = [F.frontend(src, f, sw, sh, W, H, orc.img_resample_yuv420, deint, crop, pad, color) for f in frames]
    state = N.new_state()
    want = NT.encode_stream([tuple(p) for p in planes], W, H, NR, LAM, state=state, qbias=QBIAS)
    s = Pictures(src, sw, sh, N_FRAMES).fill(frames).to_dev()
    got, got_state = _one_call(ctx, pkg, src, s, sw, sh, pkg.Frontend(*fe_args), "both")
    assert chunks_of(*got) == want
    assert [int(x) for x in got[1]] == [sum(len(c) for c in want[:i]) for i in range(N_FRAMES)]
    assert (got[0][sum(len(c) for c in want):] == 0).all() and (got_state == state).all()
    # the levers did something behind the front end too
    assert want != N.encode_stream([tuple(p) for p in planes], W, H, NR, qbias=QBIAS)


def test_refusals(ctx, pkg):
    """q == NULL, nr > 0 with a null d_state, and what the entries behind refuse of nr, lambda and trellis: AMVHIP_ERR_ARG
    before anything is written"""
    import torch
    src, sw, sh, fe_args, frames = _source("stages")
    fe = pkg.Frontend(*fe_args)
    s = Pictures(src, sw, sh, N_FRAMES).fill(frames).to_dev()
    cap = ctx.encode_bound(W, H) * N_FRAMES
    blob = torch.full((cap,), 0xA5, dtype=torch.uint8, device="cuda:0")
    offs = torch.full((N_FRAMES,), -1, dtype=torch.int64, device="cuda:0")
    lens = torch.full((N_FRAMES,), -1, dtype=torch.int32, device="cuda:0")
    state = torch.arange(65, dtype=torch.int32, device="cuda:0")
    bad = [None, pkg.Quant(0, NR, 0, 0, None), pkg.Quant(0, NR, 1, LAM, None), pkg.Quant(0, ctx.encode_nr_max(W, H) + 1, 1, LAM, state),
           pkg.Quant(0, NR, 1, ctx.encode_trellis_lambda_max() + 1, state), pkg.Quant(0, NR, 2, LAM, state), pkg.Quant(256, NR, 1, LAM, state),
           pkg.Quant(0, NR, 1, LAM, state.data_ptr() + 2)]
    for q in bad:
        with pytest.raises(pkg.AmvHipError, match=r"\(-1\)"):
            ctx.encode_frontend_quant_stream_dev(src, s.pic(), sw, sh, N_FRAMES, fe, W, H, q, blob, cap, offs, lens, stream())
    with pytest.raises(pkg.AmvHipError, match=r"\(-1\)"):                # an odd band, as in the entry without a request
        ctx.encode_frontend_quant_stream_dev(src, s.pic(), sw, sh, N_FRAMES, pkg.Frontend(1, (3, 0, 0, 0)), W, H, pkg.Quant(0, NR, 1, LAM, state),
                                             blob, cap, offs, lens, stream())
    torch.cuda.synchronize()
    assert (blob.cpu().numpy() == 0xA5).all() and (offs.cpu().numpy() == -1).all() and (lens.cpu().numpy() == -1).all()
    assert (state.cpu().numpy() == np.arange(65)).all()
    # lambda is not read without the trellis, and a null state is fine without -nr
    ok = pkg.Quant(QBIAS, 0, 0, 0xFFFFFFFF, None)
    ctx.encode_frontend_quant_stream_dev(src, s.pic(), sw, sh, N_FRAMES, fe, W, H, ok, blob, cap, offs, lens, stream())
    torch.cuda.synchronize()
    assert (lens.cpu().numpy() > 4).all()
