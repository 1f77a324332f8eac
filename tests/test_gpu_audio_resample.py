"""The audio resampler on the device (amvhip_audio_resample_*): bit-exact with outputs of the real reference
(tests/golden/ref_audio_resample.json) and with the CPU restatement (audio_resample_ref.py), in its batch and its streaming
form, and composed with the ADPCM-AMV encoder as the `-ac 1 -ar 22050` audio path of AMVmuxer/Makefile:16."""
import ctypes
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
import audio_resample_ref as R

FIXTURE = json.load(open(os.path.join(GOLDEN, "ref_audio_resample.json")))["cases"]


def _inputs(c):
    return R.make_input(c["input"]["kind"], c["input"]["seed"], c["input"]["frames"], c["in_ch"])


def run_batch(ctx, pkg, streams, in_ch, in_rate, out_ch, out_rate, gap_seed=None):
    """streams (interleaved int16 arrays) -> device outputs, one batch_dev call; gap_seed: odd gaps between streams, so
    that offsets are not 16-byte aligned"""
    import torch
    rng = np.random.default_rng(gap_seed) if gap_seed is not None else None
    pcm_offs, out_offs, nsamp, lens, pos, opos = [], [], [], [], 0, 0
    for s in streams:
        pos += int(rng.integers(0, 9)) if rng is not None else 0
        pcm_offs.append(pos)
        nsamp.append(len(s) // in_ch)
        pos += len(s)
        opos += int(rng.integers(0, 9)) if rng is not None else 0
        out_offs.append(opos)
        lens.append(pkg.audio_resample_out_samples(in_rate, out_rate, len(s) // in_ch) * out_ch)
        opos += lens[-1]
    pcm = np.zeros(pos + 8, np.int16)
    for o, s in zip(pcm_offs, streams):
        pcm[o:o + len(s)] = s
    dev = torch.device("cuda:0")
    d_pcm = torch.from_numpy(pcm).to(dev)
    d_out = torch.full((opos + 8,), 0x5A5A, dtype=torch.int16, device=dev)
    t = lambda a: torch.from_numpy(np.array(a, np.uint64).view(np.int64)).to(dev)
    ctx.audio_resample_batch_dev(d_pcm, t(pcm_offs), t(nsamp), len(streams), in_ch, in_rate, d_out, t(out_offs), out_ch,
                                 out_rate, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    gaps = np.ones(out.size, bool)
    for o, n in zip(out_offs, lens):
        gaps[o:o + n] = False
    assert (out[gaps] == 0x5A5A).all(), "the kernel wrote outside the streams' outputs"
    return [out[o:o + n] for o, n in zip(out_offs, lens)]


@pytest.mark.gpu
def test_batch_matches_the_reference_fixture(ctx, pkg):
    """every whole-stream case of the fixture (all rates into 22050, all channel modes, noise / square / silence, streams
    shorter than the filter), one batch per format"""
    groups = {}
    for c in FIXTURE:
        if c["packets"] is None:
            groups.setdefault((c["in_ch"], c["in_rate"], c["out_ch"], c["out_rate"]), []).append(c)
    assert len(groups) >= 32
    for (ic, ir, oc, orate), cases in groups.items():
        outs = run_batch(ctx, pkg, [_inputs(c) for c in cases], ic, ir, oc, orate, gap_seed=ir + ic)
        for c, o in zip(cases, outs):
            assert len(o) == c["out_frames"] * oc
            if "samples" in c:
                assert o.tolist() == c["samples"], c
            assert R.fnv1a64(o.tobytes()) == c["fnv"], c


@pytest.mark.gpu
@pytest.mark.parametrize("in_ch,in_rate,out_ch,out_rate,n", [
    (2, 44100, 1, 22050, 3000), (1, 48000, 1, 22050, 700), (2, 96000, 2, 22050, 200), (1, 8000, 2, 22050, 300),
    (1, 22050, 1, 44100, 100), (2, 11025, 2, 48000, 50), (2, 32000, 1, 22050, 1), (1, 16000, 1, 22050, 7),
    (1, 192000, 1, 1000, 3), (2, 1000, 2, 192000, 3)])
def test_ragged_batches_match_the_restatement(ctx, pkg, in_ch, in_rate, out_ch, out_rate, n):
    """ragged batches, 2 frames to 10 s per stream, unaligned offsets, downsampling and upsampling"""
    rng = np.random.default_rng(in_rate * 7 + n)
    budget = 2_500_000                                           # CPU restatement: about this many output frames a case
    frames = [int(v) for v in np.exp(rng.uniform(np.log(2), np.log(10 * in_rate), n))]
    frames[0] = 10 * in_rate                                     # one stream of 10 s
    if n > 1:
        frames[1] = 2
    while sum(pkg.audio_resample_out_samples(in_rate, out_rate, f) for f in frames) > budget:
        i = int(np.argmax(frames[1:])) + 1 if n > 1 else 0
        frames[i] //= 2
    kinds = ("noise", "square", "noise", "silence")
    streams = [R.make_input(kinds[i % 4], 1000 + i, f, in_ch) for i, f in enumerate(frames)]
    outs = run_batch(ctx, pkg, streams, in_ch, in_rate, out_ch, out_rate, gap_seed=n)
    for i, (s, o) in enumerate(zip(streams, outs)):
        want = R.resample_whole(s, in_ch, in_rate, out_ch, out_rate)
        assert o.tobytes() == want.tobytes(), (i, frames[i])


@pytest.mark.gpu
def test_host_buffer_form(ctx, pkg):
    streams = [R.make_input("noise", 77 + i, f, 2) for i, f in enumerate((44100, 3, 1000, 39, 40, 41))]
    pos, offs, outs = 0, [], []
    for s in streams:
        offs.append(pos + 1)
        pos += len(s) + 1
    pcm = np.zeros(pos, np.int16)
    for o, s in zip(offs, streams):
        pcm[o:o + len(s)] = s
    lens = [pkg.audio_resample_out_samples(44100, 22050, len(s) // 2) for s in streams]
    out_offs = np.cumsum([3] + lens[:-1]).astype(np.uint64) + np.arange(len(lens), dtype=np.uint64)
    out = np.full(int(out_offs[-1]) + lens[-1] + 5, 77, np.int16)
    ctx.audio_resample_batch(pcm, pcm.size, np.array(offs, np.uint64), np.array([len(s) // 2 for s in streams], np.uint64),
                             len(streams), 2, 44100, out, out.size, out_offs, 1, 22050)
    for s, o, n in zip(streams, out_offs, lens):
        assert out[int(o):int(o) + n].tobytes() == R.resample_whole(s, 2, 44100, 1, 22050).tobytes()
    assert out[0] == 77 and out[-1] == 77
    with pytest.raises(pkg.AmvHipError):                          # too small an output
        ctx.audio_resample_batch(pcm, pcm.size, np.array(offs, np.uint64), np.array([len(s) // 2 for s in streams], np.uint64),
                                 len(streams), 2, 44100, out, 10, out_offs, 1, 22050)


@pytest.mark.gpu
def test_streaming_matches_the_reference_fixture(ctx, pkg):
    """audio_resample per packet: every case of the fixture, the first packets that wrap the mirrored head included"""
    for c in FIXTURE:
        x = _inputs(c)
        sizes = R.packet_sizes(c["packets"], c["input"]["frames"])
        r = ctx.audio_resampler(c["out_ch"], c["in_ch"], c["out_rate"], c["in_rate"])
        outs, counts, pos = [], [], 0
        for nb in sizes:
            o = r.resample(x[pos * c["in_ch"]:(pos + nb) * c["in_ch"]])
            pos += nb
            outs.append(o)
            counts.append(len(o) // c["out_ch"])
        r.close()
        out = np.concatenate(outs)
        assert len(counts) == c["calls"] and sum(counts) == c["out_frames"], c
        assert R.fnv1a64(np.array(counts, np.int32).tobytes()) == c["counts_fnv"], c
        assert R.fnv1a64(out.tobytes()) == c["fnv"], c


@pytest.mark.gpu
def test_streaming_keeps_the_position_across_calls(ctx, pkg):
    """upsampling in tiny packets and downsampling in large ones, against the restatement line by line"""
    for in_ch, in_rate, out_ch, out_rate, spec in ((1, 8000, 2, 44100, {"first": 1, "seed": 3, "max": 5}),
                                                   (2, 48000, 1, 22050, {"seed": 4, "max": 9000}),
                                                   (2, 44100, 2, 22050, {"first": 2, "seed": 5, "max": 40})):
        x = R.make_input("noise", in_rate, 20000, in_ch)
        sizes = R.packet_sizes(spec, 20000)
        want, want_counts = R.resample_packets(x, in_ch, in_rate, out_ch, out_rate, sizes)
        r = ctx.audio_resampler(out_ch, in_ch, out_rate, in_rate)
        got, pos = [], 0
        for nb, wc in zip(sizes, want_counts):
            o = r.resample(x[pos * in_ch:(pos + nb) * in_ch])
            pos += nb
            assert len(o) == wc * out_ch
            got.append(o)
        r.close()
        assert np.concatenate(got).tobytes() == want.tobytes()


@pytest.mark.gpu
def test_ac1_ar22050_audio_path(ctx, pkg, orc):
    """`-ac 1 -ar 22050` of AMVmuxer/Makefile:16: 44.1 kHz stereo -> amvhip_audio_resample_batch_dev -> chunks framed by
    amvhip_amv_audio_pairs -> amvhip_adpcm_encode_batch_dev with the step index carried == the oracle's ADPCM-AMV encoder
    on the restated PCM"""
    import torch
    lib = pkg.load_library()
    dev = torch.device("cuda:0")
    frames = 3 * 44100 + 777
    x = R.make_input("noise", 9, frames, 2)
    x[: 2 * 20000] = R.make_input("square", 9, 20000, 2)        # full scale at the start
    n_out = pkg.audio_resample_out_samples(44100, 22050, frames)
    d_pcm = torch.from_numpy(x).to(dev)
    d_mono = torch.zeros(n_out, dtype=torch.int16, device=dev)
    zero = torch.zeros(1, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    ctx.audio_resample_batch_dev(d_pcm, zero, torch.tensor([frames], dtype=torch.int64, device=dev), 1, 2, 44100, d_mono, zero,
                                 1, 22050, st)
    mono = R.resample_whole(x, 2, 44100, 1, 22050)
    torch.cuda.synchronize()
    assert d_mono.cpu().numpy().tobytes() == mono.tobytes()
    # framing: adpcm.c:469-477 for frame_size 1378 (amvenc.c:276-281 at 16 fps)
    fs = lib.amvhip_amv_audio_frame_size(22050, 1, 16)
    extra, written = ctypes.c_uint32(0), ctypes.c_uint64(0)
    offs, nsamp, pos = [], [], 0
    while True:
        pairs = lib.amvhip_amv_audio_pairs(fs, 22050, ctypes.byref(extra), ctypes.byref(written))
        if pos + 2 * pairs > n_out:
            break
        offs.append(pos)
        nsamp.append(2 * pairs)
        pos += 2 * pairs
    n = len(offs)
    assert n > 20
    blob_offs = np.cumsum([0] + [8 + s // 2 for s in nsamp[:-1]]).astype(np.uint64)
    cap = int(blob_offs[-1]) + 8 + nsamp[-1] // 2
    d_blob = torch.zeros(cap, dtype=torch.uint8, device=dev)
    ctx.adpcm_encode_batch_dev(d_mono, torch.from_numpy(np.array(offs, np.int64)).to(dev),
                               torch.from_numpy(np.array(nsamp, np.uint32).view(np.int32)).to(dev), n, None, d_blob,
                               torch.from_numpy(blob_offs.view(np.int64)).to(dev), st)
    torch.cuda.synchronize()
    blob = d_blob.cpu().numpy()
    step = 0
    for i in range(n):
        want, step = orc.adpcm_encode_chunk(mono[offs[i]:offs[i] + nsamp[i]], step)
        o = int(blob_offs[i])
        assert blob[o:o + len(want)].tobytes() == want, i
