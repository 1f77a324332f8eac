"""-nr and the trellis quantiser in one call, restated in Python by composing nr_ref and trellis_ref (a helper of the tests).

    dct_quantize_trellis_c   libavcodec/mpegvideo_enc.c:2987-2990   s->dsp.fdct(block); if (s->dct_error_sum) s->denoise_dct(s, block);

The reference denoises right behind the fdct and searches on what comes out.  So, per frame:

    coef = fdct(blocks)                                   nr_ref
    offsets = frame_start(state, nr)                      nr_ref: update_noise_reduction
    coef = denoise_blocks(state, offsets, coef)           nr_ref: denoise_dct_c -- the sums are taken of the outputs as the
                                                          fdct left them, then the dead zone is applied
    levels = quantize_trellis(coef)                       trellis_ref: the DC amvo_quantize_block's of the denoised DC, the
                                                          AC levels the walk's on the denoised outputs

    product mode     encode_stream: what amvhip_encode_*_nr_trellis_stream* code (samples - 128, the DC as DC + 8192 in
                     the sums and the dead zone, AMV's fixed steps and code: see the two parents)
    reference mode   reference_blocks: dct_quantize_trellis_c as tests/golden/make_ref_nr_trellis_golden.py feeds the real
                     one -- un-shifted sample blocks, a hand-filled dct_error_sum / dct_count / dct_offset -- for the fixture
                     tests/golden/ref_nr_trellis.json.  Two wrong models are its variants, which the maker tells apart from
                     the reference: search_undenoised (the walk sees the fdct's outputs, not the denoised ones) and
                     sum_denoised (the sums are taken behind the dead zone).
"""
import numpy as np

import nr_ref as N
import trellis_ref as T


def encode_stream(frames, w, h, nr, lam, state=None, qbias=0, truncate=True, halve=True, want_coef=False, faults=()):
    """frames: [(y, cb, cr)] planes of 2-D uint8 -> the chunks (or, want_coef, the zig-zag lines per frame); state (65 int64,
    N.new_state() when None) changes in place.  nr = 0 leaves it alone and gives T.encode_frames.  truncate / halve: as in
    N.frame_start; faults: N.faults_of, handed on"""
    if state is None:
        state = N.new_state()
    outside = N.outside_blocks(w, h) if "padding_not_summed" in N.faults_of(faults) else None
    out = []
    for y, cb, cr in frames:
        coef = N.fdct(N.frame_blocks(y, cb, cr, w, h, 128))
        if nr:
            coef = N.denoise_blocks(state, N.frame_start(state, nr, truncate, halve, faults), coef, N.DC_SHIFT, faults, outside)
            if faults:
                coef = N._int16(coef)
        zz = T.quantize_trellis(coef, qbias, lam)
        out.append(zz if want_coef else N._chunk(zz))
    return out


# ---- reference mode ----------------------------------------------------------------------------------------------------------

def reference_state(offsets_seed):
    """a seeded state in the middle of a stream and the offsets update_noise_reduction makes of it -> (state of 65 int64,
    offsets of 64): what the fixture's harness writes into dct_error_sum[1], dct_count[1] and dct_offset[1].  Mean magnitudes
    of 2 .. 120 per AC position (8192 at the DC, un-shifted samples) under an nr of 300, 1200 or 3000: offsets from 2 to
    1500, the DC's 0"""
    rng = np.random.default_rng(offsets_seed)
    count = 4000
    mean = rng.integers(2, 121, 64)
    mean[0] = 8192
    state = np.concatenate([count * mean + rng.integers(0, count, 64), [count]]).astype(np.int64)
    nr = int(rng.choice([300, 1200, 3000]))
    offsets = N.frame_start(state.copy(), nr)
    return state, offsets


def reference_blocks(samples, qscale, lam, length, esc_length, state, offsets, search_undenoised=False, sum_denoised=False):
    """samples: [(64,) un-shifted, row-major] -> int16 [blocks, 65]: the levels as dct_quantize_trellis_c leaves them with a
    dct_error_sum set, then its return value; state changes in place as denoise_dct_c changes it (offsets stay: they are
    the frame's)"""
    out = []
    for s in samples:
        raw = N.fdct(np.asarray(s)[None])
        den = N.denoise_blocks(state, offsets, raw, 0)
        if sum_denoised:                                   # (wrong) the sums behind the dead zone
            state[:64] += np.abs(den[0]) - np.abs(raw[0])
        levels, last = T.trellis_block_reference((raw if search_undenoised else den)[0], qscale, lam, length, esc_length)
        out.append(levels + [last])
    return np.array(out, np.int16)
