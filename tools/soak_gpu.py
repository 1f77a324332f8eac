#!/usr/bin/env python3
"""Soak runs of the HIP path against the CPU oracle, longer and wider than the test suite's cases (run on the GPU box:
`gpurun -- python tools/soak_gpu.py adpcm 0 150`).  Each seed draws its own geometry / content / damage; a run prints one
line per mismatch and a summary, and exits non-zero if anything differed.

  adpcm  LO HI   chained IMA-ADPCM encode of ragged streams (a few hundred to a few thousand chunks, some empty or short),
                 three times each, every byte against the oracle's sequential encode.  Round 4: two holes in the index
                 chain's list handling passed every test and showed up here within forty streams.
  decode LO HI   batches of random size and content (synthetic, noise, flat, noisy synthetic), a third of the chunks damaged
                 or cut, every entropy lane count, both output modes: pixels and statuses against the oracle.
  ffmpeg LO HI   the same kind of batches through AMVHIP_FLAG_FFMPEG (planar YUVJ420P, the fork's own arithmetic and flip; odd
                 sizes too), every second seed with AMVHIP_FLAG_FFMPEG_KEEP over a buffer of random bytes: every byte against
                 the oracle's restatement -- whole blocks in front of a chunk's first error written, nothing else touched.
  encode LO HI   random geometries, strides, channel orders, quantiser biases and content: chunks against the oracle's.
  trellis LO HI  the trellis entry on random small geometries (up to ~2 000 blocks a seed: the model is Python), channel
                 orders, quantiser biases, lambdas from 0 to the bound and content, in both entropy modes: chunks against
                 the product mode of tests/trellis_ref.py.
  qns LO HI      the -qns entry on random small geometries (up to ~1 000 blocks a seed: the model is Python), channel orders,
                 quantiser biases, qns 1 .. 3, lambda2 from 0 to the bound, behind the plain quantiser or the trellis, in
                 both entropy modes: chunks against the product mode of tests/qns_ref.py.
  rate LO HI     the rate entries on random small geometries (up to ~600 blocks a seed and ladders of 1 .. 6 rungs in any
                 order, duplicates included: the model is Python), quantiser biases, every third seed behind -nr from a seeded
                 state, budgets drawn per frame around the model's own lengths and floors (so that frames land on every rung,
                 take redo passes and run over), uniform every fourth seed, in both entropy modes: d_bits of the probe,
                 chunks, d_rung and the state against tests/rate_ref.py.
  requant LO HI  the requant entries on seeded chunks of random small geometries, odd sizes included (up to ~600 blocks a seed:
                 the model is Python): the oracle's synthetic frames and crafted blocks at the edges of the range rule, a third
                 of the chunks damaged -- a flipped byte, a cut, junk behind the scan -- one lambda from 0 to the bound and a
                 ladder of 1 .. 6 rungs in any order with budgets drawn per frame around the model's own lengths, in both
                 entropy modes: chunks, offsets, d_status, d_err, d_bits and d_rung against tests/requant_ref.py.
  retable LO HI  the re-table entries on seeded 48x32-or-smaller pictures coded as the reference's encoder codes them
                 (tests/retable_ref.reference_chunks) at a qscale drawn per frame, and on the oracle's synthetic chunks read against
                 seeded tables of steps 1 .. 40: 1 .. 4 tables a call named by d_table_of (a bad index among them every fourth
                 seed), a fifth of the chunks cut, one lambda from 0 to the bound, a ladder of 1 .. 5 rungs with budgets per
                 frame around the model's lengths and a total around its sums, in both entropy modes: chunks, offsets, d_status,
                 d_err, d_bits, d_rung and d_clip against tests/retable_ref.py.
  clip LO HI     the clip entries on soak_rate's geometries, ladders, -nr states and budgets per frame (a third without a cap),
                 every fifth seed through the requant entry on chunks of which a quarter are cut; the total drawn around the
                 model's own S(c) and F(c), 0 and 2^64 - 1 among them (so that clips stay, move after coding, pass rungs on their
                 floor sums and run over), in both entropy modes: chunks, offsets, d_rung, d_clip, d_status and the state against
                 tests/clip_ref.py, and the model's device walk against its definition.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402
from conftest import SEED  # noqa: E402


def soak_adpcm(pkg, orc, lo, hi):
    ctx = pkg.Context(0)
    bad = repaired = 0
    for seed in range(lo, hi):
        rng = np.random.default_rng(seed)
        n = int(rng.integers(200, 6000))
        sizes = [1378 if rng.integers(0, 10) else 2 * int(rng.integers(0, 700)) for _ in range(n)]
        pcm_offs = np.cumsum([0] + sizes).astype(np.uint64)
        pcm = orc.synth_audio(SEED + seed, 777, int(pcm_offs[-1]) + 2)
        offs = np.cumsum([0] + [8 + s // 2 for s in sizes]).astype(np.uint64)
        want, idx = [], 0
        for i in range(n):
            seg = pcm[int(pcm_offs[i]):int(pcm_offs[i + 1])]
            if seg.size:
                chunk, idx = orc.adpcm_encode_chunk(seg, idx)
            else:
                chunk = bytes([0, 0, idx, 0, 0, 0, 0, 0])
            want.append(chunk)
        want = b"".join(want)
        for rep in range(3):
            blob = np.full(int(offs[-1]), 0xEE, np.uint8)
            ctx.adpcm_encode_batch(pcm, pcm.size, pcm_offs[:-1].copy(), np.array(sizes, np.uint32), n, None, blob, blob.size, offs[:-1].copy())
            if ctx.adpcm_chain_stats()["exhaustive"]:      # the chain's check (or its settle kernel) sent the stream down the slow route
                repaired += 1
                print("exhaustive route taken: adpcm seed", seed, "rep", rep, "chunks", n, ctx.adpcm_chain_stats(), flush=True)
            if blob.tobytes() != want:
                bad += 1
                d = np.nonzero(blob != np.frombuffer(want, np.uint8))[0]
                ch = int(np.searchsorted(offs, d[0], side="right") - 1)
                print("MISMATCH adpcm seed", seed, "rep", rep, "chunks", n, "bytes", d.size, "first in chunk", ch, "at", int(d[0] - offs[ch]),
                      ctx.adpcm_chain_stats(), flush=True)
    print("adpcm: streams that took the exhaustive route (none expected on ordinary audio):", repaired)
    return bad


def soak_decode(pkg, orc, lo, hi):
    import test_gpu_parity as T
    bad = 0
    for seed in range(lo, hi):
        rng = np.random.default_rng(seed)
        w, h, n = 2 * int(rng.integers(8, 220)), 2 * int(rng.integers(8, 160)), int(rng.integers(3, 90))
        chunks = []
        for t in range(n):
            kind = int(rng.integers(0, 4))
            if kind == 0:
                src = orc.synth_frame(SEED, 1000 * seed + t, w, h)
            elif kind == 1:
                src = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
            elif kind == 2:
                src = np.full((h, w, 3), int(rng.integers(0, 256)), np.uint8)
            else:
                src = (orc.synth_frame(SEED, t, w, h).astype(np.int32) + rng.integers(-40, 41, (h, w, 3))).clip(0, 255).astype(np.uint8)
            c = bytearray(orc.encode_frame(src, w, h, qbias=int(rng.integers(0, 2)) * 128))
            if rng.random() < 0.35 and len(c) > 8:
                for _ in range(int(rng.integers(1, 5))):
                    c[int(rng.integers(2, len(c) - 2))] ^= 1 << int(rng.integers(0, 8))
            if rng.random() < 0.1:
                c = c[: int(rng.integers(2, len(c)))]
            chunks.append(bytes(c))
        flags = seed & 1
        want, wst = T._oracle_decode(orc, chunks, w, h, flags)
        for lanes in ("1", "2", "16", None):
            if lanes:
                os.environ["AMVHIP_SYNC_LANES"] = lanes
            else:
                os.environ.pop("AMVHIP_SYNC_LANES", None)
            ctx = pkg.Context(0)
            got, st = T._gpu_decode(ctx, chunks, w, h, flags, pad_front=int(rng.integers(0, 4)))
            ctx.close()
            if not ((st == wst).all() and (got == want).all()):
                bad += 1
                print("MISMATCH decode seed", seed, w, h, n, "lanes", lanes, flush=True)
    os.environ.pop("AMVHIP_SYNC_LANES", None)
    return bad


def soak_ffmpeg(pkg, orc, lo, hi):
    import torch
    import test_gpu_parity as T
    bad = 0
    for seed in range(lo, hi):
        rng = np.random.default_rng(seed)
        w, h, n = int(rng.integers(16, 400)), int(rng.integers(16, 300)), int(rng.integers(3, 60))
        ew, eh = w + (w & 1), h + (h & 1)            # (the encoder takes even sizes; the decoder is told the odd one)
        chunks = []
        for t in range(n):
            kind = int(rng.integers(0, 3))
            if kind == 0:
                src = orc.synth_frame(SEED, 1000 * seed + t, ew, eh)
            elif kind == 1:
                src = rng.integers(0, 256, (eh, ew, 3)).astype(np.uint8)
            else:
                src = (orc.synth_frame(SEED, t, ew, eh).astype(np.int32) + rng.integers(-40, 41, (eh, ew, 3))).clip(0, 255).astype(np.uint8)
            c = bytearray(orc.encode_frame(src, ew, eh, qbias=int(rng.integers(0, 2)) * 128))
            if rng.random() < 0.4 and len(c) > 12:
                for _ in range(int(rng.integers(1, 5))):
                    c[int(rng.integers(4, len(c) - 2))] ^= 1 << int(rng.integers(0, 8))
            if rng.random() < 0.15:
                c = c[: int(rng.integers(2, len(c)))]
            chunks.append(bytes(c))
        keep = bool(seed & 1)
        fb = orc.decode_frame_ffmpeg(chunks[0], w, h)[0].size
        before = rng.integers(0, 256, (n, fb), dtype=np.uint8)
        want, wst = [], []
        for i, c in enumerate(chunks):
            o, st, _ = orc.decode_frame_ffmpeg_keep(c, w, h, before[i]) if keep else orc.decode_frame_ffmpeg(c, w, h)
            want.append(o)
            wst.append(st)
        want, wst = np.stack(want), np.array(wst, np.int32)
        blob, offs, lens, nbytes = T._blob_of(chunks, int(rng.integers(0, 4)))
        flags = pkg.FLAG_FFMPEG | (pkg.FLAG_FFMPEG_KEEP if keep else 0)
        for lanes in ("1", "4", "64", None):
            if lanes:
                os.environ["AMVHIP_SYNC_LANES"] = lanes
            else:
                os.environ.pop("AMVHIP_SYNC_LANES", None)
            ctx = pkg.Context(0)
            d_out = torch.from_numpy(before.copy()).to("cuda:0")
            d_st = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
            ctx.decode_batch_dev(T._t(blob), nbytes, T._t(offs), T._t(lens), n, w, h, flags, d_out, d_st, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            ctx.close()
            if not ((d_st.cpu().numpy() == wst).all() and (d_out.cpu().numpy() == want).all()):
                bad += 1
                print("MISMATCH ffmpeg seed", seed, w, h, n, "keep" if keep else "plain", "lanes", lanes, flush=True)
    os.environ.pop("AMVHIP_SYNC_LANES", None)
    return bad


def soak_encode(pkg, orc, lo, hi):
    import torch
    import test_gpu_parity as T
    ctx = pkg.Context(0)
    bad = 0
    for seed in range(lo, hi):
        rng = np.random.default_rng(seed)
        w, h, n = 2 * int(rng.integers(4, 330)), 2 * int(rng.integers(4, 250)), int(rng.integers(1, 40))
        n = max(1, min(n, 6_000_000 // (w * h)))
        bgr, qbias = int(rng.integers(0, 2)), 128 * int(rng.integers(0, 2))
        stride = w * 3 + int(rng.integers(0, 3)) * 5
        kind = int(rng.integers(0, 5))
        if kind == 0:
            pix = rng.integers(0, 256, (n, h, w, 3)).astype(np.uint8)
        elif kind == 1:
            pix = np.stack([orc.synth_frame(SEED, 31 * seed + t, w, h) for t in range(n)])
        elif kind == 2:
            pix = np.full((n, h, w, 3), int(rng.integers(0, 256)), np.uint8)
        elif kind == 3:
            pix = np.stack([orc.synth_frame(SEED, 7 * seed + t, w, h) for t in range(n)]).astype(np.int32)
            pix = (pix + rng.integers(-60, 61, pix.shape)).clip(0, 255).astype(np.uint8)
        else:                                       # a flat picture with islands of noise
            pix = np.full((n, h, w, 3), 128, np.uint8)
            for _ in range(int(rng.integers(1, 30))):
                y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
                patch = pix[int(rng.integers(0, n)), y:y + 8, x:x + 8]
                patch[...] = rng.integers(0, 256, patch.shape)
        src = np.zeros((n, h, stride), np.uint8)
        src[:, :, : w * 3] = pix.reshape(n, h, w * 3)
        src[:, :, w * 3:] = 0xEE
        cap = ctx.encode_bound(w, h) * n
        d_blob = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
        d_offs = torch.zeros(n, dtype=torch.int64, device="cuda:0")
        d_lens = torch.zeros(n, dtype=torch.int32, device="cuda:0")
        ctx.encode_batch_dev(T._t(src), stride, bgr, n, w, h, qbias, d_blob, cap, d_offs, d_lens)
        torch.cuda.synchronize()
        blob, offs, lens = d_blob.cpu().numpy(), d_offs.cpu().numpy(), d_lens.cpu().numpy()
        for i in range(n):
            want = orc.encode_frame(np.ascontiguousarray(pix[i]), w, h, bgr=bool(bgr), qbias=qbias)
            if int(lens[i]) != len(want) or blob[int(offs[i]):int(offs[i]) + len(want)].tobytes() != want:
                bad += 1
                print("MISMATCH encode seed", seed, w, h, n, "frame", i, "kind", kind, flush=True)
                break
    return bad


def soak_trellis(pkg, orc, lo, hi):
    import torch
    import pixel_builder as pb
    import test_gpu_parity as T
    import trellis_ref as R
    ctx = pkg.Context(0)
    bad = 0
    for seed in range(lo, hi):
        rng = np.random.default_rng(seed)
        w, h = 2 * int(rng.integers(4, 120)), 2 * int(rng.integers(4, 90))
        n = max(1, min(int(rng.integers(1, 8)), 2000 // (6 * ((w + 15) // 16) * ((h + 15) // 16))))
        bgr, qbias = int(rng.integers(0, 2)), int(rng.choice([0, 128, int(rng.integers(0, 256))]))
        lam = int(rng.choice([0, 3481, R.LAMBDA_MAX, int(rng.integers(0, R.LAMBDA_MAX + 1)), int(rng.integers(0, 20000))]))
        kind = int(rng.integers(0, 3))
        if kind == 0:
            pix = rng.integers(0, 256, (n, h, w, 3)).astype(np.uint8)
        elif kind == 1:
            pix = np.stack([orc.synth_frame(SEED, 31 * seed + t, w, h) for t in range(n)])
        else:
            pix = np.stack([orc.synth_frame(SEED, 7 * seed + t, w, h) for t in range(n)]).astype(np.int32)
            pix = (pix + rng.integers(-40, 41, pix.shape)).clip(0, 255).astype(np.uint8)
        frames = [pb.to_planes(orc, pix[t], w, h, bgr) for t in range(n)]
        want = [R.N._chunk(zz) for zz in R.encode_frames(frames, w, h, qbias, lam, want_coef=True)]
        cap = ctx.encode_bound(w, h) * n
        for mode in (pkg.ENTROPY_AUTO, pkg.ENTROPY_SERIAL):
            ctx.set_entropy_mode(mode)
            d_blob = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
            d_offs = torch.zeros(n, dtype=torch.int64, device="cuda:0")
            d_lens = torch.zeros(n, dtype=torch.int32, device="cuda:0")
            ctx.encode_trellis_batch_dev(T._t(pix), w * 3, bgr, n, w, h, qbias, lam, d_blob, cap, d_offs, d_lens)
            torch.cuda.synchronize()
            blob, offs, lens = d_blob.cpu().numpy(), d_offs.cpu().numpy(), d_lens.cpu().numpy()
            for i in range(n):
                if int(lens[i]) != len(want[i]) or blob[int(offs[i]):int(offs[i]) + len(want[i])].tobytes() != want[i]:
                    bad += 1
                    print("MISMATCH trellis seed", seed, w, h, n, "frame", i, "kind", kind, "qbias", qbias, "lambda", lam, "mode", mode, flush=True)
                    break
        ctx.set_entropy_mode(pkg.ENTROPY_AUTO)
    return bad


def soak_qns(pkg, orc, lo, hi):
    import torch
    import pixel_builder as pb
    import qns_ref as Q
    import test_gpu_parity as T
    import trellis_ref as R
    ctx = pkg.Context(0)
    bad = 0
    for seed in range(lo, hi):
        rng = np.random.default_rng(seed)
        w, h = 2 * int(rng.integers(4, 100)), 2 * int(rng.integers(4, 70))
        n = max(1, min(int(rng.integers(1, 6)), 1000 // (6 * ((w + 15) // 16) * ((h + 15) // 16))))
        bgr, qbias = int(rng.integers(0, 2)), int(rng.choice([0, 128, int(rng.integers(0, 256))]))
        qns = int(rng.integers(1, 4))
        lambda2 = int(rng.choice([0, 6962, Q.LAMBDA2_MAX, int(rng.integers(0, Q.LAMBDA2_MAX + 1)), int(rng.integers(0, 40000))]))
        lam = int(rng.choice([0, 3481]))             # the trellis in front of it, every second seed
        trellis = seed & 1
        kind = int(rng.integers(0, 3))
        if kind == 0:
            pix = rng.integers(0, 256, (n, h, w, 3)).astype(np.uint8)
        elif kind == 1:
            pix = np.stack([orc.synth_frame(SEED, 31 * seed + t, w, h) for t in range(n)])
        else:
            pix = np.stack([orc.synth_frame(SEED, 7 * seed + t, w, h) for t in range(n)]).astype(np.int32)
            pix = (pix + rng.integers(-40, 41, pix.shape)).clip(0, 255).astype(np.uint8)
        frames = [pb.to_planes(orc, pix[t], w, h, bgr) for t in range(n)]
        base = R.encode_frames(frames, w, h, qbias, lam, want_coef=True) if trellis else R.encode_frames_plain(frames, w, h, qbias, want_coef=True)
        want = [R.N._chunk(zz) for zz in Q.refine_lines(frames, w, h, base, qns, lambda2)]
        cap = ctx.encode_bound(w, h) * n
        for mode in (pkg.ENTROPY_AUTO, pkg.ENTROPY_SERIAL):
            ctx.set_entropy_mode(mode)
            d_blob = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
            d_offs = torch.zeros(n, dtype=torch.int64, device="cuda:0")
            d_lens = torch.zeros(n, dtype=torch.int32, device="cuda:0")
            ctx.encode_qns_stream_dev(T._t(pix), w * 3, bgr, n, w, h, pkg.Quant(qbias, 0, trellis, lam, None), qns, lambda2, d_blob, cap, d_offs,
                                      d_lens)
            torch.cuda.synchronize()
            blob, offs, lens = d_blob.cpu().numpy(), d_offs.cpu().numpy(), d_lens.cpu().numpy()
            for i in range(n):
                if int(lens[i]) != len(want[i]) or blob[int(offs[i]):int(offs[i]) + len(want[i])].tobytes() != want[i]:
                    bad += 1
                    print("MISMATCH qns seed", seed, w, h, n, "frame", i, "kind", kind, "qbias", qbias, "qns", qns, "lambda2", lambda2, "trellis",
                          trellis, lam, "mode", mode, flush=True)
                    break
        ctx.set_entropy_mode(pkg.ENTROPY_AUTO)
    print("the most changes a block took:", Q.most_changes())
    return bad


def soak_rate(pkg, orc, lo, hi):
    import torch
    import rate_ref as R
    import test_gpu_parity as T
    ctx = pkg.Context(0)
    bad = frames_seen = redone = over = 0
    for seed in range(lo, hi):
        rng = np.random.default_rng(seed)
        w, h = 2 * int(rng.integers(4, 60)), 2 * int(rng.integers(4, 50))
        blocks = 6 * ((w + 15) // 16) * ((h + 15) // 16)
        n = max(1, min(int(rng.integers(1, 7)), 600 // blocks))
        qbias = int(rng.choice([0, 128, int(rng.integers(0, 256))]))
        rungs = int(rng.integers(1, 7))
        pool = [0, 400, 3481, 20000, R.T.LAMBDA_MAX, int(rng.integers(0, R.T.LAMBDA_MAX + 1)), int(rng.integers(0, 30000))]
        ladder = [int(rng.choice(pool)) for _ in range(rungs)]
        if seed & 1:
            ladder.sort()
        nr = int(rng.integers(1, ctx.encode_nr_max(w, h) + 1)) if seed % 3 == 0 else 0
        state = None
        if nr:
            count = int(rng.integers(1, 65000))
            state = np.concatenate([rng.integers(0, 200, 64) * count, [count]]).astype(np.int64)
        frames = R.N.stream(w, h, [R.KINDS[int(rng.integers(0, 4))] for _ in range(n)], 1000 + seed)
        bits = R.bits_table(frames, w, h, qbias, nr, state, ladder)
        lens = R.lens_table(frames, w, h, qbias, nr, state, ladder)
        B = []
        for i in range(n):
            r = int(rng.integers(0, rungs))
            B.append(max(0, int(rng.choice([lens[i][r], lens[i][r] - 1, R.floor_bytes(int(bits[i][r])), R.floor_bytes(int(bits[i][r])) - 1, 7,
                                            0xFFFFFFFF, int(rng.integers(0, int(lens[i].max()) + 2))]))))
        uniform = seed % 4 == 3
        if uniform:
            B = [B[0]] * n
        want, want_rungs, want_state = R.encode(frames, w, h, qbias, nr, state, ladder, B)
        frames_seen += n
        redone += sum(R.device_walk(bits[i], lens[i], B[i])[2] > 1 for i in range(n))
        over += sum(1 for r in want_rungs if r & R.OVER)
        n_pad = 8
        Y = np.full((n, h, w + n_pad), 0xEE, np.uint8)
        Cb, Cr = np.full((n, h // 2, w // 2 + n_pad), 0xEE, np.uint8), np.full((n, h // 2, w // 2 + n_pad), 0xEE, np.uint8)
        for i, (y, cb, cr) in enumerate(frames):
            Y[i, :, :w], Cb[i, :, :w // 2], Cr[i, :, :w // 2] = y, cb, cr
        planes = (T._t(Y), T._t(Cb), T._t(Cr), w + n_pad, w // 2 + n_pad, h * (w + n_pad), (h // 2) * (w // 2 + n_pad), n, w, h)
        cap = ctx.encode_bound(w, h) * n
        for mode in (pkg.ENTROPY_AUTO, pkg.ENTROPY_SERIAL):
            ctx.set_entropy_mode(mode)
            d_state = None if state is None else T._t(state.astype(np.int32))
            d_bits = torch.zeros((n, rungs), dtype=torch.int32, device="cuda:0")
            ctx.encode_yuv420_rate_probe_dev(*planes, pkg.Quant(qbias, nr, 1, 0, d_state), ladder, d_bits)
            d_blob = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
            d_offs = torch.zeros(n, dtype=torch.int64, device="cuda:0")
            d_lens = torch.zeros(n, dtype=torch.int32, device="cuda:0")
            d_rung = torch.zeros(n, dtype=torch.int32, device="cuda:0")
            d_budget = None if uniform else T._t(np.array(B, np.uint32))
            ctx.encode_yuv420_rate_stream_dev(*planes, pkg.Quant(qbias, nr, 1, 0, d_state), pkg.Rate(ladder, budget=B[0], d_budget=d_budget),
                                              d_blob, cap, d_offs, d_lens, d_rung)
            torch.cuda.synchronize()
            blob, offs, got_lens = d_blob.cpu().numpy(), d_offs.cpu().numpy(), d_lens.cpu().numpy()
            ok = (d_bits.cpu().numpy().view(np.uint32) == bits).all() and d_rung.cpu().numpy().view(np.uint32).tolist() == want_rungs
            ok = ok and (state is None or (d_state.cpu().numpy() == want_state).all())
            ok = ok and all(int(got_lens[i]) == len(want[i]) and blob[int(offs[i]):int(offs[i]) + len(want[i])].tobytes() == want[i] for i in range(n))
            if not ok:
                bad += 1
                print("MISMATCH rate seed", seed, w, h, n, "qbias", qbias, "nr", nr, "ladder", ladder, "budgets", B, "uniform", uniform, "mode", mode,
                      flush=True)
        ctx.set_entropy_mode(pkg.ENTROPY_AUTO)
    print("frames", frames_seen, "coded more than once", redone, "over every rung", over)
    return bad


def soak_requant(pkg, orc, lo, hi):
    import torch
    import requant_ref as Q
    import test_gpu_parity as T
    ctx = pkg.Context(0)
    bad = frames_seen = not_coded = out_of_range = 0
    for seed in range(lo, hi):
        rng = np.random.default_rng(seed)
        w, h = int(rng.integers(1, 120)), int(rng.integers(1, 100))
        blocks = Q.nblocks(w, h)
        n = max(1, min(int(rng.integers(1, 9)), 600 // blocks))
        chunks = Q.synth_chunks(w + (w & 1), h + (h & 1), n, seed=SEED + seed, qbias=int(rng.choice([0, 128])))
        for i in range(n):
            kind = int(rng.integers(0, 9))
            c = bytearray(chunks[i])
            if kind == 0 and len(c) > 8:                                    # a flipped byte inside the scan
                c[int(rng.integers(2, len(c) - 2))] ^= 1 << int(rng.integers(0, 8))
            elif kind == 1:                                                 # cut
                c = c[: int(rng.integers(2, len(c)))]
            elif kind == 2:                                                 # junk behind the scan
                c = c[:-2] + bytes(rng.integers(0, 255, 3, dtype=np.uint8)) + b"\xff\xd9"
            elif kind == 3:                                                 # a block at an edge of the range rule, in or out
                zz = Q.decode(chunks[i], w, h)[0].copy()
                b = int(rng.integers(0, blocks))
                k = int(rng.integers(1, 64))
                edge = Q.COEF_MOST // (8 * int(Q.T.QUANT[Q.comp_of(b)][k])) + int(rng.integers(0, 2))
                zz[b, k] = edge if rng.integers(0, 2) else -edge
                if rng.integers(0, 2) and Q.comp_of(b) == 0:
                    zz[b] = Q.block_of({**Q.AT_ENERGY_MOST, 59: 15 + int(rng.integers(0, 2))}, dc=int(zz[b, 0]))
                c = Q.N._chunk(zz)
            chunks[i] = bytes(c)
        lam = int(rng.choice([0, 200, 3481, 20000, Q.LAMBDA_MAX, int(rng.integers(0, Q.LAMBDA_MAX + 1))]))
        rungs = int(rng.integers(1, 7))
        ladder = [int(rng.choice([0, 1000, 3481, 20000, Q.LAMBDA_MAX, int(rng.integers(0, 60000))])) for _ in range(rungs)]
        if seed & 1:
            ladder.sort()
        want, status, err = Q.requant(chunks, w, h, lam)
        bits = Q.bits_table(chunks, w, h, ladder)
        sizes = [[len(c) if c else 0 for c in Q.requant(chunks, w, h, x)[0]] for x in ladder]
        B = [max(0, int(rng.choice([sizes[int(rng.integers(0, rungs))][i], sizes[int(rng.integers(0, rungs))][i] - 1, 7, 0xFFFFFFFF])))
             for i in range(n)]
        want_rate, _, want_rungs = Q.rate(chunks, w, h, ladder, B)
        frames_seen += n
        not_coded += sum(1 for x in status if x)
        out_of_range += sum(1 for x in status if x == Q.ST_RANGE)
        blob, offs, lens = Q.pack(chunks)
        ins = (T._t(blob), int(lens.sum()), T._t(offs), T._t(lens), n, w, h)
        cap = sum(len(c) for c in chunks) + 64

        def same(d_blob, d_offs, d_lens, chunks_want):
            got, o, ln = d_blob.cpu().numpy(), d_offs.cpu().numpy(), d_lens.cpu().numpy()
            pos = 0
            for i, c in enumerate(chunks_want):
                size = len(c) if c else 0
                if (int(o[i]), int(ln[i])) != (pos, size) or (size and got[pos: pos + size].tobytes() != c):
                    return False
                pos += size
            return True

        for mode in (pkg.ENTROPY_AUTO, pkg.ENTROPY_SERIAL):
            ctx.set_entropy_mode(mode)
            outs = [(torch.zeros(cap, dtype=torch.uint8, device="cuda:0"), torch.zeros(n, dtype=torch.int64, device="cuda:0"),
                     torch.zeros(n, dtype=torch.int32, device="cuda:0"), torch.full((n,), -1, dtype=torch.int32, device="cuda:0")) for _ in range(2)]
            d_err = torch.full((n, 3), -1, dtype=torch.int64, device="cuda:0")
            d_bits = torch.full((n, rungs), -1, dtype=torch.int32, device="cuda:0")
            d_rung = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
            ctx.requant_stream_dev(*ins, lam, outs[0][0], cap, *outs[0][1:], d_err)
            ctx.requant_rate_probe_dev(*ins, ladder, d_bits)
            ctx.requant_rate_stream_dev(*ins, pkg.Rate(ladder, budget=1, d_budget=T._t(np.array(B, np.uint32))), outs[1][0], cap, *outs[1][1:], d_rung)
            torch.cuda.synchronize()
            ok = same(*outs[0][:3], want) and same(*outs[1][:3], want_rate) and d_err.cpu().numpy().tolist() == err
            ok = ok and outs[0][3].cpu().numpy().tolist() == status and outs[1][3].cpu().numpy().tolist() == status
            ok = ok and (d_bits.cpu().numpy().view(np.uint32) == bits).all() and d_rung.cpu().numpy().view(np.uint32).tolist() == want_rungs
            if not ok:
                bad += 1
                print("MISMATCH requant seed", seed, w, h, n, "lambda", lam, "ladder", ladder, "budgets", B, "status", status, "mode", mode, flush=True)
        ctx.set_entropy_mode(pkg.ENTROPY_AUTO)
    print("frames", frames_seen, "not coded", not_coded, "of them out of range", out_of_range)
    return bad


def soak_retable(pkg, orc, lo, hi):
    import torch
    import clip_ref as C
    import retable_ref as RT
    import test_gpu_parity as T
    ctx = pkg.Context(0)
    bad = frames_seen = not_coded = bad_index = 0
    for seed in range(lo, hi):
        rng = np.random.default_rng(seed)
        n = int(rng.integers(1, 7))
        count = int(rng.integers(1, 5))
        table_of = [int(rng.integers(0, count)) for _ in range(n)]
        if seed % 3:                                                        # the reference's encoder, a qscale per table
            w, h = 16 * int(rng.integers(1, 4)), 16 * int(rng.integers(1, 3))
            qscales = [int(rng.integers(1, 32)) for _ in range(count)]
            tables = [RT.reference_tables(q) for q in qscales]
            frames = RT.N.stream(w, h, [str(rng.choice(["ramp", "texture", "noise", "flat"])) for _ in range(n)], 5000 + seed)
            chunks = [RT.reference_chunks([frames[i]], w, h, qscales[table_of[i]])[0] for i in range(n)]
        else:                                                               # the oracle's chunks read against seeded tables
            w, h = int(rng.integers(1, 60)), int(rng.integers(1, 50))
            tables = [[[int(x) for x in rng.integers(1, 41, 64)] for _ in range(2)] for _ in range(count)]
            chunks = RT.Q.synth_chunks(w + (w & 1), h + (h & 1), n, seed=SEED + seed)
        for i in range(n):
            if rng.integers(0, 5) == 0:
                chunks[i] = chunks[i][: int(rng.integers(2, len(chunks[i])))]
        if seed % 4 == 0:
            table_of[int(rng.integers(0, n))] = count + int(rng.integers(0, 200))
        d_table_of = None if count == 1 and seed % 4 else T._t(np.array(table_of, np.uint8))
        if d_table_of is None:
            table_of = None
        lam = int(rng.choice([0, 200, 3481, 20000, RT.LAMBDA_MAX, int(rng.integers(0, RT.LAMBDA_MAX + 1))]))
        rungs = int(rng.integers(1, 6))
        ladder = sorted(int(rng.choice([0, 1000, 3481, 20000, RT.LAMBDA_MAX, int(rng.integers(0, 60000))])) for _ in range(rungs))
        want, status, err = RT.retable(chunks, w, h, tables, table_of, lam)
        bits = RT.bits_table(chunks, w, h, tables, table_of, ladder)
        lens, coded = RT.clip_lens(chunks, w, h, tables, table_of, ladder)
        B = [max(0, int(rng.choice([lens[i][int(rng.integers(0, rungs))], lens[i][int(rng.integers(0, rungs))] - 1, 7, 0xFFFFFFFF]))) for i in range(n)]
        want_rate, _, want_rungs = RT.rate(chunks, w, h, tables, table_of, ladder, B)
        S = C.sums(lens, B, coded)
        total = max(0, int(rng.choice(S)) - int(rng.integers(0, 2)))
        want_clip = RT.clip(chunks, w, h, tables, table_of, ladder, B, total)
        frames_seen += n
        not_coded += sum(1 for x in status if x)
        bad_index += sum(1 for x in status if x == RT.ST_TABLE)
        blob, offs, lens_in = RT.Q.pack(chunks)
        ins = (T._t(blob), int(lens_in.sum()), T._t(offs), T._t(lens_in), n, w, h)
        cap = 4 * sum(len(c) for c in chunks) + 64 * n + 64

        def same(d_blob, d_offs, d_lens, chunks_want):
            got, o, ln = d_blob.cpu().numpy(), d_offs.cpu().numpy(), d_lens.cpu().numpy()
            pos = 0
            for i, c in enumerate(chunks_want):
                size = len(c) if c else 0
                if (int(o[i]), int(ln[i])) != (pos, size) or (size and got[pos: pos + size].tobytes() != c):
                    return False
                pos += size
            return True

        for mode in (pkg.ENTROPY_AUTO, pkg.ENTROPY_SERIAL):
            ctx.set_entropy_mode(mode)
            outs = [(torch.zeros(cap, dtype=torch.uint8, device="cuda:0"), torch.zeros(n, dtype=torch.int64, device="cuda:0"),
                     torch.zeros(n, dtype=torch.int32, device="cuda:0"), torch.full((n,), -1, dtype=torch.int32, device="cuda:0")) for _ in range(3)]
            d_err = torch.full((n, 3), -1, dtype=torch.int64, device="cuda:0")
            d_bits = torch.full((n, rungs), -1, dtype=torch.int32, device="cuda:0")
            d_rung = [torch.full((n,), -1, dtype=torch.int32, device="cuda:0") for _ in range(2)]
            d_clip = torch.full((2,), -1, dtype=torch.int64, device="cuda:0")
            rt = pkg.Retable(tables, d_table_of)
            rate = pkg.Rate(ladder, budget=1, d_budget=T._t(np.array(B, np.uint32)))
            ctx.retable_stream_dev(*ins, rt, lam, outs[0][0], cap, *outs[0][1:], d_err)
            ctx.retable_rate_probe_dev(*ins, rt, ladder, d_bits)
            ctx.retable_rate_stream_dev(*ins, rt, rate, outs[1][0], cap, *outs[1][1:], d_rung[0])
            ctx.retable_clip_stream_dev(*ins, rt, rate, total, outs[2][0], cap, *outs[2][1:], d_rung[1], d_clip)
            torch.cuda.synchronize()
            ok = same(*outs[0][:3], want) and same(*outs[1][:3], want_rate) and same(*outs[2][:3], want_clip[0]) and d_err.cpu().numpy().tolist() == err
            ok = ok and all(o[3].cpu().numpy().tolist() == status for o in outs)
            ok = ok and (d_bits.cpu().numpy().view(np.uint32) == bits).all() and d_rung[0].cpu().numpy().view(np.uint32).tolist() == want_rungs
            ok = ok and d_rung[1].cpu().numpy().view(np.uint32).tolist() == want_clip[2] and d_clip.cpu().numpy().view(np.uint64).tolist() == list(want_clip[3])
            if not ok:
                bad += 1
                print("MISMATCH retable seed", seed, w, h, n, "tables", count, table_of, "lambda", lam, "ladder", ladder, "budgets", B, "total", total,
                      "status", status, "mode", mode, flush=True)
        ctx.set_entropy_mode(pkg.ENTROPY_AUTO)
    print("frames", frames_seen, "not coded", not_coded, "of them with a bad index", bad_index)
    return bad


def soak_clip(pkg, orc, lo, hi):
    import torch
    import clip_ref as C
    import rate_ref as R
    import requant_ref as Q
    import test_gpu_parity as T
    ctx = pkg.Context(0)
    bad = frames_seen = bumps = flagged = passes_most = 0
    for seed in range(lo, hi):
        rng = np.random.default_rng(seed)
        w, h = 2 * int(rng.integers(4, 60)), 2 * int(rng.integers(4, 50))
        blocks = 6 * ((w + 15) // 16) * ((h + 15) // 16)
        n = max(1, min(int(rng.integers(1, 7)), 600 // blocks))
        qbias = int(rng.choice([0, 128, int(rng.integers(0, 256))]))
        rungs = int(rng.integers(1, 7))
        pool = [0, 400, 3481, 20000, R.T.LAMBDA_MAX, int(rng.integers(0, R.T.LAMBDA_MAX + 1)), int(rng.integers(0, 30000))]
        ladder = [int(rng.choice(pool)) for _ in range(rungs)]
        if seed & 1:
            ladder.sort()
        nr = int(rng.integers(1, ctx.encode_nr_max(w, h) + 1)) if seed % 3 == 0 else 0
        state = None
        if nr:
            count = int(rng.integers(1, 65000))
            state = np.concatenate([rng.integers(0, 200, 64) * count, [count]]).astype(np.int64)
        frames = R.N.stream(w, h, [R.KINDS[int(rng.integers(0, 4))] for _ in range(n)], 1000 + seed)
        requant_source = seed % 5 == 4                                   # every fifth seed: chunks in, some of them damaged
        if requant_source:
            chunks = Q.synth_chunks(w, h, n, seed=SEED + seed, qbias=int(rng.choice([0, 128])))
            for i in range(n):
                if rng.integers(0, 4) == 0:
                    chunks[i] = chunks[i][: int(rng.integers(2, len(chunks[i])))]
            lens, coded = C.requant_lens(chunks, w, h, ladder)
            bits = Q.bits_table(chunks, w, h, ladder)
        else:
            bits = R.bits_table(frames, w, h, qbias, nr, state, ladder)
            lens, coded = R.lens_table(frames, w, h, qbias, nr, state, ladder), None
        B = []
        for i in range(n):
            r = int(rng.integers(0, rungs))
            B.append(max(0, int(rng.choice([lens[i][r], lens[i][r] - 1, R.floor_bytes(int(bits[i][r])), 7, 0xFFFFFFFF, 0xFFFFFFFF,
                                            int(rng.integers(0, int(lens[i].max()) + 2))]))))
        uniform = seed % 4 == 3
        if uniform:
            B = [B[0]] * n
        S, F = C.sums(lens, B, coded), C.floor_sums(bits, B, coded)
        totals = [x + d for x in S + F for d in (-1, 0, 1)] + [0, C.U64_MAX, int(rng.integers(0, max(S) + 2))]
        total = max(0, totals[int(rng.integers(0, len(totals)))])        # (picked by index: 2^64 - 1 is no numpy integer)
        walk = C.device_walk(bits, lens, B, total, coded)
        frames_seen += n
        bumps += len(walk[6]) - 1
        flagged += int(walk[1])
        passes_most = max(passes_most, walk[4])
        cap = ctx.encode_bound(w, h) * n
        d_budget = None if uniform else T._t(np.array(B, np.uint32))      # (kept alive here: the Rate holds the address alone)
        rate = pkg.Rate(ladder, budget=B[0], d_budget=d_budget)
        if requant_source:
            want, status, want_rungs, want_clip = C.requant(chunks, w, h, ladder, B, total)
            blob, offs, in_lens = Q.pack(chunks)
            ins = (T._t(blob), int(in_lens.sum()), T._t(offs), T._t(in_lens), n, w, h)
        else:
            want, want_rungs, want_clip, want_state = C.encode(frames, w, h, qbias, nr, state, ladder, B, total)
            n_pad = 8
            Y = np.full((n, h, w + n_pad), 0xEE, np.uint8)
            Cb, Cr = np.full((n, h // 2, w // 2 + n_pad), 0xEE, np.uint8), np.full((n, h // 2, w // 2 + n_pad), 0xEE, np.uint8)
            for i, (y, cb, cr) in enumerate(frames):
                Y[i, :, :w], Cb[i, :, :w // 2], Cr[i, :, :w // 2] = y, cb, cr
            planes = (T._t(Y), T._t(Cb), T._t(Cr), w + n_pad, w // 2 + n_pad, h * (w + n_pad), (h // 2) * (w // 2 + n_pad), n, w, h)
        for mode in (pkg.ENTROPY_AUTO, pkg.ENTROPY_SERIAL):
            ctx.set_entropy_mode(mode)
            d_blob = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
            d_offs = torch.zeros(n, dtype=torch.int64, device="cuda:0")
            d_lens = torch.zeros(n, dtype=torch.int32, device="cuda:0")
            d_rung = torch.zeros(n, dtype=torch.int32, device="cuda:0")
            d_clip = torch.full((2,), -1, dtype=torch.int64, device="cuda:0")
            if requant_source:
                d_status = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
                ctx.requant_clip_stream_dev(*ins, rate, total, d_blob, cap, d_offs, d_lens, d_status, d_rung, d_clip)
            else:
                d_state = None if state is None else T._t(state.astype(np.int32))
                ctx.encode_yuv420_clip_stream_dev(*planes, pkg.Quant(qbias, nr, 1, 0, d_state), rate, total, d_blob, cap, d_offs, d_lens, d_rung,
                                                  d_clip)
            torch.cuda.synchronize()
            blob_got, offs_got, got_lens = d_blob.cpu().numpy(), d_offs.cpu().numpy(), d_lens.cpu().numpy()
            ok = d_rung.cpu().numpy().view(np.uint32).tolist() == want_rungs
            ok = ok and [int(x) for x in d_clip.cpu().numpy().view(np.uint64)] == list(want_clip)
            ok = ok and (walk[0] | (R.OVER if walk[1] else 0), walk[2]) == tuple(want_clip) and walk[3] == want_rungs
            if requant_source:
                ok = ok and d_status.cpu().numpy().tolist() == status
            else:
                ok = ok and (state is None or (d_state.cpu().numpy() == want_state).all())
            pos = 0
            for i, c in enumerate(want):
                size = len(c) if c else 0
                ok = ok and (int(offs_got[i]), int(got_lens[i])) == (pos, size) and (not size or blob_got[pos: pos + size].tobytes() == c)
                pos += size
            if not ok:
                bad += 1
                print("MISMATCH clip seed", seed, w, h, n, "requant" if requant_source else "encode", "qbias", qbias, "nr", nr, "ladder", ladder,
                      "budgets", B, "uniform", uniform, "total", total, "mode", mode, flush=True)
        ctx.set_entropy_mode(pkg.ENTROPY_AUTO)
    print("frames", frames_seen, "moves of the clip", bumps, "clips over every rung", flagged, "the most passes of a call", passes_most)
    return bad


def main():
    if len(sys.argv) != 4 or sys.argv[1] not in ("adpcm", "decode", "ffmpeg", "encode", "trellis", "qns", "rate", "requant", "retable", "clip"):
        raise SystemExit(__doc__)
    what, lo, hi = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    pkg = entry.build()
    orc = entry.load_oracle()
    orc.lib()
    bad = {"adpcm": soak_adpcm, "decode": soak_decode, "ffmpeg": soak_ffmpeg, "encode": soak_encode, "trellis": soak_trellis,
           "qns": soak_qns, "rate": soak_rate, "requant": soak_requant, "retable": soak_retable, "clip": soak_clip}[what](pkg, orc, lo, hi)
    print("soak", what, "seeds", lo, "..", hi - 1, "mismatches:", bad)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
