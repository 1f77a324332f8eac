"""The reconstruction kernels on crafted coefficient blocks (tests/coef_builder.py), against the oracle, on a real MI355X.

Every frame of the builder's corpus -- one coefficient at every scan position, every shape the reference's IDCT
shortcuts look for, outputs on each side of the iclp clamp, every colour channel on each side of its clamps, full blocks
of +-1023 under the ends of int16, the int16 wraps of the FFmpeg mode, nmcu_ok at every place of a segment, widths and
heights that end inside an MCU -- sits between ordinary frames in one batch per geometry, in an output buffer filled
with a pattern, so that a store outside a frame's rows shows in its neighbours.

Dense form (amvhip_reconstruct_dev; both zig-zag tables and FFmpeg-compat; the launch whole and in parts of 3 frames):
every byte of every frame is the builder's picture for every case inside what include/amvhip.h promises -- all of D
(what a scan can carry), and E up to |AC * step| <= 100 000 -- and in FFmpeg-compat for every case.  For the E cases
beyond the bound in the amvlib modes the header promises only that the frame is written and nothing else is: the
frame's bytes do not depend on what the buffer held, its row padding is zero, and its neighbours are exact.

Records form (amvhip_decode_batch_dev, a default context and AMVHIP_ENTROPY_SERIAL): every D case a scan can carry, as
the chunk scan_builder writes for it -- the same bytes.

A failure names the case, the mode and the first differing byte.  What the E cases beyond the bound gave on the
MI355X is in DESIGN.md ("What the stage accessor promises").
"""
import numpy as np
import pytest

import coef_builder as cb
import scan_builder as sb
from test_gpu_parity import _blob_of, _t

pytestmark = pytest.mark.gpu

MODES = ("amvlib", "zigzag_fixed", "ffmpeg")


@pytest.fixture(scope="module")
def batches(orc):
    cases, _ = cb.corpus(orc)
    out = cb.batches(cases)
    for b in out:
        w, h = b["w"], b["h"]
        frames = list(zip(b["coef"], b["nmcu_ok"]))
        b["want"] = {"amvlib": np.stack([cb.picture(orc, c, w, h, int(ok), 0) for c, ok in frames]),
                     "zigzag_fixed": np.stack([cb.picture(orc, c, w, h, int(ok), 1) for c, ok in frames]),
                     "ffmpeg": np.stack([cb.picture_ffmpeg(orc, c, w, h, int(ok)) for c, ok in frames])}
        b["name"] = {i: c.name for i, c in zip(b["where"], b["cases"])}
        b["case"] = {i: c for i, c in zip(b["where"], b["cases"])}
    return out


def _flags(pkg, mode):
    return {"amvlib": 0, "zigzag_fixed": pkg.FLAG_ZIGZAG_FIXED, "ffmpeg": pkg.FLAG_FFMPEG}[mode]


def _first_difference(b, mode, i, got, want):
    """the case's name (or the neighbour's place), the mode and the first differing byte, as a pixel where there is one"""
    at = int(np.flatnonzero(got.reshape(-1) != want.reshape(-1))[0])
    name = b["name"].get(i, "ordinary frame #%d (beside %s)" % (i, b["name"].get(i - 1, b["name"].get(i + 1))))
    if mode == "ffmpeg":
        where = "byte %d of the planes" % at
    else:
        row, col = divmod(at, got.shape[-1])
        where = "stored row %d (picture row %d), pixel %d, channel %s" % (row, b["h"] - 1 - row, col // 3, "BGR"[col % 3]) \
            if col < b["w"] * 3 else "stored row %d, padding byte %d" % (row, col - b["w"] * 3)
    return "%s [%dx%d] mode %s: %s: got %d, want %d" % (name, b["w"], b["h"], mode, where, got.reshape(-1)[at], want.reshape(-1)[at])


def _check(b, mode, got, promised):
    want = b["want"][mode]
    for i in range(len(want)):
        if promised(i) and not (got[i] == want[i]).all():
            pytest.fail(_first_difference(b, mode, i, got[i], want[i]))


def _reconstruct(ctx, pkg, b, mode, fill):
    import torch
    n, w, h = len(b["coef"]), b["w"], b["h"]
    shape = (n, ctx.yuv420_frame_bytes(w, h)) if mode == "ffmpeg" else (n, h, ctx.stride(w))
    assert shape[1:] == b["want"][mode].shape[1:]
    d_out = torch.full(shape, fill, dtype=torch.uint8, device="cuda:0")
    ctx.reconstruct_dev(_t(b["coef"]), _t(b["nmcu_ok"]), n, w, h, _flags(pkg, mode), d_out)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


@pytest.mark.parametrize("most", [None, "3"])
@pytest.mark.parametrize("mode", MODES)
def test_crafted_coefficients_dense_form(ctx, pkg, batches, monkeypatch, mode, most):
    if most:
        monkeypatch.setenv("AMVHIP_RECON_MOST", most)       # (read at every launch)
    else:
        monkeypatch.delenv("AMVHIP_RECON_MOST", raising=False)
    beyond = {}
    for b in batches:
        got = _reconstruct(ctx, pkg, b, mode, 0x5A)
        outside = lambda i: mode != "ffmpeg" and i in b["case"] and not b["case"][i].in_bound
        _check(b, mode, got, lambda i: not outside(i))
        loose = [i for i in range(len(got)) if outside(i)]
        if loose:
            # beyond the bound: every byte of the frame is written (the same bytes over another fill), the padding is the
            # oracle's zeros, and -- checked above -- the frames on both sides are exact
            again = _reconstruct(ctx, pkg, b, mode, 0xA5)
            for i in loose:
                name = b["name"][i]
                assert (got[i] == again[i]).all(), "%s mode %s: bytes of the frame depend on what the buffer held" % (name, mode)
                assert (got[i][:, b["w"] * 3:] == 0).all(), "%s mode %s: row padding written" % (name, mode)
                diff = (got[i] != b["want"][mode][i])[:, : b["w"] * 3].reshape(b["h"], b["w"], 3).any(2)
                # (which 8x8 luma blocks or 16x16 chroma areas: counted per MCU)
                mcus = {(r // 16, c // 16) for r, c in zip(*np.nonzero(diff[::-1]))}
                case = b["case"][i]
                far = (np.abs(case.coef.astype(np.int64)) * cb.steps_of(len(case.coef)))[:, 1:].max(1) > cb.AC_BOUND
                mcw = (b["w"] + 15) // 16
                assert mcus <= {divmod(int(m), mcw) for m in np.nonzero(far)[0] // 6}, \
                    "%s mode %s: pixels differ in an MCU all of whose blocks are inside the bound" % (name, mode)
                beyond[name] = (int(diff.sum()), len(mcus))
    print("E cases beyond the bound, mode %s, most %s: {case: (pixels, MCUs) that differ from the reference}: %s" % (mode, most, beyond))


@pytest.mark.parametrize("entropy", ["auto", "serial"])
def test_crafted_coefficients_records_form(ctx, pkg, orc, batches, entropy):
    import torch
    ctx.set_entropy_mode(pkg.ENTROPY_SERIAL if entropy == "serial" else pkg.ENTROPY_AUTO)
    try:
        ran = 0
        for b in batches:
            w, h = b["w"], b["h"]
            # the cases a scan can carry, each still between two ordinary frames
            keep = [i for i in range(len(b["coef"])) if i not in b["case"] or not b["case"][i].dense_only]
            keep = [i for i in keep if i in b["case"] or (i - 1 in keep or i + 1 in keep)]
            if not any(i in b["case"] for i in keep):
                continue
            chunks = [b["case"][i].chunk() if i in b["case"] else
                      sb.assemble(sb.blocks_from_coefficients(b["coef"][i])).chunk for i in keep]
            sub = {"w": w, "h": h, "want": {m: v[keep] for m, v in b["want"].items()},
                   "name": {k: b["name"][i] for k, i in enumerate(keep) if i in b["name"]}}
            blob, offs, lens, nbytes = _blob_of(chunks, pad_front=1)
            n = len(chunks)
            for mode in MODES:
                shape = (n, ctx.yuv420_frame_bytes(w, h)) if mode == "ffmpeg" else (n, h, ctx.stride(w))
                d_out = torch.full(shape, 0x5A, dtype=torch.uint8, device="cuda:0")
                d_st = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
                ctx.decode_batch_dev(_t(blob), nbytes, _t(offs), _t(lens), n, w, h, _flags(pkg, mode), d_out, d_st,
                                     torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                st = d_st.cpu().numpy()
                assert (st == 0).all(), (entropy, mode, [sub["name"].get(int(k), k) for k in np.nonzero(st)[0]])
                _check(sub, mode, d_out.cpu().numpy(), lambda i: True)
            ran += sum(i in b["case"] for i in keep)
        assert ran >= 25, ran
    finally:
        ctx.set_entropy_mode(pkg.ENTROPY_AUTO)
