"""The video encoder kernels on crafted pictures (tests/pixel_builder.py), against the oracle, on a real MI355X.

Every frame of the builder's corpus -- every AC symbol and DC difference 8-bit samples reach, zero runs to 62, blocks of
63 coefficients, segments of 60 / 64 / 65 symbols, lanes that start inside a block, runs of 256 and 257 bits, DC steps at
every segment's first MCU, windows that flush with 0 .. 7 bits carried over, rounds that do not fit, FF bytes at every
place of a word and of a flush tile, every tail length, the transform's largest outputs, the quantiser's thresholds from
both sides, RGB sums on both sides of a rounding step, sizes that end inside an MCU -- sits between ordinary frames in
one batch per geometry and kind, its rows padded with a poison byte, in a blob filled with a pattern.

Chunks: planes through amvhip_encode_yuv420_batch_dev, pixels through amvhip_encode_batch_dev, under AMVHIP_ENTROPY_AUTO
(the one-kernel coder, hand-backs to the one-lane route) and AMVHIP_ENTROPY_SERIAL (the one-lane route alone), qbias 0
and 128: offsets, lengths and every byte are the oracle's, and the blob behind the last chunk is untouched.  A failure
names the case, the mode and the first difference as (MCU, block, symbol), and says whether the coefficients (the front
half) or only their coding differ.  Coefficients: amvhip_encode_coefs_dev of the pixels is the oracle's want_coef.  The
chunks decode on the GPU to the oracle decoder's pictures.
"""
import numpy as np
import pytest

import pixel_builder as pb
from test_gpu_parity import _gpu_decode, _t

pytestmark = pytest.mark.gpu

FILL = 0xA5


@pytest.fixture(scope="module")
def corpus(orc):
    cases, _ = pb.corpus(orc)
    bs = pb.batches(orc, cases)
    for b in bs:
        b["want"] = {q: [f.chunk(orc, q) for f in b["frames"]] for q in (0, 128)}
        b["lines"] = {q: [f.lines(orc, q) for f in b["frames"]] for q in (0, 128)}
    return bs


def _describe(orc, b, i, mode, got, want, lines):
    """the case (or the neighbour's place), the mode, the first differing byte as (MCU, block, symbol), and which half"""
    f = b["frames"][i]
    name = f.name if f.group else "%s (beside %s)" % (f.name, b["frames"][i - 1 if i else 1].name)
    at = next((k for k in range(min(len(got), len(want))) if got[k] != want[k]), min(len(got), len(want)))
    mine, st = orc.entropy_blocks(got, len(lines)) if len(got) >= 4 else (lines[:0], 1)
    bad = next((k for k in range(len(lines)) if k >= len(mine) or (mine[k] != lines[k]).any()), None)
    if bad is None:
        where = "every coefficient decodes as the oracle's: the coder's stuffing, padding or trailer"
    else:
        sym = "none decoded"
        if bad < len(mine):
            k = int(np.flatnonzero(mine[bad] != lines[bad])[0])
            sym = "%d (coefficient %d: got %d, want %d)" % (0 if k == 0 else 1 + int((lines[bad][1:k] != 0).sum()), k, mine[bad][k], lines[bad][k])
        where = "MCU %d, block %d, symbol %s -- the front half or the coder: see the coefficients test" % (bad // 6, bad % 6, sym)
    return "%s [%dx%d %s] %s: chunk byte %d of %d (got %d bytes): %s" % (name, b["w"], b["h"], b["kind"], mode, at, len(want), len(got), where)


def _encode(ctx, b, qbias, form):
    """-> (blob, offs, lens, cap) of the batch through the entry `form` takes"""
    import torch
    n, w, h = b["n"], b["w"], b["h"]
    cap = sum(len(c) for c in b["want"][qbias]) + 4099
    d_blob = torch.full((cap,), FILL, dtype=torch.uint8, device="cuda:0")
    d_offs = torch.full((n,), -1, dtype=torch.int64, device="cuda:0")
    d_lens = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    if form == "planes":
        Y, Cb, Cr = b["planes"]
        ctx.encode_yuv420_batch_dev(_t(Y), _t(Cb), _t(Cr), b["ys"], b["cs"], h * b["ys"], (h // 2) * b["cs"], n, w, h, qbias, d_blob, cap, d_offs, d_lens)
    else:
        ctx.encode_batch_dev(_t(b["pix"]), b["stride"], 1 if b["kind"] == "bgr" else 0, n, w, h, qbias, d_blob, cap, d_offs, d_lens)
    torch.cuda.synchronize()
    return d_blob.cpu().numpy(), d_offs.cpu().numpy(), d_lens.cpu().numpy(), cap


def _check(orc, b, qbias, mode, blob, offs, lens):
    want = b["want"][qbias]
    pos, bad = 0, []
    for i, w in enumerate(want):
        o, l = int(offs[i]), int(lens[i])
        got = blob[o: o + max(l, 0)].tobytes() if 0 <= o <= len(blob) else b""
        if (o, l) != (pos, len(w)) or got != w:
            # (a wrong length moves every later offset: the chunk is read where it should be)
            bad.append((i, pos, o, l))
        pos += len(w)
    if bad:
        i, at, o, l = bad[0]
        w = want[i]
        pytest.fail(_describe(orc, b, i, mode, blob[at: at + (l if l > 0 else len(w))].tobytes(), w, b["lines"][qbias][i])
                    + "; offset %d (want %d), length %d (want %d); %d of the batch's %d frames differ, the cases among them: %s" % (
                        o, at, l, len(w), len(bad), b["n"], [b["frames"][k].name for k, _, _, _ in bad if b["frames"][k].group][:8]))
    assert (blob[pos:] == FILL).all(), "%dx%d %s %s: byte %d behind the last chunk written" % (
        b["w"], b["h"], b["kind"], mode, pos + int(np.flatnonzero(blob[pos:] != FILL)[0]))


def _forms(b):
    return ("planes",) if b["kind"] == "yuv" else ("pix", "planes")


@pytest.mark.parametrize("qbias", [0, 128])
@pytest.mark.parametrize("entropy", ["auto", "serial"])
def test_crafted_pictures_chunks(ctx, pkg, orc, corpus, entropy, qbias):
    ctx.set_entropy_mode(pkg.ENTROPY_SERIAL if entropy == "serial" else pkg.ENTROPY_AUTO)
    try:
        for b in corpus:
            for form in _forms(b):
                blob, offs, lens, _ = _encode(ctx, b, qbias, form)
                _check(orc, b, qbias, "entropy %s, qbias %d, %s" % (entropy, qbias, form), blob, offs, lens)
    finally:
        ctx.set_entropy_mode(pkg.ENTROPY_AUTO)


@pytest.mark.parametrize("qbias", [0, 128])
def test_crafted_pictures_coefficients(ctx, orc, corpus, qbias):
    """the front half alone: the pixels' lines through amvhip_encode_coefs_dev; the planes' lines out of the GPU's chunk"""
    import torch
    for b in corpus:
        n, w, h = b["n"], b["w"], b["h"]
        want = np.stack(b["lines"][qbias])
        if b["kind"] != "yuv":
            d_coef = torch.full(want.shape, 0x5A5A, dtype=torch.int16, device="cuda:0")
            ctx.encode_coefs_dev(_t(b["pix"]), b["stride"], 1 if b["kind"] == "bgr" else 0, n, w, h, qbias, d_coef)
            torch.cuda.synchronize()
            got = d_coef.cpu().numpy()
        else:
            blob, offs, lens, _ = _encode(ctx, b, qbias, "planes")
            got = np.full(want.shape, 0x5A5A, np.int16)
            for i in range(n):
                mine, st = orc.entropy_blocks(blob[int(offs[i]): int(offs[i]) + int(lens[i])].tobytes(), want.shape[1])
                got[i, : len(mine)] = mine
        if not (got == want).all():
            i, blk, k = (int(x) for x in np.argwhere(got != want)[0])
            which = "the front half (amvhip_encode_coefs_dev)" if b["kind"] != "yuv" else \
                "the GPU chunk's coefficients (the front half where the pixel cases of this test pass, else the coder)"
            pytest.fail("%s [%dx%d %s] qbias %d: %s: MCU %d, block %d, coefficient %d: got %d, want %d" % (
                b["frames"][i].name, w, h, b["kind"], qbias, which, blk // 6, blk % 6, k, got[i, blk, k], want[i, blk, k]))


def test_crafted_pictures_hand_backs(ctx, orc, corpus):
    """the frames the window cannot hold, among frames it can: the builder's model, fed the oracle's bits per round, says
    at least one frame per sub-case is handed back (after bytes were written; before any); every chunk of those batches
    is the oracle's"""
    for qbias in (0, 128):
        counts = {}
        for b in corpus:
            if not any(c.group == 5 for c in b["cases"]):
                continue
            for f, lines in zip(b["frames"], b["lines"][qbias]):
                m_bits = pb.frame_model(lines, b["w"], b["h"])["round_bits"]
                m = pb.window_walk(m_bits)
                if m["handed_back"] is not None:
                    last = m["handed_back"] == len(m_bits) - 1 > 0 and m["wrote_before"]
                    key = "last" if last else ("first" if m["handed_back"] == 0 else "other")
                    counts[key] = counts.get(key, 0) + 1
                counts["kept"] = counts.get("kept", 0) + (m["handed_back"] is None)
            blob, offs, lens, _ = _encode(ctx, b, qbias, "planes")
            _check(orc, b, qbias, "entropy auto, qbias %d, planes" % qbias, blob, offs, lens)
        print("qbias %d: frames handed back by sub-case, and kept: %s" % (qbias, counts))
        assert counts.get("last", 0) >= 1 and counts.get("first", 0) >= 1 and counts["kept"] >= 1, counts


def test_crafted_pictures_round_trip(ctx, orc, corpus):
    """the GPU's chunks of the crafted pictures decode on the GPU (default flags), status 0, to the oracle decoder's pictures"""
    for b in corpus:
        blob, offs, lens, _ = _encode(ctx, b, 0, "planes")
        chunks = [blob[int(o): int(o) + int(l)].tobytes() for o, l in zip(offs, lens)]
        got, st = _gpu_decode(ctx, chunks, b["w"], b["h"])
        for i, want_chunk in enumerate(b["want"][0]):
            want, want_st, _ = orc.decode_frame(want_chunk, b["w"], b["h"])
            assert want_st == 0 and st[i] == 0, (b["frames"][i].name, int(st[i]))
            assert (got[i] == want).all(), "%s [%dx%d]: the decoded picture differs" % (b["frames"][i].name, b["w"], b["h"])
