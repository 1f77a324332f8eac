"""pixfmt_builder.py without a GPU: the searches find what the module's docstring says they find (and why the rest cannot
be found), and the pictures built from them do in img_convert_ref what they were sought for."""
import numpy as np

import img_convert_ref as R
import pixfmt_builder as B


def test_rgb_in_thresholds_met():
    met_all = 0
    for src, dst in B.RGB_IN_PAIRS:
        patches, met = B.rgb_in_patches(dst)
        want = {"y1023", "y0", "u4095+", "u4095-", "v4095+", "v4095-", "v0+", "v0-"} | ({"u0+", "u0-"} if dst == R.YUVJ420P else set())
        assert set(met) == want, (R.NAMES[src], R.NAMES[dst])
        met_all += len(met)
        # the eight corners are there, and patches of four different pixels
        colours = {tuple(p) for q in patches.tolist() for p in q}
        assert set(B.CORNERS) <= colours
        assert sum(len({tuple(p) for p in q}) == 4 for q in patches.tolist()) >= 8
    assert (B.RGB_IN_THRESHOLDS, met_all) == (40, B.RGB_IN_THRESHOLDS_MET) == (40, 34)
    # why six cannot be met: towards YUV420P every Cb weight is even, the rounding term odd
    _, _, wu, _ = B.rgb_in_weights(R.YUV420P)
    assert wu == (-152, -298, 450) and all(w % 2 == 0 for w in wu) and ((R.ONE_HALF << 2) - 1) % 2 == 1


def test_rgb_in_pictures_sit_on_the_steps():
    """through img_convert_ref itself: raising one channel of the pixel found by one step moves the luma where the numerator
    was 1023 mod 1024, lowering it moves the luma where it was 0; the chroma of a found patch is the floor of a negative
    quotient (an arithmetic shift), not its truncation"""
    for src, dst in B.RGB_IN_PAIRS:
        patches, _ = B.rgb_in_patches(dst)
        yn, un, vn = B.rgb_in_numerators(dst, patches)
        for w in (32, 22):
            planes, h = B.rgb_picture(src, patches, w)
            y, cb, cr = R.convert(src, planes, dst, w, h)
            per_row = w // 2
            for k in range(len(patches)):
                r0, c0 = 2 * (k // per_row), 2 * (k % per_row)
                assert y[r0:r0 + 2, c0:c0 + 2].reshape(-1).tolist() == (yn[k] >> 10).tolist()
                assert cb[r0 // 2, c0 // 2] == (un[k] >> 12) + 128 and cr[r0 // 2, c0 // 2] == (vn[k] >> 12) + 128
        neg = (un < 0) & (un % 4096 != 0)
        assert neg.any() and ((un[neg] >> 12) != -((-un[neg]) >> 12)).all()


def test_rgb_out_thresholds_met():
    steps = values = colours = 0
    for src in B.RGB_OUT_SOURCES:
        triples, met = B.rgb_out_triples(src)
        steps += len(met["steps"])
        values += met["values"]
        colours += len(met["colours"])
        for ch in "rgb":
            for name in ("=-1", "=0", "=255", "=256", "<-100", ">355", "neg%0"):
                if (src, ch, name) != (R.YUVJ420P, "b", "neg%0"):
                    assert ch + name in met["steps"], (R.NAMES[src], ch, name)
        assert "gneg%1023" in met["steps"]
        assert {"r=0", "g=0", "b=0", "g=255"} <= set(met["colours"])
    assert B.RGB_OUT_THRESHOLDS == {"steps": 48, "values": 1536, "colours": 12}
    assert {"steps": steps, "values": values, "colours": colours} == B.RGB_OUT_THRESHOLDS_MET == {"steps": 43, "values": 1536, "colours": 10}
    # why the rest cannot be: even numerators from YUV420P, a multiple of four for r from YUVJ420P
    F = R.FIX
    assert [F(255.0 / 219.0), F(1.402 * 255.0 / 224.0), F(1.772 * 255.0 / 224.0)] == [1192, 1634, 2066] and F(1.402) % 4 == 0


def test_rgb_out_pictures_reach_every_value_and_every_dropped_bit():
    for src in B.RGB_OUT_SOURCES:
        triples, met = B.rgb_out_triples(src)
        for w in (32, 22):
            planes, h = B.yuv_picture(triples, w)
            rgb = R.convert(src, planes, R.RGB24, w, h)[0].reshape(h, w, 3)
            for ch in range(3):
                assert set(rgb[:, :, ch].reshape(-1).tolist()) == set(range(256)), (R.NAMES[src], ch)
            seen = {tuple(p) for p in rgb.reshape(-1, 3).tolist()}
            for name in met["colours"]:
                ch, hi = "rgb".index(name[0]), int(name[2:])
                assert tuple(hi if k == ch else 255 - hi for k in range(3)) in seen
            # both sides of every boundary of the bits RGB565 / RGB555 drop: all 32 (64) codes of every field appear
            for dst, gbits in ((R.RGB565, 6), (R.RGB555, 5)):
                q = R.convert(src, planes, dst, w, h)[0].reshape(h, w, 2).astype(np.int32)
                v = q[:, :, 0] | (q[:, :, 1] << 8)
                assert set((v & 31).reshape(-1).tolist()) == set(range(32))
                assert set(((v >> 5) & ((1 << gbits) - 1)).reshape(-1).tolist()) == set(range(1 << gbits))
                assert set((v >> (5 + gbits)).reshape(-1).tolist()) == set(range(32))


def test_value_and_shrink_pictures():
    for src in R.PLANAR:
        for w, h in ((32, 32), (14, 74)):
            pic = B.value_picture(src, w, h)
            assert [p.shape for p in pic] == R.plane_shapes(src, w, h)
            for dst in (R.YUV420P, R.YUVJ420P):
                if dst == src:
                    continue
                out = R.convert(src, pic, dst, w, h)
                ranged = (src in R.JPEG) != (dst in R.JPEG)
                tabs = (("y_jpeg_to_ccir", "c_jpeg_to_ccir") if src in R.JPEG else ("y_ccir_to_jpeg", "c_ccir_to_jpeg")) if ranged else None
                for p, plane in enumerate(out):                 # every entry of the plane's table (or every value) comes out
                    want = set(R.TABLES[tabs[min(p, 1)]].tolist()) if ranged else set(range(256))
                    assert set(plane.reshape(-1).tolist()) == want, (R.NAMES[src], R.NAMES[dst], p)
    sums = sorted({a + b for a, b in B.SHRINK12_PAIRS})
    assert {0, 1, 2, 509, 510} <= set(sums)
    sums = {sum(q) for q in B.SHRINK22_QUADS}
    assert {0, 1, 2, 3, 1017, 1018, 1019, 1020} <= sums and {s % 4 for s in sums if 500 < s < 520} == {0, 1, 2, 3}
    for src in R.P422 + R.P444:
        for w in (32, 14):
            pic = B.shrink_picture(src, w)
            assert [p.shape for p in pic] == R.plane_shapes(src, w, 2)
            R.convert(src, pic, R.YUV420P, w, 2)
