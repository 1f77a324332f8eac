"""A literal restatement of the reference's postprocessing (AMVmuxer/ffmpeg/libpostproc: postprocess.c and the C path of
postprocess_template.c) for modes made of H_DEBLOCK, V_DEBLOCK, DERING and FORCE_QUANT, on planes whose pitch is their width.

It walks what postProcess_C walks, in its order: the copyAhead block copy, the first-row prologue through tempDst, the
`y + 15 >= height` detour through tempSrc / tempDst with its line duplication and copy-back, "only deblock if we have 2 blocks",
vertClassify_C / horizClassify_C (with nonBQP = 0: see postprocess_plane), the C low-pass and default filters, the C dering (threshold 20,
QP2 = QP / 2 + 1, in place in raster order) and the dering call behind the x loop whose window hangs over the row's end.
tempSrc and tempDst live in a Context as they live in a PPContext: zeroed when made, kept from plane to plane.

`trace` (a dict) counts the branches taken; `faults` (a set of names out of FAULTS) each break one rule, for tests that show
the fixture can tell.  tests/golden/ref_postprocess.json pins all of it to the real function."""
import numpy as np

V_DEBLOCK, H_DEBLOCK, DERING, FORCE_QUANT = 0x01, 0x02, 0x04, 0x200000
FILTER_BITS = V_DEBLOCK | H_DEBLOCK | DERING
DERING_THRESHOLD = 20
FAULTS = ("dering_window_left", "qp2_no_plus_one", "flatness_ge", "first_last_le", "no_line_duplication", "no_row_end_call", "h_before_v")

# shortName, longName, chromDefault, minLumQuality, minChromQuality, mask (postprocess.c:120-141); None: not built here
_FILTERS = (("hb", "hdeblock", 1, 1, 3, H_DEBLOCK), ("vb", "vdeblock", 1, 2, 4, V_DEBLOCK), ("h1", "x1hdeblock", 1, 1, 3, None),
            ("v1", "x1vdeblock", 1, 2, 4, None), ("ha", "ahdeblock", 1, 1, 3, None), ("va", "avdeblock", 1, 2, 4, None),
            ("dr", "dering", 1, 5, 6, DERING), ("al", "autolevels", 0, 1, 2, None), ("lb", "linblenddeint", 1, 1, 4, None),
            ("li", "linipoldeint", 1, 1, 4, None), ("ci", "cubicipoldeint", 1, 1, 4, None), ("md", "mediandeint", 1, 1, 4, None),
            ("fd", "ffmpegdeint", 1, 1, 4, None), ("l5", "lowpass5", 1, 1, 4, None), ("tn", "tmpnoise", 1, 7, 8, None),
            ("fq", "forcequant", 1, 0, 0, FORCE_QUANT))
_REPLACE = {"default": "hdeblock:a,vdeblock:a,dering:a", "de": "hdeblock:a,vdeblock:a,dering:a"}
_REPLACE_NOT_BUILT = ("fast", "fa", "ac")


def _strtol(s):
    """strtol(s, &tail, 0) -> (value, whether any character was taken)"""
    i, n = 0, len(s)
    while i < n and s[i] in " \t\n\v\f\r":
        i += 1
    sign = 1
    if i < n and s[i] in "+-":
        sign = -1 if s[i] == "-" else 1
        i += 1
    base = 10
    if s[i:i + 2].lower() == "0x" and i + 2 < n and s[i + 2] in "0123456789abcdefABCDEF":
        base, i = 16, i + 2
    elif i < n and s[i] == "0":
        base = 8
    digits = "0123456789abcdef"[:base]
    j = i
    while j < n and s[j].lower() in digits:
        j += 1
    if j == i:
        return 0, False
    return sign * int(s[i:j], base), True


def parse_mode(name, quality):
    """pp_get_mode_by_name_and_quality (postprocess.c:744-934) -> dict(lumMode, chromMode, baseDcDiff, flatnessThreshold,
    forcedQuant), or None where the reference returns NULL or the name asks for a filter that is not built here"""
    if len(name) >= 500:
        return None
    m = {"lumMode": 0, "chromMode": 0, "baseDcDiff": 256 // 8, "flatnessThreshold": 56 - 16 - 1, "forcedQuant": 0}
    error = 0
    queue = [t for t in name.replace("/", ",").split(",") if t]
    budget = 64
    while queue:
        budget -= 1
        if budget < 0:
            return None
        parts = [p for p in queue.pop(0).split(":") if p]
        if not parts:
            return None
        filter_name, q, chrom, luma, enable, options = parts[0], 1000000, -1, -1, 1, []
        if filter_name.startswith("-"):
            enable, filter_name = 0, filter_name[1:]
        for option in parts[1:]:
            if option in ("autoq", "a"):
                q = quality
            elif option in ("nochrom", "y"):
                chrom = 0
            elif option in ("chrom", "c"):
                chrom = 1
            elif option in ("noluma", "n"):
                luma = 0
            else:
                options.append(option)
            if len(options) >= 9:
                break
        unknown = len(options)
        ok = False
        if filter_name in _REPLACE_NOT_BUILT:
            return None
        if filter_name in _REPLACE:
            queue = _REPLACE[filter_name].split(",") + queue
            ok = True
        for short, long_, chrom_default, min_lum, min_chrom, mask in _FILTERS:
            if filter_name not in (short, long_):
                continue
            if mask is None:
                return None
            m["lumMode"] &= ~mask
            m["chromMode"] &= ~mask
            ok = True
            if not enable:
                break
            if q >= min_lum and luma:
                m["lumMode"] |= mask
            if chrom == 1 or (chrom == -1 and chrom_default):
                if q >= min_chrom:
                    m["chromMode"] |= mask
            if mask in (V_DEBLOCK, H_DEBLOCK):
                for o, text in enumerate(options[:2]):
                    val, taken = _strtol(text)
                    if not taken:
                        break
                    unknown -= 1
                    if o == 0:
                        m["baseDcDiff"] = val
                    else:
                        m["flatnessThreshold"] = val
            elif mask == FORCE_QUANT:
                m["forcedQuant"] = 15
                for text in options[:1]:
                    val, taken = _strtol(text)
                    if not taken:
                        break
                    unknown -= 1
                    m["forcedQuant"] = val
        if not ok:
            error += 1
        error += unknown
    if error:
        return None
    if not (m["lumMode"] | m["chromMode"]) & FORCE_QUANT:
        m["forcedQuant"] = 0
    return m


class Context:
    """the two buffers of a PPContext this path uses, av_mallocz'd: 24 lines of the widest pitch"""

    def __init__(self, width):
        stride = (width + 15) & ~15
        self.stride = stride
        self.temp_src = bytearray(stride * 24)
        self.temp_dst = bytearray(stride * 24)


def _count(trace, key):
    if trace is not None:
        trace[key] = trace.get(key, 0) + 1


def _classify(b, o, step, line, c, qp, horiz):
    """vertClassify_C (horiz False: o is the block's line 0, step = the pitch) / horizClassify_C (o is dst[0], line = pitch)"""
    dc_offset = ((c["nonBQP"] * c["baseDcDiff"]) >> 8) + 1
    dc_threshold = dc_offset * 2 + 1
    num_eq = 0
    if horiz:
        for y in range(8):
            p = o + y * line
            for i in range(7):
                if 0 <= b[p + i] - b[p + i + 1] + dc_offset < dc_threshold:
                    num_eq += 1
    else:
        s = o + 4 * step
        for y in range(7):
            p = s + y * step
            for i in range(8):
                if 0 <= b[p + i] - b[p + i + step] + dc_offset < dc_threshold:
                    num_eq += 1
    flat = num_eq >= c["flatnessThreshold"] if "flatness_ge" in c["faults"] else num_eq > c["flatnessThreshold"]
    if not flat:
        return 2

    def bad(a, z):                     # (unsigned)(a - z + 2 * QP) > 4 * QP
        v = a - z + 2 * qp
        return v < 0 or v > 4 * qp
    if horiz:
        p = o
        for _ in range(2):
            if bad(b[p], b[p + 5]):
                return 0
            p += line
            if bad(b[p + 2], b[p + 7]):
                return 0
            p += line
            if bad(b[p + 4], b[p + 1]):
                return 0
            p += line
            if bad(b[p + 6], b[p + 3]):
                return 0
            p += line
    else:
        s = o + 4 * step
        for x in (0, 4):
            if bad(b[s + x], b[s + x + 5 * step]):
                return 0
            if bad(b[s + 1 + x + 2 * step], b[s + 1 + x + 7 * step]):
                return 0
            if bad(b[s + 2 + x + 4 * step], b[s + 2 + x + 1 * step]):
                return 0
            if bad(b[s + 3 + x + 6 * step], b[s + 3 + x + 3 * step]):
                return 0
    return 1


def _low_pass(b, o, step, line, c, qp, trace, tag):
    """doVertLowPass (o = src + stride * 3, step = pitch, line = 1) / doHorizLowPass_C (o = dst - 1, step = 1, line = pitch):
    b[o] is the tap before the eight, b[o + 9 * step] the one behind"""
    le = "first_last_le" in c["faults"]
    for k in range(8):
        p = o + k * line
        v = [b[p + i * step] for i in range(10)]
        d0, d9 = abs(v[0] - v[1]), abs(v[8] - v[9])
        near0 = d0 <= qp if le else d0 < qp
        near9 = d9 <= qp if le else d9 < qp
        first = v[0] if near0 else v[1]
        last = v[9] if near9 else v[8]
        _count(trace, tag + ("_first_near" if near0 else "_first_far"))
        _count(trace, tag + ("_last_near" if near9 else "_last_far"))
        s = [0] * 10
        s[0] = 4 * first + v[1] + v[2] + v[3] + 4
        s[1] = s[0] - first + v[4]
        s[2] = s[1] - first + v[5]
        s[3] = s[2] - first + v[6]
        s[4] = s[3] - first + v[7]
        s[5] = s[4] - v[1] + v[8]
        s[6] = s[5] - v[2] + last
        s[7] = s[6] - v[3] + last
        s[8] = s[7] - v[4] + last
        s[9] = s[8] - v[5] + last
        for i in range(8):
            b[p + (i + 1) * step] = ((s[i] + s[i + 2] + 2 * v[i + 1]) >> 4) & 255
        _count(trace, tag + "_lowpass")


def _def_filter(b, o, step, line, qp, trace, tag):
    """doVertDefFilter (o = src + stride * 3) / doHorizDefFilter_C (o = dst - 1): taps l1 .. l8 = b[o + step .. o + 8 * step]"""
    for k in range(8):
        p = o + k * line
        v = [b[p + i * step] for i in range(9)]
        middle = 5 * (v[5] - v[4]) + 2 * (v[3] - v[6])
        if abs(middle) < 8 * qp:
            q = int((v[4] - v[5]) / 2)                       # C division truncates towards zero
            left = 5 * (v[3] - v[2]) + 2 * (v[1] - v[4])
            right = 5 * (v[7] - v[6]) + 2 * (v[5] - v[8])
            d = max(abs(middle) - min(abs(left), abs(right)), 0)
            d = (5 * d + 32) >> 6
            d *= (1 if -middle > 0 else -1)                   # FFSIGN(a) = a > 0 ? 1 : -1
            if q > 0:
                d = max(d, 0)
                if d > q:
                    d = q
                    _count(trace, tag + "_def_clamped_pos")
            else:
                d = min(d, 0)
                if d < q:
                    d = q
                    _count(trace, tag + "_def_clamped_neg")
            if d:
                _count(trace, tag + "_def_moved")
            b[p + 4 * step] = (v[4] - d) & 255
            b[p + 5 * step] = (v[5] + d) & 255
            _count(trace, tag + "_def_low_energy")
        else:
            _count(trace, tag + "_def_high_energy")


def _dering(b, o, stride, c, qp, trace, tag):
    """dering_C (postprocess_template.c:1412-1543): o is the window's corner"""
    qp2 = qp // 2 if "qp2_no_plus_one" in c["faults"] else qp // 2 + 1
    mn, mx = 255, 0
    for y in range(1, 9):
        row = b[o + stride * y + 1:o + stride * y + 9]
        mx = max(mx, max(row))
        mn = min(mn, min(row))
    avg = (mn + mx + 1) >> 1
    if mx - mn < DERING_THRESHOLD:
        _count(trace, tag + "_dering_flat%d" % (mx - mn) if mx - mn == DERING_THRESHOLD - 1 else tag + "_dering_flat")
        return
    _count(trace, tag + "_dering_range%d" % (mx - mn) if mx - mn == DERING_THRESHOLD else tag + "_dering_ranged")
    s = [0] * 10
    for y in range(10):
        t = 0
        for i in range(10):
            if b[o + stride * y + i] > avg:
                t += 1 << i
        t |= (~t & 0xFFFF) << 16
        t &= (t << 1) & (t >> 1)
        s[y] = t
    for y in range(1, 9):
        t = s[y - 1] & s[y] & s[y + 1]
        t |= t >> 16
        s[y - 1] = t
    for y in range(1, 9):
        t = s[y - 1]
        for x in range(1, 9):
            if t & (1 << x):
                p = o + stride * y + x
                f = (b[p - stride - 1] + 2 * b[p - stride] + b[p - stride + 1] + 2 * b[p - 1] + 4 * b[p] + 2 * b[p + 1]
                     + b[p + stride - 1] + 2 * b[p + stride] + b[p + stride + 1])
                f = (f + 8) >> 4
                if b[p] + qp2 < f:
                    b[p] = (b[p] + qp2) & 255
                    _count(trace, tag + "_dering_plus")
                elif b[p] - qp2 > f:
                    b[p] = (b[p] - qp2) & 255
                    _count(trace, tag + "_dering_minus")
                else:
                    if f != b[p]:
                        _count(trace, tag + "_dering_plain")
                    b[p] = f


def postprocess_plane(src, width, height, mode, qp, base_dc_diff=32, flatness_threshold=39, ctx=None, trace=None, tag="y",
                      faults=(), prefill=0):
    """postProcess_C on one plane of pitch `width` -> a new uint8 [height, width].  mode: V_DEBLOCK | H_DEBLOCK | DERING.

    nonBQP: pp_postprocess (postprocess.c:1052-1106) swaps a forced or absent QP table for its own one-row table with
    QPStride = 0, and then fills nonBQPTable from `mbHeight * QPStride` = 0 entries: the table stays as av_mallocz left it, so
    c.nonBQP is 0 -- not QP & 0x3F -- and dcOffset is 1 whatever the QP and baseDcDiff.  The fixture decides: with QP & 0x3F the
    32x24 luma plane already departs.

    DERING without V_DEBLOCK copies one line ahead only; the row-end window of strip y then reads columns 0, 1 of line y + 9 of
    the destination before anyone has written them (`prefill` here): the result is no function of the picture, and the
    library refuses the mode."""
    assert width % 8 == 0 and width >= 8 and height >= 8 and 0 <= qp <= 63
    src = np.ascontiguousarray(src, np.uint8).reshape(height, width)
    ctx = ctx or Context(width)
    assert ctx.stride >= width
    stride = width
    c = {"baseDcDiff": base_dc_diff, "flatnessThreshold": flatness_threshold, "faults": frozenset(faults), "nonBQP": 0}
    assert c["faults"] <= set(FAULTS)
    # one line in front of each plane: the detour at y = 0 copies the line above the destination (and never uses it)
    S = bytearray(stride) + bytearray(src.tobytes())
    D = bytearray([prefill]) * (stride * (height + 1))
    s0 = d0 = stride
    ts, td = ctx.temp_src, ctx.temp_dst
    if mode & V_DEBLOCK:
        copy_ahead = 13
    elif mode & DERING:
        copy_ahead = 9
    else:
        copy_ahead = 8
    copy_ahead -= 8

    def block_copy(db, do, sb, so):
        for i in range(8):
            db[do + stride * i:do + stride * i + 8] = sb[so + stride * i:so + stride * i + 8]

    # the first row of blocks, through tempDst
    dst_block = stride
    for x in range(0, width, 8):
        block_copy(td, dst_block + stride * 8 + x, S, s0 + x)
        p = dst_block + stride * 8 + x
        for i in range(1, 4):
            td[p - i * stride:p - i * stride + 8] = td[p:p + 8]
    D[d0:d0 + copy_ahead * stride] = td[9 * stride:(9 + copy_ahead) * stride]

    for y in range(0, height, 8):
        sb, so = S, s0 + y * stride
        db, do = D, d0 + y * stride
        detour = y + 15 >= height
        if detour:
            n = max(height - y - copy_ahead, 0)
            ts[stride * copy_ahead:stride * (copy_ahead + n)] = S[so + stride * copy_ahead:so + stride * (copy_ahead + n)]
            if "no_line_duplication" not in c["faults"]:
                for i in range(max(height - y, 8), copy_ahead + 8):
                    ts[stride * i:stride * (i + 1)] = S[s0 + stride * (height - 1):s0 + stride * height]
            n = min(height - y + 1, copy_ahead + 1)
            td[0:n * stride] = D[do - stride:do - stride + n * stride]
            if "no_line_duplication" not in c["faults"]:
                for i in range(height - y + 1, copy_ahead + 1):
                    td[stride * i:stride * (i + 1)] = D[d0 + stride * (height - 1):d0 + stride * height]
            db, do = td, stride
            sb, so = ts, 0

        def vertical(x):
            if y + 8 < height and mode & V_DEBLOCK:
                t = _classify(db, do + x, stride, 1, c, qp, False)
                _count(trace, tag + "_v_class%d" % t)
                if t == 1:
                    _low_pass(db, do + x + stride * 3, stride, 1, c, qp, trace, tag + "_v")
                elif t == 2:
                    _def_filter(db, do + x + stride * 3, stride, 1, qp, trace, tag + "_v")

        def horizontal(x):
            if mode & H_DEBLOCK:
                t = _classify(db, do + x - 4, 1, stride, c, qp, True)
                _count(trace, tag + "_h_class%d" % t)
                if t == 1:
                    _low_pass(db, do + x - 5, 1, stride, c, qp, trace, tag + "_h")
                elif t == 2:
                    _def_filter(db, do + x - 5, 1, stride, qp, trace, tag + "_h")

        shift = 9 if "dering_window_left" in c["faults"] else 8
        for x in range(0, width, 8):
            block_copy(db, do + x + stride * copy_ahead, sb, so + x + stride * copy_ahead)
            if "h_before_v" in c["faults"]:
                if x - 8 >= 0:
                    horizontal(x)
                vertical(x)
            else:
                vertical(x)
                if x - 8 >= 0:
                    horizontal(x)
            if x - 8 >= 0 and mode & DERING and y > 0:
                _dering(db, do + x - stride - shift, stride, c, qp, trace, tag)
        if mode & DERING and y > 0 and "no_row_end_call" not in c["faults"]:
            o = do + width - stride - shift
            before = bytes(db[o + stride + i * stride + 8] for i in range(8))
            _dering(db, o, stride, c, qp, trace, tag)
            if before != bytes(db[o + stride + i * stride + 8] for i in range(8)):
                _count(trace, tag + "_row_end_changed")
        if detour:
            D[d0 + y * stride:d0 + height * stride] = td[stride:stride * (1 + height - y)]
    return np.frombuffer(bytes(D[d0:]), np.uint8).reshape(height, width).copy()


def postprocess(planes, width, height, m, qp=None, ctx=None, trace=None, faults=(), prefill=0):
    """pp_postprocess for PP_FORMAT_420 -> [Y, U, V].  m: a parse_mode dict; qp overrides the mode's (a frame's own QP)"""
    if qp is None:
        qp = m["forcedQuant"] if m["lumMode"] & FORCE_QUANT else 1
    qp &= 0xFF
    ctx = ctx or Context(width)
    out = [postprocess_plane(planes[0], width, height, m["lumMode"] & FILTER_BITS, qp, m["baseDcDiff"], m["flatnessThreshold"], ctx, trace,
                             "y", faults, prefill)]
    for i in (1, 2):
        if m["chromMode"]:
            out.append(postprocess_plane(planes[i], width >> 1, height >> 1, m["chromMode"] & FILTER_BITS, qp, m["baseDcDiff"],
                                         m["flatnessThreshold"], ctx, trace, "c", faults, prefill))
        else:
            out.append(np.array(planes[i], np.uint8).reshape(height >> 1, width >> 1).copy())
    return out


def fnv1a64(data):
    h = 0xcbf29ce484222325
    for b in bytes(data):
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h
