"""Writes AMV scans symbol by symbol (a helper of the tests, imported as test_gpu_parity imports test_oracle_pin).

An encoder that quantises real pictures writes a small part of what a valid scan may hold: about half of the AC
symbols, magnitudes up to size 7, DC differences that never make a predictor wrap, nothing near the record space the
decoder gives a frame.  Here a frame is written from a list of blocks, so that a test can put any symbol at any place:

    block = (dc_diff, items, eob)
        dc_diff  the DC difference (-2047 .. 2047; the DC tables have sizes 0 .. 11), or None: no DC symbol (the
                 items start where the decoder expects one)
        items    AC items in stream order: (run, value) with value != 0, "ZRL" (sixteen zeros), or a raw bit string
                 such as "1" * 16 (no code of any table: the decoder stops there)
        eob      write the end-of-block symbol after the items

Blocks come in MCU order, six to an MCU (Y0 Y1 Y2 Y3 Cb Cr; tables 0/2 for Y, 1/3 for Cb and Cr).  `assemble` writes
FF D8, the symbols MSB first, pads the last byte with 1-bits, puts 00 behind every FF and ends with FF D9 (mjpegenc.c's
encode_block, stuffing, escape_FF and trailer); it can cut the chunk at a bit, leave out the EOI or pad with 0-bits.
`expected_coefficients` is what a decoder must make of a valid frame: zig-zag lines, the DC accumulated per component
and wrapped as int16 (AmvJpeg.c:1200-1221).  `model_decode` is a plain restatement of the serial decoder (AmvJpeg.c:842-974
with the oracle's statuses) over the bytes, for the frames that are not valid.

The tables are the JPEG K.3 specifications (ITU-T T.81 Annex K), as amvlib and mjpeg.c hold them.
"""
import numpy as np

ST_FORMAT, ST_OVERRUN, ST_TRUNCATED = 1, 2, 4

BITS = (
    (0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0),             # DC luma
    (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0),             # DC chroma
    (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d),          # AC luma
    (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77),          # AC chroma
)
_VAL_DC = tuple(range(12))
_VAL_AC_LUMA = bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f0"
    "2433627282090a161718191a25262728292a3435363738393a43444546474849"
    "4a535455565758595a636465666768696a737475767778797a83848586878889"
    "8a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5"
    "c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8"
    "f9fa")
_VAL_AC_CHROMA = bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0"
    "156272d10a162434e125f11718191a262728292a35363738393a434445464748"
    "494a535455565758595a636465666768696a737475767778797a828384858687"
    "88898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3"
    "c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8"
    "f9fa")
VALS = (_VAL_DC, _VAL_DC, tuple(_VAL_AC_LUMA), tuple(_VAL_AC_CHROMA))
ZRL, EOB = 0xF0, 0x00
COMP_OF = (0, 0, 0, 0, 1, 2)


def _canonical(bits, vals):
    """symbol -> (length, code): ff_mjpeg_build_huffman_codes (mjpeg.c:129-147)"""
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            codes[vals[k]] = (length, code)
            code += 1
            k += 1
        code <<= 1
    return codes


CODES = tuple(_canonical(b, v) for b, v in zip(BITS, VALS))
# 16-bit window -> (length, symbol), None where no code starts the window (the all-ones prefix)
_LOOKUP = []
for _codes in CODES:
    _tab = [None] * 65536
    for _sym, (_n, _c) in _codes.items():
        _lo = _c << (16 - _n)
        _tab[_lo: _lo + (1 << (16 - _n))] = [(_n, _sym)] * (1 << (16 - _n))
    _LOOKUP.append(_tab)
del _codes, _tab, _sym, _n, _c, _lo


def size_of(v):
    return abs(v).bit_length()


def magnitude_bits(v):
    """the size low bits of v (v > 0) or of v - 1 (v < 0), mjpegenc.c:366-369"""
    s = size_of(v)
    return format((v if v > 0 else v + (1 << s) - 1), "0%db" % s) if s else ""


def tables_of(k):
    """(DC table, AC table) of block k of an MCU"""
    return (0, 2) if k < 4 else (1, 3)


def block_symbols(block, k):
    """-> [(table, symbol or None for raw bits, bit string)] of one block, k = its place in the MCU"""
    dc_diff, items, eob = block
    dct, act = tables_of(k)
    out = []
    if dc_diff is not None:
        s = size_of(dc_diff)
        if s > 11:
            raise ValueError("DC difference %d needs size %d" % (dc_diff, s))
        n, c = CODES[dct][s]
        out.append((dct, s, format(c, "0%db" % n) + magnitude_bits(dc_diff)))
    for it in items:
        if isinstance(it, str) and it == "ZRL":
            n, c = CODES[act][ZRL]
            out.append((act, ZRL, format(c, "0%db" % n)))
        elif isinstance(it, str):
            out.append((act, None, it))
        else:
            run, v = it
            s = size_of(v)
            if not (0 <= run <= 15 and 1 <= s <= 10):
                raise ValueError("no AC symbol for run %d value %d" % (run, v))
            n, c = CODES[act][(run << 4) | s]
            out.append((act, (run << 4) | s, format(c, "0%db" % n) + magnitude_bits(v)))
    if eob:
        n, c = CODES[act][EOB]
        out.append((act, EOB, format(c, "0%db" % n)))
    return out


def _stuff(raw):
    out = bytearray()
    for b in raw:
        out.append(b)
        if b == 0xFF:
            out.append(0)
    return bytes(out)


class Frame:
    """an assembled chunk and where its symbols are.  syms: [(block, table, symbol, first bit, bit string)]; raw: the scan
    bytes before stuffing (padding included); nbits: scan bits before padding"""

    def __init__(self, chunk, syms, raw, nbits):
        self.chunk, self.syms, self.raw, self.nbits = chunk, syms, raw, nbits


def assemble(blocks, cut_bit=None, eoi=True, pad="1"):
    """blocks (MCU order) -> Frame.  cut_bit: the chunk keeps the scan bytes wholly in front of that bit and no EOI;
    eoi=False: no FF D9; pad="0": the last byte is filled with 0-bits instead of 1-bits"""
    syms, parts, pos = [], [], 0
    for b, blk in enumerate(blocks):
        for table, sym, bits in block_symbols(blk, b % 6):
            syms.append((b, table, sym, pos, bits))
            parts.append(bits)
            pos += len(bits)
    bits = "".join(parts)
    nbits = len(bits)
    bits += pad * (-nbits % 8)
    raw = int(bits, 2).to_bytes(len(bits) // 8, "big") if bits else b""
    if cut_bit is not None:
        return Frame(b"\xff\xd8" + _stuff(raw[: cut_bit // 8]), syms, raw, nbits)
    return Frame(b"\xff\xd8" + _stuff(raw) + (b"\xff\xd9" if eoi else b""), syms, raw, nbits)


def expected_coefficients(blocks):
    """[len(blocks), 64] int16 zig-zag lines of a valid frame, DC = the running sum per component, wrapped as int16"""
    coef = np.zeros((len(blocks), 64), np.int64)
    pred = [0, 0, 0]
    for b, (dc_diff, items, eob) in enumerate(blocks):
        if dc_diff is None:
            raise ValueError("block %d has no DC symbol: not a valid frame" % b)
        c = COMP_OF[b % 6]
        pred[c] = (pred[c] + dc_diff + 32768) % 65536 - 32768
        coef[b, 0] = pred[c]
        i = 1
        for it in items:
            if isinstance(it, str) and it != "ZRL":
                raise ValueError("block %d holds raw bits: not a valid frame" % b)
            run, v = (15, 0) if it == "ZRL" else it
            if i + run > 63:
                raise ValueError("block %d runs past index 63" % b)
            i += run
            coef[b, i] = v
            i += 1
        if i < 64 and not eob:
            raise ValueError("block %d ends at index %d without an end-of-block symbol" % (b, i))
        if i == 64 and eob:
            raise ValueError("block %d is full: the decoder reads no end-of-block symbol there" % b)
    return coef.astype(np.int16)


def blocks_from_coefficients(coef):
    """[n, 64] zig-zag lines, DC not predicted (what an encoder quantised) -> blocks as encode_block codes them
    (mjpegenc.c:390-431): the DC difference to the component's previous DC, zero runs of 16 or more as ZRL, an
    end-of-block symbol unless the last coefficient is non-zero"""
    pred, out = [0, 0, 0], []
    for b, line in enumerate(np.asarray(coef, np.int64)):
        c = COMP_OF[b % 6]
        diff, pred[c] = int(line[0]) - pred[c], int(line[0])
        nz = np.nonzero(line[1:])[0]
        last = int(nz[-1]) + 1 if nz.size else 0
        items, run = [], 0
        for i in range(1, last + 1):
            v = int(line[i])
            if v == 0:
                run += 1
                continue
            while run >= 16:
                items.append("ZRL")
                run -= 16
            items.append((run, v))
            run = 0
        out.append((diff, items, last < 63))
    return out


def records_of(blocks):
    """(records, symbols): one record per DC and per non-zero AC coefficient (what the entropy stage hands the
    reconstruction), one symbol per code in the stream (end-of-block and ZRL included)"""
    rec = sym = 0
    for dc_diff, items, eob in blocks:
        rec += (dc_diff is not None) + sum(1 for it in items if not isinstance(it, str) and it[1] != 0)
        sym += (dc_diff is not None) + len(items) + (1 if eob else 0)
    return rec, sym


def record_space(chunk_len, nblocks):
    """the records a frame is given (amv_host_plan.h entropy_plan: 2 per chunk byte + 2 per block + 64, no more than
    66 per block, in whole lines of 32)"""
    hi = (nblocks * 66 + 95) & ~31
    return (min(2 * chunk_len + 2 * nblocks + 64, hi) + 31) // 32 * 32


def model_decode(chunk, nmcu):
    """the serial decoder over the bytes: -> (coef [nmcu*6, 64] int16 of the whole MCUs before the first error, zeros
    after; status; MCUs decoded; whole blocks decoded; coef [blocks, 64] of every whole block before the first error;
    (records, symbols) the walk decoded -- past a cut, the zeros decode too: luma blocks full of -1).  The byte after every FF is dropped unseen (AmvJpeg.c:1061-1071),
    bytes past the chunk read as zero, TRUNCATED when more bits were consumed than the chunk held (17 for a run of
    ones that is no code, :887)"""
    data, valid, p = bytearray(), 0, 2
    while p < len(chunk):
        data.append(chunk[p])
        valid += 8
        p += 2 if chunk[p] == 0xFF else 1
    data += bytes(nmcu * 6 * 64 * 4 + 8)            # zeros past the end: more than any walk reads
    bits = int.from_bytes(bytes(data), "big")
    total = len(data) * 8
    t = 0
    coef = np.zeros((nmcu * 6, 64), np.int64)
    pred = [0, 0, 0]
    st = 0
    blocks_ok = 0
    walked = [0, 0]   # records, symbols the walk decoded

    def window(t):
        return (bits >> (total - t - 16)) & 0xFFFF

    for b in range(nmcu * 6):
        dct, act = tables_of(b % 6)
        blk = [0] * 64
        i = 0
        while i < 64:
            e = _LOOKUP[dct if i == 0 else act][window(t)]
            if e is None:
                t += 17
                st = ST_FORMAT
                break
            n, sym = e
            t += n
            walked[1] += 1
            walked[0] += i == 0 or (sym & 15) != 0
            run, s = sym >> 4, sym & 15
            v = 0
            if s:
                m = (bits >> (total - t - s)) & ((1 << s) - 1)
                t += s
                v = m if m >> (s - 1) else m - (1 << s) + 1
            if i == 0:
                blk[0] = v
                i = 1
            elif run == 0 and s == 0:
                break
            else:
                if i + run > 63:
                    st = ST_OVERRUN
                    break
                i += run
                blk[i] = v
                i += 1
        if st:
            break
        c = COMP_OF[b % 6]
        pred[c] = (pred[c] + blk[0] + 32768) % 65536 - 32768
        blk[0] = pred[c]
        coef[b] = blk
        blocks_ok += 1
    if t > valid:
        st |= ST_TRUNCATED
    ok = blocks_ok // 6
    whole = coef.copy()
    coef[ok * 6:] = 0
    return coef.astype(np.int16), st, ok, blocks_ok, whole[:blocks_ok].astype(np.int16), tuple(walked)


# ------------------------------------------------------------------------------------------------ the corpus

def mcus(w, h):
    return ((w + 15) // 16) * ((h + 15) // 16)


def _extremes(s):
    """both magnitude extremes of size s, both signs"""
    if s == 0:
        return [0]
    return sorted({1 << (s - 1), (1 << s) - 1, -(1 << (s - 1)), -((1 << s) - 1)})


def _filler(rng, k, big=False):
    """a valid block of ordinary content: a small DC difference, a few AC values of sizes 1..4 (1..10 with big), EOB"""
    items, i = [], 1
    for _ in range(int(rng.integers(0, 9))):
        run = int(rng.integers(0, 6))
        if i + run > 63:
            break
        s = int(rng.integers(1, 11 if big else 5))
        v = int(rng.integers(1 << (s - 1), 1 << s)) * (1 if rng.random() < 0.5 else -1)
        items.append((run, v))
        i += run + 1
    return (int(rng.integers(-40, 41)), items, i < 64)


class _Packer:
    """AC items of one table class into blocks: an item that does not fit closes the block (with an end-of-block symbol
    unless the block is full)"""

    def __init__(self):
        self.blocks, self.items, self.i = [], [], 1

    def add(self, it):
        run = 15 if it == "ZRL" else it[0]
        if self.i + run > 63:
            self.close()
        self.items.append(it)
        self.i += run + 1
        if self.i == 64:
            self.close()

    def close(self):
        if self.items:
            self.blocks.append((self.items, self.i < 64))
        self.items, self.i = [], 1


def _lay_out(rng, n_mcu, luma, chroma, dc_luma, dc_chroma, big_filler=False):
    """blocks of the two classes (lists of (items, eob)) into MCUs, DC differences from the two lists in turn; filler
    behind"""
    out, li, ci, dl, dc = [], 0, 0, 0, 0
    for m in range(n_mcu):
        for k in range(6):
            src, idx = (luma, li) if k < 4 else (chroma, ci)
            if idx < len(src):
                dlist = dc_luma if k < 4 else dc_chroma
                d = dlist[(dl if k < 4 else dc) % len(dlist)]
                if k < 4:
                    li, dl = li + 1, dl + 1
                else:
                    ci, dc = ci + 1, dc + 1
                out.append((d,) + tuple(src[idx]))
            else:
                out.append(_filler(rng, k, big_filler))
    if li < len(luma) or ci < len(chroma):
        raise ValueError("the blocks do not fit %d MCUs" % n_mcu)
    return out


def _every_symbol(rng, n_mcu):
    luma, chroma = _Packer(), _Packer()
    for t, pk in ((2, luma), (3, chroma)):
        items = [(sym >> 4, v) for sym in CODES[t] if sym & 15 for v in _extremes(sym & 15)]
        items += ["ZRL"] * 24
        for j in rng.permutation(len(items)):
            pk.add(items[int(j)])
        pk.close()
    dcs = [[v for s in range(12) for v in _extremes(s)] for _ in range(2)]
    for d in dcs:
        rng.shuffle(d)
    return _lay_out(rng, n_mcu, luma.blocks, chroma.blocks, dcs[0], dcs[1])


def _longest(rng, n_mcu, long_mcus):
    """run 0 / size 10 and run 15 / size 10 (16-bit codes + 10 magnitude bits) back to back, size-11 DC differences"""
    out = []
    for m in range(n_mcu):
        for k in range(6):
            if m >= long_mcus:
                out.append(_filler(rng, k))
                continue
            v = lambda: int(rng.choice([1023, -1023, 512, -512, 777, -600]))
            dc = int(rng.choice([2047, -2047, 1024, -1024, 1500]))
            if (m + k) % 3 == 2:
                out.append((dc, [(15, v()), (15, v()), (15, v()), (14, v())], False))
            else:
                out.append((dc, [(0, v()) for _ in range(63)], False))
    return out


def _dense(rng, n_mcu, per_block):
    """per_block[b] AC values of +-1 in block b (63: the block is full, no end-of-block symbol)"""
    dc = rng.integers(-1, 2, n_mcu * 6).tolist()
    sign = (rng.integers(0, 2, (n_mcu * 6, 63)) * 2 - 1).tolist()
    return [(dc[b], [(0, v) for v in sign[b][: per_block[b]]], per_block[b] < 63) for b in range(n_mcu * 6)]


def _zrl_edges(rng, n_mcu):
    v = lambda: int(rng.choice([1, -1, 5, -300, 1023]))
    patterns = [
        [(0, 1)] * 47 + ["ZRL"],                                   # ZRL at index 48 fills the block: no EOB
        [(15, v()), (15, v()), (15, v()), (13, v()), (0, v())],   # a value at 63: no EOB
        [(0, v()), "ZRL"],                                         # ZRL, then EOB
        ["ZRL", "ZRL", "ZRL", (3, v())],                           # ZRL x3, then a value
        [(0, 2)] * 47 + [(15, v())],                               # run 15 at index 48
        ["ZRL", "ZRL", "ZRL", (14, v())],                          # ZRL x3, run 14: a value at 63
        ["ZRL"],                                                   # ZRL alone, then EOB
    ]
    out = []
    for b in range(n_mcu * 6):
        if b % 5 == 1:
            p = patterns[(b // 5) % len(patterns)]
            i = 1 + sum(16 if it == "ZRL" else it[0] + 1 for it in p)
            out.append((int(rng.integers(-5, 6)), list(p), i < 64))
        else:
            out.append(_filler(rng, b % 6))
    return out


def _dc_wrap(rng, n_mcu, sign):
    out = []
    for b in range(n_mcu * 6):
        d = sign * 2047 if rng.random() < 0.8 else -sign * int(rng.integers(1, 2048))
        items = _filler(rng, b % 6)[1]
        out.append((d, items, (1 + sum(r + 1 for r, _ in items)) < 64))
    return out


def _ff_bytes(rng, n_mcu):
    """magnitudes whose bits are all ones (255, 511, 1023 ...), so FF lands at every byte offset; the scan's last byte is
    FF too (the last block ends at 63 with 1023 and the padding is ones)"""
    out = []
    for b in range(n_mcu * 6):
        items, i = [], 1
        while True:
            run = int(rng.integers(0, 3))
            if i + run > 63 or len(items) > 6:
                break
            s = int(rng.integers(6, 11))
            items.append((run, int(rng.choice([(1 << s) - 1, 1 << (s - 1), -((1 << s) - 1)]))))
            i += run + 1
        out.append((int(rng.choice([2047, 1023, 255, -5])), items, i < 64))
    out[-1] = (0, [(0, 1)] * 62 + [(0, 1023)], False)
    return out


def _random_valid(rng, n_mcu):
    """every kind of symbol at random: sizes 1..10, runs, ZRL, DC differences of every size"""
    out = []
    for b in range(n_mcu * 6):
        items, i = [], 1
        for _ in range(int(rng.integers(0, 20))):
            if rng.random() < 0.08 and i + 15 <= 63:
                items.append("ZRL")
                i += 16
                continue
            run = int(rng.integers(0, 16))
            if i + run > 63:
                break
            s = int(rng.integers(1, 11))
            items.append((run, int(rng.choice(_extremes(s)))))
            i += run + 1
        s = int(rng.integers(0, 12))
        out.append((int(rng.choice(_extremes(s))), items, i < 64))
    return out


def _align_last(blocks, want_mod, rng):
    """append (0, +-1) items to the frame's last block until its end-of-block symbol starts at bit want_mod (mod 8), or
    (want_mod None) the scan ends on a byte boundary; returns the blocks"""
    blocks = list(blocks)
    for _ in range(64):
        f = assemble(blocks)
        last = f.syms[-1]
        ok = (f.nbits % 8 == 0) if want_mod is None else (last[2] == EOB and last[3] % 8 == want_mod)
        if ok:
            return blocks
        d, items, eob = blocks[-1]
        i = 1 + sum(16 if it == "ZRL" else it[0] + 1 for it in items)
        if i >= 60:
            items = []
        blocks[-1] = (d, items + [(0, int(rng.choice([1, -1])))], True)
    raise ValueError("could not align the last block")


class Case:
    """one corpus frame: name, geometry, blocks, the chunk; valid frames carry their expected coefficients (coef), every
    frame the model decoder's (want_coef, status, ok = MCUs decoded, blocks_ok); over: more records than the record space
    holds (the entropy stage must hand the frame to its serial kernel), under: fits with room to spare in every kernel's
    record layout"""

    def __init__(self, name, w, h, blocks, **kw):
        self.name, self.w, self.h, self.blocks = name, w, h, blocks
        self.frame = assemble(blocks, **kw)
        self.chunk = self.frame.chunk
        self.want_coef, self.status, self.ok, self.blocks_ok, self.want_blocks, self.walked = model_decode(self.chunk, mcus(w, h))
        try:   # a valid frame: the decoder must give back what was written (a cut chunk is not one)
            self.coef = expected_coefficients(blocks) if kw.get("cut_bit") is None else None
        except ValueError:
            self.coef = None
        self.records, self.symbols, self.space, self.over, self.under = budget(self.walked, len(self.chunk), len(blocks))


def budget(walked, chunk_len, nblocks):
    """(records, symbols) a decoder walks -> (records, symbols, record space, over, under).  over: more records than
    the space holds, in any layout; under: room to spare in every kernel's layout -- one lane per frame writes a slot per
    symbol (end-of-block and ZRL included) in lines of 32, several lanes start each lane's records on a piece of 8 (up to
    64 lanes)"""
    records, symbols = walked
    space = record_space(chunk_len, nblocks)
    return records, symbols, space, records > space, (symbols + 31) // 32 * 32 <= space and records + 64 * 7 <= space


def corpus(seed=0x5CA9):
    """named crafted frames: 160x120 unless the name says otherwise"""
    rng = np.random.default_rng(seed)
    W, H = 160, 120
    N = mcus(W, H)
    cases = []
    add = lambda name, blocks, w=W, h=H, **kw: cases.append(Case(name, w, h, blocks, **kw))
    add("every_symbol_a", _every_symbol(rng, N))
    add("every_symbol_b", _every_symbol(rng, N))
    add("longest", _longest(rng, N, 16))
    add("dense_all_ac", _dense(rng, N, [63] * (N * 6)))
    # just under / just over the record space: m or m + 1 values of +-1 in every block, as many blocks with m + 1 as keep
    # the frame under (the last such frame) or make it over (the first)
    def dense_mix(m, nb):
        return _dense(np.random.default_rng(seed + m), N, [m + 1] * nb + [m] * (N * 6 - nb))

    def fits(blocks, want):
        return budget(records_of(blocks), len(assemble(blocks).chunk), len(blocks))[3 if want == "over" else 4]

    def first(lo, hi, pred):   # the first n in [lo, hi) with pred(n) (pred is monotone), or hi
        while lo < hi:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if pred(mid) else (mid + 1, hi)
        return lo

    m = first(1, 63, lambda m: not fits(dense_mix(m, 0), "under")) - 1
    add("dense_just_under", dense_mix(m, first(0, N * 6 + 1, lambda nb: not fits(dense_mix(m, nb), "under")) - 1))
    m = first(1, 63, lambda m: fits(dense_mix(m + 1, 0), "over"))
    add("dense_just_over", dense_mix(m, first(0, N * 6 + 1, lambda nb: fits(dense_mix(m, nb), "over"))))
    add("zrl_eob_edges", _zrl_edges(rng, N))
    for k, (name, p) in enumerate((("zrl_at_49", ["ZRL"]), ("run15_at_49", [(15, 3)]))):
        for blk in (6 * 11 + 2, 6 * 57 + 4 + k):
            blocks = [_filler(rng, b % 6) for b in range(N * 6)]
            blocks[blk] = (1, [(0, 1)] * 48 + p, True)
            add("%s_block%d" % (name, blk), blocks)
    add("dc_wrap_up", _dc_wrap(rng, N, 1))
    add("dc_wrap_down", _dc_wrap(rng, N, -1))
    add("ff_bytes", _ff_bytes(rng, N))
    # a run of sixteen 1-bits (no code) in block k of the first, a middle and the last MCU; at the DC symbol in even k
    for m in (0, N // 2, N - 1):
        for k in range(6):
            blocks = [_filler(rng, b % 6) for b in range(N * 6)]
            b = m * 6 + k
            blocks[b] = (None, ["1" * 16], False) if k % 2 == 0 else (3, [(0, 2), (1, -1), "1" * 16], False)
            add("noncode_mcu%d_block%d" % (m, k), blocks)
    # ... within the last 17 bits of the chunk: the 17th bit the decoder reads is padding, the EOI's FF, or past the end
    tail = [_filler(rng, b % 6) for b in range(N * 6)]
    for j in range(8):
        blocks = list(tail)
        blocks[-1] = (2, [(0, 1)] * j + ["1" * 16], False)
        add("noncode_tail%d" % j, blocks)
        add("noncode_tail%d_no_eoi" % j, blocks, eoi=False)
        start = assemble(blocks).syms[-1][3]
        for cut in (start + 4, start + 12, start + 16):
            add("noncode_tail%d_cut%d" % (j, cut - start), blocks, cut_bit=cut)
    # cuts: inside a 16-bit code, inside magnitude bits, inside the last EOB, exactly after the last symbol
    base = _every_symbol(np.random.default_rng(seed + 1), N)
    f = assemble(base)
    mid = [s for s in f.syms if s[0] > 240 and s[2] is not None]
    c16 = next(s for s in mid if s[2] != EOB and CODES[s[1]][s[2]][0] == 16 and (s[3] + 1) // 8 * 8 + 8 < s[3] + 16)
    add("cut_in_16bit_code", base, cut_bit=(c16[3] // 8 + 1) * 8)
    cm = next(s for s in mid if s[1] >= 2 and (s[2] & 15) >= 8 and
              s[3] + CODES[s[1]][s[2]][0] < (s[3] + CODES[s[1]][s[2]][0]) // 8 * 8 + 8 < s[3] + len(s[4]))
    add("cut_in_magnitude", base, cut_bit=((cm[3] + CODES[cm[1]][cm[2]][0]) // 8 + 1) * 8)
    eob7 = _align_last([_filler(rng, b % 6) for b in range(N * 6)], 7, rng)
    last = assemble(eob7).syms[-1]
    add("cut_in_last_eob", eob7, cut_bit=last[3] + 1)
    aligned = _align_last([_filler(rng, b % 6) for b in range(N * 6)], None, rng)
    fa = assemble(aligned)
    add("cut_after_last_symbol", aligned, cut_bit=fa.nbits)
    add("cut_one_byte_early", aligned, cut_bit=fa.nbits - 8)
    add("no_eoi_byte_aligned", aligned, eoi=False)
    add("zero_padding", _random_valid(rng, N), pad="0")
    # other geometries
    for w, h in ((16, 16), (130, 98), (336, 32), (320, 240)):
        add("random_%dx%d" % (w, h), _random_valid(rng, mcus(w, h)), w, h)
        add("dc_wrap_%dx%d" % (w, h), _dc_wrap(rng, mcus(w, h), 1 if w != 130 else -1), w, h)
    add("every_symbol_320x240", _every_symbol(rng, mcus(320, 240)), 320, 240)
    return cases
