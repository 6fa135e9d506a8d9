"""Deflate streams for the decoders of csrc/oip_inflate.h (host: tests/test_deflate_cpu.py, device: tests/test_gpu_deflate.py).

Three parts, none of which shares anything with the product's decoder:
  * trace(stream): a bit-level inflate in Python that also reports what the stream holds -- block types, the longest literal/length
    and distance codes, the smallest and largest distance, the longest match, the repeat codes of the code-length alphabet ... --
    and raises Reject(rule) for a stream that breaks a rule of include/oip_c.h (oip_tiff_deflate_decode_u16);
  * a Deflate WRITER that emits stored, fixed and dynamic blocks from explicit code lengths and an explicit token list, for the
    states zlib's own compressor does not reach on small inputs (and for every stream that must be refused);
  * CASES: name -> Case(stream, the bytes it decodes to or None, the capacity it is decoded into, the event it is named for).
Every test asserts case.event(trace) first, and that zlib agrees (check_against_zlib)."""
import collections
import functools
import zlib

import numpy as np

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
         16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


class Reject(Exception):
    """the stream breaks the rule named by args[0]"""


# ---- the tracer ------------------------------------------------------------------------------------------------------------------
class Trace:
    def __init__(self):
        self.out = bytearray()
        self.cinfo = None
        self.blocks = []                # BTYPE of every block
        self.stored_lens = []
        self.max_lit_len = self.max_dist_len = self.max_match = self.max_dist = 0
        self.min_dist = None
        self.repeats = set()            # code-length symbols 16 / 17 / 18 seen
        self.repeat_across = set()      # ... whose run starts among the literal/length lengths and ends among the distances
        self.matches = []               # (output offset, length, distance)
        self.length_symbols = set()
        self.hlit_hdist = []            # (HLIT + 257, HDIST + 1) of every dynamic block
        self.single_dist_code = False
        self.single_lit_code = False
        self.end_bit = None             # bit position behind the final block
        self.trailer = None             # True: present and right; False: fewer than four bytes left
        self.trailing = 0               # bytes behind the trailer


def _kraft(lens, which):
    count = collections.Counter(l for l in lens if l)
    left, mx = 1, max(count) if count else 0
    for l in range(1, 16):
        left = left * 2 - count.get(l, 0)
        if left < 0:
            raise Reject("oversubscribed " + which)
    if left > 0 and (which == "code-length code" or mx > 1):
        raise Reject("incomplete " + which)
    return left > 0 and mx == 1


def canonical(lens):
    """symbol -> (code, length), RFC 1951 3.2.2"""
    count = collections.Counter(l for l in lens if l)
    code, nxt = 0, {}
    for l in range(1, 16):
        code = (code + count.get(l - 1, 0)) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def trace(stream):
    t = Trace()
    data = bytes(stream)
    nbits = len(data) * 8
    pos = 0

    def bits(k):
        nonlocal pos
        if pos + k > nbits:
            raise Reject("truncated")
        v = (int.from_bytes(data[pos >> 3:(pos >> 3) + 4], "little") >> (pos & 7)) & ((1 << k) - 1)
        pos += k
        return v

    def symbol(table, which):
        code = 0
        for l in range(1, 16):
            code = (code << 1) | bits(1)
            if (l, code) in table:
                return table[(l, code)]
        raise Reject("no code: " + which)

    def inverse(lens):
        return {(l, c): s for s, (c, l) in canonical(lens).items()}

    cmf, flg = bits(8), bits(8)
    if cmf & 15 != 8 or cmf >> 4 > 7 or ((cmf << 8) | flg) % 31 or flg & 0x20:
        raise Reject("header")
    t.cinfo = cmf >> 4
    final = 0
    while not final:
        final, btype = bits(1), bits(2)
        t.blocks.append(btype)
        if btype == 3:
            raise Reject("block type")
        if btype == 0:
            pos = (pos + 7) & ~7
            ln, nln = bits(16), bits(16)
            if ln ^ 0xFFFF != nln:
                raise Reject("stored length")
            if pos + 8 * ln > nbits:
                raise Reject("truncated")
            t.out += data[pos >> 3:(pos >> 3) + ln]
            t.stored_lens.append(ln)
            pos += 8 * ln
            continue
        if btype == 1:
            lit_lens, dist_lens = FIXED_LIT, FIXED_DIST
        else:
            nlen, ndist, ncode = bits(5) + 257, bits(5) + 1, bits(4) + 4
            if nlen > 286 or ndist > 30:
                raise Reject("too many symbols")
            t.hlit_hdist.append((nlen, ndist))
            cl = [0] * 19
            for i in range(ncode):
                cl[CL_ORDER[i]] = bits(3)
            _kraft(cl, "code-length code")
            cltab = inverse(cl)
            lens = []
            while len(lens) < nlen + ndist:
                s = symbol(cltab, "code-length code")
                if s < 16:
                    lens.append(s)
                    continue
                if s == 16:
                    if not lens:
                        raise Reject("repeat without previous")
                    val, rep = lens[-1], 3 + bits(2)
                elif s == 17:
                    val, rep = 0, 3 + bits(3)
                else:
                    val, rep = 0, 11 + bits(7)
                if len(lens) + rep > nlen + ndist:
                    raise Reject("repeat overrun")
                t.repeats.add(s)
                if len(lens) < nlen < len(lens) + rep:
                    t.repeat_across.add(s)
                lens += [val] * rep
            if lens[256] == 0:
                raise Reject("no end-of-block")
            lit_lens, dist_lens = lens[:nlen], lens[nlen:]
            if _kraft(lit_lens, "literal/length set"):
                t.single_lit_code = True
            if _kraft(dist_lens, "distance set"):
                t.single_dist_code = True
        t.max_lit_len = max(t.max_lit_len, max(lit_lens))
        t.max_dist_len = max(t.max_dist_len, max(dist_lens))
        ltab, dtab = inverse(lit_lens), inverse(dist_lens)
        while True:
            s = symbol(ltab, "literal/length")
            if s < 256:
                t.out.append(s)
                continue
            if s == 256:
                break
            if s > 285:
                raise Reject("literal/length symbol")
            t.length_symbols.add(s)
            L = LBASE[s - 257] + bits(LEXT[s - 257])
            d = symbol(dtab, "distance")
            if d > 29:
                raise Reject("distance symbol")
            D = DBASE[d] + bits(DEXT[d])
            if D > len(t.out):
                raise Reject("distance too far")
            t.matches.append((len(t.out), L, D))
            t.max_match = max(t.max_match, L)
            t.max_dist = max(t.max_dist, D)
            t.min_dist = D if t.min_dist is None else min(t.min_dist, D)
            for _ in range(L):
                t.out.append(t.out[-D])
    t.end_bit = pos
    pos = (pos + 7) & ~7
    left = len(data) - (pos >> 3)
    if left >= 4:
        if int.from_bytes(data[pos >> 3:(pos >> 3) + 4], "big") != zlib.adler32(bytes(t.out)):
            raise Reject("adler")
        t.trailer, t.trailing = True, left - 4
    else:
        t.trailer = False
    t.out = bytes(t.out)
    return t


# ---- the writer ------------------------------------------------------------------------------------------------------------------
class BitWriter:
    def __init__(self):
        self.acc = self.n = 0
        self.out = bytearray()

    def bits(self, v, k):                       # a number, least significant bit first
        self.acc |= (v & ((1 << k) - 1)) << self.n
        self.n += k
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c):                          # a Huffman code (code, length), most significant bit first
        for i in range(c[1] - 1, -1, -1):
            self.bits((c[0] >> i) & 1, 1)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def bitlen(self):
        return len(self.out) * 8 + self.n

    def done(self):
        self.align()
        return bytes(self.out)


def length_symbol(L):
    if L == 258:
        return 285, 0, 0
    i = max(k for k in range(28) if LBASE[k] <= L)
    return 257 + i, LEXT[i], L - LBASE[i]


def dist_symbol(D):
    i = max(k for k in range(30) if DBASE[k] <= D)
    return i, DEXT[i], D - DBASE[i]


def complete_lengths(symbols, size):
    """code lengths (a list of `size`) of a complete code over `symbols` (two at least), as flat as it can be"""
    symbols = sorted(set(symbols))
    k = len(symbols)
    assert k >= 2
    m = (k - 1).bit_length()
    short = (1 << m) - k
    lens = [0] * size
    for i, s in enumerate(symbols):
        lens[s] = m - 1 if i < short else m
    return lens


def put_tokens(bw, tokens, lit_lens, dist_lens, eob=True):
    """tokens: a literal (int), a match (L, D), ("lsym", s): the bare literal/length symbol s, ("dsym", L, s): a match of length L
    whose distance is the bare symbol s"""
    lc, dc = canonical(lit_lens), canonical(dist_lens)
    for tok in tokens:
        if isinstance(tok, int):
            bw.code(lc[tok])
        elif tok[0] == "lsym":
            bw.code(lc[tok[1]])
        else:
            s, e, v = length_symbol(tok[1] if tok[0] == "dsym" else tok[0])
            bw.code(lc[s]); bw.bits(v, e)
            if tok[0] == "dsym":
                bw.code(dc[tok[2]])
            else:
                s, e, v = dist_symbol(tok[1])
                bw.code(dc[s]); bw.bits(v, e)
    if eob:
        bw.code(lc[256])


def stored_block(bw, data, final, nlen=None):
    bw.bits(final, 1); bw.bits(0, 2); bw.align()
    bw.bits(len(data), 16); bw.bits((len(data) ^ 0xFFFF) if nlen is None else nlen, 16)
    bw.out += data


def fixed_block(bw, tokens, final, eob=True):
    bw.bits(final, 1); bw.bits(1, 2)
    put_tokens(bw, tokens, FIXED_LIT, FIXED_DIST, eob)


def dynamic_header(bw, final, lit_lens, dist_lens, cl_ops=None, cl_lens=None):
    """cl_ops: the code-length symbols that spell lit_lens + dist_lens, as (symbol, extra value); default: one plain length each"""
    if cl_ops is None:
        cl_ops = [(l, 0) for l in list(lit_lens) + list(dist_lens)]
    if cl_lens is None:
        used = {s for s, _ in cl_ops}
        cl_lens = complete_lengths(used | ({18, 17} if len(used) < 2 else set()), 19)
    ncode = max(4, max(i for i in range(19) if cl_lens[CL_ORDER[i]]) + 1)
    bw.bits(final, 1); bw.bits(2, 2)
    bw.bits(len(lit_lens) - 257, 5); bw.bits(len(dist_lens) - 1, 5); bw.bits(ncode - 4, 4)
    for i in range(ncode):
        bw.bits(cl_lens[CL_ORDER[i]], 3)
    cc = canonical(cl_lens)
    for s, v in cl_ops:
        bw.code(cc[s])
        if s >= 16:
            bw.bits(v, {16: 2, 17: 3, 18: 7}[s])


def dynamic_block(bw, tokens, final, lit_lens, dist_lens, cl_ops=None, cl_lens=None, eob=True):
    dynamic_header(bw, final, lit_lens, dist_lens, cl_ops, cl_lens)
    put_tokens(bw, tokens, lit_lens, dist_lens, eob)


def zwrap(body, out, cinfo=7, adler=None, cmf=None, flg=None, trailer=True):
    cmf = (cinfo << 4) | 8 if cmf is None else cmf
    if flg is None:
        flg = (31 - (cmf << 8) % 31) % 31
    a = zlib.adler32(out) if adler is None else adler
    return bytes([cmf, flg]) + body + (a.to_bytes(4, "big") if trailer else b"")


def expand(tokens, prefix=b""):
    """what a token list decodes to"""
    out = bytearray(prefix)
    for tok in tokens:
        if isinstance(tok, int):
            out.append(tok)
        else:
            for _ in range(tok[0]):
                out.append(out[-tok[1]])
    return bytes(out)


# ---- the cases -------------------------------------------------------------------------------------------------------------------
# out: the bytes an accepted stream decodes to, None for a stream that must be refused; cap: the size of the strip it stands for
# (len(out) unless the case is about the size rule); zlib_says: "ok" (zlib.decompress returns out), "partial" (no or cut trailer:
# a decompressobj returns out and is not at eof), "error", or None where the rule is the TIFF reader's and not zlib's.
Case = collections.namedtuple("Case", "stream out cap zlib_says event")


def _noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _text(n, seed):
    """compressible bytes: short words from a small alphabet"""
    rng = np.random.default_rng(seed)
    words = [bytes(rng.integers(97, 105, int(k), dtype=np.uint8)) for k in rng.integers(2, 9, 40)]
    out = bytearray()
    while len(out) < n:
        out += words[int(rng.integers(0, 40))]
    return bytes(out[:n])


def _compress(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
    return c.compress(data) + c.flush()


def _accepted():
    c = {}

    def add(name, stream, out, event, zlib_says="ok"):
        assert len(out) % 2 == 0 and len(out) >= 2, name       # a strip of 16-bit samples
        c[name] = Case(bytes(stream), bytes(out), len(out), zlib_says, event)

    # -- what zlib's compressor reaches on small inputs
    d = _noise(70000, 1)
    add("zlib_level0_two_stored", _compress(d, 0), d, lambda t: t.blocks == [0, 0] and t.stored_lens == [65535, 4465])
    d = _text(3000, 2)
    add("zlib_fixed", _compress(d, 6, zlib.Z_FIXED), d, lambda t: set(t.blocks) == {1} and t.max_match > 3)
    d = _text(3000, 3)
    add("zlib_huffman_only", _compress(d, 6, zlib.Z_HUFFMAN_ONLY), d, lambda t: set(t.blocks) == {2} and not t.matches)
    d = np.full(2048, 4242, "<u2").tobytes()
    add("zlib_constant_u16", _compress(d, 6), d, lambda t: (258, 2) in {(m[1], m[2]) for m in t.matches})
    rng = np.random.default_rng(4)
    d = (rng.geometric(0.08, 120000) - 1).clip(0, 255).astype(np.uint8).tobytes()
    add("zlib_geometric_level9", _compress(d, 9), d,
        lambda t: t.max_lit_len >= 13 and t.max_dist_len >= 11 and t.max_dist > 32000 and t.repeats == {16, 17, 18})
    z = zlib.compressobj(6)
    parts = [_text(16, 5), _text(6000, 6), _noise(300, 7)]
    s = z.compress(parts[0]) + z.flush(zlib.Z_SYNC_FLUSH) + z.compress(parts[1]) + z.flush(zlib.Z_FULL_FLUSH) + z.compress(parts[2]) + z.flush()
    add("zlib_flushes_five_blocks", s, b"".join(parts), lambda t: len(t.blocks) >= 5 and set(t.blocks) == {0, 1, 2} and 0 in t.stored_lens)
    d = _text(700, 8)
    add("zlib_cinfo1", _compress(d, 6, wbits=9), d, lambda t: t.cinfo == 1)

    # -- what it does not: from the writer
    def one(tokens, lit_lens=None, dist_lens=None, prefix=b"", **kw):
        """[stored block with `prefix`] + one final block with `tokens`: fixed, or dynamic where code lengths are given"""
        bw = BitWriter()
        if prefix:
            for i in range(0, len(prefix), 65535):
                stored_block(bw, prefix[i:i + 65535], 0)
        if lit_lens is None:
            fixed_block(bw, tokens, 1)
        else:
            dynamic_block(bw, tokens, 1, lit_lens, dist_lens, **kw)
        out = expand(tokens, prefix)
        return zwrap(bw.done(), out), out

    # lengths 1, 2, ..., 14, 15, 15 are complete: literals 0..12 get 1..13 bits, 'a' 14, 'b' 15, end-of-block 15; the same shape
    # over the first 16 distance symbols gives distance 129 (symbol 14) and 193 (symbol 15) 15-bit codes
    lit = [0] * 257
    for i in range(13):
        lit[i] = i + 1
    lit[97], lit[98], lit[256] = 14, 15, 15
    dist = list(range(1, 16)) + [15]
    lit2 = list(lit) + [0] * 8
    lit2[97], lit2[264] = 0, 14                               # length 10 on a 14-bit code instead of 'a'
    s, o = one([0, 1, 98, 12] * 60 + [(10, 193), (10, 129), 98, 0], lit2, dist)
    add("writer_15bit_codes", s, o, lambda t: t.max_lit_len == 15 and t.max_dist_len == 15 and {m[2] for m in t.matches} == {193, 129})
    s, o = one([0, 97, 98, 11, 12, 97, 98, 0], lit, [1, 1])
    add("writer_14_and_15bit_literals", s, o, lambda t: t.max_lit_len == 15 and not t.matches and t.out.count(97) == 2)

    p = _noise(32768, 9)
    s, o = one([(40, 32768), 7, 7], prefix=p)
    add("writer_distance_32768", s, o, lambda t: t.max_dist == 32768)
    s, o = one([65, (258, 1), 66])
    add("writer_d1_l258_symbol285", s, o, lambda t: t.matches == [(1, 258, 1)] and 285 in t.length_symbols)
    for D in (63, 64, 65):
        toks = list(_noise(70, 10 + D))
        for L in (3, 64, 65, 258):
            toks += [(L, D), 200 + L % 50]
        s, o = one(toks + [1] * (len(expand(toks)) % 2))
        add("writer_wave_width_d%d" % D, s, o, lambda t, D=D: [m[1:] for m in t.matches] == [(L, D) for L in (3, 64, 65, 258)])
    p = _noise(32700, 11)
    s, o = one([(258, 100), 9, 9], prefix=p)
    add("writer_match_straddles_32768", s, o, lambda t: t.matches[0][0] < 32768 < t.matches[0][0] + t.matches[0][1])
    p = _noise(65536 - 200, 12)
    s, o = one([(200, 32768)], prefix=p)
    add("writer_d32768_ends_at_the_wrap", s, o, lambda t: t.matches == [(65336, 200, 32768)] and len(t.out) == 65536)
    p = _noise(32768 - 100, 13)
    s, o = one([(100, 64), 5, 5], prefix=p)
    add("writer_match_ends_at_32768", s, o, lambda t: t.matches[0][0] + t.matches[0][1] == 32768)

    lit = complete_lengths(range(286), 286)
    dist = complete_lengths(range(30), 30)
    s, o = one([0, 255, 17, (258, 1), (3, 2), 44, (4, 4), 45], lit, dist)
    add("writer_hlit286_hdist30", s, o, lambda t: t.hlit_hdist == [(286, 30)])

    # The lengths of symbols 258 and 259 and of all four distance symbols are 2: after a plain 2 for symbol 258, one repeat code 16
    # (x5) spells symbol 259 and the four distances.  Kraft: 254 literals share a quarter, 256, 258 and 259 take a quarter each.
    lit = [l + 2 for l in complete_lengths(range(254), 254)] + [0, 0, 2, 0, 2, 2]
    dist = [2, 2, 2, 2]
    assert sum(2.0 ** -l for l in lit if l) == 1.0 and len(lit) == 260
    ops = [(l, 0) for l in lit[:259]] + [(16, 2)]
    s, o = one([3, 200, 7, (5, 3), (4, 1), 3, 3], lit, dist, cl_ops=ops)
    add("writer_repeat16_across_the_boundary", s, o, lambda t: t.repeat_across == {16})

    lit = complete_lengths([65, 66, 256, 257, 258, 260], 261)
    s, o = one([65, 66, (3, 1), (4, 1), (6, 1), 65], lit, [1])
    add("writer_single_distance_code", s, o, lambda t: t.single_dist_code and t.min_dist == t.max_dist == 1)
    lit = [0] * 256 + [1]
    bw = BitWriter()
    stored_block(bw, b"only the end", 0)
    dynamic_block(bw, [], 1, lit, [0])
    add("writer_end_of_block_is_the_only_code", zwrap(bw.done(), b"only the end"), b"only the end", lambda t: t.single_lit_code and t.blocks == [0, 2])

    toks = [200, 201, 202, 203, 204, 205]                     # 3 + 6 x 9 + 7 bits = 64
    s, o = one(toks)
    add("writer_ends_on_a_byte_boundary", s, o, lambda t: t.end_bit % 8 == 0 and t.blocks == [1])

    # -- the trailer
    d = _text(500, 14)
    s = _compress(d)
    for cut in (1, 3, 4):
        add("trailer_cut_by_%d" % cut, s[:-cut], d, lambda t: t.trailer is False, "partial")
    add("trailing_bytes_are_ignored", s + b"\x00\xff trailing", d, lambda t: t.trailer is True and t.trailing == 11, "partial")
    return c


def _rejected():
    c = {}

    def add(name, stream, rule, cap=128, zlib_says="error"):
        c[name] = Case(bytes(stream), None, cap, zlib_says, rule)

    d = bytes(range(64))
    good = _compress(d)
    body = good[2:-4]
    add("header_cm_7", zwrap(body, d, cmf=0x77), "header")
    add("header_cinfo_8", zwrap(body, d, cmf=0x88), "header")
    add("header_fcheck", zwrap(body, d, flg=good[1] ^ 1), "header")
    add("header_fdict", zwrap(body, d, cmf=0x78, flg=0xBB), "header")              # 0x78BB: FDICT set, FCHECK valid
    assert 0x78BB % 31 == 0 and 0xBB & 0x20

    def wrap(build, out=b""):
        bw = BitWriter()
        build(bw)
        return zwrap(bw.done(), out)

    def btype3(bw):
        stored_block(bw, d, 0); bw.bits(1, 1); bw.bits(3, 2)
    add("block_type_3", wrap(btype3), "block type")
    add("stored_len_nlen", wrap(lambda bw: stored_block(bw, d, 1, nlen=0x1234)), "stored length")

    ok_lit = complete_lengths([0, 1, 2, 256], 257)

    def hdr(lit, dist, **kw):
        def build(bw):
            stored_block(bw, d, 0)
            dynamic_header(bw, 1, lit, dist, **kw)
            bw.bits(0, 32)
        return wrap(build)

    cl = [0] * 19
    cl[0] = cl[1] = cl[2] = 1
    add("code_length_code_oversubscribed", hdr(ok_lit, [1, 1], cl_lens=cl, cl_ops=[]), "oversubscribed code-length code")
    cl = [0] * 19
    cl[0], cl[2] = 1, 2
    add("code_length_code_incomplete", hdr(ok_lit, [1, 1], cl_lens=cl, cl_ops=[]), "incomplete code-length code")
    over = list(ok_lit)
    over[3] = 1
    add("literal_set_oversubscribed", hdr(over, [1, 1]), "oversubscribed literal/length set")
    inc = list(ok_lit)
    inc[2] = 0                                                # 0, 1, 256 at two bits: a quarter of the code space is left
    add("literal_set_incomplete", hdr(inc, [1, 1]), "incomplete literal/length set")
    add("distance_set_oversubscribed", hdr(ok_lit, [1, 1, 1]), "oversubscribed distance set")
    add("distance_set_incomplete", hdr(ok_lit, [2, 2]), "incomplete distance set")
    add("repeat_16_first", hdr(ok_lit, [1, 1], cl_ops=[(16, 0), (2, 0)], cl_lens=complete_lengths([2, 16], 19)), "repeat without previous")
    ops = [(l, 0) for l in ok_lit] + [(1, 0), (18, 0)]
    add("repeat_past_the_end", hdr(ok_lit, [1, 1], cl_ops=ops), "repeat overrun")
    noeob = complete_lengths([0, 1, 2, 3], 257)
    add("no_end_of_block_code", hdr(noeob, [1, 1]), "no end-of-block")
    lit287 = complete_lengths(range(287), 287)
    add("hlit_287", hdr(lit287, [1, 1]), "too many symbols")
    add("hdist_31", hdr(ok_lit, complete_lengths(range(31), 31)), "too many symbols")

    def fixed(tokens, out=b""):
        def build(bw):
            stored_block(bw, d, 0)
            fixed_block(bw, tokens, 1)
        return wrap(build, out)
    add("literal_length_symbol_286", fixed([65, ("lsym", 286), 66]), "literal/length symbol")
    add("literal_length_symbol_287", fixed([65, ("lsym", 287), 66]), "literal/length symbol")
    add("distance_symbol_30", fixed([65, ("dsym", 3, 30), 66]), "distance symbol")
    add("distance_symbol_31", fixed([65, ("dsym", 3, 31), 66]), "distance symbol")
    add("distance_before_the_start", fixed([65, (3, 66)]), "distance too far")          # 65 bytes are there
    add("distance_before_the_start_of_an_empty_output", wrap(lambda bw: fixed_block(bw, [(3, 1)], 1)), "distance too far")

    def single(bw):
        stored_block(bw, d, 0)
        lit = complete_lengths([65, 256, 257], 258)
        dynamic_header(bw, 1, lit, [1])
        c = canonical(lit)
        bw.code(c[65]); bw.code(c[257]); bw.bits(1, 1)        # the one distance code is "0"; "1" is no code
        bw.bits(0, 16)
    add("bits_that_are_no_distance_code", wrap(single), "no code: distance")
    add("adler_mismatch", good[:-4] + bytes([good[-4] ^ 1]) + good[-3:], "adler")
    return c


# rule (what trace() raises) -> (the status of csrc/oip_inflate.h, the words of the error that names it)
CAUSE = {
    "header": (1, "bad zlib header"), "block type": (2, "invalid block type"), "stored length": (3, "stored block lengths do not match"),
    "too many symbols": (4, "too many length or distance symbols"), "oversubscribed code-length code": (5, "invalid code-length code"),
    "incomplete code-length code": (5, "invalid code-length code"), "repeat without previous": (6, "length repeat with no previous length"),
    "repeat overrun": (7, "length repeat past the last symbol"), "no end-of-block": (8, "missing end-of-block code"),
    "oversubscribed literal/length set": (9, "invalid literal/length code lengths"), "incomplete literal/length set": (9, "invalid literal/length code lengths"),
    "oversubscribed distance set": (10, "invalid distance code lengths"), "incomplete distance set": (10, "invalid distance code lengths"),
    "literal/length symbol": (11, "invalid literal/length code"), "no code: literal/length": (11, "invalid literal/length code"),
    "distance symbol": (12, "invalid distance code"), "no code: distance": (12, "invalid distance code"),
    "distance too far": (13, "distance too far back"), "truncated": (14, "stream ends inside a block"), "adler": (16, "Adler-32 mismatch"),
}


@functools.lru_cache(maxsize=None)
def accepted():
    return _accepted()


@functools.lru_cache(maxsize=None)
def rejected():
    return _rejected()


@functools.lru_cache(maxsize=None)
def size_cases():
    """the TIFF reader's own rule: a stream decodes to exactly its strip (zlib has no opinion)"""
    d = _text(400, 20)
    s = _compress(d)
    return {"decodes_to_more": Case(s, None, 398, None, "size"), "decodes_to_fewer": Case(s, None, 402, None, "size")}


@functools.lru_cache(maxsize=None)
def truncation_stream():
    """a short stream with a stored, a fixed and a dynamic block; every prefix of it is a test"""
    z = zlib.compressobj(6)
    a, b = _text(16, 21), _text(260, 22)
    s = z.compress(a) + z.flush(zlib.Z_FULL_FLUSH) + z.compress(b) + z.flush()
    t = trace(s)
    assert set(t.blocks) == {0, 1, 2} and t.out == a + b, t.blocks
    return s, a + b


@functools.lru_cache(maxsize=None)
def traced(name):
    case = {**accepted(), **rejected(), **size_cases()}[name]
    try:
        return trace(case.stream)
    except Reject as e:
        return e


def check_event(name):
    """the stream still holds what the case is named for (accepted: its event and its bytes; rejected: the rule it breaks)"""
    case = {**accepted(), **rejected(), **size_cases()}[name]
    t = traced(name)
    if case.out is not None:
        assert not isinstance(t, Reject), (name, t)
        assert t.out == case.out and case.event(t), name
    elif case.event == "size":
        assert len(t.out) != case.cap
    else:
        assert isinstance(t, Reject) and t.args[0] == case.event, (name, t)


def check_against_zlib(name):
    case = {**accepted(), **rejected(), **size_cases()}[name]
    if case.zlib_says == "ok":
        assert zlib.decompress(case.stream) == case.out, name
    elif case.zlib_says == "partial":
        z = zlib.decompressobj()
        assert z.decompress(case.stream) == case.out, name
    elif case.zlib_says == "error":
        try:
            zlib.decompress(case.stream)
        except zlib.error:
            return
        raise AssertionError("zlib accepts " + name)


def truncation_is_tolerated(cut):
    """what the rules say about the first `cut` bytes of truncation_stream(): True where only (part of) the trailer is missing"""
    s, _ = truncation_stream()
    return cut >= len(s) - 4


def pack(streams):
    """streams one behind the other at even offsets, a few bytes in front, as a TIFF file holds its strips"""
    blob, off, ln = bytearray(b"\x00" * 6), [], []
    for s in streams:
        if len(blob) & 1:
            blob.append(0)
        off.append(len(blob)); ln.append(len(s))
        blob += s
    return np.frombuffer(bytes(blob), dtype=np.uint8).copy(), off, ln


def write_case_files(directory):
    """<name>.z, <name>.out for the accepted ones, and cases.txt (`name accept|reject cap status`, status -1 where the size alone
    is wrong) for tests/cpp/inflate_test.cpp;
    trunc.z / trunc.out is the truncation stream, flip<k>.z the three short streams of its mutation sweep"""
    import os
    lines = []
    for name, case in {**accepted(), **rejected(), **size_cases()}.items():
        open(os.path.join(directory, name + ".z"), "wb").write(case.stream)
        if case.out is not None:
            open(os.path.join(directory, name + ".out"), "wb").write(case.out)
        status = 0 if case.out is not None else CAUSE[case.event][0] if case.event in CAUSE else -1
        lines.append("%s %s %d %d" % (name, "accept" if case.out is not None else "reject", case.cap, status))
    open(os.path.join(directory, "cases.txt"), "w").write("\n".join(lines) + "\n")
    s, out = truncation_stream()
    open(os.path.join(directory, "trunc.z"), "wb").write(s)
    open(os.path.join(directory, "trunc.out"), "wb").write(out)
    flips = [s, accepted()["writer_single_distance_code"].stream, _compress(_text(120, 23), 6, zlib.Z_FIXED)]
    for k, f in enumerate(flips):
        open(os.path.join(directory, "flip%d.z" % k), "wb").write(f)
    return len(lines)
