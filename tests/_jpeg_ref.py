"""A restatement in numpy / plain Python of the baseline JPEG coder that include/oip_c.h defines (oip_jpeg_scan_u8,
oip_jpeg_interval_host, oip_write_jpeg_u8): ITU-T T.81 SOF0 in a JFIF 1.01 wrapper, 8 bits, grey or YCbCr 4:4:4, the typical
Huffman tables of Annex K.3, one restart interval per row of 8 x 8 blocks.  It takes no code from the product: the tables are typed
from the standard here, the DCT table comes from its formula, the zigzag order from its walk.  encode() returns the file, the bytes of
every interval and a trace of what was emitted; parse_segments() reads the marker segments of a JFIF file back."""
import math
from collections import namedtuple

import numpy as np

# ---- T.81 Annex K.1 / K.2: the base quantisation tables, natural (row-major) order -----------------------------------------
K1_LUMA = [16, 11, 10, 16, 24, 40, 51, 61,
           12, 12, 14, 19, 26, 58, 60, 55,
           14, 13, 16, 24, 40, 57, 69, 56,
           14, 17, 22, 29, 51, 87, 80, 62,
           18, 22, 37, 56, 68, 109, 103, 77,
           24, 35, 55, 64, 81, 104, 113, 92,
           49, 64, 78, 87, 103, 121, 120, 101,
           72, 92, 95, 98, 112, 100, 103, 99]
K2_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99,
             18, 21, 26, 66, 99, 99, 99, 99,
             24, 26, 56, 99, 99, 99, 99, 99,
             47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32

# ---- T.81 Annex K.3: the typical Huffman tables (BITS: codes of each length 1..16; HUFFVAL: the symbols in code order) ------
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
    0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0,
    0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49,
    0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
    0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5,
    0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71,
    0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0,
    0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
    0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa])

Trace = namedtuple("Trace", "dc_categories ac_symbols zrl no_eob stuffed")
Encoded = namedtuple("Encoded", "file intervals trace qtables")


def zigzag():
    """natural index of zigzag position 0..63 (T.81 figure 5): the anti-diagonals, alternating direction"""
    order = []
    for s in range(15):
        cells = [(v, s - v) for v in range(8) if 0 <= s - v < 8]           # (row v, column u), v ascending
        if s % 2 == 0:
            cells.reverse()                                                # even diagonals run upwards
        order += [v * 8 + u for v, u in cells]
    return order


ZIGZAG = zigzag()


def dct_table():
    """T[k][n] = rint(8192 c_k cos((2n + 1) k pi / 16)), c_0 = sqrt(1/8), c_k = 1/2"""
    t = np.zeros((8, 8), dtype=np.int64)
    for k in range(8):
        c = math.sqrt(1.0 / 8.0) if k == 0 else 0.5
        for n in range(8):
            t[k, n] = int(np.rint(8192.0 * c * math.cos((2 * n + 1) * k * math.pi / 16.0)))
    return t


def qtable(base, quality):
    """the IJG rule, natural order"""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [min(max((b * scale + 50) // 100, 1), 255) for b in base]


def huffman_codes(bits, vals):
    """{symbol: (code, length)} of T.81 Annex C"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def ycbcr(rgb):
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11058 * r - 21710 * g + 32768 * b + 8421375) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + 8421375) >> 16
    return np.stack([y, cb, cr], axis=-1)


def quantised_blocks(lines, quality):
    """lines: (<= 8, w) or (<= 8, w, 3) uint8, the lines of one interval -> (mcus, nch, 64) quantised coefficients in zigzag order"""
    lines = np.asarray(lines)
    nch = 1 if lines.ndim == 2 else 3
    s = lines.astype(np.int64).reshape(lines.shape[0], lines.shape[1], nch)
    if nch == 3:
        s = ycbcr(s)
    h, w = s.shape[:2]
    s = np.pad(s, ((0, 8 - h), (0, -w % 8), (0, 0)), mode="edge")           # last column, then last line, repeated
    mcus = s.shape[1] // 8
    blk = s.reshape(8, mcus, 8, nch).transpose(1, 3, 0, 2) - 128            # (mcu, c, y, x)
    T = dct_table()
    t = (np.einsum("kn,mcyn->mcyk", T, blk) + 512) >> 10                    # rows: t[y][k]
    F = (np.einsum("vy,mcyk->mcvk", T, t) + 32768) >> 16                    # columns: F[v][k]
    F = F.reshape(mcus, nch, 64)
    q = np.array([qtable(K1_LUMA, quality)] + [qtable(K2_CHROMA, quality)] * (nch - 1), dtype=np.int64)[None]
    qf = np.sign(F) * ((2 * np.abs(F) + q) // (2 * q))
    return qf[:, :, ZIGZAG]


class _Bits:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, v, n):
        self.acc = (self.acc << n) | v
        self.n += n
        while self.n >= 8:
            self.n -= 8
            self.out.append((self.acc >> self.n) & 0xff)
        self.acc &= (1 << self.n) - 1

    def finish(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)                   # padded with 1-bits
        return bytes(self.out)


def _magnitude(v):
    size = int(abs(v)).bit_length()
    return size, (v if v >= 0 else v - 1) & ((1 << size) - 1)


def encode_interval(lines, quality, trace=None):
    """the bytes of one restart interval (T.81 F.1.2; stuffed; without its RSTn)"""
    co = quantised_blocks(lines, quality)
    nch = co.shape[1]
    dc_codes = [huffman_codes(*DC_LUMA)] + [huffman_codes(*DC_CHROMA)] * 2
    ac_codes = [huffman_codes(*AC_LUMA)] + [huffman_codes(*AC_CHROMA)] * 2
    dcs, acs, zrl, no_eob = set(), set(), 0, 0
    bits = _Bits()
    pred = [0] * nch
    for m in range(co.shape[0]):
        for c in range(nch):
            z = co[m, c].tolist()
            size, mag = _magnitude(z[0] - pred[c])
            pred[c] = z[0]
            dcs.add(size)
            code, n = dc_codes[c][size]
            bits.put((code << size) | mag, n + size)
            run = 0
            for k in range(1, 64):
                if z[k] == 0:
                    run += 1
                    continue
                while run > 15:
                    bits.put(*ac_codes[c][0xf0])
                    zrl += 1
                    run -= 16
                size, mag = _magnitude(z[k])
                acs.add((run, size))
                code, n = ac_codes[c][(run << 4) | size]
                bits.put((code << size) | mag, n + size)
                run = 0
            if run:
                bits.put(*ac_codes[c][0x00])
            else:
                no_eob += 1
    raw = bits.finish()
    if trace is not None:
        trace["dc"] |= dcs
        trace["ac"] |= acs
        trace["zrl"] += zrl
        trace["no_eob"] += no_eob
        trace["stuffed"] += raw.count(b"\xff")
    return raw.replace(b"\xff", b"\xff\x00")


def _segment(marker, body):
    return bytes([0xff, marker]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)


def headers(w, h, nch, quality):
    """SOI .. SOS: APP0 (JFIF 1.01, no units, 1 : 1), a DQT and the DHTs per table in use, SOF0, DRI, SOS"""
    out = b"\xff\xd8" + _segment(0xe0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    tables = [qtable(K1_LUMA, quality)] + ([qtable(K2_CHROMA, quality)] if nch == 3 else [])
    for i, t in enumerate(tables):
        out += _segment(0xdb, bytes([i]) + bytes(t[n] for n in ZIGZAG))
    out += _segment(0xc0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([nch]) +
                    b"".join(bytes([c + 1, 0x11, min(c, 1)]) for c in range(nch)))
    for i, (dc, ac) in enumerate([(DC_LUMA, AC_LUMA), (DC_CHROMA, AC_CHROMA)][:1 if nch == 1 else 2]):
        out += _segment(0xc4, bytes([0x00 | i]) + bytes(dc[0]) + bytes(dc[1]))
        out += _segment(0xc4, bytes([0x10 | i]) + bytes(ac[0]) + bytes(ac[1]))
    out += _segment(0xdd, ((w + 7) // 8).to_bytes(2, "big"))
    out += _segment(0xda, bytes([nch]) + b"".join(bytes([c + 1, 0x11 * min(c, 1)]) for c in range(nch)) + bytes([0, 63, 0]))
    return out


def assemble(w, h, nch, quality, intervals):
    out = bytearray(headers(w, h, nch, quality))
    for k, iv in enumerate(intervals):
        if k:
            out += bytes([0xff, 0xd0 + (k - 1) % 8])
        out += iv
    return bytes(out + b"\xff\xd9")


def encode(img, quality, only=None):
    """img: (h, w) or (h, w, 3) uint8.  only: the intervals to encode (default all; then .file is None)"""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim in (2, 3)
    h, w = img.shape[:2]
    nch = 1 if img.ndim == 2 else 3
    t = {"dc": set(), "ac": set(), "zrl": 0, "no_eob": 0, "stuffed": 0}
    ks = range((h + 7) // 8) if only is None else only
    intervals = [encode_interval(img[8 * k:8 * k + 8], quality, t) for k in ks]
    tables = [qtable(K1_LUMA, quality)] + ([qtable(K2_CHROMA, quality)] if nch == 3 else [])
    return Encoded(assemble(w, h, nch, quality, intervals) if only is None else None, intervals,
                   Trace(t["dc"], t["ac"], t["zrl"], t["no_eob"], t["stuffed"]), tables)


def parse_segments(data):
    """the marker segments in front of the scan: {'dqt': {id: [64 natural order]}, 'dht': {(class, id): (bits, vals)},
    'sof0': (precision, h, w, [(id, sampling, tq)]), 'dri': n, 'sos': ([(id, tables)], ss, se, ahal), 'app0': bytes, 'scan': offset}"""
    assert data[:2] == b"\xff\xd8"
    out = {"dqt": {}, "dht": {}}
    p = 2
    while True:
        assert data[p] == 0xff, p
        m = data[p + 1]
        n = int.from_bytes(data[p + 2:p + 4], "big")
        body = data[p + 4:p + 2 + n]
        p += 2 + n
        if m == 0xdb:
            while body:
                assert body[0] >> 4 == 0                                    # 8-bit entries
                t = [0] * 64
                for k in range(64):
                    t[ZIGZAG[k]] = body[1 + k]
                out["dqt"][body[0] & 15] = t
                body = body[65:]
        elif m == 0xc4:
            while body:
                bits = list(body[1:17])
                out["dht"][(body[0] >> 4, body[0] & 15)] = (bits, list(body[17:17 + sum(bits)]))
                body = body[17 + sum(bits):]
        elif m == 0xc0:
            nc = body[5]
            out["sof0"] = (body[0], int.from_bytes(body[1:3], "big"), int.from_bytes(body[3:5], "big"),
                           [(body[6 + 3 * c], body[7 + 3 * c], body[8 + 3 * c]) for c in range(nc)])
        elif m == 0xdd:
            out["dri"] = int.from_bytes(body[:2], "big")
        elif m == 0xe0:
            out["app0"] = bytes(body)
        elif m == 0xda:
            nc = body[0]
            out["sos"] = ([(body[1 + 2 * c], body[2 + 2 * c]) for c in range(nc)], body[1 + 2 * nc], body[2 + 2 * nc], body[3 + 2 * nc])
            out["scan"] = p
            return out
        else:
            assert 0xe1 <= m <= 0xef or m == 0xfe, "marker %02x" % m         # APPn / COM of other writers


# ---- test images (seeded; shared by the CPU and the GPU tests so that both see the same restated bytes) ------------------------
def noise(h, w, nch, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w) if nch == 1 else (h, w, 3), dtype=np.uint8)


def scene(h, w, nch, seed):
    """smooth, with noise of sigma 4"""
    y, x = np.mgrid[0:h, 0:w]
    base = 128 + 70 * np.sin(x / 23.0) * np.cos(y / 31.0) + 30 * np.sin((x + y) / 7.0)
    if nch == 3:
        base = np.stack([base, np.roll(base, 11, 1), 255 - base], -1)
    return np.clip(base + np.random.default_rng(seed).normal(0, 4, base.shape), 0, 255).astype(np.uint8)


def extremes(h, w, nch=1, seed=0):
    """8 x 8 blocks in turn all 0, all 255, and 0 in the left / 255 in the right half"""
    by, bx = np.mgrid[0:h, 0:w]
    kind = ((by // 8) * ((w + 7) // 8) + bx // 8) % 3
    return np.where(kind == 0, 0, np.where(kind == 1, 255, np.where(bx % 8 < 4, 0, 255))).astype(np.uint8)


def checker(h, w, nch=1, seed=0):
    y, x = np.mgrid[0:h, 0:w]
    return (((x + y) & 1) * 255).astype(np.uint8)


def flat(h, w, nch, seed):
    """every 8 x 8 block (and channel) one value of its own"""
    small = np.random.default_rng(seed).integers(0, 256, ((h + 7) // 8, (w + 7) // 8) if nch == 1 else ((h + 7) // 8, (w + 7) // 8, 3), dtype=np.uint8)
    return np.ascontiguousarray(np.repeat(np.repeat(small, 8, 0), 8, 1)[:h, :w])


# (name, maker, w, h, nch, quality): the smallest shapes at which the coder can go wrong -- one block, one pixel, padding on both
# axes, 65 blocks an interval (a second round with a carried DC term and bit position), 10 intervals (RST7 -> RST0), RGB with
# padding, RGB of 66 blocks an interval (an MCU straddles the rounds) -- with the contents that reach the coder's edges
CASES = [
    ("grey_8x8_noise_q50", noise, 8, 8, 1, 50),
    ("grey_1x1_noise_q50", noise, 1, 1, 1, 50),
    ("grey_9x7_noise_q100", noise, 9, 7, 1, 100),
    ("grey_520x24_scene_q90", scene, 520, 24, 1, 90),
    ("grey_520x24_noise_q100", noise, 520, 24, 1, 100),
    ("grey_520x24_extremes_q100", extremes, 520, 24, 1, 100),
    ("grey_520x24_checker_q12", checker, 520, 24, 1, 12),
    ("grey_16x80_noise_q1", noise, 16, 80, 1, 1),
    ("rgb_13x67_noise_q50", noise, 13, 67, 3, 50),
    ("rgb_176x8_scene_q100", scene, 176, 8, 3, 100),
    ("rgb_176x8_noise_q100", noise, 176, 8, 3, 100),
    ("rgb_176x8_noise_q1", noise, 176, 8, 3, 1),
    ("rgb_40x16_flat_q50", flat, 40, 16, 3, 50),
]


def case_image(name):
    for k, (n, make, w, h, nch, q) in enumerate(CASES):
        if n == name:
            return make(h, w, nch, 100 + k), q
    raise KeyError(name)


def assert_case_preconditions(name, trace):
    """what a case is there for, asked of the restatement's trace so that the fixture cannot go soft"""
    if "extremes" in name:
        assert 11 in trace.dc_categories and any(size == 10 for _, size in trace.ac_symbols), (trace.dc_categories, trace.ac_symbols)
    if "checker" in name:
        assert trace.zrl >= 1 and trace.no_eob >= 1, (trace.zrl, trace.no_eob)
    if "flat" in name:
        assert not trace.ac_symbols and trace.zrl == 0 and trace.no_eob == 0
    if "noise_q100" in name:
        assert trace.stuffed >= 1
