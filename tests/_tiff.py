"""Minimal reader / writer for little-endian TIFF / BigTIFF with 16-bit chunky strips, uncompressed or LZW
with predictor 1 or 2 (what csrc/oip_tiff.hpp, cv::imwrite and GDAL's GTiff driver write).  Tests only: an
implementation of TIFF 6.0 section 13 (LZW) and section 14 (predictor) independent of the C++ codec."""
import struct

import numpy as np


def lzw_decode(data: bytes) -> bytes:
    """TIFF LZW: MSB-first 9..12-bit codes, Clear 256, EOI 257, early change"""
    table = [bytes([i]) for i in range(256)] + [b"", b""]
    out = bytearray()
    width, acc, nbits, old = 9, 0, 0, None
    for byte in data:
        acc = (acc << 8) | byte
        nbits += 8
        while nbits >= width:
            code = (acc >> (nbits - width)) & ((1 << width) - 1)
            nbits -= width
            if code == 257:
                return bytes(out)
            if code == 256:
                table = table[:258]
                width, old = 9, None
                continue
            if old is None:
                entry = table[code]
            elif code < len(table):
                entry = table[code]
                table.append(old + entry[:1])
            else:
                assert code == len(table), "corrupt LZW stream"
                entry = old + old[:1]
                table.append(entry)
            out += entry
            old = entry
            if len(table) >= (1 << width) - 1 and width < 12:
                width += 1
    return bytes(out)


def lzw_encode(data: bytes) -> bytes:
    codes = {bytes([i]): i for i in range(256)}
    out, acc, nbits = bytearray(), 0, 0
    width, nxt = 9, 258

    def put(code, w):
        nonlocal acc, nbits
        acc = (acc << w) | code
        nbits += w
        while nbits >= 8:
            out.append((acc >> (nbits - 8)) & 0xFF)
            nbits -= 8

    put(256, width)
    ent = b""
    for b in data:
        cur = ent + bytes([b])
        if cur in codes:
            ent = cur
            continue
        put(codes[ent], width)
        codes[cur] = nxt
        nxt += 1
        ent = bytes([b])
        if nxt == 4094:
            put(256, width)
            codes = {bytes([i]): i for i in range(256)}
            width, nxt = 9, 258
        elif nxt == (1 << width) and width < 12:
            width += 1
    if ent:
        put(codes[ent], width)
        nxt += 1
        if nxt == 4094:
            put(256, width)
            width = 9
        elif nxt == (1 << width) and width < 12:
            width += 1
    put(257, width)
    if nbits:
        out.append((acc << (8 - nbits)) & 0xFF)
    return bytes(out)


class LzwTrace:
    """What lzw_trace saw: `stream` (the encoded bytes), `codes` -- one (value, width, kwkwk, pos) per emitted code, ClearCode and
    EndOfInformation included; kwkwk: the value is the entry the previous miss assigned, so the decoder meets code == its own next;
    pos: index of the input byte whose miss sent the code, len(data) for what goes out after the last byte -- `clears` (indices
    into codes), `end_next` (next after the final code's increment, before a ClearCode that increment may cause), `eoi_width`,
    `last_byte` (what the LAST input byte caused inside the loop: "clear", "widen10" / "widen11" / "widen12" or None) and
    `max_next` (the highest value next reached: clear_at, where a variant's threshold was really met)."""

    def __init__(self):
        self.stream, self.codes, self.clears = b"", [], []
        self.end_next = self.eoi_width = self.max_next = 0
        self.last_byte = None

    def kwkwk_values(self):
        return {v for v, _, k, _ in self.codes if k}

    def last_data_code(self):
        """the last code that is neither ClearCode nor EndOfInformation"""
        return [c for c in self.codes if c[0] not in (256, 257)][-1]


def lzw_trace(data: bytes, clear_at=4094, extra_clear_every=0, double_clear=False, leading_clear=True, trailing_bytes=0) -> LzwTrace:
    """The dictionary coder of lzw_encode once more, recording the events of the stream (LzwTrace).  With the defaults the stream is
    lzw_encode's (libtiff's).  The knobs write streams that are legal TIFF LZW but that libtiff's encoder never produces:
    clear_at -- the value of next at which ClearCode is sent (4094 libtiff; 4095; 4096: the table really full, TIFF 6.0's text);
    extra_clear_every=N -- a ClearCode after every N-th assigned entry as well, in the middle of a half-filled table;
    double_clear -- every ClearCode twice; leading_clear=False -- the strip does not start with one; trailing_bytes=k -- k junk
    bytes after EndOfInformation."""
    assert clear_at in (4094, 4095, 4096)
    t = LzwTrace()
    codes = {bytes([i]): i for i in range(256)}
    out, acc, nbits = bytearray(), 0, 0
    width, nxt, assigned, fresh = 9, 258, 0, None              # fresh: the entry the previous miss assigned

    def put(code, w, kwkwk, pos):
        nonlocal acc, nbits
        t.codes.append((code, w, kwkwk, pos))
        acc = (acc << w) | code
        nbits += w
        while nbits >= 8:
            out.append((acc >> (nbits - 8)) & 0xFF)
            nbits -= 8

    def clear(pos):
        nonlocal codes, width, nxt, fresh
        for _ in range(2 if double_clear else 1):
            t.clears.append(len(t.codes))
            put(256, width, False, pos)
            width = 9
        codes = {bytes([i]): i for i in range(256)}
        nxt, fresh = 258, None

    if leading_clear:
        clear(0)
    ent = b""
    for i, b in enumerate(data):
        cur = ent + bytes([b])
        t.last_byte = None
        if cur in codes:
            ent = cur
            continue
        put(codes[ent], width, codes[ent] == fresh, i)
        codes[cur] = fresh = nxt
        nxt += 1
        assigned += 1
        t.max_next = max(t.max_next, nxt)
        ent = bytes([b])
        if nxt == clear_at:
            clear(i)
            t.last_byte = "clear"
        elif nxt == (1 << width) and width < 12:
            width += 1
            t.last_byte = "widen%d" % width
        if extra_clear_every and assigned % extra_clear_every == 0 and nxt != 258:
            clear(i)
    if ent:
        put(codes[ent], width, codes[ent] == fresh, len(data))
        nxt += 1
        t.max_next = max(t.max_next, nxt)
        t.end_next = nxt
        if nxt == clear_at:
            clear(len(data))
        elif nxt == (1 << width) and width < 12:
            width += 1
    t.eoi_width = width
    put(257, width, False, len(data))
    if nbits:
        out.append((acc << (8 - nbits)) & 0xFF)
    t.stream = bytes(out) + b"\xa5" * trailing_bytes
    return t


def lzw_encode_variant(data: bytes, **knobs) -> bytes:
    """a foreign-but-legal stream for `data` (the knobs of lzw_trace)"""
    return lzw_trace(data, **knobs).stream


def read_tags(path):
    """directory only (no pixel decoding)"""
    return read_tiff_u16(path, tags_only=True)[1]


def read_tiff_u16(path, tags_only=False):
    with open(path, "rb") as f:
        buf = f.read()
    assert buf[:2] == b"II"
    ver = struct.unpack_from("<H", buf, 2)[0]
    big = ver == 43
    assert ver in (42, 43)
    if big:
        assert struct.unpack_from("<HH", buf, 4) == (8, 0)
        ifd = struct.unpack_from("<Q", buf, 8)[0]
        n = struct.unpack_from("<Q", buf, ifd)[0]
        ent, esz, osz, ofmt = ifd + 8, 20, 8, "<Q"
    else:
        ifd = struct.unpack_from("<I", buf, 4)[0]
        n = struct.unpack_from("<H", buf, ifd)[0]
        ent, esz, osz, ofmt = ifd + 2, 12, 4, "<I"
    tsize = {3: 2, 4: 4, 16: 8}
    tfmt = {3: "<H", 4: "<I", 16: "<Q"}
    tags = {}
    for i in range(n):
        o = ent + i * esz
        tid, typ = struct.unpack_from("<HH", buf, o)
        cnt = struct.unpack_from(ofmt, buf, o + 4)[0]
        voff = o + 4 + osz
        if cnt * tsize[typ] > osz:
            voff = struct.unpack_from(ofmt, buf, voff)[0]
        tags[tid] = [struct.unpack_from(tfmt[typ], buf, voff + k * tsize[typ])[0] for k in range(cnt)]
    if tags_only:
        return None, tags, big
    w, h, spp = tags[256][0], tags[257][0], tags.get(277, [1])[0]
    assert tags[258] == [16] * spp and tags[259][0] in (1, 5) and tags.get(284, [1]) == [1] and tags.get(339, [1] * spp) == [1] * spp
    strips = [buf[o:o + c] for o, c in zip(tags[273], tags[279])]
    if tags[259][0] == 5:
        strips = [lzw_decode(st) for st in strips]
    data = b"".join(strips)
    img = np.frombuffer(data, np.uint16).reshape(h, w, spp).copy()
    if tags.get(317, [1])[0] == 2:
        img = np.cumsum(img.astype(np.uint32), axis=1).astype(np.uint16)          # per channel along the row, mod 2^16
    if spp == 1:
        img = img.reshape(h, w)
    return img, tags, big


def write_tiff_u16(path, arr, lzw=False, predictor=1, rows_per_strip=None):
    """Minimal classic-TIFF writer (chunky; uncompressed single strip, or LZW strips with predictor 1 / 2) for
    test inputs; samples in file order."""
    import struct
    a = np.ascontiguousarray(arr, dtype="<u2")
    if a.ndim == 2:
        a = a[:, :, None]
    h, w, s = a.shape
    if lzw:
        return _write_tiff_lzw(path, a, predictor, rows_per_strip or h)
    data = a.tobytes()
    extra = b""
    off_extra = 8 + len(data)

    def arr_tag(vals):
        nonlocal extra
        o = off_extra + len(extra)
        extra += struct.pack("<%dH" % len(vals), *vals)
        return o

    tags = [(256, 4, 1, w), (257, 4, 1, h)]
    tags.append((258, 3, s, arr_tag([16] * s) if s > 2 else 16 | (16 << 16) * (s == 2)))
    tags += [(259, 3, 1, 1), (262, 3, 1, 2 if s == 4 else 1), (273, 4, 1, 8), (277, 3, 1, s), (278, 4, 1, h),
             (279, 4, 1, len(data)), (284, 3, 1, 1)]
    if s == 4:
        tags.append((338, 3, 1, 2))
    tags.append((339, 3, s, arr_tag([1] * s) if s > 2 else 1 | (1 << 16) * (s == 2)))
    if len(extra) & 1:
        extra += b"\0"
    ifd = off_extra + len(extra)
    with open(path, "wb") as f:
        f.write(b"II" + struct.pack("<HI", 42, ifd))
        f.write(data)
        f.write(extra)
        f.write(struct.pack("<H", len(tags)))
        for t in tags:
            f.write(struct.pack("<HHII", *t))
        f.write(struct.pack("<I", 0))


def write_tiff_lzw_strips(path, strips, shape, predictor, rows_per_strip):
    """a classic TIFF around LZW strips somebody else encoded; shape: (rows, width, samples per pixel)"""
    _write_tiff_lzw(path, np.zeros(shape, dtype="<u2"), predictor, rows_per_strip, strips=list(strips))


def _write_tiff_lzw(path, a, predictor, rps, strips=None):
    h, w, s = a.shape
    if strips is not None:
        assert len(strips) == (h + rps - 1) // rps
    elif predictor == 2:
        d = a.astype(np.int64)
        d[:, 1:, :] = d[:, 1:, :] - a[:, :-1, :].astype(np.int64)
        a = (d & 0xFFFF).astype("<u2")
    if strips is None:
        strips = [lzw_encode(a[r:r + rps].tobytes()) for r in range(0, h, rps)]
    body, offs = b"", []
    for st in strips:
        if len(body) & 1:
            body += b"\0"
        offs.append(8 + len(body))
        body += st
    if len(body) & 1:
        body += b"\0"
    extra = b""
    base = 8 + len(body)

    def arr_tag(vals, fmt="H"):
        nonlocal extra
        o = base + len(extra)
        extra += struct.pack("<%d%s" % (len(vals), fmt), *vals)
        if len(extra) & 1:
            extra += b"\0"
        return o

    n = len(strips)
    tags = [(256, 4, 1, w), (257, 4, 1, h),
            (258, 3, s, arr_tag([16] * s) if s > 2 else 16 | (16 << 16) * (s == 2)),
            (259, 3, 1, 5), (262, 3, 1, 2 if s == 4 else 1),
            (273, 4, n, arr_tag(offs, "I") if n > 1 else offs[0]), (277, 3, 1, s), (278, 4, 1, rps),
            (279, 4, n, arr_tag([len(st) for st in strips], "I") if n > 1 else len(strips[0])), (284, 3, 1, 1),
            (317, 3, 1, predictor)]
    if s == 4:
        tags.append((338, 3, 1, 2))
    tags.append((339, 3, s, arr_tag([1] * s) if s > 2 else 1 | (1 << 16) * (s == 2)))
    ifd = base + len(extra)
    with open(path, "wb") as f:
        f.write(b"II" + struct.pack("<HI", 42, ifd))
        f.write(body)
        f.write(extra)
        f.write(struct.pack("<H", len(tags)))
        for t in tags:
            f.write(struct.pack("<HHII", *t))
        f.write(struct.pack("<I", 0))


def write_raw_tiff(path, tags, payload=b"", big=False, magic=None, order=b"II", ifd_at=None, count=None):
    """A little-endian TIFF / BigTIFF put together entry by entry, for files that are wrong in one chosen way.  `payload` lies right
    behind the header (offset 8, BigTIFF 16), then the out-of-line values, then the directory.  tags: {id: (type, [values])} -- the
    values go inline where they fit the entry -- or {id: (type, count, field)}: the entry as given, whatever it says.  magic, order,
    ifd_at and count (of entries) overwrite what the header and the directory would say."""
    osz, ofmt = (8, "<Q") if big else (4, "<I")
    tfmt = {3: "H", 4: "I", 16: "Q"}
    base = (16 if big else 8) + len(payload)
    extra, entries = b"", []
    for tid in sorted(tags):
        t = tags[tid]
        if len(t) == 3:
            entries.append((tid, t[0], t[1], struct.pack(ofmt, t[2])))
            continue
        raw = struct.pack("<%d%s" % (len(t[1]), tfmt[t[0]]), *t[1])
        if len(raw) <= osz:
            field = raw.ljust(osz, b"\0")
        else:
            extra += b"\0" * (len(extra) & 1)
            field = struct.pack(ofmt, base + len(extra))
            extra += raw
        entries.append((tid, t[0], len(t[1]), field))
    extra += b"\0" * (len(extra) & 1)
    ifd = base + len(extra) if ifd_at is None else ifd_at
    n = len(entries) if count is None else count
    with open(path, "wb") as f:
        if big:
            f.write(order + struct.pack("<HHHQ", 43 if magic is None else magic, 8, 0, ifd))
        else:
            f.write(order + struct.pack("<HI", 42 if magic is None else magic, ifd))
        f.write(payload)
        f.write(extra)
        f.write(struct.pack("<Q" if big else "<H", n))
        for tid, typ, cnt, field in entries:
            f.write(struct.pack("<HH", tid, typ) + struct.pack(ofmt, cnt) + field)
        f.write(struct.pack(ofmt, 0))
