"""A classic little-endian TIFF of 16-bit samples around compressed strips or tiles, written with zlib: the Deflate files another
program makes (COMPRESS=DEFLATE, rio-cogeo's default profile).  Nothing of the product is used."""
import struct
import zlib

import numpy as np


def predict2(block):
    """TIFF predictor 2 on a (rows, width, spp) block of u16: each sample minus the same channel of the pixel before, mod 2^16"""
    d = block.astype(np.int64)
    d[:, 1:, :] = d[:, 1:, :] - block[:, :-1, :].astype(np.int64)
    return (d & 0xFFFF).astype("<u2")


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
    return c.compress(data) + c.flush()


def blocks_of(img, spp, rps=None, tile=None):
    """the (rows, width, spp) blocks of the file in file order: strips of rps rows, or zero-padded TW x TL tiles, row-major"""
    a = np.asarray(img)
    h = a.shape[0]
    x = a.reshape(h, -1, spp)
    w = x.shape[1]
    if tile is None:
        rps = rps or h
        return [x[r:r + rps] for r in range(0, h, rps)]
    TW, TL = tile
    tx, ty = -(-w // TW), -(-h // TL)
    pad = np.zeros((ty * TL, tx * TW, spp), np.uint16)
    pad[:h, :w] = x
    return [pad[j * TL:(j + 1) * TL, i * TW:(i + 1) * TW] for j in range(ty) for i in range(tx)]


def streams_of(img, spp, predictor=2, rps=None, tile=None, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    return [deflate((predict2(b) if predictor == 2 else b.astype("<u2")).tobytes(), level, strategy) for b in blocks_of(img, spp, rps, tile)]


def write(path, img, spp, predictor=2, rps=None, tile=None, level=6, compression=8, streams=None, strategy=zlib.Z_DEFAULT_STRATEGY,
          tags_override=None):
    """img: (h, w * spp) u16.  streams: the encoded strips / tiles where somebody else made them (a corrupt one among them, say).
    tags_override: {tag: (type, count, value)} replaces or adds directory entries (value None drops the tag)."""
    a = np.asarray(img)
    h = a.shape[0]
    w = a.reshape(h, -1, spp).shape[1]
    if tile is None:
        rps = rps or h
    if streams is None:
        streams = streams_of(a, spp, predictor, rps, tile, level, strategy)
    body, offs = bytearray(), []
    for st in streams:
        if len(body) & 1:
            body += b"\0"
        offs.append(8 + len(body))
        body += st
    if len(body) & 1:
        body += b"\0"
    extra = b""
    base = 8 + len(body)

    def arr(vals, fmt):
        nonlocal extra
        o = base + len(extra)
        extra += struct.pack("<%d%s" % (len(vals), fmt), *vals)
        if len(extra) & 1:
            extra += b"\0"
        return o

    n = len(streams)
    lens = [len(s) for s in streams]
    tags = {256: (4, 1, w), 257: (4, 1, h), 258: (3, spp, arr([16] * spp, "H") if spp > 2 else 16 | (16 << 16) * (spp == 2)),
            259: (3, 1, compression), 262: (3, 1, 2 if spp == 4 else 1), 277: (3, 1, spp), 284: (3, 1, 1), 317: (3, 1, predictor),
            339: (3, spp, arr([1] * spp, "H") if spp > 2 else 1 | (1 << 16) * (spp == 2))}
    if tile is None:
        tags.update({273: (4, n, arr(offs, "I") if n > 1 else offs[0]), 278: (4, 1, rps), 279: (4, n, arr(lens, "I") if n > 1 else lens[0])})
    else:
        tags.update({322: (4, 1, tile[0]), 323: (4, 1, tile[1]), 324: (4, n, arr(offs, "I") if n > 1 else offs[0]),
                     325: (4, n, arr(lens, "I") if n > 1 else lens[0])})
    if spp == 4:
        tags[338] = (3, 1, 2)
    for k, v in (tags_override or {}).items():
        if v is None:
            tags.pop(k, None)
        else:
            tags[k] = v
    ifd = base + len(extra)
    with open(path, "wb") as f:
        f.write(b"II" + struct.pack("<HI", 42, ifd))
        f.write(body)
        f.write(extra)
        f.write(struct.pack("<H", len(tags)))
        for k in sorted(tags):
            f.write(struct.pack("<HHII", k, *tags[k]))
        f.write(struct.pack("<I", 0))
    return offs, lens
