"""numpy restatement of the tile-major form (include/oip_c.h: oip_retile_u16 / oip_untile_u16) and a reader and a small writer
of tiled TIFF / BigTIFF of 16-bit chunky samples, every directory, uncompressed or LZW (through tests/_tiff.py's coders) with
predictor 2 along each row of a tile.  Tests only; independent of the C++ codec.

An image is (h, w * spp) uint16.  Tiles are T x T; the grid has tx = ceil(w / T) by ty = ceil(h / T) tiles, row-major.  Sample
(r, c, ch) of tile (j, i) is image sample (min(j T + r, h - 1), min(i T + c, w - 1), ch): edge tiles replicate the last column
(per channel) and the last line."""
import struct

import numpy as np

import _tiff


def grid(w, h, T):
    return -(-w // T), -(-h // T)


def retile(img, spp, T, tile_row0=0, tile_rows=None, TL=None):
    """(h, w * spp) -> (tile_rows * tx, TL, T * spp): the tiles of tile rows [tile_row0, tile_row0 + tile_rows), T wide and TL
    (default T) long"""
    a = np.asarray(img)
    h = a.shape[0]
    x = a.reshape(h, -1, spp)
    w = x.shape[1]
    TL = TL or T
    tx, ty = -(-w // T), -(-h // TL)
    if tile_rows is None:
        tile_rows = ty - tile_row0
    rows = np.minimum(np.arange(tile_row0 * TL, (tile_row0 + tile_rows) * TL), h - 1)
    cols = np.minimum(np.arange(tx * T), w - 1)
    p = x[rows][:, cols]                                        # (tile_rows * TL, tx * T, spp)
    p = p.reshape(tile_rows, TL, tx, T, spp).transpose(0, 2, 1, 3, 4)
    return np.ascontiguousarray(p).reshape(tile_rows * tx, TL, T * spp)


def untile(tiles, w, h, spp, T, TL=None):
    """the inverse on all tile rows: (ty * tx, TL, T * spp) -> (h, w * spp); the padding is dropped"""
    TL = TL or T
    tx, ty = -(-w // T), -(-h // TL)
    p = np.asarray(tiles).reshape(ty, tx, TL, T, spp).transpose(0, 2, 1, 3, 4).reshape(ty * TL, tx * T, spp)
    return np.ascontiguousarray(p[:h, :w]).reshape(h, w * spp)


def read_tiled_dirs(path):
    """every directory of a tiled file, in chain order: ([{"img", "tiles", "tags", "offset", "next"}], big).  img: (h, w * spp)
    uint16; tiles: (n, TL, TW * spp) as stored, padding included"""
    with open(path, "rb") as f:
        buf = f.read()
    assert buf[:2] == b"II"
    ver = struct.unpack_from("<H", buf, 2)[0]
    assert ver in (42, 43)
    big = ver == 43
    if big:
        assert struct.unpack_from("<HH", buf, 4) == (8, 0)
        ifd = struct.unpack_from("<Q", buf, 8)[0]
        cfmt, csz, esz, osz, ofmt = "<Q", 8, 20, 8, "<Q"
    else:
        ifd = struct.unpack_from("<I", buf, 4)[0]
        cfmt, csz, esz, osz, ofmt = "<H", 2, 12, 4, "<I"
    tsize = {3: 2, 4: 4, 16: 8}
    tfmt = {3: "<H", 4: "<I", 16: "<Q"}
    dirs, seen = [], set()
    while ifd:
        assert ifd not in seen and ifd + csz <= len(buf), "directory chain is broken"
        seen.add(ifd)
        n = struct.unpack_from(cfmt, buf, ifd)[0]
        tags, order = {}, []
        for i in range(n):
            o = ifd + csz + i * esz
            tid, typ = struct.unpack_from("<HH", buf, o)
            cnt = struct.unpack_from(ofmt, buf, o + 4)[0]
            voff = o + 4 + osz
            if cnt * tsize[typ] > osz:
                voff = struct.unpack_from(ofmt, buf, voff)[0]
            tags[tid] = [struct.unpack_from(tfmt[typ], buf, voff + k * tsize[typ])[0] for k in range(cnt)]
            order.append(tid)
        assert order == sorted(order), "tags are not in ascending order"
        nxt = struct.unpack_from(ofmt, buf, ifd + csz + n * esz)[0]
        w, h, spp = tags[256][0], tags[257][0], tags.get(277, [1])[0]
        assert tags[258] == [16] * spp and tags[259][0] in (1, 5) and tags.get(284, [1]) == [1] and tags.get(339, [1] * spp) == [1] * spp
        assert 273 not in tags and 278 not in tags and 279 not in tags, "strip tags in a tiled directory"
        TW, TL = tags[322][0], tags[323][0]
        tx, ty = -(-w // TW), -(-h // TL)
        assert len(tags[324]) == len(tags[325]) == tx * ty
        assert all(o % 2 == 0 and o + c <= len(buf) for o, c in zip(tags[324], tags[325]))
        raw = [buf[o:o + c] for o, c in zip(tags[324], tags[325])]
        if tags[259][0] == 5:
            raw = [_tiff.lzw_decode(t) for t in raw]
        for k, t in enumerate(raw):
            assert len(t) == TW * TL * spp * 2, "tile %d has the wrong size" % k
        tiles = np.frombuffer(b"".join(raw), np.uint16).reshape(tx * ty, TL, TW, spp)
        if tags.get(317, [1])[0] == 2:
            tiles = np.cumsum(tiles.astype(np.uint32), axis=2).astype(np.uint16)     # per channel along each row of a tile
        tiles = tiles.reshape(tx * ty, TL, TW * spp)
        dirs.append({"img": untile(tiles, w, h, spp, TW, TL), "tiles": tiles, "tags": tags, "offset": ifd, "next": nxt})
        ifd = nxt
    return dirs, big


def assert_is_cog(path, levels, spp, T, big=None, compression=None):
    """the file's directories are exactly `levels` ((h, w * spp) arrays, the image first): pixels, the replicated padding of
    every tile, the tags, a chain that ends in 0, and every directory and table ahead of every tile"""
    dirs, is_big = read_tiled_dirs(path)
    assert len(dirs) == len(levels), (len(dirs), len(levels))
    if big is not None:
        assert is_big == big
    first = min(min(d["tags"][324]) for d in dirs)
    for k, (d, lv) in enumerate(zip(dirs, levels)):
        t = d["tags"]
        assert t.get(254) == ([1] if k else None), (k, t.get(254))
        assert t[322] == [T] and t[323] == [T] and t.get(277, [1])[0] == spp
        assert t[262] == [2 if spp == 4 else 1] and (t.get(338) == [2]) == (spp == 4)
        if compression is not None:
            assert t[259] == [compression], (k, t[259])
        assert (t.get(317) == [2]) == (t[259] == [5])
        assert d["img"].shape == lv.shape, (k, d["img"].shape, lv.shape)
        assert np.array_equal(d["img"], lv), "level %d differs" % k
        assert np.array_equal(d["tiles"], retile(lv, spp, T)), "level %d: the padding of a tile is not the replicated edge" % k
        assert d["offset"] < first and (d["next"] == 0) == (k == len(dirs) - 1)
    order = [o for d in dirs for o in d["tags"][324]]
    assert order == sorted(order), "payloads are not in directory and tile order"
    return dirs


def write_tiled_u16(path, img, spp, TW, TL, lzw=True):
    """a classic tiled TIFF of one directory with TW x TL tiles (any positive sizes), LZW with predictor 2 or uncompressed,
    zero padding in the edge tiles: the kind of file another writer makes"""
    a = np.asarray(img)
    h = a.shape[0]
    x = a.reshape(h, -1, spp)
    w = x.shape[1]
    tx, ty = -(-w // TW), -(-h // TL)
    pad = np.zeros((ty * TL, tx * TW, spp), np.uint16)
    pad[:h, :w] = x
    body, offs, lens = b"", [], []
    for j in range(ty):
        for i in range(tx):
            t = pad[j * TL:(j + 1) * TL, i * TW:(i + 1) * TW].astype(np.int64)
            if lzw:
                t[:, 1:] = t[:, 1:] - t[:, :-1].copy()
                enc = _tiff.lzw_encode((t & 0xFFFF).astype("<u2").tobytes())
            else:
                enc = t.astype("<u2").tobytes()
            if len(body) & 1:
                body += b"\0"
            offs.append(8 + len(body))
            lens.append(len(enc))
            body += enc
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

    n = len(offs)
    tags = [(256, 4, 1, w), (257, 4, 1, h), (258, 3, spp, arr([16] * spp, "H") if spp > 2 else 16),
            (259, 3, 1, 5 if lzw else 1), (262, 3, 1, 2 if spp == 4 else 1), (277, 3, 1, spp), (284, 3, 1, 1)]
    if lzw:
        tags.append((317, 3, 1, 2))
    tags += [(322, 4, 1, TW), (323, 4, 1, TL), (324, 4, n, arr(offs, "I") if n > 1 else offs[0]), (325, 4, n, arr(lens, "I") if n > 1 else lens[0])]
    if spp == 4:
        tags.append((338, 3, 1, 2))
    tags.append((339, 3, spp, arr([1] * spp, "H") if spp > 2 else 1))
    ifd = base + len(extra)
    with open(path, "wb") as f:
        f.write(b"II" + struct.pack("<HI", 42, ifd))
        f.write(body)
        f.write(extra)
        f.write(struct.pack("<H", len(tags)))
        for t in tags:
            f.write(struct.pack("<HHII", *t))
        f.write(struct.pack("<I", 0))
