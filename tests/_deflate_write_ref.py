"""A reader of the Deflate TIFFs the project writes, independent of the C++ codec: every directory of a little-endian TIFF / BigTIFF
of 16-bit chunky samples in strips or tiles, compression 8 (each strip or tile inflated with Python's zlib) or 1, predictor 2 undone
per channel along each row.  And what the tests of the encoder share: the stored bound, the predictor-2 bytes of an image's strips,
the blocky and noise fixtures of the ratio conditions.  Tests only."""
import struct
import zlib

import numpy as np

import _cog_ref as cog
import _deflate_tiff as T


def stored_bound(n):
    """all of a stream in stored blocks of at most 65535 bytes: 2 header + 5 a block + 4 trailer"""
    return n + 5 * -(-n // 65535) + 6 if n else 11


def huffman_only(data):
    """the size of zlib's stream with Z_HUFFMAN_ONLY, made the way tests/_deflate_tiff.py makes its streams"""
    return len(T.deflate(data, 6, zlib.Z_HUFFMAN_ONLY))


def strip_bytes(img, spp, rps=None, tile=None):
    """the predictor-2 byte streams of an image's strips (rps rows) or zero-padded tiles, in file order"""
    return [T.predict2(b).tobytes() for b in T.blocks_of(img, spp, rps, tile)]


def blocks(h, w, spp, seed, b=8):
    """tests/test_gpu_cog_cli.py::_blocks: (h, w * spp), b x b blocks of 12-bit noise with 30 % no data and a few 65535"""
    rng = np.random.default_rng(seed)
    x = rng.integers(1, 4096, (-(-h // b), -(-w // b), spp)).astype(np.uint16)
    x[rng.random(x.shape) < 0.30] = 0
    x[rng.random(x.shape) < 0.02] = 65535
    return np.ascontiguousarray(np.repeat(np.repeat(x, b, axis=0), b, axis=1)[:h, :w]).reshape(h, w * spp)


def noise12(h, w, spp, seed):
    return np.random.default_rng(seed).integers(64, 4096, (h, w * spp)).astype(np.uint16)


def ratio_fixtures():
    """{name: (streams' input bytes, factor)}: the total of the encoder's streams must be <= factor x the total of zlib's
    Z_HUFFMAN_ONLY streams"""
    n4, n1 = noise12(512, 512, 4, 21), noise12(600, 1000, 1, 22)
    m, p = blocks(900, 700, 4, 1, 28), blocks(600, 1000, 1, 2)
    return {
        "noise_4_strips16": (strip_bytes(n4, 4, rps=16), 1.02),
        "noise_4_tile512": (strip_bytes(n4, 4, tile=(512, 512)), 1.02),
        "noise_1_strips32": (strip_bytes(n1, 1, rps=32), 1.02),
        "blocky_4_strips11": (strip_bytes(m, 4, rps=11), 0.5),
        "blocky_4_tiles128": (strip_bytes(m, 4, tile=(128, 128)), 0.5),
        "blocky_1_strips32": (strip_bytes(p, 1, rps=32), 0.5),
        "blocky_1_tiles256": (strip_bytes(p, 1, tile=(256, 256)), 0.5),
    }


def read_dirs(path):
    """every directory in chain order: ([{"img", "chunks", "streams", "tags", "offset", "next", "tiled"}], big).  img: (h, w * spp)
    uint16; chunks: (n, rows, width * spp) as stored, padding of tiles included; streams: the compressed bytes"""
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
        assert tags[258] == [16] * spp and tags.get(284, [1]) == [1] and tags.get(339, [1] * spp) == [1] * spp
        comp, pred = tags[259][0], tags.get(317, [1])[0]
        assert comp in (1, 8), comp
        tiled = 322 in tags
        if tiled:
            assert 273 not in tags and 278 not in tags and 279 not in tags, "strip tags in a tiled directory"
            cw, ch = tags[322][0], tags[323][0]
            offs, lens = tags[324], tags[325]
            nchunks = -(-w // cw) * -(-h // ch)
            rows = [ch] * nchunks
        else:
            cw, ch = w, tags[278][0]
            offs, lens = tags[273], tags[279]
            nchunks = -(-h // ch)
            rows = [min(ch, h - k * ch) for k in range(nchunks)]
        assert len(offs) == len(lens) == nchunks
        assert all(o % 2 == 0 and o + c <= len(buf) for o, c in zip(offs, lens)), "a strip or tile at an odd offset or past the file"
        streams = [buf[o:o + c] for o, c in zip(offs, lens)]
        raw = []
        for k, s in enumerate(streams):
            if comp == 8:
                z = zlib.decompressobj()
                s = z.decompress(s)
                assert z.eof and not z.unused_data, "strip or tile %d: zlib wants more, or less" % k
            assert len(s) == rows[k] * cw * spp * 2, "strip or tile %d has the wrong size" % k
            a = np.frombuffer(s, "<u2").reshape(rows[k], cw, spp)
            if pred == 2:
                a = np.cumsum(a.astype(np.uint32), axis=1).astype(np.uint16)
            raw.append(a.reshape(rows[k], cw * spp))
        img = cog.untile(np.stack(raw), w, h, spp, cw, ch) if tiled else np.concatenate(raw, axis=0)
        dirs.append({"img": img, "chunks": raw, "streams": streams, "tags": tags, "offset": ifd, "next": nxt, "tiled": tiled})
        ifd = nxt
    return dirs, big


def assert_deflate_tags(d, spp):
    t = d["tags"]
    assert t[259] == [8] and t.get(317) == [2], (t[259], t.get(317))
    assert t.get(277, [1])[0] == spp and t[262] == [2 if spp == 4 else 1] and (t.get(338) == [2]) == (spp == 4)


def assert_is_deflate_cog(path, levels, spp, tile, big=None):
    """tests/_cog_ref.py::assert_is_cog for compression 8: the file's directories are exactly `levels`, every tile a zlib stream
    with the replicated edge as padding, tags 259 = 8 and 317 = 2, every directory and table ahead of every tile"""
    dirs, is_big = read_dirs(path)
    assert len(dirs) == len(levels), (len(dirs), len(levels))
    if big is not None:
        assert is_big == big
    first = min(min(d["tags"][324]) for d in dirs)
    for k, (d, lv) in enumerate(zip(dirs, levels)):
        t = d["tags"]
        assert d["tiled"] and t.get(254) == ([1] if k else None), (k, t.get(254))
        assert t[322] == [tile] and t[323] == [tile]
        assert_deflate_tags(d, spp)
        assert d["img"].shape == lv.shape and np.array_equal(d["img"], lv), "level %d differs" % k
        assert np.array_equal(np.stack(d["chunks"]), cog.retile(lv, spp, tile)), "level %d: the padding of a tile is not the replicated edge" % k
        assert d["offset"] < first and (d["next"] == 0) == (k == len(dirs) - 1)
    order = [o for d in dirs for o in d["tags"][324]]
    assert order == sorted(order), "payloads are not in directory and tile order"
    return dirs
