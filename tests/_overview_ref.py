"""numpy restatement of the overview pyramid (include/oip_c.h: oip_halve_u16, oip_overview_levels) and a reader of every
directory of a classic or BigTIFF file of 16-bit chunky strips (tests/_tiff.py reads the first directory only; its LZW decoder
is used here).  Tests only.

Level k >= 1 of an image has ceil(w / 2) x ceil(h / 2) of level k - 1's pixels; a sample is the mean of the up-to-four samples
of its 2 x 2 block of level k - 1 that lie inside it and are >= valid_min: (S + n // 2) // n, or 0 where n == 0."""
import struct

import numpy as np

import _tiff


def halve(img, valid_min=1, spp=1):
    """one level: (h, w * spp) uint16 -> (ceil(h / 2), ceil(w / 2) * spp) uint16"""
    a = np.asarray(img)
    h = a.shape[0]
    x = a.reshape(h, -1, spp).astype(np.int64)
    w = x.shape[1]
    H, W = (h + 1) // 2, (w + 1) // 2
    v = np.zeros((2 * H, 2 * W, spp), np.int64)
    ok = np.zeros((2 * H, 2 * W, spp), bool)
    ok[:h, :w] = x >= valid_min                                # samples outside the level never count
    v[:h, :w] = x
    v[~ok] = 0
    S = v.reshape(H, 2, W, 2, spp).sum(axis=(1, 3))
    n = ok.reshape(H, 2, W, 2, spp).sum(axis=(1, 3))
    out = np.where(n == 0, 0, (S + n // 2) // np.maximum(n, 1))
    return out.astype(np.uint16).reshape(H, W * spp)


def pyramid(img, levels, valid_min=1, spp=1):
    """[level 1, ..., level `levels`], each from the one before"""
    out, cur = [], np.asarray(img)
    for _ in range(levels):
        cur = halve(cur, valid_min, spp)
        out.append(cur)
    return out


def default_levels(w, h):
    """the smallest n >= 1 with ceil(w / 2^n) <= 256 and ceil(h / 2^n) <= 256, at most 16"""
    n = 1
    while n < 16 and (-(-w // (1 << n)) > 256 or -(-h // (1 << n)) > 256):
        n += 1
    return n


def read_tiff_dirs(path):
    """every directory of the file, in chain order: ([{"img", "tags", "offset", "next"}], big).  img: (h, w) or (h, w, spp)
    uint16; tags: id -> list of values; offset: where the directory lies; next: the offset it chains to (0 in the last)"""
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
        rps = tags[278][0]
        assert len(tags[273]) == len(tags[279]) == -(-h // rps)
        strips = [buf[o:o + c] for o, c in zip(tags[273], tags[279])]
        assert all(o + c <= len(buf) for o, c in zip(tags[273], tags[279]))
        if tags[259][0] == 5:
            strips = [_tiff.lzw_decode(st) for st in strips]
        for k, st in enumerate(strips):
            assert len(st) == min(rps, h - k * rps) * w * spp * 2, "strip %d has the wrong size" % k
        img = np.frombuffer(b"".join(strips), np.uint16).reshape(h, w, spp).copy()
        if tags.get(317, [1])[0] == 2:
            img = np.cumsum(img.astype(np.uint32), axis=1).astype(np.uint16)
        dirs.append({"img": img.reshape(h, w) if spp == 1 else img, "tags": tags, "offset": ifd, "next": nxt})
        ifd = nxt
    return dirs, big


def assert_is_pyramid(path, want, spp, big=None, compression=None):
    """the file's directories are exactly the levels `want` ((h, w * spp) arrays): pixels, tag 254 = 1 in each, a chain that
    ends in 0"""
    dirs, is_big = read_tiff_dirs(path)
    assert len(dirs) == len(want), (len(dirs), len(want))
    if big is not None:
        assert is_big == big
    for k, (d, lv) in enumerate(zip(dirs, want)):
        assert d["tags"].get(254) == [1], (k, d["tags"].get(254))
        assert d["tags"].get(277, [1])[0] == spp
        if compression is not None:
            assert d["tags"][259] == [compression], (k, d["tags"][259])
        assert d["img"].reshape(d["img"].shape[0], -1).shape == lv.shape, (k, d["img"].shape, lv.shape)
        assert np.array_equal(d["img"].reshape(lv.shape), lv), "level %d differs" % (k + 1)
        assert (d["next"] == 0) == (k == len(dirs) - 1)
    return dirs
