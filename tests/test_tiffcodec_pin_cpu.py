"""CPU: the TIFF codec (csrc/oip_tiff.hpp, csrc/oip_tifftiled.hpp) pinned to what it did before its readers and writers were
folded into one directory reader and one directory emitter: what read_tiff_layout / read_tiff_u16 / read_tiff_u8 say of a set of
small files with one fault each (and of sound files next to them), and the SHA-256 of every file the three writers produce over a
small grid.  tests/cpp/tiffcodec_pin.cpp is the stand-alone program (ASan + UBSan); the two fixtures under tests/golden were
recorded from it by tests/golden/make_tiffcodec_pins.py and are not regenerated."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import _deflate_tiff as DT
import _tiff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def build_program(d):
    exe = os.path.join(str(d), "tiffcodec_pin")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                    "-I" + os.path.join(ROOT, "opticalimageprocessor_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "tiffcodec_pin.cpp"),
                    "-o", exe], check=True)
    return exe


def _codes(codes):
    """LZW codes as a decoder would read them: 9 bits first, wider as its table grows (early change), back to 9 after ClearCode"""
    acc = nbits = 0
    width, nxt, old = 9, 258, False
    out = bytearray()
    for c in codes:
        acc, nbits = (acc << width) | c, nbits + width
        while nbits >= 8:
            out.append((acc >> (nbits - 8)) & 0xFF)
            nbits -= 8
        if c == 256:
            width, nxt, old = 9, 258, False
        elif not old:
            old = True
        else:
            nxt += 1
            if nxt >= (1 << width) - 1 and width < 12:
                width += 1
    if nbits:
        out.append((acc << (8 - nbits)) & 0xFF)
    return bytes(out)


def _pixels(h, w, spp, seed):
    return ((np.arange(h * w * spp, dtype=np.uint64) * 2654435761 + seed >> 11) & 0xFFFF).astype("<u2").reshape(h, w, spp)


def _pad_tiles(img, T):
    return [b.astype("<u2") for b in DT.blocks_of(img.reshape(img.shape[0], -1), img.shape[2], tile=(T, T))]


def write_reader_files(d):
    """the files, each with one fault or none; returns the lines of the program's list"""
    lines = []

    def u16(name, tags, payload=b"", **kw):
        _tiff.write_raw_tiff(os.path.join(d, name), tags, payload, **kw)
        lines.append("u16 " + os.path.join(d, name))

    def u8(name, tags, payload=b"", **kw):
        _tiff.write_raw_tiff(os.path.join(d, name), tags, payload, **kw)
        lines.append("u8 " + os.path.join(d, name))

    S, L, Q = 3, 4, 16
    img = _pixels(3, 5, 1, 1)                                            # 5 x 3 x 1: 30 bytes at offset 8
    raw = img.tobytes()

    def strips(over=None, at=8):
        t = {256: (L, [5]), 257: (L, [3]), 258: (S, [16]), 259: (S, [1]), 262: (S, [1]), 273: (L, [at]), 277: (S, [1]), 278: (L, [3]),
             279: (L, [30]), 284: (S, [1]), 339: (S, [1])}
        t.update(over or {})
        return {k: v for k, v in t.items() if v is not None}

    # ---- sound files ----
    u16("ok_strip", strips(), raw)
    u16("ok_strip_big", strips({273: (Q, [16]), 279: (Q, [30])}, at=16), raw, big=True)
    u16("ok_three_strips", strips({278: (L, [1]), 273: (L, [8, 18, 28]), 279: (L, [10, 10, 10])}), raw)
    u16("ok_rps_beyond_height", strips({278: (L, [1000])}), raw)
    u16("ok_no_rps", strips({278: None}), raw)
    u16("ok_unknown_type_and_empty_tag", strips({305: (2, 4, 0x41424300), 306: (S, 0, 0)}), raw)
    img4 = _pixels(5, 7, 4, 2)                                           # 7 x 5 x 4
    for pred in (1, 2):
        for rps in (2, 5):
            src = DT.predict2(img4) if pred == 2 else img4
            st = [_tiff.lzw_encode(src[r:r + rps].tobytes()) for r in range(0, 5, rps)]
            _tiff.write_tiff_lzw_strips(os.path.join(d, "ok_lzw_p%d_r%d" % (pred, rps)), st, (5, 7, 4), pred, rps)
            lines.append("u16 " + os.path.join(d, "ok_lzw_p%d_r%d" % (pred, rps)))
            DT.write(os.path.join(d, "ok_deflate_p%d_r%d" % (pred, rps)), img4.reshape(5, 28), 4, pred, rps=rps)
            lines.append("u16 " + os.path.join(d, "ok_deflate_p%d_r%d" % (pred, rps)))
    DT.write(os.path.join(d, "ok_deflate_old_number"), img4.reshape(5, 28), 4, 2, rps=2, compression=32946)
    lines.append("u16 " + os.path.join(d, "ok_deflate_old_number"))
    # tiles: 21 x 19 in 16 x 16 tiles (2 x 2, edge tiles), 3 samples
    img3 = _pixels(19, 21, 3, 3)
    tiles = _pad_tiles(img3, 16)

    def tiled(streams, comp, pred=1, TW=16, TL=16, w=21, h=19, over=None):
        body, offs = b"", []
        for st in streams:
            body += b"\0" * (len(body) & 1)
            offs.append(8 + len(body))
            body += st
        t = {256: (L, [w]), 257: (L, [h]), 258: (S, [16, 16, 16]), 259: (S, [comp]), 262: (S, [1]), 277: (S, [3]), 284: (S, [1]), 317: (S, [pred]),
             322: (L, [TW]), 323: (L, [TL]), 324: (L, offs), 325: (L, [len(s) for s in streams]), 339: (S, [1, 1, 1])}
        t.update(over or {})
        return {k: v for k, v in t.items() if v is not None}, body

    u16("ok_tiles_none", *tiled([t.tobytes() for t in tiles], 1))
    for pred in (1, 2):
        src = [DT.predict2(t) if pred == 2 else t for t in tiles]
        u16("ok_tiles_lzw_p%d" % pred, *tiled([_tiff.lzw_encode(t.tobytes()) for t in src], 5, pred))
        u16("ok_tiles_deflate_p%d" % pred, *tiled([DT.deflate(t.tobytes()) for t in src], 8, pred))
    # ---- the header and the directory ----
    u16("big_endian", strips(), raw, order=b"MM")
    u16("magic_44", strips(), raw, magic=44)
    u16("magic_high_byte", strips(), raw, magic=42 + 256)
    u16("empty_directory", strips(), raw, count=0)
    u16("directory_of_5000", strips(), raw, count=5000)
    u16("directory_beyond_the_file", strips(), raw, ifd_at=4000)
    u16("directory_cut", strips(), raw, count=40)
    u16("header_only_6_bytes", {}, b"")
    with open(os.path.join(d, "header_only_6_bytes"), "r+b") as f:
        f.truncate(6)
    lines.append("u16 " + os.path.join(d, "absent_file"))
    u16("tag_larger_than_file", strips({273: (L, 1 << 20, 8)}), raw)
    u16("tag_values_beyond_the_file", strips({273: (L, 3, 5000), 279: (L, 3, 5000), 278: (L, [1])}), raw)
    u16("mixed_depths", strips({258: (S, [16, 8]), 277: (S, [2])}), raw)
    u16("strip_and_tile_tags", strips({322: (L, [16])}), raw)
    # ---- encoding ----
    u16("compression_7", strips({259: (S, [7])}), raw)
    u16("compression_32773", strips({259: (S, [32773])}), raw)
    u16("predictor_3", strips({317: (S, [3])}), raw)
    u16("predictor_0", strips({317: (S, [0])}), raw)
    u16("bits_8", strips({258: (S, [8])}), raw)
    u16("bits_missing", strips({258: None}), raw)
    u16("format_signed", strips({339: (S, [2])}), raw)
    u16("planar_2", strips({284: (S, [2])}), raw)
    # ---- geometry ----
    u16("width_missing", strips({256: None}), raw)
    u16("height_0", strips({257: (L, [0])}), raw)
    u16("width_2_31", strips({256: (L, [1 << 31])}), raw)
    u16("height_2_31", strips({257: (L, [1 << 31])}), raw)
    u16("samples_0", strips({277: (S, [0])}), raw)
    u16("samples_17", strips({277: (S, [17])}), raw)
    u16("tile_length_missing", *tiled([t.tobytes() for t in tiles], 1, over={323: None}))
    u16("tile_width_0", *tiled([t.tobytes() for t in tiles], 1, TW=0))
    u16("strip_offsets_missing", strips({273: None}), raw)
    u16("strip_tags_missing", strips({273: None, 279: None}), raw)
    u16("strip_tables_differ", strips({273: (L, [8, 18]), 278: (L, [2])}), raw)
    u16("tile_offsets_missing", *tiled([t.tobytes() for t in tiles], 1, over={324: None}))
    u16("image_of_2_46_bytes", strips({256: (L, [0x7FFFFFFF]), 257: (L, [0x7FFFFFFF]), 258: (S, [16] * 16), 277: (S, [16])}), raw)
    u16("tile_of_4_gib", *tiled([t.tobytes() for t in tiles], 1, TW=65536, TL=65536))
    u16("tile_of_4_gib_by_samples", *tiled([t.tobytes() for t in tiles], 1, TW=65536, TL=32767))
    u16("tile_count", *tiled([t.tobytes() for t in tiles[:3]], 1))
    t, body = tiled([t.tobytes() for t in tiles], 1)
    u16("tile_outside_the_file", {**t, 324: (L, t[324][1][:3] + [1 << 20])}, body)
    u16("tile_length_beyond_the_file", {**t, 325: (L, [1536, 1536, 1536, 1 << 20])}, body)
    u16("uncompressed_tile_size", *tiled([tiles[0].tobytes(), tiles[1].tobytes(), tiles[2].tobytes()[:-2], tiles[3].tobytes()], 1))
    # ---- plausibility bounds ----
    one = _tiff.lzw_encode(bytes(64))
    u16("implausible_lzw_tiles", *tiled([one] * 4, 5, TW=4096, TL=4096, w=8192, h=8192))
    u16("implausible_deflate_tiles", *tiled([DT.deflate(bytes(64))] * 4, 8, TW=4096, TL=4096, w=8192, h=8192))
    u16("implausible_lzw_strips", strips({259: (S, [5]), 256: (L, [30000]), 257: (L, [30000]), 278: (L, [30000]), 279: (L, [len(one)])}), one)
    z = DT.deflate(bytes(64))
    u16("implausible_deflate_strips", strips({259: (S, [8]), 256: (L, [30000]), 257: (L, [30000]), 278: (L, [30000]), 279: (L, [len(z)])}), z)
    # (what is just inside the bounds is refused later, by the decoder: 2560 and 1032 bytes of image for each byte present, plus 16)
    u16("plausible_lzw_strip_that_is_short", strips({259: (S, [5]), 256: (L, [1280]), 257: (L, [len(one) + 16]), 278: (L, [len(one) + 16]),
                                                       279: (L, [len(one)])}), one)
    u16("plausible_deflate_strip_that_is_short", strips({259: (S, [8]), 256: (L, [516]), 257: (L, [len(z) + 16]), 278: (L, [len(z) + 16]),
                                                           279: (L, [len(z)])}), z)
    # ---- strips ----
    u16("strip_count", strips({278: (L, [2])}), raw)
    u16("strip_outside_the_file", strips({273: (L, [1 << 20])}), raw)
    u16("strip_length_beyond_the_file", strips({279: (L, [1 << 20])}), raw)
    u16("strip_sizes_exceed", strips({278: (L, [2]), 273: (L, [8, 8]), 279: (L, [20, 20])}), raw)
    u16("strip_sizes_short", strips({279: (L, [28])}), raw)
    # ---- decoding ----
    def lzw_strip(stream):
        return strips({259: (S, [5]), 279: (L, [len(stream)])}), stream

    u16("lzw_bad_first_code", *lzw_strip(_codes([256, 300, 257])))
    u16("lzw_code_beyond_the_table", *lzw_strip(_codes([256, 65, 400, 257])))
    u16("lzw_table_full", *lzw_strip(_codes([256] + [65] * 3900)))
    u16("lzw_short_strip", *lzw_strip(_tiff.lzw_encode(raw[:28])))
    u16("lzw_long_strip", *lzw_strip(_tiff.lzw_encode(raw + b"ab")))
    u16("lzw_no_end_code", *lzw_strip(_tiff.lzw_encode(raw)[:-1]))
    src = [t.tobytes() for t in tiles]
    u16("lzw_bad_first_code_in_tile_2", *tiled([_tiff.lzw_encode(s) for s in src[:2]] + [_codes([256, 300, 257])] + [_tiff.lzw_encode(src[3])], 5))
    u16("lzw_short_tile_3", *tiled([_tiff.lzw_encode(s) for s in src[:3]] + [_tiff.lzw_encode(src[3][:-6])], 5))

    def deflate_strip(stream):
        return strips({259: (S, [8]), 279: (L, [len(stream)])}), stream

    good = DT.deflate(raw)
    u16("deflate_block_type_3", *deflate_strip(good[:2] + bytes([good[2] | 6]) + good[3:]))
    u16("deflate_cut", *deflate_strip(good[:len(good) // 2]))
    u16("deflate_adler", *deflate_strip(good[:-1] + bytes([good[-1] ^ 1])))
    u16("deflate_short_strip", *deflate_strip(DT.deflate(raw[:28])))
    u16("deflate_long_strip", *deflate_strip(DT.deflate(raw + b"ab")))
    u16("deflate_cut_tile_1", *tiled([DT.deflate(src[0]), DT.deflate(src[1])[:9], DT.deflate(src[2]), DT.deflate(src[3])], 8))
    u16("deflate_short_tile_0", *tiled([DT.deflate(src[0][:-2])] + [DT.deflate(s) for s in src[1:]], 8))
    # ---- the 8-bit reader: a 5 x 3 mask ----
    m = bytes(range(15))

    def mask(over=None):
        t = {256: (L, [5]), 257: (L, [3]), 258: (S, [8]), 259: (S, [1]), 262: (S, [1]), 273: (L, [8]), 277: (S, [1]), 278: (L, [3]), 279: (L, [15]),
             284: (S, [1])}
        t.update(over or {})
        return {k: v for k, v in t.items() if v is not None}

    u8("m_ok", mask(), m)
    u8("m_ok_three_strips", mask({278: (L, [1]), 273: (L, [8, 13, 18]), 279: (L, [5, 5, 5])}), m)
    u8("m_ok_no_rps", mask({278: None}), m)
    u8("m_big_endian", mask(), m, order=b"MM")
    u8("m_bigtiff", mask({273: (Q, [16]), 279: (Q, [15])}), m, big=True)
    u8("m_magic_44", mask(), m, magic=44)
    u8("m_empty_directory", mask(), m, count=0)
    u8("m_directory_of_5000", mask(), m, count=5000)
    u8("m_directory_beyond_the_file", mask(), m, ifd_at=4000)
    lines.append("u8 " + os.path.join(d, "absent_file"))
    u8("m_tag_larger_than_file", mask({273: (L, 1 << 20, 8)}), m)
    u8("m_long8_tag_is_skipped", mask({278: (Q, 1, 1)}), m)
    u8("m_mixed_depths", mask({258: (S, [8, 16])}), m)
    for tag in (322, 323, 324, 325):
        u8("m_tile_tag_%d" % tag, mask({tag: (L, [16])}), m)
    u8("m_compression_5", mask({259: (S, [5])}), m)
    u8("m_bits_16", mask({258: (S, [16])}), m)
    u8("m_bits_missing", mask({258: None}), m)
    u8("m_samples_3", mask({277: (S, [3]), 258: (S, [8, 8, 8])}), m)
    u8("m_planar_2", mask({284: (S, [2])}), m)
    u8("m_width_0", mask({256: (L, [0])}), m)
    u8("m_height_2_31", mask({257: (L, [1 << 31])}), m)
    u8("m_strip_tags_missing", mask({273: None}), m)
    u8("m_image_of_2_32_bytes", mask({256: (L, [0x7FFFFFFF]), 257: (L, [3])}), m)
    u8("m_strip_count", mask({278: (L, [2])}), m)
    u8("m_strip_outside_the_file", mask({273: (L, [1 << 20])}), m)
    u8("m_strip_size", mask({279: (L, [14])}), m)
    # the 16-bit reader on a mask and the other way round
    u16("mask_read_as_16_bit", mask(), m)
    u8("m_16_bit_file", strips(), raw)
    return lines


def collect_reader(program, d):
    lines = write_reader_files(d)
    with open(os.path.join(d, "list.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([program, "read", os.path.join(d, "list.txt")], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-3000:]
    out = {}
    for line in r.stdout.splitlines():
        name, what, text = line.split("\t")
        out.setdefault(name, {})[what] = text
    assert len(out) == len({l.split("/")[-1] for l in lines})
    return out


def collect_writers(program, d):
    out = {}
    for big in ("0", "1"):
        sub = os.path.join(d, "big" + big)
        os.mkdir(sub)
        r = subprocess.run([program, "write", sub], capture_output=True, text=True, env=dict(os.environ, OIP_TIFF_THREADS="3", OIP_TIFF_FORCE_BIG=big))
        assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-3000:]
        for name in sorted(os.listdir(sub)):
            with open(os.path.join(sub, name), "rb") as f:
                data = f.read()
            assert data[2] == (42 if big == "0" or name.startswith("u8_") else 43)
            out["big%s/%s" % (big, name)] = "%d %s" % (len(data), hashlib.sha256(data).hexdigest())
    return out


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_program(tmp_path_factory.mktemp("tiffcodec_pin"))


def _golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def test_readers_say_what_they_said(program, tmp_path):
    want, got = _golden("tiff_refusals.json"), collect_reader(program, str(tmp_path))
    assert set(got) == set(want)
    for name in want:
        assert got[name] == want[name], name


def test_every_refusal_a_header_can_reach_is_pinned():
    """the words of every fail(...) of the two readers that a file of a few hundred bytes can reach occur in the fixture"""
    said = json.dumps(_golden("tiff_refusals.json"))
    for words in ("only little-endian TIFF is supported", "not a TIFF file", "implausible directory", "truncated file", "cannot open file",
                  "tag larger than the file", "mixed sample depths", "strip tags and tile tags are both present", "compression 7 is not supported (none, LZW",
                  "predictor 3 is not supported", "only chunky unsigned 16-bit samples are supported", "missing or implausible geometry",
                  "a tiled TIFF needs TileWidth and TileLength, both positive", "missing tile tags", "missing strip tags", "implausible image size",
                  "a tile of 4 GiB or more", "tile count does not match the tile grid", "tile outside the file",
                  "an uncompressed tile does not have the size of a tile", "image size is implausible for its compressed tiles",
                  "image size is implausible for its compressed strips", "strip count does not match RowsPerStrip", "strip outside the file",
                  "strip sizes exceed the image", "strip sizes do not cover the image", "corrupt LZW stream (bad first code)",
                  "corrupt LZW stream (code beyond the table)", "corrupt LZW stream (table full without ClearCode)", "strip 0 decodes to 28 bytes, 30 expected",
                  "tile 3 decodes to", "corrupt Deflate stream (invalid block type) in strip 0 of [@]", "corrupt Deflate stream (more bytes than expected)",
                  "in tile 1 of [@]", "read 8-bit TIFF [@]: BigTIFF is not supported (a mask is a classic TIFF)", "tiled TIFF is not supported (strips only)",
                  "is not supported (a mask is uncompressed)", "16-bit samples are not supported (a mask has 8)",
                  "3 samples per pixel are not supported (a mask has 1)", "read 8-bit TIFF [@]: implausible image size"):
        assert words in said, words


def test_writers_write_what_they_wrote(program, tmp_path):
    want, got = _golden("tiff_writer_digests.json"), collect_writers(program, str(tmp_path))
    assert set(got) == set(want)
    for name in want:
        assert got[name] == want[name], name
