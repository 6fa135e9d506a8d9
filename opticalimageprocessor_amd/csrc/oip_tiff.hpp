// oip_tiff.hpp -- dependency-free codec for the 16-bit TIFF / BigTIFF files on either side of the hot path.
//
// SURVEY 8f ranks 1 and 2.  The reference writes and reads its TIFFs through two libraries that are not
// available here:
//   * cv::imwrite(".TIFF") of a CV_16UC4 Mat (preproc.h:167-185; StitchTiff, imageop.h:390-402): OpenCV's TIFF
//     encoder defaults to LZW with the horizontal predictor, and converts BGRA -> RGBA on the way out;
//   * GDAL GTiff: stitched PAN as a 1-band file with default creation options (imageop.h:316-328: no
//     compression), stitched MSS with COMPRESS=LZW PREDICTOR=2 (imageop.h:460-567);
//   * cv::imread of those files (imageop.h:380-388).
// This codec writes and reads little-endian baseline strips, chunky samples, unsigned 16 bit, classic TIFF or
// BigTIFF (when the file would pass 4 GiB, as GDAL does with BIGTIFF=IF_NEEDED), uncompressed (259 = 1) or LZW
// (259 = 5) with predictor 1 or 2 (317) -- so the files the reference itself produces can be consumed and the
// files written here open in cv::imread / GDAL.  Pixel payloads match the reference's; file bytes need not
// (strip sizes and tag order are the libraries' own).  Strips are encoded / decoded on a few threads.
// The reader also takes Deflate (259 = 8, or 32946: zlib streams, what COMPRESS=DEFLATE and most archive COGs hold) through
// the decoder of oip_inflate.h, and the writers take TIFF_DEFLATE (259 = 8, predictor 2): zlib streams of the encoder of
// oip_deflate.h, in the strips and tiles LZW has.  No product defaults to it (--tiff-compress deflate asks for it).
//
// LZW as TIFF 6.0 section 13 specifies it and libtiff implements it: MSB-first codes of 9..12 bits, ClearCode
// 256, EndOfInformation 257, first free code 258, every strip starts with ClearCode; the encoder widens the
// code after assigning entry 511 / 1023 / 2047 (the decoder, whose table lags by one entry, widens when ITS
// next free code is 511 / 1023 / 2047 -- TIFF's "early change") and emits ClearCode when entry 4093 is assigned.
// Predictor 2 on 16-bit samples: each sample minus the same channel of the previous pixel, modulo 2^16.
//
// Channel order: OpenCV stores a 4-channel Mat (c0,c1,c2,c3) as samples (c2,c1,c0,c3); `opencv_order`
// reproduces that, so files written here round-trip through cv::imread exactly like the reference's.
#pragma once

#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <future>
#include <memory>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "oip_deflate.h"
#include "oip_inflate.h"
#include "oip_tiffstreams.h"

namespace OIPGPU {

// (TIFF_DEFLATE: 8, Adobe Deflate, is what is written; its older number 32946 is read as the same thing)
enum TiffCompression { TIFF_NONE = 1, TIFF_LZW = 5, TIFF_DEFLATE = 8 };

namespace tiffdetail {

// CPUs this process may actually use: the cgroup's CPU quota where there is one (a container that shows all 256 hardware threads
// of the host and grants 16 CPUs of time -- cpu.max = "1600000 100000" -- is the normal case for one rank of a GPU node), else
// the hardware's count.  More runnable threads than the quota only get the whole group throttled.
inline int cpu_budget()
{
    static const int n = [] {
        int hw = (int)std::thread::hardware_concurrency();
        if (hw < 1) hw = 1;
        long quota = -1, period = 0;
        if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {                  // cgroup v2: "<quota|max> <period>"
            char q[32] = {0};
            if (fscanf(f, "%31s %ld", q, &period) == 2 && strcmp(q, "max") != 0) quota = atol(q);
            fclose(f);
        } else if (FILE *g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {   // cgroup v1
            if (fscanf(g, "%ld", &quota) != 1) quota = -1;
            fclose(g);
            if (FILE *h = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (fscanf(h, "%ld", &period) != 1) period = 0; fclose(h); }
        }
        if (quota > 0 && period > 0) {
            const int c = (int)((quota + period - 1) / period);
            if (c >= 1 && c < hw) hw = c;
        }
        return hw;
    }();
    return n;
}

// threads of the host strip encoder / decoder: the CPUs the process may use, at most 64 (OIP_TIFF_THREADS overrides, up to 128).
// Device-resident products and LZW inputs do not come here: their strips are coded on the device (csrc/tifflzw.hip).
inline int worker_count()
{
    static const int n = [] {
        const char *e = getenv("OIP_TIFF_THREADS");
        int v = e ? atoi(e) : cpu_budget();
        const int cap = e ? 128 : 64;
        return v < 1 ? 1 : (v > cap ? cap : v);
    }();
    return n;
}

// run fn(i, t) for i in [0, n) on a few threads; t < worker_count() is the index of the thread that runs it
template <typename F> inline void parallel_for_t(size_t n, F fn)
{
    const int nt = (int)std::min<size_t>(n, (size_t)worker_count());
    if (nt <= 1) { for (size_t i = 0; i < n; ++i) fn(i, 0); return; }
    std::vector<std::thread> th;
    std::vector<std::string> errs(nt);
    for (int t = 0; t < nt; ++t)
        th.emplace_back([&, t] {
            try { for (size_t i = t; i < n; i += nt) fn(i, t); }
            catch (const std::exception &e) { errs[t] = e.what(); }
        });
    for (auto &x : th) x.join();
    for (auto &e : errs) if (!e.empty()) throw std::runtime_error(e);
}
template <typename F> inline void parallel_for(size_t n, F fn) { parallel_for_t(n, [&](size_t i, int) { fn(i); }); }

// The string table of the encoder: open addressing over 16384 slots (4x the 4094 entries), a slot = (generation << 20) |
// (prefix code << 8) | byte.  ClearCode starts a new GENERATION instead of wiping the table -- sensor data barely compresses
// (a code per 1.3 bytes), so the table fills every ~5 KB of input and wiping 64 KB each time cost more than the coding itself.
struct LzwTable {
    static constexpr int kHash = 1 << 14;
    uint32_t key[kHash];
    uint16_t code[kHash];
    uint32_t gen = 0;
    LzwTable() { memset(key, 0, sizeof key); }
    void clear()
    {
        if (++gen == (1u << 12)) { memset(key, 0, sizeof key); gen = 1; }      // generation 0 is never current: zeroed slots are empty
    }
};

// encodes n bytes into dst (lzw_worst(n) bytes, oip_tiffstreams.h); returns the encoded size
inline size_t lzw_encode_to(const uint8_t *src, size_t n, uint8_t *dst)
{
    static thread_local std::unique_ptr<LzwTable> tab;  // ~96 KB, once per encoding thread
    if (!tab) tab.reset(new LzwTable());
    tab->clear();
    uint8_t *o = dst;
    uint64_t acc = 0;
    int nbits = 0;
    auto put = [&](unsigned code, int width) {
        acc = (acc << width) | code;
        nbits += width;
        while (nbits >= 8) { *o++ = (uint8_t)(acc >> (nbits - 8)); nbits -= 8; }
    };
    int width = 9, next = 258;
    put(256, width);
    if (n == 0) {
        put(257, width);
        if (nbits > 0) *o++ = (uint8_t)(acc << (8 - nbits));
        return (size_t)(o - dst);
    }
    uint32_t gen = tab->gen << 20;
    int ent = src[0];
    for (size_t i = 1; i < n; ++i) {
        const int c = src[i];
        const uint32_t key = gen | ((uint32_t)ent << 8) | (uint32_t)c;
        unsigned h = ((((uint32_t)ent << 8) | (uint32_t)c) * 2654435761u) >> 18;
        bool found = false;
        for (;;) {
            const uint32_t k = tab->key[h];
            if (k == key) { ent = tab->code[h]; found = true; break; }
            if ((k >> 20) != (gen >> 20)) break;                            // empty in this generation
            h = (h + 1) & (LzwTable::kHash - 1);
        }
        if (found) continue;
        put((unsigned)ent, width);
        ent = c;
        tab->key[h] = key;
        tab->code[h] = (uint16_t)next++;
        if (next == 4094) {                        // table full: clear (libtiff: free_ent == CODE_MAX - 1)
            put(256, width);
            tab->clear();
            gen = tab->gen << 20;
            width = 9;
            next = 258;
        } else if (next == (1 << width) && width < 12) {
            ++width;
        }
    }
    put((unsigned)ent, width);
    ++next;                                        // libtiff's LZWPostEncode: the last code counts as an entry too
    if (next == 4094) { put(256, width); width = 9; }
    else if (next == (1 << width) && width < 12) ++width;
    put(257, width);
    if (nbits > 0) *o++ = (uint8_t)(acc << (8 - nbits));
    return (size_t)(o - dst);
}

// returns the number of bytes produced (at most cap); throws on a corrupt stream
inline size_t lzw_decode(const uint8_t *src, size_t n, uint8_t *dst, size_t cap)
{
    uint16_t prefix[4096];
    uint8_t suffix[4096], first[4096];
    uint16_t length[4096];
    for (int i = 0; i < 256; ++i) { prefix[i] = 0xFFFF; suffix[i] = (uint8_t)i; first[i] = (uint8_t)i; length[i] = 1; }
    int width = 9, next = 258, old = -1;
    uint64_t acc = 0;
    int nbits = 0;
    size_t pos = 0, produced = 0;
    for (;;) {
        while (nbits < width) {
            if (pos >= n) return produced;          // stream ends without EOI: tolerated, as libtiff does
            acc = (acc << 8) | src[pos++];
            nbits += 8;
        }
        const int code = (int)((acc >> (nbits - width)) & ((1u << width) - 1));
        nbits -= width;
        if (code == 257) break;
        if (code == 256) { width = 9; next = 258; old = -1; continue; }
        if (old < 0) {
            if (code >= 256) throw std::runtime_error("corrupt LZW stream (bad first code)");
            if (produced < cap) dst[produced] = (uint8_t)code;
            ++produced;
            old = code;
            continue;
        }
        // A conforming encoder sends ClearCode when it assigns entry 4093, so the decoder's table never reaches 4096
        // entries; a stream that keeps sending codes without clearing is corrupt (libtiff: "Corrupted LZW table").
        if (next >= 4096) throw std::runtime_error("corrupt LZW stream (table full without ClearCode)");
        int emit = code;
        if (code >= next) {
            if (code != next) throw std::runtime_error("corrupt LZW stream (code beyond the table)");
            // KwKwK: old string + its first byte
            prefix[next] = (uint16_t)old; suffix[next] = first[old]; first[next] = first[old]; length[next] = (uint16_t)(length[old] + 1);
            emit = next;
        } else {
            prefix[next] = (uint16_t)old; suffix[next] = first[code]; first[next] = first[old]; length[next] = (uint16_t)(length[old] + 1);
        }
        const size_t len = length[emit];
        if (produced + len <= cap) {
            uint8_t *p = dst + produced + len;
            for (int c = emit; c != 0xFFFF; c = prefix[c]) *--p = suffix[c];
        } else {
            // tail of a strip that decodes to more than expected: keep what fits
            std::vector<uint8_t> tmp(len);
            uint8_t *p = tmp.data() + len;
            for (int c = emit; c != 0xFFFF; c = prefix[c]) *--p = suffix[c];
            if (produced < cap) memcpy(dst + produced, tmp.data(), cap - produced);
        }
        produced += len;
        ++next;
        if (next >= (1 << width) - 1 && width < 12) ++width;       // early change
        old = code;
        if (produced >= cap && pos >= n) break;
    }
    return produced;
}

// One zlib stream of a Deflate TIFF (csrc/oip_inflate.h, the decoder the device runs as well) into dst[0, cap); returns the number
// of bytes produced (at most cap); throws on a corrupt stream with the cause named.  `what` names the stream ("strip 3").
inline size_t deflate_decode(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, const std::string &what)
{
    thread_local std::unique_ptr<oipinflate::Shared> work;
    if (!work) work.reset(new oipinflate::Shared);
    size_t got = 0;
    const int st = oipinflate::inflate_host(src, n, dst, cap, &got, work.get());
    if (st != oipinflate::kOk) throw std::runtime_error(std::string("corrupt Deflate stream (") + oipinflate::status_text(st) + ") in " + what);
    return got;
}

inline void predictor2_encode(uint16_t *row, size_t width, int spp)
{
    for (size_t i = width * spp - 1; i >= (size_t)spp; --i) row[i] = (uint16_t)(row[i] - row[i - spp]);
}
inline void predictor2_decode(uint16_t *row, size_t width, int spp)
{
    for (size_t i = spp; i < width * spp; ++i) row[i] = (uint16_t)(row[i] + row[i - spp]);
}

// one compressed strip or tile (TIFF_LZW, or Deflate) into dst[0, cap); returns the bytes produced.  `what` names it in Deflate's refusals.
inline size_t decode_chunk(uint64_t compression, const uint8_t *src, size_t n, uint8_t *dst, size_t cap, const std::string &what)
{
    return compression == TIFF_LZW ? lzw_decode(src, n, dst, cap) : deflate_decode(src, n, dst, cap, what);
}

// a row of 4-sample pixels into OpenCV's sample order
inline void swap_row(const uint16_t *src, uint16_t *dst, size_t width)
{
    for (size_t x = 0; x < width; ++x) {
        dst[4 * x + 0] = src[4 * x + 2];
        dst[4 * x + 1] = src[4 * x + 1];
        dst[4 * x + 2] = src[4 * x + 0];
        dst[4 * x + 3] = src[4 * x + 3];
    }
}

// the most an encoded strip or tile of n bytes takes (LZW: oip_tiffstreams.h; Deflate: all of it in stored blocks, oip_deflate.h)
inline size_t chunk_worst(size_t n, int compression) { return compression == TIFF_DEFLATE ? oipdeflate::stored_bound(n) : lzw_worst(n); }

// One strip or tile of an LZW or Deflate file: `rows` rows of `width` pixels from src into buf (swap: in OpenCV's order), differenced
// along each row (predictor 2) and encoded into dst (chunk_worst of the chunk's bytes); returns the encoded size.  Deflate: the host
// instantiation of the coder the device runs (csrc/oip_deflate.h), so a file is the same bytes whoever encoded it.
inline size_t encode_chunk(const uint16_t *src, long rows, size_t width, int spp, bool swap, uint16_t *buf, uint8_t *dst, int compression = TIFF_LZW)
{
    const size_t rw = width * spp;
    for (long r = 0; r < rows; ++r) {
        uint16_t *d = buf + (size_t)r * rw;
        if (swap) swap_row(src + (size_t)r * rw, d, width); else memcpy(d, src + (size_t)r * rw, rw * 2);
        predictor2_encode(d, width, spp);
    }
    const size_t n = (size_t)rows * rw * 2;
    if (compression != TIFF_DEFLATE) return lzw_encode_to((const uint8_t *)buf, n, dst);
    thread_local std::unique_ptr<oipdeflate::Shared> work;
    if (!work) work.reset(new oipdeflate::Shared);
    const size_t size = oipdeflate::deflate_host((const uint8_t *)buf, n, dst, oipdeflate::stored_bound(n), work.get());
    if (!size) throw std::runtime_error("Deflate encoder: a strip or tile of 4 GiB or more");
    return size;
}

// n bytes at offset `at` of fd, however many calls it takes; `who` names the writer in the error
inline void pwrite_all(int fd, const void *p, size_t n, uint64_t at, const char *who)
{
    size_t w = 0;
    while (w < n) {
        const ssize_t r = pwrite(fd, (const char *)p + w, n - w, (off_t)(at + w));
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) throw std::runtime_error(std::string(who) + ": write failed");
        w += (size_t)r;
    }
}

// Classic TIFF offsets are 32 bit.  LZW can also GROW a chunk: at worst one 12-bit code per byte (x1.5), so the choice is made on
// the worst case of the payload of all directories and a classic file can never overflow half-way (BigTIFF is always valid): the
// header, page-aligned payload, the chunk tables, the directories.  OIP_TIFF_FORCE_BIG: test hook, BigTIFF at any size.
// Deflate: a chunk of c bytes is at most c + 5 ceil(c / 65535) + 6 (stored blocks, oip_deflate.h) plus a byte to the next even offset.
inline uint64_t worst_payload(uint64_t bytes, int compression, uint64_t nchunks = 1)
{
    if (compression == TIFF_DEFLATE) return bytes + 5 * (bytes / 65535 + nchunks) + 12 * nchunks;
    return compression == TIFF_LZW ? bytes + bytes / 2 : bytes;
}
inline bool needs_bigtiff(uint64_t worst, uint64_t nchunks)
{
    bool big = worst + nchunks * 16 + 16384 > 0xFFFFF000ull;
    if (const char *e = getenv("OIP_TIFF_FORCE_BIG")) big = big || atoi(e) != 0;
    return big;
}

inline void put_le(std::vector<unsigned char> &out, uint64_t v, size_t n)
{
    for (size_t i = 0; i < n; ++i) out.push_back((unsigned char)(v >> (8 * i)));
}

// One directory as the three writers emit it: the tags of a chunky unsigned image in strips or tiles, in tag order, in classic or
// BigTIFF entries.  The writers differ in where their out-of-line values lie (what does not fit an entry: fits()), not in what a
// directory says.
struct TiffDirectory {
    bool big = false;
    bool reduced = false;                   // NewSubfileType (254) = 1: a reduced-resolution image
    uint64_t width = 0, height = 0;
    int spp = 1, bits = 16, compression = TIFF_NONE;
    bool sample_format = true;              // SampleFormat (339) = unsigned; the 8-bit writer leaves it out
    uint64_t bitsAt = 0, formatAt = 0;      // where BitsPerSample / SampleFormat lie, 0: in their entries
    uint64_t tile = 0;                      // 0: strips of rows_per_strip rows (273 / 278 / 279), else tile x tile tiles (322 - 325)
    uint64_t rows_per_strip = 0;
    uint64_t nchunks = 0, offsets = 0, counts = 0;   // of the strips or tiles: the one value, or where the table lies

    size_t field() const { return big ? 8 : 4; }
    bool fits(uint64_t count, size_t size) const { return count * size <= field(); }
    static uint64_t shorts(int n, uint16_t v) { uint64_t x = 0; for (int i = 0; i < n; ++i) x |= (uint64_t)v << (16 * i); return x; }

    // the entry count, the entries and the offset of the next directory
    void append_to(std::vector<unsigned char> &out, uint64_t next) const
    {
        struct Tag { uint16_t id, type; uint64_t count, value; };
        const uint16_t SHORT = 3, LONG = 4, otype = big ? 16 : LONG;      // (16: LONG8)
        const uint64_t n = (uint64_t)spp;
        std::vector<Tag> tags = {{256, LONG, 1, width}, {257, LONG, 1, height}, {258, SHORT, n, bitsAt ? bitsAt : shorts(spp, (uint16_t)bits)},
                                 {259, SHORT, 1, (uint64_t)compression}, {262, SHORT, 1, (uint64_t)(spp >= 3 ? 2 : 1)},     // RGB / BlackIsZero
                                 {277, SHORT, 1, n}, {284, SHORT, 1, 1}};                                                    // chunky
        if (reduced) tags.push_back({254, LONG, 1, 1});
        if (!tile) tags.insert(tags.end(), {{273, otype, nchunks, offsets}, {278, LONG, 1, rows_per_strip}, {279, otype, nchunks, counts}});
        else tags.insert(tags.end(), {{322, LONG, 1, tile}, {323, LONG, 1, tile}, {324, otype, nchunks, offsets}, {325, otype, nchunks, counts}});
        if (compression == TIFF_LZW || compression == TIFF_DEFLATE) tags.push_back({317, SHORT, 1, 2});   // horizontal predictor
        if (spp == 4) tags.push_back({338, SHORT, 1, 2});                  // unassociated alpha
        if (sample_format) tags.push_back({339, SHORT, n, formatAt ? formatAt : shorts(spp, 1)});
        std::sort(tags.begin(), tags.end(), [](const Tag &a, const Tag &b) { return a.id < b.id; });
        put_le(out, tags.size(), big ? 8 : 2);
        for (const Tag &t : tags) { put_le(out, t.id, 2); put_le(out, t.type, 2); put_le(out, t.count, field()); put_le(out, t.value, field()); }
        put_le(out, next, field());
    }
};

// A TIFF file open for reading: guarded reads, and refusals in the words of the reader that opened it (`reader` [path]: ...)
struct TiffSource {
    std::unique_ptr<FILE, int (*)(FILE *)> f;
    std::string prefix;
    uint64_t size = 0;
    TiffSource(const std::string &path, const char *reader) : f(fopen(path.c_str(), "rb"), fclose), prefix(std::string(reader) + " [" + path + "]: ")
    {
        if (!f) throw std::runtime_error("cannot open file [" + path + "]");
        if (fseeko(f.get(), 0, SEEK_END)) fail("seek failed");
        size = (uint64_t)ftello(f.get());
    }
    [[noreturn]] void fail(const std::string &m) const { throw std::runtime_error(prefix + m); }
    void read(uint64_t off, void *p, size_t n) const
    {
        if (off > size || n > size - off) fail("truncated file");
        if (fseeko(f.get(), (off_t)off, SEEK_SET) || fread(p, 1, n, f.get()) != n) fail("truncated file");
    }
};

// The first directory of a little-endian TIFF or BigTIFF: tag(id, count, val) for every entry of type SHORT, LONG or LONG8 that has
// values, in file order; val(k) is its k-th value, from the entry or from where the entry points.  no_bigtiff: the words in which
// a reader of classic files refuses BigTIFF -- such a reader does not take LONG8 entries either.
template <typename F> inline void read_directory(const TiffSource &src, const char *no_bigtiff, F tag)
{
    unsigned char h[16];
    src.read(0, h, 8);
    if (h[0] != 'I' || h[1] != 'I') src.fail("only little-endian TIFF is supported");
    const bool big = h[2] == 43;
    if (big && h[3] == 0 && no_bigtiff) src.fail(no_bigtiff);
    if ((h[2] != 42 && !big) || h[3] != 0) src.fail("not a TIFF file");
    uint64_t ifd = 0, n = 0;
    if (big) { src.read(8, &ifd, 8); src.read(ifd, &n, 8); }
    else { memcpy(&ifd, h + 4, 4); src.read(ifd, &n, 2); }
    if (n == 0 || n > 4096) src.fail("implausible directory");
    const uint64_t ent = ifd + (big ? 8 : 2);
    const size_t esz = big ? 20 : 12, osz = big ? 8 : 4;
    for (uint64_t i = 0; i < n; ++i) {
        unsigned char e[20];
        src.read(ent + i * esz, e, esz);
        uint16_t id, type;
        memcpy(&id, e, 2); memcpy(&type, e + 2, 2);
        uint64_t cnt = 0;
        memcpy(&cnt, e + 4, osz);
        const int ts = type == 3 ? 2 : (type == 4 ? 4 : (type == 16 && !no_bigtiff ? 8 : 0));
        if (!ts || cnt == 0) continue;                                          // unknown type / empty tag: not ours
        if (cnt > src.size / (uint64_t)ts) src.fail("tag larger than the file");
        std::vector<unsigned char> raw((size_t)cnt * ts);
        if (cnt * ts <= osz) memcpy(raw.data(), e + 4 + osz, (size_t)cnt * ts);
        else { uint64_t o = 0; memcpy(&o, e + 4 + osz, osz); src.read(o, raw.data(), raw.size()); }
        tag(id, cnt, [&](uint64_t k) { uint64_t v = 0; memcpy(&v, raw.data() + k * ts, ts); return v; });
    }
}

}  // namespace tiffdetail

class TiffWriterU16 {
public:
    // rows are appended top to bottom with write_rows(); close() writes the directory.
    // compression: TIFF_NONE, TIFF_LZW (always with predictor 2, what cv::imwrite and the reference's GDAL call use) or
    // TIFF_DEFLATE (259 = 8, predictor 2 as well: zlib streams of csrc/oip_deflate.h, in the strips LZW has)
    // overview_levels = n > 0: the file is the external overview file (<product>.ovr) of a width x height product instead --
    // n directories, directory k the pyramid's level k + 1 (each half the one before, rounded up), every one with the tags of a
    // product of its geometry plus NewSubfileType (254) = 1, chained by their next-directory offsets.  The rows of level 1 come
    // first; next_directory() goes on to the next level.  n = 0 is the one-image file: no tag 254, the one directory linked from the header.
    TiffWriterU16(const std::string &path, int width, long height, int spp, bool opencv_order, int compression = TIFF_NONE, int overview_levels = 0)
        : mW(width), mH(height), mSpp(spp), mSwap(opencv_order && spp == 4), mComp(compression)
    {
        mLevelsLeft = overview_levels;
        if (width <= 0 || height <= 0 || (spp != 1 && spp != 4) || overview_levels < 0) throw std::invalid_argument("TiffWriterU16: bad geometry");
        if (compression != TIFF_NONE && compression != TIFF_LZW && compression != TIFF_DEFLATE) throw std::invalid_argument("TiffWriterU16: unsupported compression");
        // classic or BigTIFF (tiffdetail::needs_bigtiff): on the worst case of the payload; an overview file: of the sum of its levels
        size_t worst = 0, nstrips = 0;
        if (overview_levels == 0) {
            set_geometry(width, height, &worst, &nstrips);
        } else {
            for (int k = overview_levels; k >= 1; --k)                         // (level 1 last: its geometry is the first directory's)
                set_geometry((int)(((long)width - 1) >> k) + 1, ((height - 1) >> k) + 1, &worst, &nstrips);
        }
        mBig = tiffdetail::needs_bigtiff(worst, nstrips);
        mF = fopen(path.c_str(), "wb");
        if (!mF) throw std::runtime_error("open file [" + path + "] failed");
        if (mBig) {
            const unsigned char h[16] = {'I', 'I', 43, 0, 8, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // directory offset patched in close()
            put(h, 16);
        } else {
            const unsigned char h[8] = {'I', 'I', 42, 0, 0, 0, 0, 0};
            put(h, 8);
        }
        mPos = mBig ? 16 : 8;
        mLink = mBig ? 8 : 4;
    }

    // geometry of the directory being written (an overview file: of the current level)
    int width() const { return mW; }
    long height() const { return mH; }
    int levels_left() const { return mLevelsLeft; }                            // overview file: levels still to come, this one included

    void write_rows(const uint16_t *rows, long count)
    {
        if (mRowsDone + count > mH) throw std::logic_error("TiffWriterU16: too many rows");
        if (mComp == TIFF_NONE) {
            std::vector<uint16_t> tmp;
            for (long r = 0; r < count; ++r) {
                if (mRowsDone % mRowsPerStrip == 0) { mStripOff.push_back(mPos); mStripLen.push_back(0); }
                const uint16_t *src = rows + (size_t)r * mW * mSpp;
                if (mSwap) { tmp.resize((size_t)mW * 4); tiffdetail::swap_row(src, tmp.data(), (size_t)mW); src = tmp.data(); }
                put(src, mRowBytes);
                mStripLen.back() += mRowBytes;
                mPos += mRowBytes;
                ++mRowsDone;
            }
            return;
        }
        // compressed: whole strips are encoded straight from the caller's rows in bounded batches (a few strips per
        // worker thread at a time) and written in order; only the rows of a strip left incomplete by this call are kept
        const size_t rw = (size_t)mW * mSpp;
        mRowsDone += count;
        const bool last = mRowsDone == mH;
        long r = 0;
        if (!mPending.empty()) {
            long have = (long)(mPending.size() / rw);
            const long take = std::min<long>(count, mRowsPerStrip - have);
            mPending.insert(mPending.end(), rows, rows + (size_t)take * rw);
            r = take;
            have += take;
            if (have == mRowsPerStrip || (last && r == count)) {
                encode_strips(mPending.data(), have);
                mPending.clear();
            }
        }
        const long full = (count - r) / mRowsPerStrip;
        // a batch: a few strips per worker thread and at least 64 MiB of rows, so that a batch is worth the threads it starts
        const long batch = std::max<long>(2 * (long)tiffdetail::worker_count(), (long)(((size_t)64 << 20) / (mRowBytes * (size_t)mRowsPerStrip)) + 1);
        for (long k0 = 0; k0 < full; k0 += batch) {
            const long nk = std::min(batch, full - k0);
            encode_strips(rows + (size_t)(r + k0 * mRowsPerStrip) * rw, nk * mRowsPerStrip);
        }
        r += full * mRowsPerStrip;
        if (r < count) {
            if (last) encode_strips(rows + (size_t)r * rw, count - r);           // the last, short strip
            else mPending.insert(mPending.end(), rows + (size_t)r * rw, rows + (size_t)count * rw);
        }
    }

    // an overview file: the current level is complete, its directory is written and the rows of the next level follow
    void next_directory()
    {
        if (!mF || mLevelsLeft < 2) throw std::logic_error("TiffWriterU16: no further directory");
        end_directory();
        --mLevelsLeft;
        size_t worst = 0, nstrips = 0;
        set_geometry((mW + 1) / 2, (mH + 1) / 2, &worst, &nstrips);
        mRowsDone = 0;
        mStripOff.clear();
        mStripLen.clear();
        mScratch.clear();                                                      // (sized for the previous level's strips)
        if (fseeko(mF, (off_t)mPos, SEEK_SET) != 0) { fclose(mF); mF = nullptr; throw std::runtime_error("TiffWriterU16: seek failed"); }
        mPositioned = false;
    }

    void close()
    {
        if (!mF) return;
        if (mLevelsLeft > 1) { fclose(mF); mF = nullptr; throw std::logic_error("TiffWriterU16: levels missing"); }
        end_directory();
        if (fclose(mF) != 0) { mF = nullptr; throw std::runtime_error("TiffWriterU16: close failed"); }
        mF = nullptr;
    }

    ~TiffWriterU16()
    {
        try { wait_write(); } catch (...) {}
        if (mF) fclose(mF);
    }
    bool bigtiff() const { return mBig; }

    // Reserve the file's blocks ahead of the pixels (uncompressed files: header + payload are known up front).  On tmpfs and
    // on extent file systems allocating the pages is the larger part of a buffered write: a product writer
    // that is idle while the strip is still being read does it then, and the payload write that follows is a copy.  Best effort.
    void preallocate()
    {
        if (mComp != TIFF_NONE || !mF) return;
        fflush(mF);
        (void)posix_fallocate(fileno(mF), 0, (off_t)(mPos + mRowBytes * (uint64_t)mH));
    }

    // Uncompressed files only: the whole pixel payload (height x width x spp samples, already in FILE sample order) is written
    // by someone else at the returned byte offset -- the staging layer, straight from HBM (oip_write_device_to_file_at) --
    // between begin_external_payload() and end_external_payload(); close() then appends the directory.
    uint64_t begin_external_payload()
    {
        if (mComp != TIFF_NONE || mRowsDone != 0) throw std::logic_error("TiffWriterU16: external payload needs an empty uncompressed file");
        if (mSwap) throw std::logic_error("TiffWriterU16: external payload is written in file sample order");
        // right behind the header, where write_rows() would put it: the file is the same bytes either way
        if (fflush(mF) != 0) throw std::runtime_error("TiffWriterU16: write failed");
        return mPos;
    }
    void end_external_payload()
    {
        for (long r = 0; r < mH; r += mRowsPerStrip) {
            const long n = std::min<long>(mRowsPerStrip, mH - r);
            mStripOff.push_back(mPos);
            mStripLen.push_back((uint64_t)n * mRowBytes);
            mPos += (uint64_t)n * mRowBytes;
        }
        mRowsDone = mH;
        if (fseeko(mF, (off_t)mPos, SEEK_SET) != 0) throw std::runtime_error("TiffWriterU16: seek failed");
    }

    // LZW and Deflate files whose strips were encoded elsewhere (the device: oip_tiff_lzw_strips_u16 / oip_tiff_deflate_strips_u16 on
    // an image in file sample order):
    // the packed strips are written by the caller at the offset begin_external_strips() returns -- where write_rows() would
    // have put the first one -- and end_external_strips() takes their offsets inside that block and their sizes.
    long rows_per_strip() const { return mRowsPerStrip; }
    uint64_t begin_external_strips()
    {
        if (mComp == TIFF_NONE || mRowsDone != 0) throw std::logic_error("TiffWriterU16: external strips need an empty LZW or Deflate file");
        if (mSwap) throw std::logic_error("TiffWriterU16: external strips are written in file sample order");
        if (fflush(mF) != 0) throw std::runtime_error("TiffWriterU16: write failed");
        return mPos;
    }
    void end_external_strips(const uint64_t *off, const uint64_t *len, size_t n, uint64_t payload_bytes)
    {
        if (n != (size_t)((mH + mRowsPerStrip - 1) / mRowsPerStrip)) throw std::logic_error("TiffWriterU16: strip count");
        if (!mBig && mPos + payload_bytes > 0xFFFFF000ull) throw std::runtime_error("TiffWriterU16: classic TIFF overflow");
        for (size_t k = 0; k < n; ++k) {
            if ((off[k] & 1) || off[k] + len[k] > payload_bytes) throw std::logic_error("TiffWriterU16: strip outside its payload");
            mStripOff.push_back(mPos + off[k]);
            mStripLen.push_back(len[k]);
        }
        mPos += payload_bytes;
        mRowsDone = mH;
        mPositioned = true;
    }

private:
    // strip geometry of a width x height image; adds what it may take in the file to *worst and its strips to *nstrips
    void set_geometry(int width, long height, size_t *worst, size_t *nstrips)
    {
        mW = width;
        mH = height;
        mRowBytes = (size_t)width * mSpp * 2;
        const size_t data = mRowBytes * (size_t)height;
        // Strips: 8 MiB uncompressed (their offsets are arithmetic); LZW: whole rows up to 64 KiB (cv::imwrite and GDAL write 8
        // KB strips; libtiff's table restarts every ~5 KB of sensor data, so the strip size does not change the ratio).  An
        // LZW strip is the unit of parallel work of whoever encodes it: a lane of the device encoder (csrc/tifflzw.hip: 25000
        // strips for a 7500 x 25000 x 4 product), a thread of the host encoder below -- both write the same strips, so a file
        // is the same bytes whoever encoded it.
        // Deflate takes the same strips: a stream is a wave of the device encoder (csrc/tiffdeflate.hip).
        mRowsPerStrip = mComp != TIFF_NONE ? (long)((64u << 10) / mRowBytes) : (long)((8u << 20) / mRowBytes);
        if (mRowsPerStrip < 1) mRowsPerStrip = 1;
        if (mRowsPerStrip > height) mRowsPerStrip = height;
        const size_t ns = ((size_t)height + mRowsPerStrip - 1) / mRowsPerStrip;
        *worst += tiffdetail::worst_payload(data, mComp, ns);
        *nstrips += ns;
    }

    // the strip tables and the directory of the image whose rows are complete, linked behind the header or the previous directory
    void end_directory()
    {
        wait_write();
        if (mRowsDone != mH || !mPending.empty()) { fclose(mF); mF = nullptr; throw std::logic_error("TiffWriterU16: rows missing"); }
        if (mPositioned && fseeko(mF, (off_t)mPos, SEEK_SET) != 0) { fclose(mF); mF = nullptr; throw std::runtime_error("TiffWriterU16: seek failed"); }
        if (mPos & 1) { const unsigned char z = 0; put(&z, 1); ++mPos; }
        // out-of-line arrays first
        const uint64_t nstrips = mStripOff.size();
        tiffdetail::TiffDirectory d;
        d.big = mBig; d.reduced = mLevelsLeft > 0; d.width = (uint64_t)mW; d.height = (uint64_t)mH; d.spp = mSpp; d.compression = mComp;
        d.rows_per_strip = (uint64_t)mRowsPerStrip; d.nchunks = nstrips; d.offsets = mStripOff[0]; d.counts = mStripLen[0];
        const size_t osz = d.field();
        if (!mBig && mPos + nstrips * 8 + 4096 > 0xFFFFFFFFull) { fclose(mF); mF = nullptr; throw std::runtime_error("TiffWriterU16: classic TIFF overflow"); }
        if (!d.fits(nstrips, osz)) {
            d.offsets = mPos; for (uint64_t v : mStripOff) putv(v, osz);
            d.counts = mPos; for (uint64_t v : mStripLen) putv(v, osz);
        }
        if (!d.fits((uint64_t)mSpp, 2)) {
            d.bitsAt = mPos; for (int i = 0; i < mSpp; ++i) putv(16, 2);
            d.formatAt = mPos; for (int i = 0; i < mSpp; ++i) putv(1, 2);
        }
        if (mPos & 1) { const unsigned char z = 0; put(&z, 1); ++mPos; }
        const uint64_t ifd = mPos;
        std::vector<unsigned char> dir;
        d.append_to(dir, 0);
        put(dir.data(), dir.size());
        mPos += dir.size();
        fseeko(mF, (off_t)mLink, SEEK_SET);
        putv_raw(ifd, osz);
        mLink = mPos - osz;
    }

    // encode `nrows` rows (whole strips, the last one possibly short) on a few threads and append them to the file.
    // No allocation per strip: a worker copies + differences a strip in a scratch buffer of its own and encodes it into its
    // region of one of two arenas that alternate between batches (the previous batch is still being written from the other).
    // Per-strip `new` of 1 + 1.5 MB on 32-64 threads made the encoder wait for the kernel's page-fault and unmap paths
    // instead of coding (round 4: the LZW product did not get faster with more threads or smaller strips until this went).
    void encode_strips(const uint16_t *rows, long nrows)
    {
        const size_t rw = (size_t)mW * mSpp;
        const long nstrips = (nrows + mRowsPerStrip - 1) / mRowsPerStrip;
        const size_t stripBytes = (size_t)mRowsPerStrip * rw * 2, worst = tiffdetail::chunk_worst(stripBytes, mComp);
        Arena &ar = mArena[mArenaCur];
        mArenaCur ^= 1;
        if (ar.cap < (size_t)nstrips * worst) { ar.p.reset(new uint8_t[(size_t)nstrips * worst]); ar.cap = (size_t)nstrips * worst; }
        if (mScratch.size() < (size_t)tiffdetail::worker_count()) mScratch.resize((size_t)tiffdetail::worker_count());
        std::vector<size_t> len((size_t)nstrips);
        uint8_t *base = ar.p.get();
        tiffdetail::parallel_for_t((size_t)nstrips, [&](size_t k, int t) {
            const long r0 = (long)k * mRowsPerStrip;
            const long n = std::min<long>(mRowsPerStrip, nrows - r0);
            if (!mScratch[(size_t)t]) mScratch[(size_t)t].reset(new uint16_t[(size_t)mRowsPerStrip * rw]);
            len[k] = tiffdetail::encode_chunk(rows + (size_t)r0 * rw, n, (size_t)mW, mSpp, mSwap, mScratch[(size_t)t].get(), base + k * worst, mComp);
        });
        // the batch goes to the file on a thread of its own (positioned writes) while the caller brings down and encodes the
        // next one; the previous batch's write is waited for -- and its error raised -- first
        wait_write();
        std::vector<uint64_t> at((size_t)nstrips);
        for (long k = 0; k < nstrips; ++k) {
            if (mPos & 1) ++mPos;                                       // strips start on even offsets (the gap reads as zero)
            if (!mBig && mPos + len[(size_t)k] > 0xFFFFF000ull) throw std::runtime_error("TiffWriterU16: classic TIFF overflow");
            at[(size_t)k] = mPos;
            mStripOff.push_back(mPos);
            mStripLen.push_back(len[(size_t)k]);
            mPos += len[(size_t)k];
        }
        if (fflush(mF) != 0) throw std::runtime_error("TiffWriterU16: write failed");
        mPositioned = true;
        const int fd = fileno(mF);
        mWrite = std::async(std::launch::async, [fd, base, worst, len, at] {
            for (size_t k = 0; k < len.size(); ++k) tiffdetail::pwrite_all(fd, base + k * worst, len[k], at[k], "TiffWriterU16");
        });
    }
    void wait_write() { if (mWrite.valid()) mWrite.get(); }

    void put(const void *p, size_t n)
    {
        if (fwrite(p, 1, n, mF) != n) throw std::runtime_error("TiffWriterU16: write failed");
    }
    void putv_raw(uint64_t v, size_t n)
    {
        unsigned char b[8];
        for (size_t i = 0; i < n; ++i) b[i] = (unsigned char)(v >> (8 * i));
        put(b, n);
    }
    void putv(uint64_t v, size_t n) { putv_raw(v, n); mPos += n; }

    FILE *mF = nullptr;
    int mW;
    long mH;
    int mSpp;
    bool mSwap, mBig = false;
    int mComp;
    size_t mRowBytes = 0;
    long mRowsPerStrip = 1, mRowsDone = 0;
    struct Arena { std::unique_ptr<uint8_t[]> p; size_t cap = 0; };
    Arena mArena[2];                                    // encoded strips of the batch being encoded / being written
    int mArenaCur = 0;
    std::vector<std::unique_ptr<uint16_t[]>> mScratch;  // one strip of differenced samples per worker
    uint64_t mPos = 0;
    int mLevelsLeft = 0;                // overview file: directories still to be written (0: a one-image file)
    uint64_t mLink = 0;                 // where the offset of the next directory goes: in the header, then in the previous directory
    std::vector<uint64_t> mStripOff, mStripLen;
    std::vector<uint16_t> mPending;
    std::future<void> mWrite;           // the batch of encoded strips being written
    bool mPositioned = false;           // positioned writes have moved past the FILE's own position
};

// Reader for little-endian, chunky, unsigned 16-bit TIFF / BigTIFF in strips or tiles, uncompressed, LZW or Deflate (predictor 1
// or 2): what the writers here (above, and oip_tifftiled.hpp), cv::imwrite and GDAL's GTiff driver (INTERLEAVE=PIXEL, with or
// without TILED=YES) produce.  Samples are returned in file order.  Every header field is checked before it sizes an allocation
// or a read.  Only the first directory is read: the internal overviews of a COG are ignored.
// Tiles (322 TileWidth, 323 TileLength, 324 TileOffsets, 325 TileByteCounts) may have any positive size; they are numbered
// row-major, every one holds TileWidth x TileLength pixels (the part outside the image is padding and is dropped), and
// predictor 2 runs along each row of a tile.
// read_tiff_layout: the checked header alone -- geometry, encoding and the table of its strips or tiles, its "chunks" -- for a
// caller that brings the chunks in itself (the device decoder: oip_host.hpp::read_tiff_to_device).
struct TiffLayout {
    uint64_t width = 0, height = 0, spp = 0, compression = 1, predictor = 1, rows_per_strip = 0;
    uint64_t tile_width = 0, tile_length = 0;          // 0: strips.  Tiled: rows_per_strip is 0 and offs / lens hold the tiles, row-major
    std::vector<uint64_t> offs, lens;
    bool tiled() const { return tile_width != 0; }
    const char *chunk_name() const { return tiled() ? "tile" : "strip"; }
    uint64_t row_bytes() const { return width * spp * 2; }
    // Chunk k holds `rows` rows of `pitch` pixels; the first `cols` pixels of each belong at (row, col) of the image and on the rows
    // below it (the rest of a tile is padding).  It decodes to bytes() bytes.
    struct Chunk {
        uint64_t row, col, rows, cols, pitch, spp;
        uint64_t bytes() const { return rows * pitch * spp * 2; }
    };
    Chunk chunk(uint64_t k) const
    {
        if (!tiled()) return {k * rows_per_strip, 0, std::min(rows_per_strip, height - k * rows_per_strip), width, width, spp};
        const uint64_t ntx = (width + tile_width - 1) / tile_width, tj = k / ntx, ti = k - tj * ntx;
        return {tj * tile_length, ti * tile_width, tile_length, std::min(tile_width, width - ti * tile_width), tile_width, spp};
    }
};

namespace tiffdetail {
inline TiffLayout read_layout(const TiffSource &src)
{
    auto fail = [&](const std::string &m) { src.fail(m); };
    const uint64_t fsize = src.size;
    TiffLayout lay;
    uint64_t &W = lay.width, &H = lay.height, &S = lay.spp, &comp = lay.compression, &pred = lay.predictor, &rps = lay.rows_per_strip;
    uint64_t &TW = lay.tile_width, &TL = lay.tile_length, planar = 1, bits = 0, fmt = 1;
    bool stripTags = false, tileTags = false;
    std::vector<uint64_t> &offs = lay.offs, &lens = lay.lens;
    S = 1;
    read_directory(src, nullptr, [&](uint16_t id, uint64_t cnt, auto val) {
        switch (id) {
            case 256: W = val(0); break;
            case 257: H = val(0); break;
            case 258: bits = val(0); for (uint64_t k = 1; k < cnt; ++k) if (val(k) != bits) fail("mixed sample depths"); break;
            case 259: comp = val(0); break;
            case 273: case 324: (id == 273 ? stripTags : tileTags) = true; offs.resize(cnt); for (uint64_t k = 0; k < cnt; ++k) offs[k] = val(k); break;
            case 277: S = val(0); break;
            case 278: rps = val(0); break;
            case 279: case 325: (id == 279 ? stripTags : tileTags) = true; lens.resize(cnt); for (uint64_t k = 0; k < cnt; ++k) lens[k] = val(k); break;
            case 284: planar = val(0); break;
            case 317: pred = val(0); break;
            case 339: fmt = val(0); break;
            case 322: tileTags = true; TW = val(0); break;
            case 323: tileTags = true; TL = val(0); break;
            default: break;
        }
    });
    if (stripTags && tileTags) fail("strip tags and tile tags are both present");
    const bool tiled = tileTags;
    if (comp == 32946) comp = TIFF_DEFLATE;                                     // the number Deflate had before Adobe's 8
    if (comp != TIFF_NONE && comp != TIFF_LZW && comp != TIFF_DEFLATE)
        fail("compression " + std::to_string(comp) + " is not supported (none, LZW and Deflate are)");
    if (pred != 1 && pred != 2) fail("predictor " + std::to_string(pred) + " is not supported");
    if (bits != 16 || fmt != 1 || planar != 1) fail("only chunky unsigned 16-bit samples are supported");
    if (!W || !H || W > 0x7FFFFFFFull || H > 0x7FFFFFFFull || S == 0 || S > 16) fail("missing or implausible geometry");
    if (tiled && (!TW || !TL)) fail("a tiled TIFF needs TileWidth and TileLength, both positive");
    if (offs.empty() || offs.size() != lens.size()) fail(tiled ? "missing tile tags" : "missing strip tags");
    const uint64_t row_bytes = W * S * 2;
    if (H > (~(uint64_t)0) / row_bytes || row_bytes * H > ((uint64_t)1 << 46)) fail("implausible image size");
    if (tiled) {
        if (TW > 0xFFFFFFFFull / TL || TW * TL > 0xFFFFFFFFull / (S * 2)) fail("a tile of 4 GiB or more");
        if (offs.size() != ((W + TW - 1) / TW) * ((H + TL - 1) / TL)) fail("tile count does not match the tile grid");
        rps = 0;
    } else {
        if (rps == 0 || rps > H) rps = H;
        if (offs.size() != (H + rps - 1) / rps) fail("strip count does not match RowsPerStrip");
    }
    // From here on strips and tiles are chunks: chunk_bytes is what a whole one decodes to, `decoded` what all of them do (the tiles
    // with their padding, the strips without the rows the last one lacks)
    const std::string chunk = tiled ? "tile" : "strip";
    const uint64_t chunk_bytes = tiled ? TW * TL * S * 2 : rps * row_bytes;
    const unsigned __int128 decoded = tiled ? (unsigned __int128)chunk_bytes * offs.size() : (unsigned __int128)row_bytes * H;
    unsigned __int128 packed = 0;
    for (size_t k = 0; k < offs.size(); ++k) {
        if (offs[k] > fsize || lens[k] > fsize - offs[k]) fail(chunk + " outside the file");
        if (tiled && comp == TIFF_NONE && lens[k] != chunk_bytes) fail("an uncompressed tile does not have the size of a tile");
        packed += lens[k];
    }
    if (!tiled && comp == TIFF_NONE) {
        uint64_t total = 0;
        for (uint64_t l : lens) { if (l > row_bytes * H - total) fail("strip sizes exceed the image"); total += l; }
        if (total != row_bytes * H) fail("strip sizes do not cover the image");
    }
    if (comp != TIFF_NONE) {
        // Header fields alone must not size the allocation: the chunks present bound what the image can decode to.
        // LZW: a 12-bit code (1.5 bytes) expands to at most 4096 - 258 bytes, 2560 for each byte of input.
        // Deflate: the densest thing a stream holds is a match: it produces at most 258 bytes (length symbol 285) and costs at least
        // 2 bits, a 1-bit length code and a 1-bit distance code.  So a byte of input decodes to at most 4 x 258 = 1032 bytes, and
        // block headers, the zlib wrapper and literals only lower that.
        if (comp == TIFF_DEFLATE)
            for (uint64_t l : lens) if (l >= oipinflate::kMaxStream) fail("a compressed " + chunk + " of 4 GiB or more");
        if (decoded / (comp == TIFF_LZW ? 2560 : 1032) > packed + 16) fail("image size is implausible for its compressed " + chunk + "s");
        if (comp == TIFF_DEFLATE && chunk_bytes >= oipinflate::kMaxStream) fail("a " + chunk + " of 4 GiB or more");
    }
    return lay;
}
}  // namespace tiffdetail

inline TiffLayout read_tiff_layout(const std::string &path) { return tiffdetail::read_layout(tiffdetail::TiffSource(path, "read TIFF")); }

// width, height and samples per pixel of a file the reader takes
inline void read_tiff_geometry(const std::string &path, int *width, long *height, int *spp)
{
    const TiffLayout lay = read_tiff_layout(path);
    *width = (int)lay.width; *height = (long)lay.height; *spp = (int)lay.spp;
}

inline void read_tiff_u16(const std::string &path, int *width, long *height, int *spp, std::vector<uint16_t> *out)
{
    const tiffdetail::TiffSource src(path, "read TIFF");
    const TiffLayout lay = tiffdetail::read_layout(src);
    const uint64_t W = lay.width, H = lay.height, S = lay.spp, comp = lay.compression, row_bytes = lay.row_bytes();
    try {
        out->resize((size_t)(W * H * S));
    } catch (const std::bad_alloc &) {
        src.fail("not enough memory for a " + std::to_string(W) + " x " + std::to_string(H) + " x " + std::to_string(S) + " image");
    }
    unsigned char *dstb = reinterpret_cast<unsigned char *>(out->data());
    if (!lay.tiled() && comp == TIFF_NONE) {
        size_t pos = 0;
        for (size_t k = 0; k < lay.offs.size(); ++k) {
            src.read(lay.offs[k], dstb + pos, (size_t)lay.lens[k]);
            pos += (size_t)lay.lens[k];
        }
    } else {
        // The chunks in batches, each decoded on a worker thread.  A strip's rows lie in the image as they lie in the strip: it is
        // decoded in place.  A tile is decoded into a buffer of its own (an uncompressed one is used as read), un-differenced along
        // its own rows, and its part inside the image copied out.
        const std::string name = lay.chunk_name();
        const size_t batch = lay.tiled() ? std::max<size_t>(1, std::min<size_t>(64, ((size_t)256 << 20) / (size_t)lay.chunk(0).bytes())) : 64;
        for (size_t k0 = 0; k0 < lay.offs.size(); k0 += batch) {
            const size_t kn = std::min(batch, lay.offs.size() - k0);
            std::vector<std::vector<unsigned char>> raw(kn);
            for (size_t j = 0; j < kn; ++j) { raw[j].resize((size_t)lay.lens[k0 + j]); src.read(lay.offs[k0 + j], raw[j].data(), raw[j].size()); }
            tiffdetail::parallel_for(kn, [&](size_t j) {
                const uint64_t k = k0 + j;
                const TiffLayout::Chunk c = lay.chunk(k);
                const size_t want = (size_t)c.bytes();
                std::vector<unsigned char> dec;
                unsigned char *data = raw[j].data();
                if (comp != TIFF_NONE) {
                    if (lay.tiled()) dec.resize(want);
                    data = lay.tiled() ? dec.data() : dstb + (size_t)(c.row * row_bytes);
                    const size_t got = tiffdetail::decode_chunk(comp, raw[j].data(), raw[j].size(), data, want, name + " " + std::to_string(k) + " of [" + path + "]");
                    if (got != want) src.fail(name + " " + std::to_string(k) + " decodes to " + std::to_string(got) + " bytes, " + std::to_string(want) + " expected");
                }
                if (!lay.tiled()) return;
                for (uint64_t r = 0; r < std::min<uint64_t>(c.rows, H - c.row); ++r) {
                    unsigned char *trow = data + (size_t)(r * c.pitch * S * 2);
                    if (lay.predictor == 2) {
                        std::vector<uint16_t> line((size_t)(c.pitch * S));     // (a tile's bytes need not be aligned for u16)
                        memcpy(line.data(), trow, line.size() * 2);
                        tiffdetail::predictor2_decode(line.data(), (size_t)c.pitch, (int)S);
                        memcpy(trow, line.data(), line.size() * 2);
                    }
                    memcpy(dstb + (size_t)(((c.row + r) * W + c.col) * S * 2), trow, (size_t)(c.cols * S * 2));
                }
            });
        }
    }
    if (!lay.tiled() && lay.predictor == 2) {
        uint16_t *px = out->data();
        tiffdetail::parallel_for((size_t)H, [&](size_t r) { tiffdetail::predictor2_decode(px + r * (size_t)(W * S), (size_t)W, (int)S); });
    }
    *width = (int)W; *height = (long)H; *spp = (int)S;
}

// like the writer class, but with an explicit sample order: out sample i = in sample order[i]
inline void write_tiff_u16_mapped(const std::string &path, const uint16_t *data, int width, long height, const int order[4],
                                  int compression = TIFF_NONE)
{
    TiffWriterU16 w(path, width, height, 4, false, compression);
    const long chunk = std::max<long>(1, (long)(((size_t)32 << 20) / ((size_t)width * 8)));
    std::vector<uint16_t> rows((size_t)chunk * width * 4);
    for (long r0 = 0; r0 < height; r0 += chunk) {
        const long n = std::min(chunk, height - r0);
        for (long r = 0; r < n; ++r) {
            const uint16_t *src = data + (size_t)(r0 + r) * width * 4;
            uint16_t *dst = rows.data() + (size_t)r * width * 4;
            for (int x = 0; x < width; ++x)
                for (int c = 0; c < 4; ++c) dst[4 * (size_t)x + c] = src[4 * (size_t)x + order[c]];
        }
        w.write_rows(rows.data(), n);
    }
    w.close();
}

inline void write_tiff_u16(const std::string &path, const uint16_t *data, int width, long height, int spp, bool opencv_order,
                           int compression = TIFF_NONE)
{
    TiffWriterU16 w(path, width, height, spp, opencv_order, compression);
    w.write_rows(data, height);             // (batches its strips itself: 2 per encoder thread at a time)
    w.close();
}

// The 8-bit sibling for the browse image of `oip quicklook`: classic little-endian TIFF, uncompressed strips of about 8 MiB,
// chunky, spp 1 (BlackIsZero) or 3 (RGB).  Tens of MB at most: no BigTIFF, no LZW, one buffered write.
inline void write_tiff_u8(const std::string &path, const uint8_t *data, int width, long height, int spp)
{
    if (width <= 0 || height <= 0 || (spp != 1 && spp != 3) || !data) throw std::invalid_argument("write_tiff_u8: bad geometry");
    const uint64_t rowBytes = (uint64_t)width * spp, total = rowBytes * (uint64_t)height;
    long rps = (long)(((uint64_t)8 << 20) / rowBytes);
    rps = rps < 1 ? 1 : (rps > height ? height : rps);
    const uint64_t nstrips = ((uint64_t)height + rps - 1) / rps;
    if (total + nstrips * 8 + 4096 > 0xFFFFF000ull) throw std::invalid_argument("write_tiff_u8: image too large for a classic TIFF");
    std::vector<unsigned char> tail;                                     // everything behind the pixels
    auto putv = [&](uint64_t v, int n) { tiffdetail::put_le(tail, v, (size_t)n); };
    uint64_t pos = 8 + total;
    if (pos & 1) { putv(0, 1); ++pos; }
    tiffdetail::TiffDirectory d;
    d.width = (uint64_t)width; d.height = (uint64_t)height; d.spp = spp; d.bits = 8; d.sample_format = false;
    d.rows_per_strip = (uint64_t)rps; d.nchunks = nstrips; d.offsets = 8; d.counts = total;
    if (!d.fits(nstrips, 4)) {
        d.offsets = pos; for (uint64_t k = 0; k < nstrips; ++k) putv(8 + k * rps * rowBytes, 4);
        d.counts = pos + nstrips * 4;
        for (uint64_t k = 0; k < nstrips; ++k) putv(std::min<uint64_t>((uint64_t)rps, (uint64_t)height - k * rps) * rowBytes, 4);
        pos += nstrips * 8;
    }
    if (!d.fits((uint64_t)spp, 2)) { d.bitsAt = pos; for (int i = 0; i < spp; ++i) putv(8, 2); pos += (uint64_t)spp * 2; }
    const uint64_t ifd = pos;
    d.append_to(tail, 0);
    unsigned char head[8] = {'I', 'I', 42, 0, 0, 0, 0, 0};
    for (int i = 0; i < 4; ++i) head[4 + i] = (unsigned char)(ifd >> (8 * i));
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) throw std::runtime_error("open file [" + path + "] failed");
    const bool ok = fwrite(head, 1, 8, f) == 8 && fwrite(data, 1, (size_t)total, f) == (size_t)total &&
                    fwrite(tail.data(), 1, tail.size(), f) == tail.size();
    if (fclose(f) != 0 || !ok) throw std::runtime_error("write file [" + path + "] failed");
}

// The reader of a mask (`oip regcheck --mask`): exactly what write_tiff_u8 writes with spp 1 -- classic little-endian TIFF,
// uncompressed, chunky, 8 bits, one sample, strips in line order -- and nothing else; what it refuses it names.  Every header
// field is checked before it sizes an allocation or a read.
inline void read_tiff_u8(const std::string &path, int *width, long *height, std::vector<uint8_t> *out)
{
    const tiffdetail::TiffSource src(path, "read 8-bit TIFF");
    auto fail = [&](const std::string &m) { src.fail(m); };
    const uint64_t fsize = src.size;
    uint64_t W = 0, H = 0, comp = 1, planar = 1, S = 1, bits = 1, rps = 0;
    std::vector<uint64_t> offs, lens;
    tiffdetail::read_directory(src, "BigTIFF is not supported (a mask is a classic TIFF)", [&](uint16_t id, uint64_t cnt, auto val) {
        switch (id) {
            case 256: W = val(0); break;
            case 257: H = val(0); break;
            case 258: bits = val(0); for (uint64_t k = 1; k < cnt; ++k) if (val(k) != bits) fail("mixed sample depths"); break;
            case 259: comp = val(0); break;
            case 273: offs.resize(cnt); for (uint64_t k = 0; k < cnt; ++k) offs[k] = val(k); break;
            case 277: S = val(0); break;
            case 278: rps = val(0); break;
            case 279: lens.resize(cnt); for (uint64_t k = 0; k < cnt; ++k) lens[k] = val(k); break;
            case 284: planar = val(0); break;
            case 322: case 323: case 324: case 325: fail("tiled TIFF is not supported (strips only)"); break;
            default: break;
        }
    });
    if (comp != TIFF_NONE) fail("compression " + std::to_string(comp) + " is not supported (a mask is uncompressed)");
    if (bits != 8) fail(std::to_string(bits) + "-bit samples are not supported (a mask has 8)");
    if (S != 1 || planar != 1) fail(std::to_string(S) + " samples per pixel are not supported (a mask has 1)");
    if (!W || !H || W > 0x7FFFFFFFull || H > 0x7FFFFFFFull) fail("missing or implausible geometry");
    if (offs.empty() || offs.size() != lens.size()) fail("missing strip tags");
    if (H > 0xFFFFFFFFull / W) fail("implausible image size");
    if (rps == 0 || rps > H) rps = H;
    if (offs.size() != (H + rps - 1) / rps) fail("strip count does not match RowsPerStrip");
    uint64_t total = 0;
    for (size_t k = 0; k < offs.size(); ++k) {
        if (offs[k] > fsize || lens[k] > fsize - offs[k]) fail("truncated file");
        if (lens[k] != std::min<uint64_t>(rps, H - k * rps) * W) fail("strip sizes do not cover the image");
        total += lens[k];
    }
    out->resize((size_t)total);
    size_t pos = 0;
    for (size_t k = 0; k < offs.size(); ++k) {
        src.read(offs[k], out->data() + pos, (size_t)lens[k]);
        pos += (size_t)lens[k];
    }
    *width = (int)W;
    *height = (long)H;
}

}  // namespace OIPGPU
