// tifflzw.hip -- the strips of an LZW TIFF product encoded on the GPU (round 4).
//
// The reference writes its aligned MSS product through cv::imwrite (preproc.h:167-185: OpenCV's TIFF encoder, LZW with the
// horizontal predictor) and the stitched MSS through GDAL with COMPRESS=LZW PREDICTOR=2 (imageop.h:460-567).  Both libraries
// encode on the host, strip by strip.  With the image already in HBM and one process per GPU -- a sixteenth of a node's host
// cores each -- that encoder was what the product waited for (0.45-0.5 s for 1.5 GB on 16 cores, csrc/oip_tiff.hpp).  TIFF
// strips are independent LZW streams, so a strip is a lane here: 25000 strips of a 7500 x 25000 x 4 image are 25000 lanes
// that each walk their 60 KB once.
//
// Per lane: the horizontal differences of its rows (predictor 2: sample minus the same channel of the previous pixel, modulo
// 2^16, restarting at every row) as a little-endian byte stream, through the string-table coder TIFF 6.0 section 13
// specifies and libtiff implements (csrc/oip_tiff.hpp::lzw_encode_to is the same coder on the host and the parity check of
// this one: tests/test_gpu_tifflzw.py compares files byte for byte): MSB-first codes of 9..12 bits, ClearCode 256 first,
// EndOfInformation 257 last, first free code 258, the code widens after entry 511 / 1023 / 2047 is assigned, ClearCode when
// entry 4093 is.  The string table is a lane's own 8192 x 8 B open-addressing table in HBM: a slot is
// (generation : 12 | prefix code : 12 | byte : 8) in its high word and the entry's code in its low word; ClearCode starts a new generation instead of wiping 64 KB.
// Every step is a dependent 8-byte load from a 2 GB region: the kernel is bound by HBM latency, not bandwidth -- ~1 us a
// byte, 60 ms for any number of strips up to the 32768 a launch takes -- which is still eight times what the host cores did.
// The encoded strips land in fixed slots (worst case: 1.5 bytes per byte); a second kernel packs them behind one another
// (even offsets, as the host writer places them; oip_tiffencode.h) so that the payload leaves the device as one block.
#include "oip_internal.h"
#include "oip_tiffdecode.h"
#include "oip_tiffencode.h"

#include <cstdint>
#include <vector>

namespace {

constexpr int kSlots = 8192;                     // per-lane table slots (4094 entries at most: load factor < 0.5)
static_assert(kOipTiffLzw.table_bytes == kSlots * sizeof(unsigned long long), "the plan's scratch holds a lane's table");
constexpr long kStripsPerLaunch = 32768;         // of the decoder

struct LzwJob {
    const uint16_t *img;
    long rows;
    int width, spp;
    long rps;                                    // rows per strip
    long nstrips, strip0;                        // strips of the image, first strip of this launch
    uint8_t *slots;
    size_t slot_bytes;                           // multiple of 4
    unsigned long long *tab;
    unsigned *len;                               // [nstrips]
    int active;                                  // lanes of a wave that take a strip
};

struct LzwState {
    unsigned long long *tab;
    unsigned *occ;                               // LDS: this lane's "slot holds an entry of the current generation" bits, word w at occ[w * stride]
    int stride;
    uint8_t *out;
    unsigned long long acc;
    unsigned o;                                  // bytes written
    int nbits, width, next, ent;
    unsigned gen;
};

__device__ __forceinline__ void lzw_put(LzwState &s, unsigned code)
{
    s.acc = (s.acc << s.width) | code;
    s.nbits += s.width;
    if (s.nbits >= 32) {
        const unsigned w = (unsigned)(s.acc >> (s.nbits - 32));
        *reinterpret_cast<unsigned *>(s.out + s.o) = __builtin_bswap32(w);       // MSB first
        s.o += 4;
        s.nbits -= 32;
    }
}

__device__ __forceinline__ void lzw_clear_occ(LzwState &s)
{
#pragma unroll 8
    for (int w = 0; w < kSlots / 32; ++w) s.occ[w * s.stride] = 0u;
}

// One byte through the coder.  Three steps out of four of sensor data are misses, and a miss that lands on an EMPTY slot --
// most of them: the table is at most half full -- does not need the slot's contents to know it: a bit per slot in LDS (1 KB per
// lane, lane-interleaved: no bank conflicts) says so, and the step costs an LDS read and two stores nobody waits for instead
// of a dependent load from HBM.  Only occupied slots are loaded (hits, and collisions with another string).
__device__ __forceinline__ void lzw_byte(LzwState &s, unsigned c)
{
    const unsigned key = ((unsigned)s.ent << 8) | c;                             // 20 bits
    const unsigned want = (s.gen << 20) | key;
    unsigned h = (key * 2654435761u) >> (32 - 13);
    for (;;) {
        const unsigned bits = s.occ[(h >> 5) * s.stride];
        if (!((bits >> (h & 31)) & 1u)) break;                                   // empty in this generation
        const unsigned long long slot = s.tab[h];
        if ((unsigned)(slot >> 32) == want) { s.ent = (int)(unsigned)slot; return; }
        h = (h + 1) & (kSlots - 1);
    }
    lzw_put(s, (unsigned)s.ent);
    s.ent = (int)c;
    s.tab[h] = ((unsigned long long)want << 32) | (unsigned)s.next;
    s.occ[(h >> 5) * s.stride] |= 1u << (h & 31);
    ++s.next;
    if (s.next == 4094) {                        // table full: clear (libtiff: free_ent == CODE_MAX - 1)
        lzw_put(s, 256u);
        ++s.gen;
        lzw_clear_occ(s);
        s.width = 9;
        s.next = 258;
    } else if (s.next == (1 << s.width) && s.width < 12) {
        ++s.width;
    }
}

__global__ __launch_bounds__(64) void lzw_strips_kernel(LzwJob j)
{
    extern __shared__ unsigned occ[];                                            // kSlots / 32 words per active lane; a workgroup is one wave
    if ((int)threadIdx.x >= j.active) return;
    const long local = (long)blockIdx.x * j.active + threadIdx.x;
    const long k = j.strip0 + local;
    if (k >= j.nstrips) return;
    LzwState s;
    s.tab = j.tab + (size_t)local * kSlots;
    s.occ = occ + threadIdx.x;
    s.stride = j.active;
    lzw_clear_occ(s);
    s.out = j.slots + (size_t)local * j.slot_bytes;
    s.acc = 0; s.o = 0; s.nbits = 0; s.width = 9; s.next = 258; s.ent = -1; s.gen = 1;
    lzw_put(s, 256u);
    const long r0 = k * j.rps;                   // (not tiff_strip_span: the loops want the end row, and from the row count the compiler
                                                 // makes other instructions than these)
    long r1 = r0 + j.rps;
    if (r1 > j.rows) r1 = j.rows;
    const size_t rowSamples = (size_t)j.width * j.spp;
    // the first byte of the strip only seeds the prefix; every later byte goes through the table
    auto feed = [&](unsigned c) {
        if (s.ent < 0) s.ent = (int)c; else lzw_byte(s, c);
    };
    if (j.spp == 4) {
        for (long r = r0; r < r1; ++r) {
            const unsigned long long *row = reinterpret_cast<const unsigned long long *>(j.img + (size_t)r * rowSamples);
            unsigned long long prev = 0, cur = row[0];
            for (int x = 0; x < j.width; ++x) {
                const unsigned long long nxt = x + 1 < j.width ? row[x + 1] : 0ull;     // in flight under this pixel's 8 bytes
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const unsigned d = ((unsigned)(cur >> (16 * c)) - (unsigned)(prev >> (16 * c))) & 0xffffu;
                    feed(d & 0xffu);
                    feed(d >> 8);
                }
                prev = cur;
                cur = nxt;
            }
        }
    } else {                                     // one sample per pixel
        for (long r = r0; r < r1; ++r) {
            const uint16_t *row = j.img + (size_t)r * rowSamples;
            unsigned prev = 0;
            for (int x = 0; x < j.width; ++x) {
                const unsigned cur = row[x];
                const unsigned d = (cur - prev) & 0xffffu;
                feed(d & 0xffu);
                feed(d >> 8);
                prev = cur;
            }
        }
    }
    lzw_put(s, (unsigned)s.ent);
    ++s.next;                                    // libtiff's LZWPostEncode: the last code counts as an entry too
    if (s.next == 4094) { lzw_put(s, 256u); s.width = 9; }
    else if (s.next == (1 << s.width) && s.width < 12) ++s.width;
    lzw_put(s, 257u);
    while (s.nbits >= 8) { s.out[s.o++] = (uint8_t)(s.acc >> (s.nbits - 8)); s.nbits -= 8; }
    if (s.nbits > 0) s.out[s.o++] = (uint8_t)(s.acc << (8 - s.nbits));
    j.len[k] = s.o;
}

// ---- the other direction: the LZW strips of a TIFF file decoded on the device ------------------------------------------------
// cv::imread of the two ALIGNED.TIFF inputs of the MSS stitch (imageop.h:380-388) decodes on the host; here the strips' bytes go
// from the file into HBM as they are (oip_read_file_to_device) and a lane decodes a strip straight into the image.  An LZW
// string is always a substring of what has already been decoded -- entry `next` is the previous string plus the first byte of
// the current one, and those are adjacent in the output -- so a table entry is (position, length) in the lane's own output and
// emitting a code is a forward byte copy inside the image (which also makes the KwKwK case, code == next, nothing special).
// Same acceptance rules as tiffdetail::lzw_decode (oip_tiff.hpp): a stream that ends without EndOfInformation is tolerated, a
// first code >= 256, a code beyond the table or a table that fills without ClearCode are corrupt; a strip must decode to
// exactly its rows.  Predictor 2 is undone by the same lane afterwards (running sums along its rows).
struct LzwDecJob {
    const uint8_t *file;
    const unsigned long long *off, *len;         // [nstrips]: strip offsets inside `file`, byte counts
    long rows;
    int width, spp;
    long rps, nstrips, strip0;
    int predictor;
    uint16_t *img;
    unsigned long long *tab;                     // per lane 4096 x (position | length << 32)
    unsigned *got;                               // [nstrips] bytes a strip decoded to
    int *status;                                 // [nstrips] 0 ok, 1 bad first code, 2 code beyond the table, 3 table full
    int active;                                  // lanes of a wave that take a strip
};

__global__ __launch_bounds__(64) void lzw_decode_kernel(LzwDecJob j)
{
    if ((int)threadIdx.x >= j.active) return;
    const long local = (long)blockIdx.x * j.active + threadIdx.x;
    const long k = j.strip0 + local;
    if (k >= j.nstrips) return;
    unsigned long long *tab = j.tab + (size_t)local * 4096;
    const uint8_t *in = j.file + j.off[k];
    const unsigned n = (unsigned)j.len[k];
    const size_t rowBytes = (size_t)j.width * j.spp * 2;
    const OipStripSpan span = tiff_strip_span(k, j.rows, j.rps);
    const long r0 = span.r0, nr = span.nr;
    uint8_t *out = reinterpret_cast<uint8_t *>(j.img) + (size_t)r0 * rowBytes;
    const unsigned cap = (unsigned)((size_t)nr * rowBytes);
    int width = 9, next = 258, status = 0;
    bool have_old = false;
    unsigned long long acc = 0;
    int nbits = 0;
    unsigned ip = 0, pos = 0, old_pos = 0, old_len = 0;
    for (;;) {
        while (nbits < width && ip < n) { acc = (acc << 8) | in[ip++]; nbits += 8; }
        if (nbits < width) break;                                              // stream ends without EOI: tolerated, as libtiff does
        const unsigned code = (unsigned)(acc >> (nbits - width)) & ((1u << width) - 1);
        nbits -= width;
        if (code == 257u) break;
        if (code == 256u) { width = 9; next = 258; have_old = false; continue; }
        if (!have_old) {
            if (code >= 256u) { status = 1; break; }
            if (pos < cap) out[pos] = (uint8_t)code;
            old_pos = pos; old_len = 1; ++pos;
            have_old = true;
            continue;
        }
        if (next >= 4096) { status = 3; break; }
        if (code > (unsigned)next) { status = 2; break; }
        const unsigned long long fresh = (unsigned long long)old_pos | ((unsigned long long)(old_len + 1) << 32);
        tab[next] = fresh;                                                     // previous string + this string's first byte
        unsigned clen = 1;
        if (code < 256u) {
            if (pos < cap) out[pos] = (uint8_t)code;
        } else {
            const unsigned long long e = code == (unsigned)next ? fresh : tab[code];
            const unsigned src = (unsigned)e;
            clen = (unsigned)(e >> 32);
            for (unsigned i = 0; i < clen; ++i)
                if (pos + i < cap) out[pos + i] = out[src + i];               // src + i < pos + i: forward copy, overlap included
        }
        old_pos = pos; old_len = clen; pos += clen;
        ++next;
        if (next >= (1 << width) - 1 && width < 12) ++width;                   // early change
        if (pos >= cap && ip >= n) break;
    }
    j.got[k] = pos;
    j.status[k] = status;
    if (status != 0 || pos != cap || j.predictor != 2) return;
    // predictor 2: every sample plus the same channel of the previous pixel, modulo 2^16, row by row
    if (j.spp == 4) {
        for (long r = 0; r < nr; ++r) {
            unsigned long long *row = reinterpret_cast<unsigned long long *>(out + (size_t)r * rowBytes);
            unsigned long long prev = row[0];
            for (int x = 1; x < j.width; ++x) {
                prev = padd16(prev, row[x]);
                row[x] = prev;
            }
        }
    } else {
        const int spp = j.spp;
        for (long r = 0; r < nr; ++r) {
            uint16_t *row = reinterpret_cast<uint16_t *>(out + (size_t)r * rowBytes);
            for (long i = spp; i < (long)j.width * spp; ++i) row[i] = (uint16_t)(row[i] + row[i - spp]);
        }
    }
}
}  // namespace

extern "C" size_t oip_tiff_lzw_worst_bytes(long rows, int width, int spp, long rows_per_strip)
{
    return plan_tiff_encode(kOipTiffLzw, rows, width, spp, rows_per_strip).worst_bytes;
}

extern "C" size_t oip_tiff_lzw_scratch_bytes(long rows, int width, int spp, long rows_per_strip)
{
    return plan_tiff_encode(kOipTiffLzw, rows, width, spp, rows_per_strip).scratch_bytes;
}

extern "C" int oip_tiff_lzw_strips_u16(oip_ctx *ctx, const uint16_t *d_img, long rows, int width, int spp, long rows_per_strip,
                                       uint8_t *d_payload, size_t payload_cap, uint64_t *strip_off, uint64_t *strip_len,
                                       size_t *payload_bytes, void *d_scratch, size_t scratch_bytes)
{
    OIP_CHECK_CTX(ctx);
    return oip_tiff_encode(ctx, "oip_tiff_lzw_strips_u16", kOipTiffLzw, d_img, rows, width, spp, rows_per_strip, d_payload, payload_cap, strip_off, strip_len,
                           payload_bytes, d_scratch, scratch_bytes, [&](long s0, long ns, const OipTiffSlots &t) {
        // Lanes of a wave that take a strip.  A wave steps at the pace of its slowest lane -- the longest probe chain, a code to
        // flush -- so 64 coders in lockstep are slower than 4 (116 -> 86 ms at 25000 strips, 76 -> 45 ms at 2000: the vector ALU
        // idles either way, and more, emptier waves give the memory system more independent chains to overlap).
        const int active = 4;
        LzwJob j{d_img, rows, width, spp, rows_per_strip, t.nstrips, s0, t.slots, t.slot_bytes, reinterpret_cast<unsigned long long *>(t.tables), t.len, active};
        // No slot is read before the lane's occupancy bit says it was written in the current generation, so the tables need no
        // initial VALUE -- but memory fresh from hipMalloc is first touched far cheaper by a linear fill than by the kernel's
        // scattered stores (a launch on untouched scratch: 250-350 ms instead of 90-120); tables and output slots alike.
        if (s0 == 0) OIP_HIP(ctx, hipMemsetAsync(t.tables, 0, t.launch_bytes, ctx->stream));
        OipProfScope prof(ctx, kOipTiffLzw.encode_scope);
        hipLaunchKernelGGL(lzw_strips_kernel, dim3((unsigned)((ns + active - 1) / active)), dim3(64), (size_t)active * (kSlots / 32) * 4, ctx->stream, j);
        return (int)OIP_OK;
    });
}

static const char *lzw_reason(int status)
{
    return status == 1 ? "bad first code" : status == 2 ? "code beyond the table" : "table full without ClearCode";
}

// (the refusals are oip_tiff_decode's and no others: the Deflate decoder has two more)
extern "C" int oip_tiff_lzw_decode_u16(oip_ctx *ctx, const uint8_t *d_file, size_t file_bytes, const uint64_t *strip_off,
                                       const uint64_t *strip_len, long nstrips, long rows, int width, int spp, long rows_per_strip,
                                       int predictor, uint16_t *d_img)
{
    OIP_CHECK_CTX(ctx);
    const long per = nstrips < kStripsPerLaunch ? nstrips : kStripsPerLaunch;                       // (a lane: 4096 table entries)
    return oip_tiff_decode(ctx, "oip_tiff_lzw_decode_u16", kOipTiffLzw.name, lzw_reason, (uint64_t)1 << 32, per > 0 ? (size_t)per * 4096 * 8 : 0, d_file, file_bytes,
                           strip_off, strip_len, nstrips, rows, width, spp, rows_per_strip, predictor, d_img, [&](const OipTiffStreams &t) {
        for (long s0 = 0; s0 < nstrips; s0 += per) {
            const long ns = nstrips - s0 < per ? nstrips - s0 : per;
            // (the decoder does not gain from emptier waves as the encoder does: 64 / 16 / 8 / 4 lanes 98 / 102 / 115 / 120 ms)
            const int active = 64;
            LzwDecJob j{d_file, t.off, t.len, rows, width, spp, rows_per_strip, nstrips, s0, predictor, d_img,
                        reinterpret_cast<unsigned long long *>(t.tables), t.got, t.status, active};
            OipProfScope prof(ctx, "lzw_decode_kernel");
            hipLaunchKernelGGL(lzw_decode_kernel, dim3((unsigned)((ns + active - 1) / active)), dim3(64), 0, ctx->stream, j);
        }
    });
}
