// oip_tiffstreams.h -- the arithmetic of the device codecs of TIFF streams (strips or tiles; tifflzw.hip, tiffdeflate.hip), with no
// HIP in it: what a codec is in numbers, the geometry and scratch of an encode call, the even-offset rule of a payload, the scratch
// of a decode call, and the rule that sends a file's streams to the device or to the host's threads.  The drivers
// (oip_tiffencode.h, oip_tiffdecode.h), the hosts (oip_host.hpp) and the host codec (oip_tiff.hpp) read it from here;
// tests/cpp/tiffstreams_test.cpp walks it on the CPU.
#pragma once

#include <cstddef>
#include <cstdint>

#include "oip_deflate.h"                     // oipdeflate::stored_bound, the Deflate codec's worst case

#if defined(__HIPCC__)
#define OIP_TIFF_HD __host__ __device__
#else
#define OIP_TIFF_HD
#endif

namespace OIPGPU {
namespace tiffdetail {
// worst case of an encoded LZW strip of n bytes: one 12-bit code per byte, plus Clear / EOI codes
inline size_t lzw_worst(size_t n) { return n + n / 2 + n / 1024 + 64; }
}  // namespace tiffdetail
}  // namespace OIPGPU

enum OipTiffDirection { OIP_TIFF_READ = 0, OIP_TIFF_WRITE = 1 };

struct OipTiffCodec {
    const char *name;                            // in the messages about a stream
    const char *timing;                          // the hosts' TIMING lines
    const char *encode_scope, *pack_scope;       // profile scopes of the encoder's two kernels
    size_t (*worst)(size_t n);                   // the most an encoded stream of n bytes takes
    size_t table_bytes;                          // encoder scratch per stream of a launch, besides its slot
    long per_launch;                             // streams an encode launch takes
    int image_align, image_align4;               // what the encoder asks of the image's address; of one with 4 samples per pixel
    // the route rule's numbers (tiff_streams_on_device): 0 streams = no rule but the knob
    size_t route_min_streams;
    uint64_t route_max_stream_bytes[2];          // [OipTiffDirection]
};

// LZW: a stream is a lane with a string table of 8192 x 8 B in the scratch; 4-sample pixels are loaded as 64-bit words.  Where its
// streams go is the knob's word alone (OIP_TIFF_GPU_LZW=0: the host's threads; same file bytes, same image -- test and A/B knob).
constexpr OipTiffCodec kOipTiffLzw = {"LZW", "tiff_lzw", "lzw_strips_kernel", "lzw_pack_kernel", OIPGPU::tiffdetail::lzw_worst, 8192 * 8, 32768, 1, 8, 0, {0, 0}};

// Deflate: a stream is a wave that keeps everything but its output in LDS; the image is addressed as u16.
// Which way the streams of a Deflate INPUT go: a wave inflates 4.1 MB/s whatever the layout and the 16 host
// threads about 60 MB/s each, so the device needs at least 16 x 60 / 4.1 = 234 streams in flight to win, and a stream's time on a
// shared device is its bytes / 4.1 MB/s.  Hence: at least 256 strips or tiles, none decoding to more than 2 MiB (the largest stream
// measured: half a second).  Everything else -- few streams, long streams -- and OIP_TIFF_GPU_DEFLATE=0 goes to the host.
// Which way the streams of a Deflate PRODUCT go.  Both ways run the same coder (csrc/oip_deflate.h) and write the same file; what
// differs is where the time goes.  Measured (profiles/deflate_encode.md, profiles/deflate_encode.json by
// profiles/deflate_encode_bench.py: 6144 x 20000 x 4 of 12-bit noise; device events, medians of 20 alternating repetitions; the
// tools' wall time twice each), device against the host's 16 threads:
//   strips of one row (48 KiB, 20000 streams)   encode 0.351 s against 0.732 s; `oip overviews` 1.01-1.13 s against 1.16-1.39 s: device
//   tiles of 128 (128 KiB, 7536 streams)        encode 0.352 s against 0.717 s; `oip cog` 1.32-1.54 s against 2.69-2.96 s:       device
//   tiles of 512 (2 MiB, 480 streams)           encode 0.379 s against 0.784 s in ONE call -- but `oip cog` 4.97-5.03 s against
//                                               3.35-3.66 s, because it encodes batch by batch: a 256 MiB batch is 120 such
//                                               streams for 512 resident waves, and a call lasts as long as its longest stream:  host
// A wave codes 5.5 MB/s, the 16 threads 1.35 GB/s together: a call wins from about 245 streams on and is at its best with 512 or
// more, so a layout goes to the device by default -- the rule being that the device beats the host by more than the 5 % box-to-box
// spread of the tool's wall time -- when it has at least 256 streams and a 256 MiB batch holds at least 512 of them (512 KiB a
// stream: tiles of 256 at 4 samples, of 512 at one; between 128 KiB and 2 MiB nothing was measured, the bound is the model's).
// OIP_TIFF_GPU_DEFLATE=0 sends everything to the host, =2 everything the device encoder takes to the device (test knob).
constexpr OipTiffCodec kOipTiffDeflate = {"Deflate", "tiff_deflate", "deflate_encode_kernel", "deflate_pack_kernel", oipdeflate::stored_bound, 0, 32768, 2, 2,
                                          256, {(uint64_t)2 << 20, (uint64_t)512 << 10}};

constexpr size_t kOipTiffEncodeMaxStrip = (size_t)1 << 30;      // the encoders count a stream's bytes in 32 bits, its worst case included

// Device (true) or the host's threads: the streams of a file being read or written, `nstreams` of at most `streamBytes` decoded
// bytes each; knob: the value of the codec's environment variable, 1 where it is not set (oip_host.hpp::tiff_device_codec reads it).
inline bool tiff_streams_on_device(const OipTiffCodec &c, OipTiffDirection dir, size_t nstreams, uint64_t streamBytes, int knob)
{
    if (knob == 0) return false;
    if (c.route_min_streams == 0) return true;
    if (dir == OIP_TIFF_WRITE && streamBytes > kOipTiffEncodeMaxStrip) return false;
    if (dir == OIP_TIFF_WRITE && knob == 2) return true;
    return nstreams >= c.route_min_streams && streamBytes <= c.route_max_stream_bytes[dir];
}

// rows [r0, r0 + nr) of an image of `rows` rows are strip k of its strips of `rps` rows; the last strip may be short
struct OipStripSpan { long r0, nr; };
OIP_TIFF_HD inline OipStripSpan tiff_strip_span(long k, long rows, long rps)
{
    OipStripSpan s{k * rps, rows - k * rps};
    if (s.nr > rps) s.nr = rps;
    return s;
}

inline size_t tiff_up256(size_t v) { return (v + 255) / 256 * 256; }

// An encode call: rows x width x spp u16 in strips of rps rows.  The scratch is [tables | slots | len | off], every part from a
// multiple of 256 bytes: tables and slots for the streams of one launch, len (u32) and off (u64) for all of them.  The sizes are
// those of any positive geometry; `refusal` says why the encoders do not take it all the same.
struct OipTiffEncodePlan {
    const char *refusal;                         // nullptr, or the words of the refusal
    long nstrips, per_launch;
    size_t strip_bytes, slot_bytes;              // a full strip's samples; its slot, a multiple of 4
    size_t o_tables, o_slots, o_len, o_off;
    size_t worst_bytes;                          // of the payload: every stream at its worst, + 2: to the next even offset, and the payload's even end
    size_t scratch_bytes;
};

inline OipTiffEncodePlan plan_tiff_encode(const OipTiffCodec &c, long rows, int width, int spp, long rps)
{
    OipTiffEncodePlan p{};
    if (rows <= 0 || width <= 0 || spp <= 0 || rps <= 0) { p.refusal = "bad argument"; return p; }
    p.nstrips = (long)(((size_t)rows + rps - 1) / rps);
    p.per_launch = p.nstrips < c.per_launch ? p.nstrips : c.per_launch;
    p.strip_bytes = (size_t)rps * width * spp * 2;
    p.slot_bytes = (c.worst(p.strip_bytes) + 3) / 4 * 4;
    p.o_tables = 0;
    p.o_slots = tiff_up256((size_t)p.per_launch * c.table_bytes);
    p.o_len = p.o_slots + tiff_up256((size_t)p.per_launch * p.slot_bytes);
    p.o_off = p.o_len + tiff_up256((size_t)p.nstrips * sizeof(unsigned));
    p.scratch_bytes = p.o_off + tiff_up256((size_t)p.nstrips * sizeof(unsigned long long));
    p.worst_bytes = (size_t)p.nstrips * (c.worst(p.strip_bytes) + 2);
    if (spp != 1 && spp != 4) p.refusal = "bad argument";
    else if (p.strip_bytes > kOipTiffEncodeMaxStrip) p.refusal = "strip larger than 1 GiB";
    return p;
}

// Streams one behind the other, each from an even offset (as the host writers place them, oip_tiff.hpp): off[k] = pos rounded up
// to even, pos += len[k]; returns the new pos.  Placing [0, k) and then [k, n) from the returned pos is placing [0, n).
inline size_t place_streams(const unsigned *len, size_t n, size_t pos, unsigned long long *off)
{
    for (size_t k = 0; k < n; ++k) {
        pos += pos & 1;
        off[k] = pos;
        pos += len[k];
    }
    return pos;
}

// the scratch of a decode call: [the codec's tables | off | len | got | status], every part from a multiple of 256 bytes
struct OipTiffDecodeLayout { size_t o_off, o_len, o_got, o_status, bytes; };
inline OipTiffDecodeLayout tiff_decode_layout(size_t table_bytes, size_t nstrips)
{
    OipTiffDecodeLayout l;
    l.o_off = tiff_up256(table_bytes);
    l.o_len = l.o_off + tiff_up256(nstrips * 8);
    l.o_got = l.o_len + tiff_up256(nstrips * 8);
    l.o_status = l.o_got + tiff_up256(nstrips * 4);
    l.bytes = l.o_status + tiff_up256(nstrips * 4);
    return l;
}
