// oip_jpeg.h -- one baseline JPEG scan coder (ITU-T T.81 SOF0, 8 bits, grey or YCbCr 4:4:4, the typical Huffman tables of
// Annex K.3, a restart interval per row of 8 x 8 blocks) for the host and for a wave of the device, written once.  No libjpeg.
// include/oip_c.h states the arithmetic to the bit (oip_jpeg_scan_u8); tests/_jpeg_ref.py restates it.  The browse JPEG of
// `oip quicklook --format jpeg` comes out of this: csrc/jpeg.hip gives it its lanes, oip_jpeg_interval_host one lane.
//
// A restart interval depends on nothing outside its own 8 image lines (the DC predictors start at 0, the bits at a byte), so the
// intervals are independent streams, as the strips of the LZW and Deflate coders are.  The encoder is templated on a lane policy
// -- lane(), sync(), scan(v) (exclusive prefix sum over the lanes), sum(v), rank(flag, &total) (set flags in the lanes below /
// in all), aor(p, v) (atomic or on a word of the work area) and tick() (a cycle counter, for the profile) -- and on the number of lanes L.  An interval is coded in rounds of
// L blocks, block g of the interval (MCU g / nch, component g % nch: for RGB the lanes go Y, Cb, Cr, Y, ...) in lane g % L:
//   - the lanes stage the round's samples in the work area: the image bytes, read where they lie at any pitch and alignment,
//     columns and lines past the image clamped to its last ones (the padding), and for RGB converted to Y, Cb, Cr on the way;
//   - every lane transforms and quantises its block in registers and leaves the 64 coefficients, in zigzag order, in the work area;
//   - the DC predecessor is the block nch lanes below, or for the first nch lanes the last block of that component of the round
//     before (sh.pred);
//   - every lane walks its coefficients once to count its bits; an exclusive prefix sum over the lanes, plus the bits the round
//     before left over (fewer than 8), gives every lane its bit position; a second walk ors its codes into the round's bit
//     buffer;
//   - the buffer's whole bytes go out L at a time: a lane's byte lands behind the bytes below it plus one for each 0xFF among
//     them (the second prefix sum, a count over flags), a 0xFF with its 0x00 behind it.  The last round pads with 1-bits first.
// What comes out is a function of the interval's 8 lines, nch and the quality alone: not of L, of the interval's index, of the
// pitch or of any alignment.
//
// Memory safety is a property of the construction: every image read is clamped to [0, w) x [0, h); a bit position is checked
// against the buffer before a word is touched (it cannot fire: a block is at most kBlockBits long, see below); every store to
// dst is guarded by cap.
#pragma once

#include <cerrno>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#define OIP_JPEG_HD __host__ __device__
#else
#define OIP_JPEG_HD
#endif
#if defined(__clang__)
#define OIP_JPEG_UNROLL _Pragma("unroll")
#else
#define OIP_JPEG_UNROLL
#endif

namespace oipjpeg {

// A DC difference is below 2^11 (a DC term lies in -1024 .. 1016) and costs at most 9 + 11 bits; an AC term is below 2^10 (the
// largest, 1020, is the (4, 4) term of a +-checkerboard of 2 x 2 cells) and costs at most 16 + 10: 20 + 63 * 26 = 1658 bits a block.
constexpr unsigned kBlockBits = 64 * 26;
constexpr unsigned kBlockBytes = kBlockBits / 8 * 2;  // every byte a stuffed 0xFF: 416, the bound of oip_jpeg_worst_bytes

// ---- the tables of T.81 Annex K (typed from the standard) ----------------------------------------------------------------------
// K.1 / K.2: base quantisation tables, natural (row-major) order
constexpr uint8_t kBaseLuma[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                                   18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t kBaseChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// the natural index of zigzag position k (figure 5)
constexpr uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                  35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// K.3: BITS (the number of codes of each length 1..16) and HUFFVAL (the symbols in code order) of the four typical tables
struct HuffSpec {
    uint8_t bits[16];
    int nvals;
    const uint8_t *vals;
};
constexpr uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t kAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
    0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
    0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
    0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
constexpr uint8_t kAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1,
    0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
    0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
    0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
    0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
// [class 0 DC / 1 AC][table 0 luma / 1 chroma]
constexpr HuffSpec kHuff[2][2] = {{{{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, 12, kDcVals}, {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, 12, kDcVals}},
                                  {{{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, 162, kAcLumaVals}, {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}, 162, kAcChromaVals}}};

// What a coder reads of them, for one quality: table 0 luma (and grey), 1 chroma
struct Tables {
    uint32_t rq[2][64];                           // zigzag order: floor(2^32 / 2q) + 1, see quantise()
    uint32_t dc[2][12];                           // by category: code << 8 | length
    uint32_t ac[2][256];                          // by run << 4 | size; 0 where T.81 has no such symbol
    uint16_t q[2][64];                            // zigzag order
};

// the IJG rule: scale = Q < 50 ? 5000 / Q : 200 - 2 Q, q = clamp((base * scale + 50) / 100, 1, 255); natural index n
inline int quant_entry(int table, int quality, int n)
{
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const int q = ((table ? kBaseChroma : kBaseLuma)[n] * scale + 50) / 100;
    return q < 1 ? 1 : (q > 255 ? 255 : q);
}

inline void make_tables(int quality, Tables *t)
{
    memset(t, 0, sizeof *t);
    for (int i = 0; i < 2; ++i) {
        for (int k = 0; k < 64; ++k) {
            const int q = quant_entry(i, quality, kNatural[k]);
            t->q[i][k] = (uint16_t)q;
            t->rq[i][k] = (uint32_t)((1ull << 32) / (2u * (unsigned)q)) + 1u;
        }
        for (int cls = 0; cls < 2; ++cls) {       // Annex C: codes of a length count up, a longer length continues doubled
            const HuffSpec &s = kHuff[cls][i];
            unsigned code = 0;
            int k = 0;
            for (unsigned len = 1; len <= 16; ++len) {
                for (int j = 0; j < s.bits[len - 1]; ++j, ++k, ++code) (cls ? t->ac[i] : t->dc[i])[s.vals[k]] = code << 8 | len;
                code <<= 1;
            }
        }
    }
}

// SOI .. SOS of the file, appended to `out` (a container with push_back): APP0 (JFIF 1.01, no units, 1 : 1, no thumbnail), a DQT per
// table in use, SOF0 (components 1..nch, 1 x 1 sampling, table 0 / 1 / 1), a DHT per table in use (DC 0, AC 0, DC 1, AC 1), DRI (one
// row of MCUs), SOS (all components, Ss 0, Se 63, Ah Al 0)
template <class Bytes>
inline void headers(int w, int h, int nch, int quality, Bytes *out)
{
    auto b = [&](unsigned v) { out->push_back((uint8_t)v); };
    auto seg = [&](unsigned marker, unsigned body) { b(0xff); b(marker); b((body + 2) >> 8); b((body + 2) & 255u); };
    b(0xff); b(0xd8);
    seg(0xe0, 14);
    const uint8_t app0[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    for (uint8_t v : app0) b(v);
    const int ntab = nch == 1 ? 1 : 2;
    for (int i = 0; i < ntab; ++i) {
        seg(0xdb, 65);
        b(i);
        for (int k = 0; k < 64; ++k) b(quant_entry(i, quality, kNatural[k]));
    }
    seg(0xc0, 6 + 3 * nch);
    b(8); b(h >> 8); b(h & 255); b(w >> 8); b(w & 255); b(nch);
    for (int c = 0; c < nch; ++c) { b(c + 1); b(0x11); b(c ? 1 : 0); }
    for (int i = 0; i < ntab; ++i)
        for (int cls = 0; cls < 2; ++cls) {
            const HuffSpec &s = kHuff[cls][i];
            seg(0xc4, 17 + s.nvals);
            b(cls << 4 | i);
            for (int k = 0; k < 16; ++k) b(s.bits[k]);
            for (int k = 0; k < s.nvals; ++k) b(s.vals[k]);
        }
    const int mcus = (w + 7) / 8;
    seg(0xdd, 2);
    b(mcus >> 8); b(mcus & 255);
    seg(0xda, 4 + 2 * nch);
    b(nch);
    for (int c = 0; c < nch; ++c) { b(c + 1); b(c ? 0x11 : 0x00); }
    b(0); b(63); b(0);
}

// ---- the coder --------------------------------------------------------------------------------------------------------------
// What one encode works in: LDS of a single-wave workgroup on the device (L = 64: about 29 KiB, five workgroups a CU), heap on the
// host (L = 1).
template <int L>
struct alignas(8) Shared {
    static constexpr int kMcus = (L + 1) / 3 + 1;                    // the MCUs that L consecutive blocks of an RGB interval touch
    static constexpr int kStage = 64 * L > 192 * kMcus ? 64 * L : 192 * kMcus;
    static constexpr unsigned kBitWords = (7 + L * kBlockBits + 7) / 32 + 2;
    uint8_t stage[kStage];                        // grey: 8 rows of 8 L samples; RGB: per component 8 rows of 8 kMcus
    uint32_t bits[kBitWords];                     // the round's bits, MSB first: stream bit i is bit 31 - i % 32 of word i / 32
    int16_t coef[64 * L];                         // zigzag position k of lane l at k * L + l
    int dcs[L];                                   // the round's quantised DC terms
    int pred[3];                                  // per component: the last DC term of the rounds before
    Tables tab;
};

struct HostLane {
    unsigned lane() const { return 0; }
    void sync() const {}
    unsigned scan(unsigned) const { return 0; }
    unsigned sum(unsigned v) const { return v; }
    unsigned rank(bool f, unsigned *total) const { *total = f; return 0; }
    void aor(uint32_t *p, uint32_t v) const { *p |= v; }
    unsigned long long tick() const { return 0; }
};

// R, G, B -> component c of Y, Cb, Cr (JFIF's BT.601 full range in 16-bit fixed point; arithmetic shifts; 0 .. 255 without a clamp)
OIP_JPEG_HD inline int ycbcr(int c, int r, int g, int b)
{
    if (c == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (c == 1) return (-11058 * r - 21710 * g + 32768 * b + 8421375) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + 8421375) >> 16;
}

template <class P, int L>
struct Encoder {
    const P &p;
    Shared<L> &sh;
    // cycles by P::tick() in the five phases of a round: staging, transform, counting (first walk and prefix sum), placing (second
    // walk), stuffing (the 0xFF count and the stores).  Read by profiles/jpeg_bench.py, by nothing else.
    enum { kStage, kTransform, kCount, kPlace, kStuff, kPhases };
    unsigned long long cycles[kPhases] = {0, 0, 0, 0, 0};

    OIP_JPEG_HD Encoder(const P &p_, Shared<L> &sh_) : p(p_), sh(sh_) {}

    // sign(f) ((2 |f| + q) / 2q) with the division as a multiplication: for m = floor(2^32 / d) + 1 and n d < 2^32,
    // floor(n m / 2^32) = floor(n / d) (m d exceeds 2^32 by at most d); here n = 2 |f| + q < 4200 and d = 2 q <= 510
    OIP_JPEG_HD static int quantise(int f, unsigned q, uint32_t rq)
    {
        const unsigned n = 2u * (unsigned)(f < 0 ? -f : f) + q;
        const int v = (int)(((unsigned long long)n * rq) >> 32);
        return f < 0 ? -v : v;
    }

    // the block at `s` (8 rows, `stride` bytes apart, 8-byte aligned) of table t: level shift, row and column pass of the
    // integer DCT, quantisation; the coefficients go to sh.coef in zigzag order; returns the DC term
    OIP_JPEG_HD int transform(const uint8_t *s, int stride, int t, unsigned lane)
    {
        // T[k][n] = rint(8192 c_k cos((2n + 1) k pi / 16)), c_0 = sqrt(1/8), c_k = 1/2
        constexpr int T[64] = {2896, 2896,  2896,  2896,  2896,  2896,  2896,  2896,  4017, 3406,  2276,  799,   -799,  -2276, -3406, -4017,
                               3784, 1567,  -1567, -3784, -3784, -1567, 1567,  3784,  3406, -799,  -4017, -2276, 2276,  4017,  799,   -3406,
                               2896, -2896, -2896, 2896,  2896,  -2896, -2896, 2896,  2276, -4017, 799,   3406,  -3406, -799,  4017,  -2276,
                               1567, -3784, 3784,  -1567, -1567, 3784,  -3784, 1567,  799,  -2276, 3406,  -4017, 4017,  -3406, 2276,  -799};
        constexpr int N[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                               35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
        int t1[64], f[64];
OIP_JPEG_UNROLL
        for (int y = 0; y < 8; ++y) {
            unsigned long long v;
            memcpy(&v, __builtin_assume_aligned(s + y * stride, 8), 8);
            int x[8];
OIP_JPEG_UNROLL
            for (int n = 0; n < 8; ++n) x[n] = (int)((v >> (8 * n)) & 255u) - 128;
OIP_JPEG_UNROLL
            for (int k = 0; k < 8; ++k) {
                int a = 512;
OIP_JPEG_UNROLL
                for (int n = 0; n < 8; ++n) a += T[k * 8 + n] * x[n];
                t1[y * 8 + k] = a >> 10;
            }
        }
OIP_JPEG_UNROLL
        for (int u = 0; u < 8; ++u)
OIP_JPEG_UNROLL
            for (int k = 0; k < 8; ++k) {
                int a = 32768;
OIP_JPEG_UNROLL
                for (int m = 0; m < 8; ++m) a += T[k * 8 + m] * t1[m * 8 + u];
                f[k * 8 + u] = a >> 16;
            }
        int dc = 0;
OIP_JPEG_UNROLL
        for (int k = 0; k < 64; ++k) {
            const int v = quantise(f[N[k]], sh.tab.q[t][k], sh.tab.rq[t][k]);
            sh.coef[k * L + (int)lane] = (int16_t)v;
            if (k == 0) dc = v;
        }
        return dc;
    }

    // T.81 F.1.2 for the lane's block: the DC difference's category and bits, then run/size symbols with ZRL (15/0) and EOB (0/0);
    // no EOB when coefficient 63 is not zero.  out(value, n): n bits, 1 <= n <= 27, MSB first
    template <class Out>
    OIP_JPEG_HD void walk(unsigned lane, int diff, int t, Out &&out) const
    {
        auto coded = [&](uint32_t entry, int v) {                                // the symbol's code, then the value's low `size` bits
            const unsigned a = (unsigned)(v < 0 ? -v : v);
            const unsigned size = a ? 32u - (unsigned)__builtin_clz(a) : 0u;
            const unsigned low = (unsigned)(v < 0 ? v - 1 : v) & ((1u << size) - 1u);
            out((entry >> 8) << size | low, (entry & 255u) + size);
        };
        auto size_of = [](int v) { const unsigned a = (unsigned)(v < 0 ? -v : v); return a ? 32u - (unsigned)__builtin_clz(a) : 0u; };
        coded(sh.tab.dc[t][size_of(diff) % 12u], diff);                          // (a category is below 12, see kBlockBits)
        unsigned run = 0;
        for (int k = 1; k < 64; ++k) {
            const int v = sh.coef[k * L + (int)lane];
            if (v == 0) { ++run; continue; }
            for (; run > 15; run -= 16) coded(sh.tab.ac[t][0xf0], 0);
            coded(sh.tab.ac[t][(run << 4 | size_of(v)) & 255u], v);
            run = 0;
        }
        if (run) coded(sh.tab.ac[t][0x00], 0);
    }

    OIP_JPEG_HD void put(unsigned pos, unsigned v, unsigned n) const         // v below 2^n at stream bit `pos` of the round
    {
        const unsigned w = pos >> 5;
        if (n == 0 || w + 1 >= Shared<L>::kBitWords) return;
        const unsigned long long x = (unsigned long long)v << (64u - (pos & 31u) - n);
        p.aor(&sh.bits[w], (uint32_t)(x >> 32));
        if ((uint32_t)x) p.aor(&sh.bits[w + 1], (uint32_t)x);
    }

    // Interval `interval` (lines 8 * interval .. + 7) of the image; its bytes go to dst[0, cap) -- dst null: nowhere -- and their
    // number comes back, whether they fitted or not.  sh.tab holds the tables of the quality.
    OIP_JPEG_HD size_t run(const uint8_t *img, long pitch, int w, long h, int nch, long interval, uint8_t *dst, size_t cap)
    {
        const unsigned lane = p.lane();
        const int mcus = (w + 7) / 8, nb = mcus * nch;
        const int stride = nch == 1 ? 8 * L : 8 * Shared<L>::kMcus;
        for (unsigned i = lane; i < Shared<L>::kBitWords; i += L) sh.bits[i] = 0;
        for (unsigned i = lane; i < 3; i += L) sh.pred[i] = 0;
        p.sync();
        unsigned carry = 0;                                                      // bits of the rounds before that did not fill a byte
        size_t out = 0;
        unsigned long long t0 = p.tick();
        auto phase = [&](int i) { const unsigned long long t1 = p.tick(); cycles[i] += t1 - t0; t0 = t1; };
        for (int g0 = 0; g0 < nb; g0 += L) {
            const int m0 = g0 / nch;
            const int m1 = (g0 + L - 1) / nch < mcus - 1 ? (g0 + L - 1) / nch : mcus - 1;
            const int npx = (m1 - m0 + 1) * 8;
            for (int y = 0; y < 8; ++y) {
                const long line = interval * 8 + y < h - 1 ? interval * 8 + y : h - 1;
                const uint8_t *row = img + (size_t)line * (size_t)pitch;
                for (int i = (int)lane; i < npx; i += L) {
                    const int x = m0 * 8 + i < w - 1 ? m0 * 8 + i : w - 1;
                    if (nch == 1) {
                        sh.stage[y * stride + i] = row[x];
                    } else {
                        const int r = row[3 * (size_t)x], g = row[3 * (size_t)x + 1], b = row[3 * (size_t)x + 2];
                        for (int c = 0; c < 3; ++c) sh.stage[(c * 8 + y) * stride + i] = (uint8_t)ycbcr(c, r, g, b);
                    }
                }
            }
            p.sync();
            phase(kStage);
            const int g = g0 + (int)lane;
            const bool active = g < nb;
            const int c = active ? g % nch : 0, t = c ? 1 : 0;
            int dc = 0;
            if (active) dc = transform(&sh.stage[c * 8 * stride + (g / nch - m0) * 8], stride, t, lane);
            sh.dcs[lane] = dc;
            p.sync();
            phase(kTransform);
            unsigned nbits = 0;
            int diff = 0;
            if (active) {
                diff = dc - ((int)lane >= nch ? sh.dcs[(int)lane - nch] : sh.pred[c]);
                walk(lane, diff, t, [&](unsigned, unsigned n) { nbits += n; });
            }
            p.sync();                                                            // sh.pred is read above and written below
            if (active && (g + nch >= g0 + L || g + nch >= nb)) sh.pred[c] = dc;
            unsigned pos = carry + p.scan(nbits);
            unsigned total = carry + p.sum(nbits);
            phase(kCount);
            if (active) walk(lane, diff, t, [&](unsigned v, unsigned n) { put(pos, v, n); pos += n; });
            if (g0 + L >= nb && (total & 7u)) {                                  // the interval ends: 1-bits up to a byte
                if (lane == 0) put(total, (1u << (8u - (total & 7u))) - 1u, 8u - (total & 7u));
                total = (total + 7u) & ~7u;
            }
            p.sync();
            phase(kPlace);
            const unsigned nbytes = total >> 3;
            for (unsigned b0 = 0; b0 < nbytes; b0 += L) {
                const unsigned i = b0 + lane;
                const bool valid = i < nbytes;
                const unsigned v = valid ? (sh.bits[i >> 2] >> (24u - 8u * (i & 3u))) & 255u : 0u;
                unsigned nff;
                const unsigned below = p.rank(v == 255u, &nff);
                const size_t o = out + lane + below;
                if (valid && dst) {
                    if (o < cap) dst[o] = (uint8_t)v;
                    if (v == 255u && o + 1 < cap) dst[o + 1] = 0;
                }
                out += (nbytes - b0 < (unsigned)L ? nbytes - b0 : (unsigned)L) + nff;
            }
            carry = total & 7u;
            const uint32_t part = (sh.bits[nbytes >> 2] >> (24u - 8u * (nbytes & 3u))) & 255u;      // the bits behind the last whole byte
            p.sync();
            for (unsigned i = lane; i <= (total + 31u) / 32u; i += L) sh.bits[i] = 0;
            p.sync();
            if (lane == 0) sh.bits[0] = part << 24;
            p.sync();
            phase(kStuff);
        }
        return out;
    }
};

// the host instantiation: interval `interval` into dst[0, cap); its size, or 0 where it does not fit
inline size_t interval_host(const uint8_t *img, long pitch, int w, long h, int nch, int quality, long interval, uint8_t *dst, size_t cap, Shared<1> *work)
{
    make_tables(quality, &work->tab);
    HostLane lane;
    Encoder<HostLane, 1> e(lane, *work);
    const size_t size = e.run(img, pitch, w, h, nch, interval, dst, cap);
    return size <= cap ? size : 0;
}

// The JFIF file of a scan: headers(), then interval k = payload[off[k], off[k] + len[k]) with RST(k mod 8) between one interval and
// the next, none behind the last, then EOI.  False with errno set where the file cannot be written.
inline bool write_file(const char *path, const uint8_t *payload, const uint64_t *off, const uint64_t *len, int w, int h, int nch, int quality)
{
    std::vector<uint8_t> head;
    headers(w, h, nch, quality, &head);
    FILE *f = fopen(path, "wb");
    if (!f) return false;
    bool ok = fwrite(head.data(), 1, head.size(), f) == head.size();
    const long n = (h + 7) / 8;
    for (long k = 0; k < n && ok; ++k) {
        const uint8_t rst[2] = {0xff, (uint8_t)(0xd0 + (k - 1) % 8)};
        if (k) ok = fwrite(rst, 1, 2, f) == 2;
        ok = ok && fwrite(payload + off[k], 1, (size_t)len[k], f) == (size_t)len[k];
    }
    const uint8_t eoi[2] = {0xff, 0xd9};
    ok = ok && fwrite(eoi, 1, 2, f) == 2;
    const int e = errno;
    if (fclose(f) != 0 && ok) return false;
    if (!ok) errno = e;
    return ok;
}

}  // namespace oipjpeg
