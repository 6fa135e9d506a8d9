// oip_inflate.h -- one zlib-stream decoder (RFC 1950 wrapper, RFC 1951 blocks) for the host's threads and for a wave of the
// device, written once.  No libz: the strips and tiles of a Deflate TIFF (compression 8, or 32946) go through this on either side
// (csrc/oip_tiff.hpp::read_tiff_u16 on the host, csrc/tiffdeflate.hip on the device).
//
// The decoder is templated on a lane policy P with lane(), nlanes(), sync(), sum(v) and uni(v): the host instantiates it with one
// lane and no-ops (HostLane below), the device with the 64 lanes of a single-wave workgroup, __syncthreads, a wave reduction and
// "this value is the same in every lane" (what is read from the tables and the staged input is; told so, the compiler keeps
// the bit buffer and everything decided from it in scalar registers and branches once for the wave).  The
// control flow is the same in every lane -- all of them hold the same bit buffer and decode the same symbol -- and only the
// bulk work is divided: staging input, copying a match, filling the primary tables, flushing the window, summing Adler-32.  The
// index arithmetic the device runs is therefore the arithmetic tests/cpp/inflate_test.cpp runs under ASan + UBSan.
//
// Memory safety is a property of the construction, not of the input:
//   - an input byte is read only at an index below the stream's length n; beyond it the reader delivers zeros and counts them,
//     and a decode that consumed one of those bits ends as kTruncated;
//   - the history window is a 32 KiB ring and every index into it is masked;
//   - a token is refused before it is written when it would carry the output past cap, so pos <= cap always and the flush to
//     `out` writes [flushed, pos) only;
//   - the tables are indexed by masked bits and by sums of their own counts; the code-length array by an index checked against
//     HLIT + HDIST (<= 316 < 320).
//
// Acceptance (the yardstick is zlib's inflate; include/oip_c.h states the rules): see Status below, one value per cause.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define OIP_INFLATE_HD __host__ __device__
#else
#define OIP_INFLATE_HD
#endif

namespace oipinflate {

constexpr unsigned kWindow = 32768, kWinMask = kWindow - 1;
constexpr unsigned kStage = 2048;                // staged input bytes
constexpr unsigned kLitBits = 10, kDistBits = 8; // primary tables; longer codes take the canonical walk
constexpr unsigned kRound = 64;                  // a match at distance >= kRound is copied in rounds of kRound bytes
constexpr unsigned kFlushAt = 16384;             // the ring goes to the image when this much of it is new
constexpr unsigned kMaxStream = 0xFFFF0000u;     // n and cap must be below this (32-bit positions with room for look-ahead)

enum Status {
    kOk = 0,
    kBadHeader = 1,        // CM != 8, CINFO > 7, FCHECK wrong or FDICT set
    kBadBlockType = 2,     // BTYPE 3
    kStoredLength = 3,     // LEN != ~NLEN
    kTooManySymbols = 4,   // HLIT > 286 or HDIST > 30
    kCodeLengthCode = 5,   // the code-length code is over-subscribed or incomplete
    kRepeatNoPrevious = 6, // repeat code 16 with no length before it
    kRepeatOverrun = 7,    // a repeat runs past HLIT + HDIST
    kNoEndOfBlock = 8,     // symbol 256 has no code
    kLitLenSet = 9,        // literal/length lengths over-subscribed, or incomplete other than zlib's exception below
    kDistSet = 10,         // distance lengths likewise.  zlib's exception, for both sets: a single code of length 1; and a
                           // distance set may have no code at all (a block of literals only)
    kBadLitLen = 11,       // symbol 286 / 287, or a bit pattern that is no code
    kBadDist = 12,         // symbol 30 / 31, or a bit pattern that is no code
    kDistTooFar = 13,      // a distance that reaches before the start of the output
    kTruncated = 14,       // the stream ends inside a block
    kTooLong = 15,         // decodes to more than cap bytes
    kAdler = 16            // the Adler-32 trailer is present and does not match
};

inline const char *status_text(int s)
{
    switch (s) {
        case kOk: return "ok";
        case kBadHeader: return "bad zlib header";
        case kBadBlockType: return "invalid block type";
        case kStoredLength: return "stored block lengths do not match";
        case kTooManySymbols: return "too many length or distance symbols";
        case kCodeLengthCode: return "invalid code-length code";
        case kRepeatNoPrevious: return "length repeat with no previous length";
        case kRepeatOverrun: return "length repeat past the last symbol";
        case kNoEndOfBlock: return "missing end-of-block code";
        case kLitLenSet: return "invalid literal/length code lengths";
        case kDistSet: return "invalid distance code lengths";
        case kBadLitLen: return "invalid literal/length code";
        case kBadDist: return "invalid distance code";
        case kDistTooFar: return "distance too far back";
        case kTruncated: return "stream ends inside a block";
        case kTooLong: return "more bytes than expected";
        case kAdler: return "Adler-32 mismatch";
        default: return "unknown";
    }
}

// What one decode works in: LDS of a workgroup on the device (about 38 KiB: four waves per CU), heap on the host.
struct alignas(16) Shared {
    uint8_t win[kWindow];                        // ring: byte p of the output at (p + woff) & kWinMask
    uint8_t stage[kStage];                       // input bytes [lo, lo + kStage) of the stream
    uint16_t ltab[1u << kLitBits];               // (symbol << 4 | length) of the code in the index's low bits, 0: longer or none
    uint16_t dtab[1u << kDistBits];
    uint16_t lcnt[16], dcnt[16];                 // codes per length
    uint16_t offs[16];
    uint16_t lsym[288], dsym[32];                // symbols in canonical order
    uint8_t lens[320];
};

struct HostLane {
    unsigned lane() const { return 0; }
    unsigned nlanes() const { return 1; }
    void sync() const {}
    unsigned sum(unsigned v) const { return v; }
    unsigned uni(unsigned v) const { return v; }
};

OIP_INFLATE_HD inline void copy16(void *dst, const void *src)
{
    __builtin_memcpy(__builtin_assume_aligned(dst, 16), __builtin_assume_aligned(src, 16), 16);
}

template <class P>
struct Decoder {
    const P &p;
    Shared &sh;
    const uint8_t *in;
    unsigned n;
    uint8_t *out;
    unsigned cap;
    unsigned long long buf = 0;                  // bit buffer, next bit at bit 0
    unsigned cnt = 0;                            // bits in it
    unsigned ip = 0;                             // bytes fetched, zeros past n included
    unsigned lo = 0, hi = 0;                     // the staged range
    unsigned pos = 0, flushed = 0, woff = 0;
    unsigned a1 = 1, a2 = 0;                     // Adler-32 of [0, flushed)

    OIP_INFLATE_HD Decoder(const P &p_, Shared &sh_, const uint8_t *in_, unsigned n_, uint8_t *out_, unsigned cap_)
        : p(p_), sh(sh_), in(in_), n(n_), out(out_), cap(cap_)
    {
        woff = (unsigned)((uintptr_t)out_ & 15u); // ring and image agree modulo 16: aligned words of one are aligned words of the other
    }

    // ---- input -------------------------------------------------------------------------------------------------------------
    OIP_INFLATE_HD void restage()
    {
        p.sync();
        const unsigned mis = (unsigned)(((uintptr_t)in + ip) & 15u);
        lo = ip >= mis ? ip - mis : 0;
        hi = lo + kStage;
        for (unsigned w = p.lane(); w < kStage / 16; w += p.nlanes()) {
            const unsigned s = lo + 16 * w;
            if (s >= n) continue;                                            // never read: next_byte() asks n first
            if (n - s >= 16 && (((uintptr_t)(in + s)) & 15u) == 0) copy16(sh.stage + 16 * w, in + s);
            else
                for (unsigned b = 0; b < 16; ++b) sh.stage[16 * w + b] = s + b < n ? in[s + b] : (uint8_t)0;
        }
        p.sync();
    }
    OIP_INFLATE_HD unsigned long long uni64(unsigned long long v) const
    {
        return ((unsigned long long)p.uni((unsigned)(v >> 32)) << 32) | p.uni((unsigned)v);
    }
    OIP_INFLATE_HD unsigned next_byte()
    {
        unsigned b = 0;
        if (ip < n) {
            if (ip < lo || ip >= hi) restage();
            b = p.uni(sh.stage[ip - lo]);
        }
        ++ip;
        return b;
    }
    // At least 57 bits in the buffer.  Where eight staged bytes of the stream lie ahead they come in as two aligned 8-byte reads
    // and as many whole bytes as fit are counted in; the bits above cnt are then the low bits of the next byte, which the next
    // refill ORs to the same place again.  Else byte by byte (a chunk's end, the stream's end, and the zeros behind it).
    OIP_INFLATE_HD void refill()
    {
        if (cnt > 56) return;
        if (ip >= lo && ip + 8 <= hi && ip + 8 <= n) {
            const unsigned o = ip - lo, i = o >> 3, s = (o & 7u) * 8;
            unsigned long long q0, q1 = 0;
            __builtin_memcpy(&q0, __builtin_assume_aligned(sh.stage + 8 * i, 8), 8);
            if (s) __builtin_memcpy(&q1, __builtin_assume_aligned(sh.stage + 8 * i + 8, 8), 8);     // (8 i + 16 <= o + 15 <= kStage + 7, and a multiple of 8)
            q0 = uni64(q0); q1 = uni64(q1);
            const unsigned long long v = s ? (q0 >> s) | (q1 << (64 - s)) : q0;
            buf |= v << cnt;
            const unsigned take = (64 - cnt) >> 3;
            ip += take; cnt += 8 * take;
            return;
        }
        while (cnt <= 56) { buf |= (unsigned long long)next_byte() << cnt; cnt += 8; }
    }
    OIP_INFLATE_HD unsigned bits(unsigned k)                                 // k <= 16, after refill()
    {
        const unsigned v = (unsigned)buf & ((1u << k) - 1);
        buf >>= k; cnt -= k;
        return v;
    }
    // a bit from beyond the stream's end has been consumed (the zeros past n are the top bits of the buffer)
    OIP_INFLATE_HD bool truncated() const { return ip > n && (ip - n) * 8 > cnt; }
    // to the next byte boundary, the buffer emptied: the next next_byte() is the byte after the last consumed bit
    OIP_INFLATE_HD void align_to_byte()
    {
        const unsigned drop = cnt & 7;
        buf >>= drop; cnt -= drop;
        ip -= cnt >> 3;
        buf = 0; cnt = 0;
    }

    // ---- output ------------------------------------------------------------------------------------------------------------
    OIP_INFLATE_HD void flush()
    {
        p.sync();
        const unsigned a = flushed, b = pos;
        for (unsigned c0 = a; c0 < b; c0 += 4096) {                          // Adler-32 in chunks whose sums fit 32 bits
            const unsigned nn = b - c0 < 4096 ? b - c0 : 4096;
            unsigned s1 = 0, s2 = 0;
            for (unsigned i = p.lane(); i < nn; i += p.nlanes()) {
                const unsigned d = sh.win[(c0 + i + woff) & kWinMask];
                s1 += d;
                s2 += (nn - i) * d;
            }
            const unsigned t1 = p.uni(p.sum(s1)), t2 = p.uni(p.sum(s2 % 65521u));
            a2 = (a2 + nn * a1 + t2) % 65521u;
            a1 = (a1 + t1) % 65521u;
        }
        // [a, b) of the output = [ga, gb) where multiples of 16 are 16-byte boundaries of the image and of the ring alike
        const unsigned ga = a + woff, gb = b + woff;
        unsigned he = (ga + 15u) & ~15u;
        if (he > gb) he = gb;
        for (unsigned g = ga + p.lane(); g < he; g += p.nlanes()) out[g - woff] = sh.win[g & kWinMask];
        const unsigned we = gb & ~15u;
        for (unsigned g = he + 16 * p.lane(); g < we; g += 16 * p.nlanes()) copy16(out + (g - woff), sh.win + (g & kWinMask));
        for (unsigned g = (we > he ? we : he) + p.lane(); g < gb; g += p.nlanes()) out[g - woff] = sh.win[g & kWinMask];
        flushed = b;
        p.sync();
    }

    // ---- Huffman codes ---------------------------------------------------------------------------------------------------------
    // lens[0, nsym) -> counts and the symbols in canonical order; with tbits the primary table.  Returns what the Kraft sum
    // leaves over: 0 complete, > 0 incomplete, < 0 over-subscribed; *maxlen the longest code.
    OIP_INFLATE_HD int build(const uint8_t *lens, unsigned nsym, uint16_t *cntv, uint16_t *symv, uint16_t *tab, unsigned tbits, unsigned *maxlen)
    {
        p.sync();
        if (p.lane() == 0) {
            for (unsigned l = 0; l < 16; ++l) cntv[l] = 0;
            for (unsigned s = 0; s < nsym; ++s) ++cntv[lens[s] & 15u];
            sh.offs[0] = 0; sh.offs[1] = 0;
            for (unsigned l = 1; l < 15; ++l) sh.offs[l + 1] = (uint16_t)(sh.offs[l] + cntv[l]);
            for (unsigned s = 0; s < nsym; ++s) {
                const unsigned l = lens[s] & 15u;
                if (l) symv[sh.offs[l]++] = (uint16_t)s;
            }
        }
        p.sync();
        int left = 1;
        unsigned mx = 0;
        for (unsigned l = 1; l <= 15; ++l) {
            left <<= 1;
            const unsigned c = p.uni(cntv[l]);
            left -= (int)c;
            if (left < 0) return left;
            if (c) mx = l;
        }
        *maxlen = mx;
        if (tbits) {
            // entry idx: the code that idx's low bits begin with, found by the walk decode() takes for the long codes
            for (unsigned idx = p.lane(); idx < (1u << tbits); idx += p.nlanes()) {
                unsigned code = 0, first = 0, index = 0, e = 0;
                for (unsigned len = 1; len <= tbits; ++len) {
                    code |= (idx >> (len - 1)) & 1u;
                    const unsigned c = cntv[len];
                    if (code < first + c) { e = ((unsigned)symv[index + (code - first)] << 4) | len; break; }
                    index += c; first += c;
                    first <<= 1; code <<= 1;
                }
                tab[idx] = (uint16_t)e;
            }
            p.sync();
        }
        return left;
    }
    // the next symbol, or -1 where the bits are no code (an incomplete set); needs 15 bits in the buffer
    OIP_INFLATE_HD int decode(const uint16_t *tab, unsigned tbits, const uint16_t *cntv, const uint16_t *symv)
    {
        if (tbits) {
            const unsigned e = p.uni(tab[(unsigned)buf & ((1u << tbits) - 1)]);
            if (e) { buf >>= (e & 15u); cnt -= (e & 15u); return (int)(e >> 4); }
        }
        unsigned code = 0, first = 0, index = 0;
        unsigned long long b = buf;
        for (unsigned len = 1; len <= 15; ++len) {
            code |= (unsigned)b & 1u;
            b >>= 1;
            const unsigned c = p.uni(cntv[len]);
            if (code < first + c) { buf >>= len; cnt -= len; return (int)p.uni(symv[index + (code - first)]); }
            index += c; first += c;
            first <<= 1; code <<= 1;
        }
        return -1;
    }

    // ---- blocks ------------------------------------------------------------------------------------------------------------
    OIP_INFLATE_HD int stored()
    {
        align_to_byte();
        unsigned v[4];
        for (int i = 0; i < 4; ++i) v[i] = next_byte();
        if (ip > n) return kTruncated;
        const unsigned len = v[0] | (v[1] << 8), nlen = v[2] | (v[3] << 8);
        if ((len ^ 0xFFFFu) != nlen) return kStoredLength;
        if (len > n - ip) return kTruncated;
        if (len > cap - pos) return kTooLong;
        for (unsigned done = 0; done < len;) {
            if (pos - flushed >= kFlushAt) flush();
            const unsigned c = len - done < 4096 ? len - done : 4096;
            p.sync();
            for (unsigned i = p.lane(); i < c; i += p.nlanes()) sh.win[(pos + i + woff) & kWinMask] = in[ip + i];   // ip + c <= n
            p.sync();
            pos += c; ip += c; done += c;
        }
        return kOk;
    }
    OIP_INFLATE_HD int fixed_tables()
    {
        p.sync();
        for (unsigned s = p.lane(); s < 320; s += p.nlanes()) sh.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
        unsigned mx;
        build(sh.lens, 288, sh.lcnt, sh.lsym, sh.ltab, kLitBits, &mx);
        build(sh.lens + 288, 32, sh.dcnt, sh.dsym, sh.dtab, kDistBits, &mx);
        return kOk;
    }
    OIP_INFLATE_HD int dynamic_tables()
    {
        refill();
        const unsigned nlen = bits(5) + 257, ndist = bits(5) + 1, ncode = bits(4) + 4;
        if (truncated()) return kTruncated;
        if (nlen > 286 || ndist > 30) return kTooManySymbols;
        const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        p.sync();
        for (unsigned s = p.lane(); s < 19; s += p.nlanes()) sh.lens[s] = 0;
        p.sync();
        for (unsigned i = 0; i < ncode; ++i) {
            refill();
            const unsigned l = bits(3);
            if (p.lane() == 0) sh.lens[order[i]] = (uint8_t)l;
        }
        if (truncated()) return kTruncated;
        unsigned mx = 0;
        if (build(sh.lens, 19, sh.lcnt, sh.lsym, nullptr, 0, &mx) != 0) return kCodeLengthCode;
        unsigned idx = 0, prev = 0;
        while (idx < nlen + ndist) {
            refill();
            const int sym = decode(nullptr, 0, sh.lcnt, sh.lsym);
            if (sym < 0) return kCodeLengthCode;
            unsigned rep = 1, val = (unsigned)sym;
            if (sym == 16) {
                if (idx == 0) return kRepeatNoPrevious;
                val = prev; rep = 3 + bits(2);
            } else if (sym == 17) { val = 0; rep = 3 + bits(3); }
            else if (sym == 18) { val = 0; rep = 11 + bits(7); }
            if (truncated()) return kTruncated;
            if (rep > nlen + ndist - idx) return kRepeatOverrun;
            if (p.lane() == 0)
                for (unsigned r = 0; r < rep; ++r) sh.lens[idx + r] = (uint8_t)val;
            idx += rep;
            prev = val;
        }
        p.sync();
        if (p.uni(sh.lens[256]) == 0) return kNoEndOfBlock;
        // zlib's rule for both sets: over-subscribed never; incomplete only as a single code of length 1 (or no code at all)
        int left = build(sh.lens, nlen, sh.lcnt, sh.lsym, sh.ltab, kLitBits, &mx);
        if (left < 0 || (left > 0 && mx > 1)) return kLitLenSet;
        left = build(sh.lens + nlen, ndist, sh.dcnt, sh.dsym, sh.dtab, kDistBits, &mx);
        if (left < 0 || (left > 0 && mx > 1)) return kDistSet;
        return kOk;
    }
    OIP_INFLATE_HD int codes()
    {
        for (;;) {
            if (pos - flushed >= kFlushAt) flush();
            if (cnt < 48) refill();                                          // a whole length/distance pair needs 48 bits
            int sym = decode(sh.ltab, kLitBits, sh.lcnt, sh.lsym);
            if (sym < 0) return truncated() ? kTruncated : kBadLitLen;
            if (sym < 256) {
                if (truncated()) return kTruncated;
                if (pos >= cap) return kTooLong;
                if (p.lane() == 0) sh.win[(pos + woff) & kWinMask] = (uint8_t)sym;
                ++pos;
                continue;
            }
            if (sym == 256) return truncated() ? kTruncated : kOk;
            unsigned s = (unsigned)sym - 257;
            if (s >= 29) return truncated() ? kTruncated : kBadLitLen;
            unsigned len;
            if (s < 8) len = 3 + s;
            else if (s == 28) len = 258;
            else { const unsigned e = (s - 4) >> 2; len = 3 + ((4 + (s & 3)) << e) + bits(e); }
            sym = decode(sh.dtab, kDistBits, sh.dcnt, sh.dsym);
            if (sym < 0 || sym >= 30) return truncated() ? kTruncated : kBadDist;
            s = (unsigned)sym;
            unsigned dist;
            if (s < 4) dist = 1 + s;
            else { const unsigned e = (s - 2) >> 1; dist = 1 + ((2 + (s & 1)) << e) + bits(e); }
            if (truncated()) return kTruncated;
            if (dist > pos) return kDistTooFar;
            if (len > cap - pos) return kTooLong;
            // the copy, by the lanes together.  Every source byte a lane reads was written before the barrier in front of it.
            p.sync();
            if (dist >= kRound) {
                for (unsigned base = 0; base < len; base += kRound) {
                    const unsigned end = len - base < kRound ? len : base + kRound;
                    for (unsigned i = base + p.lane(); i < end; i += p.nlanes())
                        sh.win[(pos + i + woff) & kWinMask] = sh.win[(pos + i - dist + woff) & kWinMask];
                    p.sync();
                }
            } else {
                // byte i is byte i mod dist of the dist bytes in front of the match: all older than the match (dist 1, length 258 included)
                for (unsigned i = p.lane(); i < len; i += p.nlanes())
                    sh.win[(pos + i + woff) & kWinMask] = sh.win[(pos - dist + i % dist + woff) & kWinMask];
                p.sync();
            }
            pos += len;
        }
    }

    // the whole stream; *got receives the bytes it produced (<= cap)
    OIP_INFLATE_HD int run(unsigned *got)
    {
        *got = 0;
        if (n >= kMaxStream || cap >= kMaxStream) return kTooLong;
        int st = kOk;
        refill();
        const unsigned cmf = bits(8), flg = bits(8);
        if (truncated()) st = kTruncated;
        else if ((cmf & 15u) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31u != 0 || (flg & 0x20u)) st = kBadHeader;
        unsigned last = 0;
        while (st == kOk && !last) {
            refill();
            last = bits(1);
            const unsigned type = bits(2);
            if (truncated()) { st = kTruncated; break; }
            if (type == 0) st = stored();
            else if (type == 3) st = kBadBlockType;
            else {
                st = type == 1 ? fixed_tables() : dynamic_tables();
                if (st == kOk) st = codes();
            }
        }
        flush();
        *got = pos;
        if (st != kOk) return st;
        // the trailer: checked where all four bytes are there (libtiff's writers end some streams without it)
        align_to_byte();
        if (ip <= n && n - ip >= 4) {
            unsigned want = 0;
            for (int i = 0; i < 4; ++i) want = (want << 8) | next_byte();
            if (want != ((a2 << 16) | a1)) return kAdler;
        }
        return kOk;
    }
};

// One zlib stream on the calling thread: src[0, n) into dst[0, cap).  Returns a Status; *got the bytes produced.
inline int inflate_host(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, size_t *got, Shared *work)
{
    *got = 0;
    if (n >= kMaxStream || cap >= kMaxStream) return kTooLong;
    HostLane lane;
    Decoder<HostLane> d(lane, *work, src, (unsigned)n, dst, (unsigned)cap);
    unsigned g = 0;
    const int st = d.run(&g);
    *got = g;
    return st;
}

}  // namespace oipinflate
