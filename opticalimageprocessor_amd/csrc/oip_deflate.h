// oip_deflate.h -- one zlib-stream encoder (RFC 1950 wrapper, RFC 1951 blocks) for the host's threads and for a wave of the
// device, written once: the mirror image of oip_inflate.h.  No libz.  The strips and tiles of a Deflate TIFF product (compression
// 8, predictor 2) come out of this on either side (csrc/oip_tiff.hpp::encode_chunk on the host, csrc/tiffdeflate.hip on the device).
//
// The encoder is templated on the lane policy of the decoder -- lane(), nlanes(), sync(), sum(v), uni(v) -- with four more members
// that the encoder's shared tables need: scan(v) (exclusive prefix sum over the lanes), amax(p, v), inc(p) and aor(p, v) (atomic
// max / increment / or on a word of the work area).  The host instantiates it with one lane and plain stores, the device with the
// 64 lanes of a single-wave workgroup and LDS atomics.  The input is a Source with at(i), byte i of the stream: plain bytes on the
// host, the predictor-2 differences of the image's rows on the device (the image is read, never written).
//
// What the coder is (all of it fixed: the output is a function of the input bytes alone -- not of the number of lanes, of the
// launch, of the stream's index or of any alignment):
//   - the input is staged kChunk bytes at a time into a 32 KiB ring (Adler-32 summed on the way in); the ring keeps the last
//     kMaxDist = 30656 bytes behind the position being coded, which is the largest distance the coder emits;
//   - matching goes in rounds of kRound = 64 positions.  Every position of a round looks up ONE candidate -- the last position
//     of an earlier round whose four bytes hash (12 bits) to the same slot -- and the position right before it (distance 1,
//     which is what finds a run), and compares up to 258 bytes; a hashed candidate counts from 4 bytes on, distance 1 from 3.
//     Then all positions of the round enter the table (the later position wins a slot).  No chains, no lazy evaluation;
//   - one lane walks the round's 64 results greedily: a match where there is one (the walk jumps over it; what it jumps over
//     beyond the round's end is never hashed), a literal otherwise;
//   - a block closes after kBlock = 16384 input bytes or kMaxMatches = 2048 matches.  Its record is two bits per position (token
//     starts here / is a match) plus one word per match; the literals are read back from the ring;
//   - per block: literal/length and distance codes from the block's histogram (symbols ranked by the lanes, the tree by the
//     in-place two-queue construction of Moffat and Katajainen, lengths limited to 15 bits -- 7 for the code-length code -- by
//     moving the Kraft excess down from the longest codes one leaf at a time).  As zlib does, a set with fewer than two used
//     symbols gets symbols 0 / 1 added, so every set sent is complete;
//   - the block is sent in the smallest of three forms: dynamic (BTYPE 2), fixed (1) or stored (0); stored wins ties.  Stored
//     blocks that follow one another are merged up to 65535 bytes (the earlier LEN / NLEN are rewritten in place).  If the stream
//     still ends up larger than n + 5 ceil(n / 65535) + 6 bytes (11 for n = 0), or would pass cap, it is written again as stored
//     blocks only, straight from the source: that size is the bound, and a cap of at least stored_bound(n) never fails;
//   - the codes of a block are placed by the lanes together: 64 positions a round, an exclusive prefix sum of the tokens' bit
//     counts gives every token its place in a 512-byte bit buffer, whole bytes of which then go to the output.
//
// Memory safety is a property of the construction: every ring index is masked, every table index is a masked hash, a symbol below
// its table's size or a position relative to the block's start (below kSpan); every store to dst is guarded by cap.
#pragma once

#include "oip_inflate.h"

#include <cstddef>
#include <cstdint>

namespace oipdeflate {

constexpr unsigned kWin = 32768, kWinMask = kWin - 1;
constexpr unsigned kChunk = 1024;                      // staged at a time
constexpr unsigned kAhead = 2 * kChunk;                // the ring is filled to less than pos + kAhead
constexpr unsigned kRound = 64;
constexpr unsigned kMaxDist = kWin - kAhead - kRound;  // 30656
constexpr unsigned kHashBits = 12;
constexpr unsigned kBlock = 16384, kMaxMatches = 2048;
constexpr unsigned kSpan = kBlock + kRound + 258;      // a block's positions: below this
constexpr unsigned kWords = (kSpan + 63) / 64;
constexpr unsigned kObufWords = 128;                   // 64 tokens of at most 48 bits, plus the carried bits: 97 words

enum Status { kOk = 0, kCapTooSmall = 1, kTooLong = 2 };

OIP_INFLATE_HD inline size_t stored_bound(size_t n) { return n ? n + 5 * ((n + 65534) / 65535) + 6 : 11; }

// What one encode works in: LDS of a workgroup on the device (66 KiB: two waves per CU), heap on the host.
struct alignas(16) Shared {
    uint8_t win[kWin];                                 // ring: byte p of the input at p & kWinMask
    unsigned head[1u << kHashBits];                    // 1 + the last position with this hash, 0: none
    unsigned mtok[kMaxMatches];                        // a match: length << 16 | distance - 1
    unsigned long long tokmap[kWords], matmap[kWords]; // bit r: a token starts at block position r / and is a match
    unsigned cand[kRound], hsh[kRound];                // a round's results and hashes
    unsigned lfreq[288], dfreq[32], cfreq[20];
    unsigned work[288];
    unsigned obuf[kObufWords + 4];
    unsigned num[40], nxt[16];
    unsigned st[8];                                    // what lane 0 hands to the others
    uint16_t order[288];
    uint16_t lcode[288], dcode[32], ccode[20];
    uint16_t clseq[320];                               // code-length symbols of a dynamic header: symbol | extra bits << 8
    uint8_t llen[288 + 32], dlen[32], clen[20];        // (llen: the distance lengths behind the HLIT literal/length ones while the header is made)
};

struct HostLane : oipinflate::HostLane {
    unsigned scan(unsigned) const { return 0; }
    void amax(unsigned *p, unsigned v) const { if (*p < v) *p = v; }
    void inc(unsigned *p) const { ++*p; }
    void aor(unsigned *p, unsigned v) const { *p |= v; }
};

struct ByteSource {
    const uint8_t *src;
    OIP_INFLATE_HD unsigned at(unsigned i) const { return src[i]; }
};

template <class P, class S>
struct Encoder {
    const P &p;
    Shared &sh;
    const S &src;
    unsigned n;
    uint8_t *dst;
    unsigned cap;
    unsigned long long acc = 0;                        // bits not yet a whole byte (the same in every lane)
    unsigned nacc = 0;
    unsigned obyte = 0;                                // bytes of the stream so far, the refused ones included
    unsigned fill = 0, pos = 0, bstart = 0, nmatch = 0, xbits = 0;
    unsigned a1 = 1, a2 = 0;
    bool chain = false;                                // the last block sent is a stored one that can still grow
    unsigned chainLen = 0, chainHdrByte = 0, chainHdrBit = 0, chainLenAt = 0;

    OIP_INFLATE_HD Encoder(const P &p_, Shared &sh_, const S &src_, unsigned n_, uint8_t *dst_, unsigned cap_)
        : p(p_), sh(sh_), src(src_), n(n_), dst(dst_), cap(cap_) {}

    // ---- output ------------------------------------------------------------------------------------------------------------
    OIP_INFLATE_HD void store_byte(unsigned b)
    {
        if (obyte < cap && p.lane() == 0) dst[obyte] = (uint8_t)b;
        ++obyte;
    }
    OIP_INFLATE_HD void put(unsigned v, unsigned nb)                          // nb <= 16, v below 2^nb, the same in every lane
    {
        acc |= (unsigned long long)v << nacc;
        nacc += nb;
        while (nacc >= 8) { store_byte((unsigned)acc & 255u); acc >>= 8; nacc -= 8; }
    }
    OIP_INFLATE_HD void pad_to_byte() { if (nacc) put(0, 8 - nacc); }

    // ---- input -------------------------------------------------------------------------------------------------------------
    OIP_INFLATE_HD void stage_chunk()
    {
        const unsigned nn = n - fill < kChunk ? n - fill : kChunk;
        unsigned s1 = 0, s2 = 0;
        for (unsigned i = p.lane(); i < nn; i += p.nlanes()) {
            const unsigned d = src.at(fill + i) & 255u;
            sh.win[(fill + i) & kWinMask] = (uint8_t)d;
            s1 += d;
            s2 += (nn - i) * d;
        }
        const unsigned t1 = p.uni(p.sum(s1)), t2 = p.uni(p.sum(s2 % 65521u));
        a2 = (a2 + nn * a1 + t2) % 65521u;
        a1 = (a1 + t1) % 65521u;
        fill += nn;
    }

    // ---- matching ----------------------------------------------------------------------------------------------------------
    OIP_INFLATE_HD unsigned match_len(unsigned q, unsigned d, unsigned maxl) const
    {
        unsigned l = 0;
        while (l < maxl && sh.win[(q + l) & kWinMask] == sh.win[(q + l - d) & kWinMask]) ++l;
        return l;
    }
    static OIP_INFLATE_HD unsigned ilog2(unsigned v) { return 31u - (unsigned)__builtin_clz(v); }   // v > 0
    static OIP_INFLATE_HD void len_symbol(unsigned len, unsigned *sym, unsigned *eb, unsigned *ev)
    {
        const unsigned l = len - 3;
        if (l < 8) { *sym = 257 + l; *eb = 0; *ev = 0; }
        else if (len == 258) { *sym = 285; *eb = 0; *ev = 0; }
        else { const unsigned e = ilog2(l) - 2; *sym = 257 + 4 * e + 4 + ((l >> e) & 3u); *eb = e; *ev = l & ((1u << e) - 1); }
    }
    static OIP_INFLATE_HD void dist_symbol(unsigned dm1, unsigned *sym, unsigned *eb, unsigned *ev)
    {
        if (dm1 < 4) { *sym = dm1; *eb = 0; *ev = 0; }
        else { const unsigned e = ilog2(dm1) - 1; *sym = 2 * e + 2 + ((dm1 >> e) & 1u); *eb = e; *ev = dm1 & ((1u << e) - 1); }
    }

    OIP_INFLATE_HD void round()
    {
        p.sync();
        for (unsigned i = p.lane(); i < kRound; i += p.nlanes()) {
            const unsigned q = pos + i;
            unsigned bl = 0, bd = 0, h = 0xffffffffu;
            if (q < n) {
                const unsigned maxl = n - q < 258 ? n - q : 258;
                if (q >= 1 && maxl >= 3) {
                    const unsigned l = match_len(q, 1, maxl);
                    if (l >= 3) { bl = l; bd = 1; }
                }
                if (n - q >= 4) {
                    const unsigned v = (unsigned)sh.win[q & kWinMask] | ((unsigned)sh.win[(q + 1) & kWinMask] << 8) |
                                       ((unsigned)sh.win[(q + 2) & kWinMask] << 16) | ((unsigned)sh.win[(q + 3) & kWinMask] << 24);
                    h = (v * 2654435761u) >> (32 - kHashBits);
                    const unsigned c = sh.head[h];
                    if (c && c <= q && q - (c - 1) <= kMaxDist && bl < maxl) {
                        const unsigned d = q - (c - 1);
                        const unsigned l = match_len(q, d, maxl);
                        if (l >= 4 && l > bl) { bl = l; bd = d; }
                    }
                }
            }
            sh.cand[i] = bl ? (bl << 16) | (bd - 1) : 0u;
            sh.hsh[i] = h;
        }
        p.sync();
        for (unsigned i = p.lane(); i < kRound; i += p.nlanes()) {
            const unsigned h = sh.hsh[i];
            if (h != 0xffffffffu) p.amax(&sh.head[h & ((1u << kHashBits) - 1)], pos + i + 1);
        }
        if (p.lane() == 0) {
            unsigned i = 0, nm = nmatch, xb = xbits;
            while (i < kRound && pos + i < n) {
                const unsigned c = sh.cand[i], rel = (pos + i - bstart) % kSpan;
                sh.tokmap[rel >> 6] |= 1ull << (rel & 63u);
                if (c && nm < kMaxMatches) {
                    sh.matmap[rel >> 6] |= 1ull << (rel & 63u);
                    sh.mtok[nm++] = c;
                    unsigned sym, eb, ev;
                    len_symbol(c >> 16, &sym, &eb, &ev);
                    ++sh.lfreq[sym]; xb += eb;
                    dist_symbol(c & 0xffffu, &sym, &eb, &ev);
                    ++sh.dfreq[sym]; xb += eb;
                    i += c >> 16;
                } else ++i;
            }
            sh.st[0] = pos + i; sh.st[1] = nm; sh.st[2] = xb;
        }
        p.sync();
        pos = p.uni(sh.st[0]); nmatch = p.uni(sh.st[1]); xbits = p.uni(sh.st[2]);
    }

    // ---- Huffman codes -----------------------------------------------------------------------------------------------------
    // freq[0, nsym) -> lens (at most maxbits) and the codes, bit-reversed for the LSB-first stream.  Fewer than two used symbols:
    // symbols 0 / 1 are counted in (freq is changed), so the set is complete.
    OIP_INFLATE_HD void build(unsigned *freq, unsigned nsym, unsigned maxbits, uint8_t *lens, uint16_t *codes)
    {
        p.sync();
        if (p.lane() == 0) {
            unsigned used = 0;
            for (unsigned s = 0; s < nsym; ++s) used += freq[s] != 0;
            for (unsigned s = 0; used < 2 && s < 2; ++s)
                if (!freq[s]) { freq[s] = 1; ++used; }
            sh.st[3] = used;
        }
        p.sync();
        const unsigned used = p.uni(sh.st[3]);
        for (unsigned s = p.lane(); s < nsym; s += p.nlanes()) {
            lens[s] = 0;
            const unsigned f = freq[s];
            if (!f) continue;
            unsigned rank = 0;
            for (unsigned t = 0; t < nsym; ++t) {
                const unsigned g = freq[t];
                rank += (g != 0) & ((g < f) | ((g == f) & (t < s)));
            }
            sh.order[rank % 288u] = (uint16_t)s;
        }
        p.sync();
        if (p.lane() == 0) {
            unsigned *A = sh.work;
            const int m = (int)used;                                           // 2 <= m <= 288
            for (int i = 0; i < m; ++i) A[i] = freq[sh.order[i]];
            // Moffat & Katajainen, "In-place calculation of minimum-redundancy codes": parents, depths of the internal nodes, leaf depths
            A[0] += A[1];
            int root = 0, leaf = 2;
            for (int next = 1; next < m - 1; ++next) {
                if (leaf >= m || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = (unsigned)next; }
                else A[next] = A[leaf++];
                if (leaf >= m || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = (unsigned)next; }
                else A[next] += A[leaf++];
            }
            A[m - 2] = 0;
            for (int next = m - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
            int avbl = 1, usd = 0, dpth = 0, next = m - 1;
            root = m - 2;
            while (avbl > 0) {
                while (root >= 0 && (int)A[root] == dpth) { ++usd; --root; }
                while (avbl > usd) { A[next--] = (unsigned)dpth; --avbl; }
                avbl = 2 * usd; ++dpth; usd = 0;
            }
            // the limit: codes longer than maxbits become maxbits long, and the Kraft sum is brought back to one by lengthening
            // the longest code that is shorter than maxbits, a leaf at a time
            unsigned *num = sh.num;
            for (unsigned l = 0; l <= maxbits; ++l) num[l] = 0;
            for (int i = 0; i < m; ++i) ++num[A[i] < maxbits ? A[i] : maxbits];
            unsigned total = 0;
            for (unsigned l = maxbits; l > 0; --l) total += num[l] << (maxbits - l);
            while (total > (1u << maxbits)) {
                --num[maxbits];
                for (unsigned l = maxbits - 1; l > 0; --l)
                    if (num[l]) { --num[l]; num[l + 1] += 2; break; }
                --total;
            }
            int j = m;
            for (unsigned l = 1; l <= maxbits; ++l)
                for (unsigned k = num[l]; k > 0 && j > 0; --k) lens[sh.order[--j]] = (uint8_t)l;
        }
        gen_codes(lens, nsym, codes);
    }
    OIP_INFLATE_HD void gen_codes(const uint8_t *lens, unsigned nsym, uint16_t *codes)
    {
        p.sync();
        if (p.lane() == 0) {
            unsigned *cnt = sh.num, *nxt = sh.nxt;
            for (unsigned l = 0; l < 16; ++l) cnt[l] = 0;
            for (unsigned s = 0; s < nsym; ++s) ++cnt[lens[s] & 15u];
            cnt[0] = 0;
            unsigned code = 0;
            nxt[0] = 0;
            for (unsigned l = 1; l < 16; ++l) { code = (code + cnt[l - 1]) << 1; nxt[l] = code; }
            for (unsigned s = 0; s < nsym; ++s) {
                const unsigned l = lens[s] & 15u;
                unsigned c = l ? nxt[l]++ : 0u, r = 0;
                for (unsigned b = 0; b < l; ++b) { r = (r << 1) | (c & 1u); c >>= 1; }
                codes[s] = (uint16_t)r;
            }
        }
        p.sync();
    }

    // ---- blocks ------------------------------------------------------------------------------------------------------------
    OIP_INFLATE_HD void begin_block()
    {
        p.sync();
        bstart = pos; nmatch = 0; xbits = 0;
        for (unsigned w = p.lane(); w < kWords; w += p.nlanes()) { sh.tokmap[w] = 0; sh.matmap[w] = 0; }
        for (unsigned s = p.lane(); s < 288; s += p.nlanes()) sh.lfreq[s] = 0;
        for (unsigned s = p.lane(); s < 32; s += p.nlanes()) sh.dfreq[s] = 0;
        p.sync();
    }

    // the tokens of [bstart, pos) with the codes in lcode / llen / dcode / dlen, then end-of-block
    OIP_INFLATE_HD void emit_tokens()
    {
        const unsigned span = pos - bstart, nw = (span + 63) / 64;
        unsigned mbase = 0;
        for (unsigned w = 0; w < nw; ++w) {
            p.sync();
            for (unsigned k = p.lane(); k < kObufWords + 4; k += p.nlanes()) sh.obuf[k] = 0;
            p.sync();
            const unsigned long long tm = sh.tokmap[w % kWords], mm = sh.matmap[w % kWords];
            unsigned base = nacc;
            for (unsigned i = p.lane(); i < 64; i += p.nlanes()) {
                unsigned long long v = 0;
                unsigned nb = 0;
                if ((tm >> i) & 1u) {
                    if ((mm >> i) & 1u) {
                        const unsigned idx = mbase + (unsigned)__builtin_popcountll(mm & ((1ull << i) - 1));
                        const unsigned t = sh.mtok[idx % kMaxMatches];
                        unsigned sym, eb, ev;
                        len_symbol(t >> 16, &sym, &eb, &ev);
                        v = sh.lcode[sym]; nb = sh.llen[sym];
                        v |= (unsigned long long)ev << nb; nb += eb;
                        dist_symbol(t & 0xffffu, &sym, &eb, &ev);
                        v |= (unsigned long long)sh.dcode[sym] << nb; nb += sh.dlen[sym];
                        v |= (unsigned long long)ev << nb; nb += eb;
                    } else {
                        const unsigned b = sh.win[(bstart + 64 * w + i) & kWinMask];
                        v = sh.lcode[b]; nb = sh.llen[b];
                    }
                }
                const unsigned off = base + p.scan(nb);
                if (nb) {
                    const unsigned k = (off >> 5) % kObufWords, s = off & 31u;
                    const unsigned long long lo = v << s;
                    if ((unsigned)lo) p.aor(&sh.obuf[k], (unsigned)lo);
                    if ((unsigned)(lo >> 32)) p.aor(&sh.obuf[k + 1], (unsigned)(lo >> 32));
                    if (s && (unsigned)(v >> (64 - s))) p.aor(&sh.obuf[k + 2], (unsigned)(v >> (64 - s)));
                }
                base += p.uni(p.sum(nb));
            }
            if (p.lane() == 0 && nacc) p.aor(&sh.obuf[0], (unsigned)acc);
            p.sync();
            const unsigned nbytes = base >> 3;                                 // (< 4 * kObufWords)
            for (unsigned k = p.lane(); k < nbytes; k += p.nlanes())
                if (obyte + k < cap) dst[obyte + k] = (uint8_t)(sh.obuf[k >> 2] >> (8 * (k & 3u)));
            obyte += nbytes;
            nacc = base & 7u;
            acc = nacc ? (p.uni(sh.obuf[nbytes >> 2]) >> (8 * (nbytes & 3u))) & ((1u << nacc) - 1) : 0u;
            mbase += (unsigned)__builtin_popcountll(mm);
        }
        p.sync();
        put(p.uni(sh.lcode[256]), p.uni(sh.llen[256]));
    }

    OIP_INFLATE_HD void emit_stored(bool final)
    {
        // the block's bytes go behind those of the stored block before them while that one has room (its LEN / NLEN, and BFINAL
        // with the stream's last byte, are rewritten where they lie: whole bytes that lane 0 stored), the rest opens a new one
        const unsigned span = pos - bstart;
        unsigned done = 0;
        do {
            unsigned take = span - done;
            if (chain && (chainLen < 65535u || take == 0)) {
                if (take > 65535u - chainLen) take = 65535u - chainLen;
                chainLen += take;
            } else {
                chainHdrByte = obyte; chainHdrBit = nacc;
                put(0, 3);
                pad_to_byte();
                chainLenAt = obyte;
                obyte += 4;
                if (take > 65535u) take = 65535u;
                chainLen = take;
                chain = true;
            }
            if (p.lane() == 0) {
                const unsigned v[4] = {chainLen & 255u, chainLen >> 8, ~chainLen & 255u, (~chainLen >> 8) & 255u};
                for (unsigned k = 0; k < 4; ++k)
                    if (chainLenAt + k < cap) dst[chainLenAt + k] = (uint8_t)v[k];
                if (final && done + take == span && chainHdrByte < cap) dst[chainHdrByte] = (uint8_t)(dst[chainHdrByte] | (1u << chainHdrBit));
            }
            for (unsigned k = p.lane(); k < take; k += p.nlanes())
                if (obyte + k < cap) dst[obyte + k] = sh.win[(bstart + done + k) & kWinMask];
            obyte += take;
            done += take;
        } while (done < span);
    }

    OIP_INFLATE_HD void end_block(bool final)
    {
        const unsigned span = pos - bstart, nw = (span + 63) / 64;
        p.sync();
        for (unsigned w = 0; w < nw; ++w) {
            const unsigned long long lit = sh.tokmap[w % kWords] & ~sh.matmap[w % kWords];
            for (unsigned i = p.lane(); i < 64; i += p.nlanes())
                if ((lit >> i) & 1u) p.inc(&sh.lfreq[sh.win[(bstart + 64 * w + i) & kWinMask]]);
        }
        if (p.lane() == 0) sh.lfreq[256] = 1;
        p.sync();
        // the cost of the fixed form, before build() adds symbols
        unsigned fx = 0;
        for (unsigned s = p.lane(); s < 288; s += p.nlanes()) fx += sh.lfreq[s] * (s < 144 ? 8u : s < 256 ? 9u : s < 280 ? 7u : 8u);
        for (unsigned s = p.lane(); s < 32; s += p.nlanes()) fx += sh.dfreq[s] * 5u;
        const unsigned fixedBits = 3 + xbits + p.uni(p.sum(fx));
        build(sh.lfreq, 286, 15, sh.llen, sh.lcode);
        build(sh.dfreq, 30, 15, sh.dlen, sh.dcode);
        // the dynamic header: the lengths of both sets as one sequence, run-length coded with 16 / 17 / 18
        if (p.lane() == 0) {
            unsigned hlit = 286, hdist = 30;
            while (hlit > 257 && sh.llen[hlit - 1] == 0) --hlit;
            while (hdist > 1 && sh.dlen[hdist - 1] == 0) --hdist;
            for (unsigned s = 0; s < hdist; ++s) sh.llen[hlit + s] = sh.dlen[s];
            for (unsigned s = 0; s < 20; ++s) sh.cfreq[s] = 0;
            const unsigned tot = hlit + hdist;
            unsigned nseq = 0, i = 0;
            while (i < tot) {
                const unsigned v = sh.llen[i];
                unsigned run = 1;
                while (i + run < tot && sh.llen[i + run] == v) ++run;
                i += run;
                bool sent = false;                                             // v itself went out right before
                while (run > 0) {
                    unsigned sym, ev = 0, take = 1;
                    if (v == 0 && run >= 11) { take = run < 138 ? run : 138; sym = 18; ev = take - 11; }
                    else if (v == 0 && run >= 3) { take = run; sym = 17; ev = take - 3; }
                    else if (v != 0 && sent && run >= 3) { take = run < 6 ? run : 6; sym = 16; ev = take - 3; }
                    else { sym = v; sent = true; }
                    sh.clseq[nseq++ % 320u] = (uint16_t)(sym | (ev << 8));
                    ++sh.cfreq[sym];
                    run -= take;
                }
            }
            sh.st[4] = hlit; sh.st[5] = hdist; sh.st[6] = nseq;
        }
        build(sh.cfreq, 19, 7, sh.clen, sh.ccode);
        const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        const unsigned hlit = p.uni(sh.st[4]), hdist = p.uni(sh.st[5]), nseq = p.uni(sh.st[6]);
        unsigned ncl = 19;
        while (ncl > 4 && p.uni(sh.clen[order[ncl - 1]]) == 0) --ncl;
        unsigned dy = 0;
        for (unsigned s = p.lane(); s < 286; s += p.nlanes()) dy += sh.lfreq[s] * sh.llen[s];
        for (unsigned s = p.lane(); s < 30; s += p.nlanes()) dy += sh.dfreq[s] * sh.dlen[s];
        for (unsigned s = p.lane(); s < 19; s += p.nlanes()) dy += sh.cfreq[s] * (sh.clen[s] + (s == 16 ? 2u : s == 17 ? 3u : s == 18 ? 7u : 0u));
        const unsigned dynBits = 3 + 14 + 3 * ncl + xbits + p.uni(p.sum(dy));
        const bool grows = chain && chainLen + span <= 65535u;                // (else: one more stored header, here or further on)
        const unsigned storedBits = 8 * span + (grows ? 0u : 3 + ((8 - ((nacc + 3) & 7u)) & 7u) + 32);
        if (storedBits <= dynBits && storedBits <= fixedBits) { emit_stored(final); return; }
        chain = false;
        if (fixedBits < dynBits) {
            p.sync();
            for (unsigned s = p.lane(); s < 288; s += p.nlanes()) sh.llen[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
            for (unsigned s = p.lane(); s < 32; s += p.nlanes()) sh.dlen[s] = 5;
            gen_codes(sh.llen, 288, sh.lcode);
            gen_codes(sh.dlen, 32, sh.dcode);
            put(final ? 1u : 0u, 1); put(1, 2);
        } else {
            put(final ? 1u : 0u, 1); put(2, 2);
            put(hlit - 257, 5); put(hdist - 1, 5); put(ncl - 4, 4);
            for (unsigned k = 0; k < ncl; ++k) put(p.uni(sh.clen[order[k]]), 3);
            for (unsigned k = 0; k < nseq; ++k) {
                const unsigned e = p.uni(sh.clseq[k % 320u]), sym = e & 255u;
                put(p.uni(sh.ccode[sym % 20u]), p.uni(sh.clen[sym % 20u]));
                if (sym == 16) put(e >> 8, 2);
                else if (sym == 17) put(e >> 8, 3);
                else if (sym == 18) put(e >> 8, 7);
            }
        }
        emit_tokens();
    }

    // the stream again, as stored blocks only: cap >= stored_bound(n) here
    OIP_INFLATE_HD void all_stored()
    {
        p.sync();
        acc = 0; nacc = 0; obyte = 0;
        put(0x78, 8); put(0x01, 8);
        unsigned done = 0;
        do {
            const unsigned c = n - done < 65535u ? n - done : 65535u;
            put(done + c == n ? 1u : 0u, 8);
            put(c, 16); put(~c & 0xffffu, 16);
            for (unsigned k = p.lane(); k < c; k += p.nlanes())
                if (obyte + k < cap) dst[obyte + k] = (uint8_t)src.at(done + k);
            obyte += c; done += c;
        } while (done < n);
    }

    // the whole stream; *size receives its bytes
    OIP_INFLATE_HD int run(unsigned *size)
    {
        *size = 0;
        if (n >= oipinflate::kMaxStream) return kTooLong;
        for (unsigned k = p.lane(); k < (1u << kHashBits); k += p.nlanes()) sh.head[k] = 0;
        put(0x78, 8); put(0x01, 8);
        begin_block();
        for (;;) {
            while (fill < n && fill < pos + kChunk) stage_chunk();
            if (pos < n) round();
            const bool final = pos >= n;
            if (final || pos - bstart >= kBlock || nmatch + kRound > kMaxMatches) {
                end_block(final);
                if (final) break;
                begin_block();
            }
        }
        pad_to_byte();
        const unsigned adler = (a2 << 16) | a1;
        put(adler >> 24, 8); put((adler >> 16) & 255u, 8); put((adler >> 8) & 255u, 8); put(adler & 255u, 8);
        const size_t bound = stored_bound(n);
        if (obyte > bound || obyte > cap) {
            if (cap < bound) return kCapTooSmall;
            all_stored();
            put(adler >> 24, 8); put((adler >> 16) & 255u, 8); put((adler >> 8) & 255u, 8); put(adler & 255u, 8);
        }
        p.sync();
        *size = obyte;
        return kOk;
    }
};

// One zlib stream on the calling thread: src[0, n) into dst[0, cap).  Returns the stream's size, or 0 when cap is too small
// (never when cap >= stored_bound(n)) or n is not below oipinflate::kMaxStream.
inline size_t deflate_host(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, Shared *work)
{
    if (n >= oipinflate::kMaxStream) return 0;
    if (cap >= oipinflate::kMaxStream) cap = oipinflate::kMaxStream - 1;
    HostLane lane;
    ByteSource s{src};
    Encoder<HostLane, ByteSource> e(lane, *work, s, (unsigned)n, dst, (unsigned)cap);
    unsigned size = 0;
    return e.run(&size) == kOk ? size : 0;
}

}  // namespace oipdeflate
