// tiffstreams_test.cpp -- the arithmetic of the device TIFF codecs (csrc/oip_tiffstreams.h) on the CPU: the encode plan's sizes and
// scratch regions against the formulas the two encoders had each for themselves, restated here independently of the header; the
// even-offset rule across a launch boundary; the decode scratch; the device-or-host route table.  Built with ASan + UBSan by
// tests/test_tiffstreams_cpu.py.
#include "oip_tiffstreams.h"

#include <cstdio>
#include <cstring>

typedef unsigned __int128 u128;

static int bad = 0, n = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++bad; printf("%s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

// the restatement: c = 0 LZW, 1 Deflate
static u128 worst_stream(int c, u128 b) { return c == 0 ? b + b / 2 + b / 1024 + 64 : b ? b + 5 * ((b + 65534) / 65535) + 6 : 11; }
static u128 up256(u128 v) { return (v + 255) / 256 * 256; }

static void plan_case(int c, long rows, int width, int spp, long rps, const char *refusal)
{
    ++n;
    const OipTiffCodec &codec = c == 0 ? kOipTiffLzw : kOipTiffDeflate;
    const OipTiffEncodePlan p = plan_tiff_encode(codec, rows, width, spp, rps);
    const char *at = "codec %d rows %ld width %d spp %d rps %ld";
    EXPECT((p.refusal == nullptr) == (refusal == nullptr) && (!refusal || strcmp(refusal, p.refusal) == 0), at, c, rows, width, spp, rps);
    if (rows <= 0 || width <= 0 || spp <= 0 || rps <= 0) {
        EXPECT(p.worst_bytes == 0 && p.scratch_bytes == 0 && p.nstrips == 0, at, c, rows, width, spp, rps);
        return;
    }
    const u128 nstrips = ((u128)rows + rps - 1) / rps, strip = (u128)rps * width * spp * 2, per = nstrips < 32768 ? nstrips : 32768;
    const u128 slot = (worst_stream(c, strip) + 3) / 4 * 4;
    const u128 tables = up256(per * (c == 0 ? 8192 * 8 : 0)), slots = up256(per * slot), len = up256(nstrips * 4), off = up256(nstrips * 8);
    EXPECT((u128)p.nstrips == nstrips && (u128)p.per_launch == per && (u128)p.strip_bytes == strip, at, c, rows, width, spp, rps);
    EXPECT((u128)p.worst_bytes == nstrips * (worst_stream(c, strip) + 2), at, c, rows, width, spp, rps);
    EXPECT((u128)p.scratch_bytes == tables + slots + len + off, at, c, rows, width, spp, rps);
    EXPECT((u128)p.slot_bytes == slot && p.slot_bytes % 4 == 0 && p.slot_bytes >= codec.worst(p.strip_bytes), at, c, rows, width, spp, rps);
    // [tables | slots | len | off]: in this order, nothing shared, every start a multiple of 256, the end the scratch's
    EXPECT(p.o_tables == 0 && (u128)p.o_slots == tables && (u128)p.o_len == tables + slots && (u128)p.o_off == tables + slots + len, at, c, rows, width, spp, rps);
    EXPECT(p.o_slots % 256 == 0 && p.o_len % 256 == 0 && p.o_off % 256 == 0 && p.scratch_bytes % 256 == 0, at, c, rows, width, spp, rps);
    EXPECT((u128)p.o_slots - p.o_tables >= per * codec.table_bytes && (u128)p.o_len - p.o_slots >= per * p.slot_bytes &&
               (u128)p.o_off - p.o_len >= nstrips * 4 && (u128)p.scratch_bytes - p.o_off >= nstrips * 8, at, c, rows, width, spp, rps);
}

static void plans()
{
    for (int c = 0; c < 2; ++c) {
        for (long rows = 1; rows <= 40; ++rows)
            for (int width = 1; width <= 9; ++width)
                for (int spp = 1; spp <= 4; spp += 3)
                    for (long rps = 1; rps <= 7; ++rps) plan_case(c, rows, width, spp, rps, nullptr);
        plan_case(c, 25000, 7500, 4, 1, nullptr);                  // a product
        plan_case(c, 70000, 7500, 4, 1, nullptr);                  // three launches; a payload past 2^32
        plan_case(c, 32768, 3, 1, 1, nullptr);                     // one launch exactly
        plan_case(c, 32769, 3, 1, 1, nullptr);
        plan_case(c, 10, 1 << 27, 4, 1, nullptr);                  // strips of exactly 1 GiB
        plan_case(c, 10, (1 << 29) + 1, 1, 1, "strip larger than 1 GiB");      // 1 GiB + 2
        plan_case(c, 3, 1 << 20, 4, 1000, "strip larger than 1 GiB");
        plan_case(c, 8, 64, 3, 2, "bad argument");                 // sizes as ever, and a refusal
        plan_case(c, 8, 64, 2, 2, "bad argument");
        plan_case(c, 8, 64, 5, 2, "bad argument");
        plan_case(c, 0, 64, 4, 2, "bad argument");
        plan_case(c, 8, 0, 4, 2, "bad argument");
        plan_case(c, 8, 64, 0, 2, "bad argument");
        plan_case(c, 8, 64, 4, 0, "bad argument");
        plan_case(c, -8, 64, 4, 2, "bad argument");
        plan_case(c, 8, -64, 4, 2, "bad argument");
        plan_case(c, 8, 64, 4, -2, "bad argument");
    }
    EXPECT(kOipTiffLzw.image_align == 1 && kOipTiffLzw.image_align4 == 8 && kOipTiffDeflate.image_align == 2 && kOipTiffDeflate.image_align4 == 2, "alignments");
}

static void spans()
{
    for (long rows = 1; rows <= 40; ++rows)
        for (long rps = 1; rps <= 45; ++rps) {
            long next = 0;
            const long nstrips = (rows + rps - 1) / rps;
            for (long k = 0; k < nstrips; ++k) {
                ++n;
                const OipStripSpan s = tiff_strip_span(k, rows, rps);
                EXPECT(s.r0 == next && s.nr >= 1 && (k + 1 < nstrips ? s.nr == rps : s.r0 + s.nr == rows), "rows %ld rps %ld strip %ld", rows, rps, k);
                next += s.nr;
            }
        }
}

static void placing()
{
    const int N = 6;
    for (int mix = 0; mix < (1 << N); ++mix)
        for (size_t start = 0; start < 3; ++start) {       // from an even and from an odd position
            ++n;
            unsigned len[N];
            for (int k = 0; k < N; ++k) len[k] = 5 + 4 * k + ((mix >> k) & 1);     // bit k: stream k is even
            unsigned long long whole[N];
            const size_t end = place_streams(len, N, start, whole);
            size_t prev = start;
            for (int k = 0; k < N; ++k) {
                EXPECT(whole[k] % 2 == 0 && whole[k] >= prev && whole[k] - prev <= 1, "mix %d start %zu stream %d at %llu after %zu", mix, start, k, whole[k], prev);
                EXPECT((whole[k] == prev) == (prev % 2 == 0), "mix %d start %zu stream %d: a pad byte exactly behind an odd end", mix, start, k);
                prev = whole[k] + len[k];
            }
            EXPECT(end == prev, "mix %d start %zu: end %zu, %zu expected", mix, start, end, prev);
            for (int cut = 0; cut <= N; ++cut) {            // the launch boundary
                unsigned long long parts[N];
                const size_t mid = place_streams(len, cut, start, parts);
                const size_t e2 = place_streams(len + cut, N - cut, mid, parts + cut);
                EXPECT(e2 == end && memcmp(parts, whole, sizeof(whole)) == 0, "mix %d start %zu cut %d", mix, start, cut);
            }
        }
}

static void decode_layout()
{
    for (size_t tables = 0; tables <= 3 * 32768; tables += 32768 - 8)
        for (size_t ns = 1; ns <= 200; ns += (ns < 70 ? 1 : 13)) {
            ++n;
            const OipTiffDecodeLayout l = tiff_decode_layout(tables, ns);
            const size_t o_off = (size_t)up256(tables), o_len = o_off + (size_t)up256(ns * 8), o_got = o_len + (size_t)up256(ns * 8),
                         o_status = o_got + (size_t)up256(ns * 4);
            EXPECT(l.o_off == o_off && l.o_len == o_len && l.o_got == o_got && l.o_status == o_status && l.bytes == o_status + (size_t)up256(ns * 4),
                   "tables %zu streams %zu", tables, ns);
        }
}

static void routes()
{
    const uint64_t KiB = 1024, MiB = 1024 * KiB, GiB = 1024 * MiB;
    struct Row { int c; OipTiffDirection dir; size_t streams; uint64_t bytes; int knob; bool device; };
    const Row table[] = {
        // LZW: the knob and nothing else
        {0, OIP_TIFF_READ, 1, 1, 0, false}, {0, OIP_TIFF_WRITE, 25000, 60000, 0, false}, {0, OIP_TIFF_READ, 1, 8 * GiB, 1, true},
        {0, OIP_TIFF_WRITE, 1, 8 * GiB, 1, true}, {0, OIP_TIFF_WRITE, 1, 60000, 2, true}, {0, OIP_TIFF_READ, 25000, 60000, -1, true},
        // Deflate, written
        {1, OIP_TIFF_WRITE, 25000, 60000, 0, false}, {1, OIP_TIFF_WRITE, 1, 2, 2, true}, {1, OIP_TIFF_WRITE, 1, GiB, 2, true},
        {1, OIP_TIFF_WRITE, 1, GiB + 1, 2, false}, {1, OIP_TIFF_WRITE, 25000, GiB + 1, 1, false},
        {1, OIP_TIFF_WRITE, 255, 60000, 1, false}, {1, OIP_TIFF_WRITE, 256, 60000, 1, true},
        {1, OIP_TIFF_WRITE, 256, 512 * KiB, 1, true}, {1, OIP_TIFF_WRITE, 256, 512 * KiB + 1, 1, false}, {1, OIP_TIFF_WRITE, 100000, 2 * MiB, 1, false},
        {1, OIP_TIFF_WRITE, 255, 512 * KiB, 3, false}, {1, OIP_TIFF_WRITE, 256, 512 * KiB, 3, true},
        // Deflate, read: the knob is on or off
        {1, OIP_TIFF_READ, 25000, 60000, 0, false}, {1, OIP_TIFF_READ, 255, 60000, 1, false}, {1, OIP_TIFF_READ, 256, 60000, 1, true},
        {1, OIP_TIFF_READ, 256, 2 * MiB, 1, true}, {1, OIP_TIFF_READ, 256, 2 * MiB + 1, 1, false}, {1, OIP_TIFF_READ, 256, 512 * KiB + 1, 1, true},
        {1, OIP_TIFF_READ, 255, 60000, 2, false}, {1, OIP_TIFF_READ, 256, 2 * MiB + 1, 2, false}, {1, OIP_TIFF_READ, 256, 2 * MiB, 2, true},
    };
    for (const Row &r : table) {
        ++n;
        EXPECT(tiff_streams_on_device(r.c == 0 ? kOipTiffLzw : kOipTiffDeflate, r.dir, r.streams, r.bytes, r.knob) == r.device,
               "codec %d dir %d streams %zu bytes %llu knob %d", r.c, (int)r.dir, r.streams, (unsigned long long)r.bytes, r.knob);
    }
}

int main()
{
    plans();
    spans();
    placing();
    decode_layout();
    routes();
    printf("%d cases, %d bad\n", n, bad);
    return bad != 0;
}
