// inflate_test.cpp -- the host instantiation of csrc/oip_inflate.h (the decoder the device runs as well) and the Deflate branch of
// read_tiff_u16 (csrc/oip_tiff.hpp).  Built with ASan + UBSan by tests/test_deflate_cpu.py.
//   inflate_test cases DIR    the files tests/_deflate_cases.py::write_case_files wrote: every case of cases.txt (accepted ones
//                             must give their bytes, rejected ones the status of their rule), every truncation of trunc.z, every
//                             single-bit flip of flip0.z, flip1.z, flip2.z.  Input and output buffers are heap blocks of exactly the
//                             stream's and the strip's size, at every alignment modulo 16, so a read or write past either is a report.
//   inflate_test tiff LIST    LIST: lines `file.tiff file.raw|- text`; read_tiff_u16 must return the samples of file.raw, or, with -,
//                             throw an error that holds `text` (underscores stand for spaces).
#include "oip_tiff.hpp"

#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

using namespace OIPGPU;

static long bad = 0;
#define CHECK(c, ...) do { if (!(c)) { ++bad; printf(__VA_ARGS__); printf("\n"); } } while (0)

static std::vector<uint8_t> slurp(const std::string &p, bool *ok = nullptr)
{
    std::vector<uint8_t> v;
    if (ok) *ok = false;
    if (FILE *f = fopen(p.c_str(), "rb")) {
        fseeko(f, 0, SEEK_END);
        v.resize((size_t)ftello(f));
        rewind(f);
        if (fread(v.data(), 1, v.size(), f) != v.size()) v.clear();
        else if (ok) *ok = true;
        fclose(f);
    }
    return v;
}

// ---- the second decoder: bit by bit, a vector for the output, code tables as lists of (length, code) -----------------------------------
// It shares nothing with oip_inflate.h but the rules of include/oip_c.h.  Returns false for a stream that breaks one.
namespace second {
struct Bits {
    const std::vector<uint8_t> &d;
    size_t pos = 0;
    bool over = false;
    explicit Bits(const std::vector<uint8_t> &v) : d(v) {}
    unsigned bit()
    {
        if (pos >= d.size() * 8) { over = true; return 0; }
        const unsigned b = (d[pos >> 3] >> (pos & 7)) & 1u;
        ++pos;
        return b;
    }
    unsigned get(int k) { unsigned v = 0; for (int i = 0; i < k; ++i) v |= bit() << i; return v; }
};
struct Code {
    std::vector<int> count = std::vector<int>(16, 0), symbol;
    int left = 1, maxlen = 0;
    explicit Code(const std::vector<int> &lens)
    {
        for (int l : lens) ++count[(size_t)l];
        count[0] = 0;
        bool overs = false;
        for (int l = 1; l < 16; ++l) { left = left * 2 - count[(size_t)l]; if (left < 0) overs = true; if (count[(size_t)l]) maxlen = l; }
        if (overs) left = -1;
        for (int l = 1; l < 16; ++l)
            for (size_t s = 0; s < lens.size(); ++s) if (lens[s] == l) symbol.push_back((int)s);
    }
    int decode(Bits &b) const
    {
        int code = 0, first = 0, index = 0;
        for (int l = 1; l < 16; ++l) {
            code |= (int)b.bit();
            if (b.over) return -1;
            if (code - count[(size_t)l] < first) return symbol[(size_t)(index + code - first)];
            index += count[(size_t)l]; first += count[(size_t)l];
            first <<= 1; code <<= 1;
        }
        return -1;
    }
};
static const int LB[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
static const int LE[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
static const int DB[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
static const int DE[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};

static bool inflate(const std::vector<uint8_t> &in, std::vector<uint8_t> &out, size_t limit)
{
    Bits b(in);
    out.clear();
    const unsigned cmf = b.get(8), flg = b.get(8);
    if (b.over || (cmf & 15) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31 || (flg & 0x20)) return false;
    for (unsigned last = 0; !last;) {
        last = b.get(1);
        const unsigned type = b.get(2);
        if (b.over || type == 3) return false;
        if (type == 0) {
            b.pos = (b.pos + 7) & ~(size_t)7;
            const unsigned len = b.get(16), nlen = b.get(16);
            if (b.over || (len ^ 0xFFFF) != nlen || b.pos / 8 + len > in.size() || out.size() + len > limit) return false;
            out.insert(out.end(), in.begin() + (long)(b.pos / 8), in.begin() + (long)(b.pos / 8 + len));
            b.pos += 8 * (size_t)len;
            continue;
        }
        std::vector<int> ll, dl;
        if (type == 1) {
            for (int s = 0; s < 288; ++s) ll.push_back(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
            dl.assign(32, 5);
        } else {
            const unsigned nl = b.get(5) + 257, nd = b.get(5) + 1, nc = b.get(4) + 4;
            if (b.over || nl > 286 || nd > 30) return false;
            static const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
            std::vector<int> cl(19, 0);
            for (unsigned i = 0; i < nc; ++i) cl[(size_t)order[i]] = (int)b.get(3);
            if (b.over) return false;
            const Code cc(cl);
            if (cc.left != 0) return false;
            std::vector<int> lens;
            while (lens.size() < nl + nd) {
                const int s = cc.decode(b);
                if (s < 0) return false;
                int val = s, rep = 1;
                if (s == 16) { if (lens.empty()) return false; val = lens.back(); rep = 3 + (int)b.get(2); }
                else if (s == 17) { val = 0; rep = 3 + (int)b.get(3); }
                else if (s == 18) { val = 0; rep = 11 + (int)b.get(7); }
                if (b.over || lens.size() + (size_t)rep > nl + nd) return false;
                lens.insert(lens.end(), (size_t)rep, val);
            }
            if (lens[256] == 0) return false;
            ll.assign(lens.begin(), lens.begin() + nl);
            dl.assign(lens.begin() + nl, lens.end());
        }
        const Code lc(ll), dc(dl);
        if (lc.left < 0 || (lc.left > 0 && lc.maxlen > 1) || dc.left < 0 || (dc.left > 0 && dc.maxlen > 1)) return false;
        for (;;) {
            const int s = lc.decode(b);
            if (s < 0) return false;
            if (s == 256) break;
            if (s < 256) { if (out.size() >= limit) return false; out.push_back((uint8_t)s); continue; }
            if (s > 285) return false;
            const size_t len = (size_t)LB[s - 257] + b.get(LE[s - 257]);
            const int d = dc.decode(b);
            if (d < 0 || d > 29) return false;
            const size_t dist = (size_t)DB[d] + b.get(DE[d]);
            if (b.over || dist > out.size() || out.size() + len > limit) return false;
            for (size_t i = 0; i < len; ++i) out.push_back(out[out.size() - dist]);
        }
    }
    const size_t at = (b.pos + 7) / 8;
    if (in.size() >= at + 4) {
        unsigned a = 1, c = 0;
        for (uint8_t v : out) { a = (a + v) % 65521u; c = (c + a) % 65521u; }
        const unsigned want = ((unsigned)in[at] << 24) | ((unsigned)in[at + 1] << 16) | ((unsigned)in[at + 2] << 8) | in[at + 3];
        if (want != ((c << 16) | a)) return false;
    }
    return true;
}
}  // namespace second

// One decode with exact-size heap blocks: the stream at (16 - ia) and the output at (16 - oa) bytes in front of their blocks' ends
// rounded to 16 -- every alignment of either -- with a guard pattern in the bytes before the output.
struct Result { int status; size_t got; std::vector<uint8_t> bytes; };
static Result decode(const std::vector<uint8_t> &z, size_t cap, unsigned ia, unsigned oa)
{
    std::unique_ptr<uint8_t[]> in(new uint8_t[z.size() + ia]), out(new uint8_t[cap + oa]);
    if (!z.empty()) memcpy(in.get() + ia, z.data(), z.size());
    memset(out.get(), 0xA5, cap + oa);
    std::unique_ptr<oipinflate::Shared> work(new oipinflate::Shared);
    Result r;
    r.status = oipinflate::inflate_host(in.get() + ia, z.size(), out.get() + oa, cap, &r.got, work.get());
    for (unsigned i = 0; i < oa; ++i) CHECK(out[i] == 0xA5, "a byte in front of the output was written");
    CHECK(r.got <= cap, "got %zu > cap %zu", r.got, cap);
    for (size_t i = r.got; i < cap; ++i) if (out[oa + i] != 0xA5) { CHECK(false, "a byte behind the decoded ones was written"); break; }
    r.bytes.assign(out.get() + oa, out.get() + oa + r.got);
    return r;
}

static int run_cases(const std::string &dir)
{
    std::ifstream list(dir + "/cases.txt");
    std::string name, kind;
    size_t cap;
    int status;
    long ncases = 0, ntrunc = 0, nflip = 0, flip_ok = 0;
    while (list >> name >> kind >> cap >> status) {
        bool ok;
        const std::vector<uint8_t> z = slurp(dir + "/" + name + ".z", &ok);
        CHECK(ok, "%s: no stream", name.c_str());
        const std::vector<uint8_t> want = kind == "accept" ? slurp(dir + "/" + name + ".out") : std::vector<uint8_t>();
        for (unsigned a = 0; a < 16; ++a) {
            const Result r = decode(z, cap, a, (a * 7 + 3) & 15);
            if (kind == "accept") CHECK(r.status == 0 && r.got == cap && r.bytes == want, "%s (alignment %u): status %d (%s), %zu of %zu bytes", name.c_str(), a, r.status,
                                        oipinflate::status_text(r.status), r.got, cap);
            else CHECK(status < 0 ? r.status != 0 || r.got != cap : r.status == status, "%s (alignment %u): status %d (%s), %zu bytes; status %d expected", name.c_str(), a,
                       r.status, oipinflate::status_text(r.status), r.got, status);
            if (a == 0) printf("case %s %d %zu\n", name.c_str(), r.status, r.got);
        }
        // and the second decoder agrees about every case whose rule is Deflate's own
        std::vector<uint8_t> o2;
        const bool ok2 = second::inflate(z, o2, (size_t)1 << 20);
        if (kind == "accept") CHECK(ok2 && o2 == want, "%s: the second decoder disagrees", name.c_str());
        else if (name.rfind("decodes_to_", 0) != 0) CHECK(!ok2, "%s: the second decoder accepts", name.c_str());
        ++ncases;
    }
    // every truncation: an error, or -- where at most the trailer is cut -- the image
    {
        const std::vector<uint8_t> z = slurp(dir + "/trunc.z"), want = slurp(dir + "/trunc.out");
        CHECK(z.size() > 8 && !want.empty(), "no truncation stream");
        for (size_t cut = 0; cut < z.size(); ++cut) {
            const std::vector<uint8_t> part(z.begin(), z.begin() + (long)cut);
            const Result r = decode(part, want.size(), (unsigned)(cut & 15), (unsigned)((cut >> 4) & 15));
            const bool image = r.status == 0 && r.got == want.size() && r.bytes == want;
            if (cut + 4 >= z.size()) CHECK(image, "truncation at %zu: the missing trailer is not tolerated (status %d)", cut, r.status);
            else CHECK(r.status != 0, "truncation at %zu: status 0, %zu bytes", cut, r.got);
            ++ntrunc;
        }
    }
    // every single-bit flip of three short streams: a status (or another size), or the bytes the second decoder gives -- and where
    // the second decoder gives the strip's bytes, so does the first
    for (int k = 0; k < 3; ++k) {
        std::vector<uint8_t> z = slurp(dir + "/flip" + std::to_string(k) + ".z"), orig;
        CHECK(second::inflate(z, orig, (size_t)1 << 20) && !orig.empty(), "flip%d: the stream itself does not decode", k);
        const size_t cap = orig.size();
        for (size_t bit = 0; bit < z.size() * 8; ++bit) {
            z[bit >> 3] ^= (uint8_t)(1u << (bit & 7));
            const Result r = decode(z, cap, (unsigned)(bit & 15), (unsigned)((bit >> 4) & 15));
            std::vector<uint8_t> o2;
            const bool ok2 = second::inflate(z, o2, cap) && o2.size() == cap;
            const bool ok1 = r.status == 0 && r.got == cap;
            CHECK(ok1 == ok2, "flip%d bit %zu: first decoder %s (status %d, %zu bytes), second %s", k, bit, ok1 ? "accepts" : "refuses", r.status, r.got,
                  ok2 ? "accepts" : "refuses");
            if (ok1 && ok2) { CHECK(r.bytes == o2, "flip%d bit %zu: different bytes", k, bit); ++flip_ok; }
            z[bit >> 3] ^= (uint8_t)(1u << (bit & 7));
            ++nflip;
        }
    }
    printf("%ld cases, %ld truncations, %ld flips (%ld still decode), %ld bad\n", ncases, ntrunc, nflip, flip_ok, bad);
    return bad ? 1 : 0;
}

static int run_tiff(const std::string &listPath)
{
    std::ifstream list(listPath);
    std::string tiff, raw, text;
    long n = 0;
    while (list >> tiff >> raw >> text) {
        for (char &c : text) if (c == '_') c = ' ';
        int w = 0, spp = 0;
        long h = 0;
        std::vector<uint16_t> img;
        std::string err;
        try { read_tiff_u16(tiff, &w, &h, &spp, &img); }
        catch (const std::exception &e) { err = e.what(); }
        if (raw == "-") CHECK(!err.empty() && err.find(text) != std::string::npos, "%s: expected an error with [%s], got [%s]", tiff.c_str(), text.c_str(), err.c_str());
        else {
            const std::vector<uint8_t> want = slurp(raw);
            CHECK(err.empty(), "%s: %s", tiff.c_str(), err.c_str());
            CHECK(img.size() * 2 == want.size() && (want.empty() || memcmp(img.data(), want.data(), want.size()) == 0), "%s: other samples (%d x %ld x %d)", tiff.c_str(), w, h, spp);
        }
        // the layout-only pass (what the device route starts from) takes and refuses the same files
        TiffLayout lay;
        std::string err2;
        try { lay = read_tiff_layout(tiff); }
        catch (const std::exception &e) { err2 = e.what(); }
        if (raw != "-") CHECK(err2.empty() && lay.compression == TIFF_DEFLATE, "%s: layout: %s", tiff.c_str(), err2.c_str());
        ++n;
    }
    printf("%ld files, %ld bad\n", n, bad);
    return bad ? 1 : 0;
}

int main(int argc, char **argv)
{
    if (argc == 3 && std::string(argv[1]) == "cases") return run_cases(argv[2]);
    if (argc == 3 && std::string(argv[1]) == "tiff") return run_tiff(argv[2]);
    printf("usage: inflate_test cases DIR | tiff LIST\n");
    return 2;
}
