// oip_warpfield.hpp -- the host side of `oip regfix` that needs no device: a regcheck report (oip_regreport.hpp writes it)
// becomes the node lattice oip_warp_grid_bicubic_u16 takes -- parse, fill of the nodes whose tile carries a flag, smoothing.
// include/oip_c.h states the three steps (oip_regfix_load_report, oip_regfix_fill, oip_regfix_smooth);
// tests/_regfix_ref.py restates them.  Free of HIP, so tests/cpp/warpfield_test.cpp runs it under ASan + UBSan.  Every
// malformed input ends in std::invalid_argument, never in a read outside a buffer.
#pragma once

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "oip_c.h"

namespace OIPGPU {

struct WarpField {
    int nx = 0, ny = 0, sx = 1, sy = 1, band2 = 1;
    long gx0 = 0, gy0 = 0, used = 0;        // used: tiles without a flag
    std::vector<int32_t> X, Y;              // Q10, row-major ny x nx
    int maxAbsY() const
    {
        int m = 0;
        for (int32_t v : Y) m = std::max(m, v < 0 ? -v : v);
        return m;
    }
};

constexpr long kWarpMaxNodes = 1L << 27;
constexpr long kWarpMaxCoord = 1L << 40;    // of a header value or a tile position: far above any raster, far below overflow

inline long WarpFloorDiv(long a, long b) { return a / b - ((a % b != 0) && ((a < 0) != (b < 0))); }

// In passes, an unset node with k >= 1 set 4-neighbours (as of the pass's start) gets floor((2 sum + k) / (2 k)) per
// component; until none is left.  False if no node is set.
inline bool FillField(int32_t *X, int32_t *Y, const uint8_t *setIn, int nx, int ny)
{
    const size_t n = (size_t)nx * ny;
    std::vector<uint8_t> set(setIn, setIn + n), next;
    size_t left = 0;
    for (size_t q = 0; q < n; ++q) left += !set[q];
    if (left == n) return false;
    while (left > 0) {
        next = set;
        for (int j = 0; j < ny; ++j)
            for (int i = 0; i < nx; ++i) {
                const size_t q = (size_t)j * nx + i;
                if (set[q]) continue;
                long k = 0, sumX = 0, sumY = 0;
                auto take = [&](size_t p) { if (set[p]) { ++k; sumX += X[p]; sumY += Y[p]; } };
                if (i > 0) take(q - 1);
                if (i + 1 < nx) take(q + 1);
                if (j > 0) take(q - nx);
                if (j + 1 < ny) take(q + nx);
                if (k == 0) continue;
                X[q] = (int32_t)WarpFloorDiv(2 * sumX + k, 2 * k);
                Y[q] = (int32_t)WarpFloorDiv(2 * sumY + k, 2 * k);
                next[q] = 1;
                --left;
            }
        set.swap(next);
    }
    return true;
}

// `passes` times [1 2 1] along the node lines, then across them, replicated edges: (a + 2 b + c + 2) >> 2
inline void SmoothField(int32_t *N, int nx, int ny, int passes)
{
    std::vector<int32_t> t((size_t)std::max(nx, ny));
    for (int p = 0; p < passes; ++p) {
        for (int j = 0; j < ny; ++j) {
            int32_t *r = N + (size_t)j * nx;
            for (int i = 0; i < nx; ++i) t[i] = (r[i > 0 ? i - 1 : 0] + 2 * r[i] + r[i + 1 < nx ? i + 1 : nx - 1] + 2) >> 2;
            std::copy(t.begin(), t.begin() + nx, r);
        }
        for (int i = 0; i < nx; ++i) {
            for (int j = 0; j < ny; ++j)
                t[j] = (N[(size_t)(j > 0 ? j - 1 : 0) * nx + i] + 2 * N[(size_t)j * nx + i] + N[(size_t)(j + 1 < ny ? j + 1 : ny - 1) * nx + i] + 2) >> 2;
            for (int j = 0; j < ny; ++j) N[(size_t)j * nx + i] = t[j];
        }
    }
}

namespace warpfield_detail {

inline std::invalid_argument bad(const std::string &what) { return std::invalid_argument("regcheck report invalid: " + what); }

// a whole token as a decimal integer of magnitude <= limit
inline long integer(const std::string &tok, const char *name, long limit)
{
    const char *d = tok.c_str();
    if (*d == '+' || *d == '-') ++d;
    if (!*d || strspn(d, "0123456789") != strlen(d) || strlen(d) > 18) throw bad(std::string(name) + " `" + tok.substr(0, 32) + "' is not an integer");
    const long v = strtol(tok.c_str(), nullptr, 10);
    if (v > limit || v < -limit) throw bad(std::string(name) + " " + tok.substr(0, 32) + " is out of range");
    return v;
}

// a whole token as a finite number
inline double number(const std::string &tok, const char *name)
{
    if (tok.empty() || tok.size() > 64 || isspace((unsigned char)tok[0])) throw bad(std::string(name) + " `" + tok.substr(0, 32) + "' is not a number");
    char *e = nullptr;
    const double v = strtod(tok.c_str(), &e);
    if (e == tok.c_str() || *e) throw bad(std::string(name) + " `" + tok.substr(0, 32) + "' is not a number");
    if (!std::isfinite(v)) throw bad(std::string(name) + " " + tok.substr(0, 32) + " is not finite");
    return v;
}

// the value of the LAST ` key=` token of the header line (the file names, which may hold anything, come first)
inline long header(const std::string &line, const char *key, long limit)
{
    const std::string k = std::string(" ") + key + "=";
    const size_t at = line.rfind(k);
    if (at == std::string::npos) throw bad(std::string("the header lacks ") + key + "=");
    const size_t a = at + k.size(), b = line.find(' ', a);
    return integer(line.substr(a, b == std::string::npos ? std::string::npos : b - a), key, limit);
}

}  // namespace warpfield_detail

// The field of a report's text.  w, h > 0: the image the field is for (a node outside it is an error); 0: not checked.
inline WarpField ParseRegReport(const std::string &text, long w, long h)
{
    using namespace warpfield_detail;
    if (text.find('\0') != std::string::npos) throw bad("not a text file");
    struct Tile { long x, y; double dx, dy; int flags; };
    std::vector<Tile> tiles;
    WarpField f;
    long scale = 0, shiftX = 0, shiftY = 0;
    size_t pos = 0;
    bool first = true;
    while (pos < text.size()) {
        size_t e = text.find('\n', pos);
        if (e == std::string::npos) e = text.size();
        std::string line = text.substr(pos, e - pos);
        pos = e + 1;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (first) {
            first = false;
            if (line.rfind("# oip regcheck ", 0) != 0) throw bad("the first line is not `# oip regcheck ...'");
            scale = header(line, "scale", 64);
            shiftX = header(line, "shift-x", kWarpMaxCoord);
            shiftY = header(line, "shift-y", kWarpMaxCoord);
            f.band2 = (int)header(line, "band2", 4);
            if (scale < 1) throw bad("scale=" + std::to_string(scale));
            if (f.band2 < 1) throw bad("band2=" + std::to_string(f.band2));
            continue;
        }
        if (line.empty() || line[0] == '#') continue;
        std::string tok[6];
        size_t a = 0;
        for (int k = 0; k < 6; ++k) {
            const size_t c = k < 5 ? line.find(',', a) : std::string::npos;
            if (k < 5 && c == std::string::npos) throw bad("tile line `" + line.substr(0, 48) + "': x,y,dx,dy,score,flags expected");
            tok[k] = line.substr(a, c == std::string::npos ? std::string::npos : c - a);
            a = c + 1;
        }
        Tile t;
        t.x = integer(tok[0], "x", kWarpMaxCoord);
        t.y = integer(tok[1], "y", kWarpMaxCoord);
        t.dx = number(tok[2], "dx");
        t.dy = number(tok[3], "dy");
        number(tok[4], "score");
        t.flags = (int)integer(tok[5], "flags", 31);                // (16: OIP_MATCH_MASKED of `regcheck --mask`)
        if (t.x < 0 || t.y < 0 || t.flags < 0) throw bad("tile line `" + line.substr(0, 48) + "': a negative position or flag");
        if (t.x % scale || t.y % scale) throw bad("tile position " + std::to_string(t.x) + "," + std::to_string(t.y) + " is not a multiple of scale");
        if ((long)tiles.size() >= kWarpMaxNodes) throw bad("more than 2^27 tiles");
        tiles.push_back(t);
    }
    if (first) throw bad("the file is empty");
    if (tiles.empty()) throw bad("no tile line");
    // a row-major regular lattice: nx tiles share the first y, then every (j, i) lies at (x0 + i stepX, y0 + j stepY)
    const long n = (long)tiles.size();
    long nx = 1;
    while (nx < n && tiles[nx].y == tiles[0].y) ++nx;
    if (n % nx != 0) throw bad("ragged lattice: " + std::to_string(n) + " tiles, " + std::to_string(nx) + " in the first line");
    const long ny = n / nx;
    const long stepX = nx > 1 ? tiles[1].x - tiles[0].x : scale, stepY = ny > 1 ? tiles[nx].y - tiles[0].y : scale;
    if (stepX <= 0 || stepY <= 0) throw bad("irregular lattice: the tiles are not in row-major order");
    for (long j = 0; j < ny; ++j)
        for (long i = 0; i < nx; ++i) {
            const Tile &t = tiles[j * nx + i];
            if (t.x != tiles[0].x + i * stepX || t.y != tiles[0].y + j * stepY)
                throw bad("irregular lattice at tile " + std::to_string(j * nx + i) + " (" + std::to_string(t.x) + "," + std::to_string(t.y) + ")");
        }
    if (stepX / scale > OIP_WARP_MAX_STEP || stepY / scale > OIP_WARP_MAX_STEP) throw bad("a lattice step above 65536");
    f.nx = (int)nx;
    f.ny = (int)ny;
    f.sx = (int)(stepX / scale);                                 // positions are multiples of scale, so are the steps
    f.sy = (int)(stepY / scale);
    f.gx0 = tiles[0].x / scale - shiftX;
    f.gy0 = tiles[0].y / scale - shiftY;
    if (w > 0 && h > 0 && (f.gx0 < 0 || f.gy0 < 0 || f.gx0 + (nx - 1) * f.sx >= w || f.gy0 + (ny - 1) * f.sy >= h))
        throw bad("a node lies outside the image of " + std::to_string(w) + " x " + std::to_string(h) + " (is this the report's image 2?)");
    f.X.assign((size_t)n, 0);
    f.Y.assign((size_t)n, 0);
    std::vector<uint8_t> set((size_t)n, 0);
    for (long q = 0; q < n; ++q) {
        const Tile &t = tiles[q];
        if (t.flags != 0) continue;
        if (std::fabs(t.dx) > 64.0 || std::fabs(t.dy) > 64.0) throw bad("a shift above 64 px at tile " + std::to_string(q));
        f.X[q] = (int32_t)std::rint(t.dx * 1024.0);
        f.Y[q] = (int32_t)std::rint(t.dy * 1024.0);
        set[q] = 1;
        ++f.used;
    }
    if (!FillField(f.X.data(), f.Y.data(), set.data(), f.nx, f.ny)) throw bad("no usable tile (every tile carries a flag)");
    return f;
}

// the text of a report file; std::runtime_error where it cannot be read
inline std::string ReadRegReport(const std::string &path)
{
    FILE *fp = fopen(path.c_str(), "rb");
    if (!fp) throw std::runtime_error("open file [" + path + "] failed: " + std::to_string(errno));
    const size_t limit = (size_t)1 << 33;                         // 64 bytes a tile of the largest lattice
    std::string text;
    char buff[65536];
    size_t got = 0;
    while (text.size() <= limit && (got = fread(buff, 1, sizeof buff, fp)) > 0) text.append(buff, got);
    const bool err = ferror(fp) != 0;
    fclose(fp);
    if (err) throw std::runtime_error("read of file [" + path + "] failed");
    if (text.size() > limit) throw warpfield_detail::bad("not a report (above 8 GiB)");
    return text;
}

}  // namespace OIPGPU
