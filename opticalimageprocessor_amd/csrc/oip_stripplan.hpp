// oip_stripplan.hpp -- the block geometry of the strip-streaming raster tools (oip_rastertools.hpp) as pure arithmetic: how
// many lines a block holds and, for block i of a line range, which lines it writes and reads, at which byte offsets, in
// which of the two device slots.  Nothing of HIP or the C ABI in here: tests/cpp/stripplan_test.cpp runs it on the CPU.
#pragma once

#include <algorithm>
#include <cstddef>

namespace OIPGPU {

// 64 MiB of lines (two such slots fill the pinned ring), rounded down to the multiple q the tool needs and never below q;
// a positive override (the test hooks of mtfc and despike) replaces it
inline long StripBlockLines(size_t lineBytes, long q = 1, long override = 0)
{
    return override > 0 ? override : std::max<long>(q, (long)(((size_t)64 << 20) / lineBytes) / q * q);
}

struct StripBlock {
    int slot;                               // which of the two device blocks of either kind
    long dstFirst, dstLines;                // the image lines [r, r + m) this block produces
    long srcFirst, srcLines;                // the image lines it reads: halo lines either side, clamped to the image
    size_t srcOffset, srcBytes;             // ... in the input file
    size_t dstOffset, dstBytes;             // ... in the product, which holds the lines of the range alone
};

// the lines [first, first + n) of an image of L lines of lineBytes bytes, in blocks of blockLines lines
struct StripPlan {
    long first, n, L, halo, blockLines;
    size_t lineBytes;

    long blocks() const { return (n + blockLines - 1) / blockLines; }
    bool secondSlot() const { return blocks() > 1; }         // a second buffer only if there is a second block
    long outLines() const { return std::min(blockLines, n); }                   // line capacity of an output buffer
    long inLines() const { return std::min(outLines() + 2 * halo, L); }         // ... of an input buffer
    StripBlock block(long i) const
    {
        StripBlock b;
        b.slot = (int)(i & 1);
        b.dstFirst = first + i * blockLines;
        b.dstLines = std::min(blockLines, first + n - b.dstFirst);
        b.srcFirst = std::max<long>(0, b.dstFirst - halo);
        b.srcLines = std::min(L, b.dstFirst + b.dstLines + halo) - b.srcFirst;
        b.srcOffset = (size_t)b.srcFirst * lineBytes;
        b.srcBytes = (size_t)b.srcLines * lineBytes;
        b.dstOffset = (size_t)(b.dstFirst - first) * lineBytes;
        b.dstBytes = (size_t)b.dstLines * lineBytes;
        return b;
    }
};

}  // namespace OIPGPU
