// oip_tiffshared.h -- TIFF arithmetic that the host codec (oip_tiff.hpp) and the host side of the device coder (tifflzw.hip) share
#pragma once

#include <cstddef>

namespace OIPGPU {
namespace tiffdetail {
// worst case of an encoded LZW strip of n bytes: one 12-bit code per byte, plus Clear / EOI codes
inline size_t lzw_worst(size_t n) { return n + n / 2 + n / 1024 + 64; }
}  // namespace tiffdetail
}  // namespace OIPGPU
