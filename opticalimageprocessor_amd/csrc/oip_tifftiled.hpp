// oip_tifftiled.hpp -- the tiled sibling of TiffWriterU16 (oip_tiff.hpp): the writer of `oip cog`.  Host code only.
//
// A little-endian TIFF / BigTIFF (the strip writer's rule, on the worst-case sum of every directory's payload; OIP_TIFF_FORCE_BIG)
// of a width x height image of spp u16 samples in T x T tiles and of its `levels` reduced-resolution levels, each half the one
// before, rounded up.  File order:
//   1. the header;
//   2. directory 0 (the image), then directories 1 .. n (levels 1 .. n, NewSubfileType 254 = 1), chained by their next-directory
//      offsets; each directory is followed by its own out-of-line values: BitsPerSample and SampleFormat where they do not fit
//      the entry, then TileOffsets, then TileByteCounts;
//   3. from an even offset, the payloads: the tiles of the image in tile order (row-major), then those of level 1, 2, .. n.
// Every directory and table has a size that follows from the geometry alone, so the head (1 + 2) is reserved at construction
// and written by close(), when the byte counts are known: all directories lie at the start of the file, where a reader that
// fetches ranges gets them with its first request.  (GDAL's COG driver writes the payloads smallest level first and a ghost
// header; this writer does neither.)
// Tags: those TiffWriterU16 writes for a product of the same geometry and spp, with 322 TileWidth, 323 TileLength, 324
// TileOffsets, 325 TileByteCounts in place of 273 / 278 / 279; 317 = 2 with LZW and Deflate.  A tile is the T x T x spp block of the
// tile-major form (include/oip_c.h: oip_retile_u16) -- edge tiles replicate the last column and line --, uncompressed or, one
// LZW or zlib (Deflate, csrc/oip_deflate.h) stream per tile, with predictor 2 along each tile row.  Tiles start on even offsets.
#pragma once

#include "oip_tiff.hpp"

namespace OIPGPU {

class TiffTiledWriterU16 {
public:
    TiffTiledWriterU16(const std::string &path, int width, long height, int spp, int tile, int compression, int levels)
        : mSpp(spp), mT(tile), mComp(compression)
    {
        if (width <= 0 || height <= 0 || (spp != 1 && spp != 4) || levels < 0 || levels > 16 || tile < 16 || tile > 1024 || tile % 16 != 0)
            throw std::invalid_argument("TiffTiledWriterU16: bad geometry");
        if (compression != TIFF_NONE && compression != TIFF_LZW && compression != TIFF_DEFLATE) throw std::invalid_argument("TiffTiledWriterU16: unsupported compression");
        mTileBytes = (uint64_t)tile * tile * spp * 2;
        uint64_t worst = 0, ntiles = 0;
        for (int k = 0; k <= levels; ++k) {
            Dir d;
            d.w = (int)(((long)width - 1) >> k) + 1;
            d.h = ((height - 1) >> k) + 1;
            d.tx = (d.w + tile - 1) / tile;
            d.ty = (d.h + tile - 1) / tile;
            d.n = (uint64_t)d.tx * (uint64_t)d.ty;
            worst += d.n * tiffdetail::worst_payload(mTileBytes, mComp);
            ntiles += d.n;
            mDirs.push_back(std::move(d));
        }
        mBig = tiffdetail::needs_bigtiff(worst, ntiles);
        // the head: where every directory and table will lie
        uint64_t pos = mBig ? 16 : 8;
        for (size_t k = 0; k < mDirs.size(); ++k) {
            Dir &d = mDirs[k];
            d.ifd = pos;
            tiffdetail::TiffDirectory &t = d.tags;
            t.big = mBig; t.reduced = k > 0; t.width = (uint64_t)d.w; t.height = (uint64_t)d.h; t.spp = mSpp; t.compression = mComp;
            t.tile = (uint64_t)mT; t.nchunks = d.n;
            std::vector<unsigned char> entries;
            t.append_to(entries, 0);
            pos += entries.size();
            if (!t.fits((uint64_t)mSpp, 2)) { t.bitsAt = pos; pos += (uint64_t)mSpp * 2; t.formatAt = pos; pos += (uint64_t)mSpp * 2; }
            if (!t.fits(d.n, t.field())) { t.offsets = pos; pos += d.n * t.field(); t.counts = pos; pos += d.n * t.field(); }
            if (pos & 1) ++pos;
        }
        mHead = mPos = pos;
        if (!mBig && mHead > 0xFFFFF000ull) throw std::runtime_error("TiffTiledWriterU16: classic TIFF overflow");
        mF = fopen(path.c_str(), "wb");
        if (!mF) throw std::runtime_error("open file [" + path + "] failed");
        // the reserved head reads as zeros until close()
        std::vector<unsigned char> z((size_t)std::min<uint64_t>(mHead, 1 << 20), 0);
        for (uint64_t done = 0; done < mHead; done += z.size()) put(z.data(), (size_t)std::min<uint64_t>(z.size(), mHead - done));
        if (fflush(mF) != 0) { fclose(mF); mF = nullptr; throw std::runtime_error("TiffTiledWriterU16: write failed"); }
    }

    // geometry of the directory being written
    int width() const { return cur().w; }
    long height() const { return cur().h; }
    long tiles_x() const { return cur().tx; }
    long tiles_y() const { return cur().ty; }
    int tile() const { return mT; }
    int level() const { return (int)mCur; }
    int levels() const { return (int)mDirs.size() - 1; }
    bool bigtiff() const { return mBig; }
    uint64_t first_payload_offset() const { return mHead; }

    // The tiles of the current directory are written by someone else (the device: tiled_image_from_device, oip_host.hpp) from the
    // offset begin_tiles() returns on; end_tiles() takes their offsets inside that block, in tile order, and their sizes.
    uint64_t begin_tiles()
    {
        if (!mF || cur().done) throw std::logic_error("TiffTiledWriterU16: the directory has its tiles");
        return mPos;
    }
    void end_tiles(const uint64_t *off, const uint64_t *len, size_t n, uint64_t payload_bytes)
    {
        Dir &d = mDirs[mCur];
        if (!mF || d.done || n != d.n) throw std::logic_error("TiffTiledWriterU16: tile count");
        if (!mBig && mPos + payload_bytes > 0xFFFFF000ull) throw std::runtime_error("TiffTiledWriterU16: classic TIFF overflow");
        d.off.resize(n);
        d.len.resize(n);
        for (size_t k = 0; k < n; ++k) {
            if ((off[k] & 1) || off[k] > payload_bytes || len[k] > payload_bytes - off[k]) throw std::logic_error("TiffTiledWriterU16: tile outside its payload");
            d.off[k] = mPos + off[k];
            d.len[k] = len[k];
        }
        mPos += payload_bytes;
        if (mPos & 1) ++mPos;
        d.done = true;
    }

    // The host path: the current directory from its tile-major form (tiles_y() * tiles_x() tiles of T x T x spp samples),
    // encoded with the host coders of oip_tiff.hpp on its threads -- the same file bytes as the device path.
    void write_tiles(const uint16_t *tileMajor)
    {
        const Dir &d = cur();
        const uint64_t at = begin_tiles();
        const int fd = fileno(mF);
        std::vector<uint64_t> off((size_t)d.n), len((size_t)d.n);
        uint64_t pos = 0;
        if (mComp == TIFF_NONE) {
            for (uint64_t k = 0; k < d.n; ++k) { off[(size_t)k] = k * mTileBytes; len[(size_t)k] = mTileBytes; }
            pos = d.n * mTileBytes;
            tiffdetail::pwrite_all(fd, tileMajor, (size_t)pos, at, "TiffTiledWriterU16");
        } else {
            const size_t tileSamples = (size_t)(mTileBytes / 2), worst = tiffdetail::chunk_worst((size_t)mTileBytes, mComp);
            const uint64_t batch = std::max<uint64_t>(2 * (uint64_t)tiffdetail::worker_count(), ((uint64_t)64 << 20) / mTileBytes + 1);
            std::unique_ptr<uint8_t[]> arena(new uint8_t[(size_t)std::min(batch, d.n) * worst]);
            std::vector<std::unique_ptr<uint16_t[]>> scratch((size_t)tiffdetail::worker_count());
            for (uint64_t k0 = 0; k0 < d.n; k0 += batch) {
                const uint64_t kn = std::min(batch, d.n - k0);
                tiffdetail::parallel_for_t((size_t)kn, [&](size_t j, int t) {
                    if (!scratch[(size_t)t]) scratch[(size_t)t].reset(new uint16_t[tileSamples]);
                    len[(size_t)(k0 + j)] = tiffdetail::encode_chunk(tileMajor + (size_t)(k0 + j) * tileSamples, mT, (size_t)mT, mSpp, false,
                                                                     scratch[(size_t)t].get(), arena.get() + j * worst, mComp);
                });
                for (uint64_t j = 0; j < kn; ++j) {
                    if (pos & 1) ++pos;                                 // tiles start on even offsets (the gap reads as zero)
                    off[(size_t)(k0 + j)] = pos;
                    tiffdetail::pwrite_all(fd, arena.get() + j * worst, (size_t)len[(size_t)(k0 + j)], at + pos, "TiffTiledWriterU16");
                    pos += len[(size_t)(k0 + j)];
                }
            }
        }
        end_tiles(off.data(), len.data(), (size_t)d.n, pos);
    }

    // the current directory is complete; the tiles of the next level follow
    void next_directory()
    {
        if (!mF || !cur().done || mCur + 1 >= mDirs.size()) throw std::logic_error("TiffTiledWriterU16: no further directory");
        ++mCur;
    }

    // writes the head
    void close()
    {
        if (!mF) return;
        if (mCur + 1 != mDirs.size() || !cur().done) { fclose(mF); mF = nullptr; throw std::logic_error("TiffTiledWriterU16: directories missing"); }
        std::vector<unsigned char> head;
        head.reserve((size_t)mHead);
        auto putv = [&](uint64_t v, size_t n) { tiffdetail::put_le(head, v, n); };
        if (mBig) { putv('I', 1); putv('I', 1); putv(43, 2); putv(8, 2); putv(0, 2); putv(mDirs[0].ifd, 8); }
        else { putv('I', 1); putv('I', 1); putv(42, 2); putv(mDirs[0].ifd, 4); }
        for (size_t k = 0; k < mDirs.size(); ++k) {
            Dir &d = mDirs[k];
            if (head.size() != d.ifd) { fclose(mF); mF = nullptr; throw std::logic_error("TiffTiledWriterU16: head layout"); }
            const bool tables = d.tags.offsets != 0;                                   // (else the one tile's values lie in the entries)
            if (!tables) { d.tags.offsets = d.off[0]; d.tags.counts = d.len[0]; }
            d.tags.append_to(head, k + 1 < mDirs.size() ? mDirs[k + 1].ifd : 0);
            if (d.tags.bitsAt) { for (int i = 0; i < mSpp; ++i) putv(16, 2); for (int i = 0; i < mSpp; ++i) putv(1, 2); }
            if (tables) { for (uint64_t v : d.off) putv(v, d.tags.field()); for (uint64_t v : d.len) putv(v, d.tags.field()); }
            if (head.size() & 1) putv(0, 1);
        }
        if (head.size() != mHead) { fclose(mF); mF = nullptr; throw std::logic_error("TiffTiledWriterU16: head layout"); }
        const bool ok = fseeko(mF, 0, SEEK_SET) == 0 && fwrite(head.data(), 1, head.size(), mF) == head.size();
        if (fclose(mF) != 0 || !ok) { mF = nullptr; throw std::runtime_error("TiffTiledWriterU16: write failed"); }
        mF = nullptr;
    }

    ~TiffTiledWriterU16() { if (mF) fclose(mF); }
    TiffTiledWriterU16(const TiffTiledWriterU16 &) = delete;
    TiffTiledWriterU16 &operator=(const TiffTiledWriterU16 &) = delete;

private:
    struct Dir {
        int w = 0;
        long h = 0, tx = 0, ty = 0;
        uint64_t n = 0;                                         // tiles
        uint64_t ifd = 0;                                       // where it lies in the head
        tiffdetail::TiffDirectory tags;                         // what it says, with the places of its out-of-line values in the head
        std::vector<uint64_t> off, len;
        bool done = false;
    };
    const Dir &cur() const { return mDirs[mCur]; }
    void put(const void *p, size_t n)
    {
        if (fwrite(p, 1, n, mF) != n) { fclose(mF); mF = nullptr; throw std::runtime_error("TiffTiledWriterU16: write failed"); }
    }

    FILE *mF = nullptr;
    int mSpp, mT, mComp;
    bool mBig = false;
    uint64_t mTileBytes = 0, mHead = 0, mPos = 0;
    std::vector<Dir> mDirs;
    size_t mCur = 0;
};

}  // namespace OIPGPU
