// oip_main.cpp -- the reference's command line (main.cpp:92-343) rebuilt on the C ABI.
//
//   oip prestitch --pan1 A.RAW --pan2 B.RAW [--rrc1 --rrc2 -s -l --stitch-overlap --stt-threshold
//                 --stt-maxdeltay -e -r/--rrc/--no-rrc -c]                     (main.cpp:112-150)
//   oip stitch --image1 L.RAW --image2 R.RAW -c/--fold-cols N [-o OUT.RAW]       (main.cpp:159-190)
//              [--balance none|offset|gain|moments --balance-lines N --feather N --valid-min N --valid-max N --min-count N]
//                                                                               see seam_options() and run_stitch()
//   oip --pan P.RAW --mss M.RAW [--do-rrc4pan --rrc-pan F --no-rrc4mss --rrc-msb1..4 F --slices
//       --ibc-sections --ibc-threshold --line-offset --lines-section --overlap-lines -k]   (:193-252)
//   oip task ...                fused flow of DOC/sample-task.sh, see run_task()
//   oip rrc-calib [--pan P.RAW --rrc-pan OUT] [--mss M.RAW --rrc-msb1..4 OUT]   derives the RRC coefficient files the
//                               actions above read from a strip's per-column statistics, see run_rrc_calib()
//   oip quicklook IMAGE [-o OUT.TIFF] [--factor 16 ...]   8-bit browse image of a strip or product, see run_quicklook()
//                 [--format jpeg [--quality 90]]            ... as a baseline JPEG (<stem>.QL.JPG), its scan encoded on the GPU
//   oip mtfc IMAGE [-o OUT] (--kernel FILE | --mtf-x M --mtf-y M)   MTF-compensation filter of a strip or product, see run_mtfc()
//   oip despike IMAGE [-o OUT] [--threshold N] [--relative R] [--bad-columns FILE] [--bil]   repair of a raw strip ahead of RRC:
//                               bad columns interpolated, impulse pixels replaced by a conditional 3 x 3 median, see run_despike();
//                               --noise REPORT [--k-sigma K] takes the threshold from the report of `oip noise`
//   oip denoise IMAGE [-o OUT] (--noise REPORT | --sigma S) [--k-sigma K] [--radius 1|2|3] [--min-members M]   noise reduction of a
//                               strip or product behind RRC and ahead of mtfc: a sigma filter whose range at every signal level
//                               comes from the report of `oip noise`, see run_denoise()
//   oip noise IMAGE [-o OUT.csv] [--block 8|16] [--bits N] [--min-blocks N] [--bil]   the noise-level function of a strip or
//                               product (sigma per signal level, the fit sigma^2 = a + b mu, SNR) in <stem>.NOISE.CSV, see run_noise()
//   oip mask IMAGE [-o OUT.TIFF] [--report OUT.csv] [--cell 4|8|16] [--bits N] [--saturation DN] [--bands B,G,R,N] [--open A] [--buffer D]
//                               which parts of a strip or product are usable: no data, saturated, cloud and its buffer per cell, in
//                               <stem>.MASK.TIFF and <stem>.MASK.CSV, see run_mask(); `regcheck --mask FILE --mask-cell C` flags the
//                               tiles that touch a masked cell
//   oip wallis IMAGE [-o OUT] [--report OUT.csv] [--block 32|64|128|256] [--contrast C] [--brightness B] [--mean M] [--std S]
//                               local brightness and contrast equalisation (the Wallis filter) of a strip or product, in
//                               <stem>.WAL.<ext> and <stem>.WAL.CSV, see run_wallis()
//   oip mtf IMAGE [-o OUT.csv] [--axis x|y|both] [--contrast-min DN] [--tv-slack DN | --noise REPORT]   the MTF at Nyquist across
//                               and along the lines from the slanted edges of a strip or product, in <stem>.MTF.CSV, see run_mtf();
//                               `mtfc --mtf REPORT [--mtf-stat median|p75|p90]` designs its filter from the report
//   oip overviews IMAGE [-o OUT] [--levels N] [--valid-min N]   the reduced-resolution pyramid of a strip or product as
//                               <IMAGE>.ovr beside it; `stitch --overviews [--levels N]` writes its product's, see run_overviews()
//   oip regcheck --image1 A [--image2 B] [--band1 k] [--band2 k] [--scale F] [--shift-x N] [--shift-y N] [--tile T] [--search S]
//                               how well two rasters are registered: tile matching (ZNCC), a shift and a score per tile and a
//                               summary in <A>.REG.CSV, see run_regcheck()
//   oip regfix --report R.CSV --image B [--bands k[,k...]|all] [--smooth N] [--width N] [-o OUT]   resamples image 2 of a regcheck
//                               report by the shift field the report holds, so that it lands on image 1, see run_regfix()
//   oip cog IMAGE [-o OUT] [--tile T] [--levels N] [--valid-min N]   the image as a tiled TIFF with its pyramid inside,
//                               <stem>.COG.TIFF, see run_cog()
//   oip rescale IMAGE [-o OUT] (--scale S | --scale-x SX | --scale-y SY | --to-width N | --to-lines N) [--kernel lanczos|cubic|linear]
//                               [--valid-min V]   the image on another pixel grid by an antialiased polyphase filter, <stem>.RSC.<ext>,
//                               see run_rescale()
//   oip pansharpen --pan P --mss M [--line-offset N] [--max-gain G] [--width N] [-o OUT] [--force] [--overviews [--levels N]]
//                               fuses the PAN strip and the aligned MSS product into a 4-band product at PAN resolution, see
//                               run_pansharpen()
//   oip -v | --version          prints 1.1
// plus --width N (pixels per PAN line; the reference hard-codes 12288, oipshared.h:28).
// `auxsep` is outside this build.  TIFF input and output go through oip_tiff.hpp (uncompressed and LZW, with
// or without the horizontal predictor, and Deflate with it: --tiff-compress deflate).  Not the reference's: --fit, --fp16-accumulate, the seam options of stitch
// (--balance, --balance-lines, --feather and their --valid-min / --valid-max / --min-count; `task` takes them too, with
// --feather-pan / --feather-mss for its two stitches), --overviews / --levels of stitch and the rrc-calib, quicklook, mtfc,
// despike, denoise, noise, mask, wallis, mtf, overviews, cog, rescale, regcheck, regfix and pansharpen sub-commands.
//
// Exit codes as the reference: usage_error -> "USAGE ERROR" + 254; any std::exception -> 2; unknown
// -> 1; help/version -> 255 (CLI11's Success + 255, main.cpp:262-263); argument errors -> CLI11's
// codes (RequiredError 106, ValidationError 105, ExtrasError 109, ConversionError 104).  A raster tool's run_* refuses bad option
// values with those; what needs the container, a file or the image is refused in its *Check (oip_rastertools.hpp) with 2 or 254.
#include <climits>
#include <cstdlib>
#include <unistd.h>
#include <map>
#include <set>

#include "oip_host.hpp"
#include "oip_rastertools.hpp"
#include "oip_multigpu.hpp"

using namespace OIPGPU;

namespace {

struct cli_error : public std::runtime_error {
    int code;
    cli_error(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

// option table: name -> takes a value?
struct Spec {
    std::map<std::string, std::string> alias;       // "-s" -> "--sections"
    std::set<std::string> valued, flags;
};

struct Parsed {
    std::map<std::string, std::string> val;
    std::set<std::string> flag;
    bool has(const std::string &k) const { return val.count(k) || flag.count(k); }
    std::string str(const std::string &k, const std::string &def = "") const { auto it = val.find(k); return it == val.end() ? def : it->second; }
    int integer(const std::string &k, int def) const
    {
        auto it = val.find(k);
        if (it == val.end()) return def;
        char *e = nullptr;
        long v = strtol(it->second.c_str(), &e, 10);
        if (!e || *e) throw cli_error(104, "Could not convert: " + k + " = " + it->second);
        return (int)v;
    }
    double real(const std::string &k, double def) const
    {
        auto it = val.find(k);
        if (it == val.end()) return def;
        char *e = nullptr;
        double v = strtod(it->second.c_str(), &e);
        if (!e || *e) throw cli_error(104, "Could not convert: " + k + " = " + it->second);
        return v;
    }
    // an integer option of the raster tools that lies in [lo, hi], or 105 and "<option>: <expected>"
    int within(const std::string &k, int def, int lo, int hi, const char *expected) const
    {
        const int v = integer(k, def);
        if (v < lo || v > hi) throw cli_error(105, k + ": " + expected);
        return v;
    }
    // ... and the ranges several of them share, each with its one message
    int valid_min() const { return within("--valid-min", 1, 0, 65535, "0 <= N <= 65535 expected"); }
    int positive_width(int def) const { return within("--width", def, 1, INT_MAX, "a positive line width expected"); }
    void valid_range(int defMin, int *lo, int *hi) const
    {
        *lo = integer("--valid-min", defMin);
        *hi = integer("--valid-max", 65535);
        if (*lo < 0 || *hi > 65535 || *lo > *hi) throw cli_error(105, "--valid-min/--valid-max: 0 <= min <= max <= 65535 expected");
    }
    // --line-offset / --lines (0: to the end); `also` is a count that `alsoKeys` names in the same message (rrc-calib's --min-count)
    void line_range(long *offset, long *lines, const std::string &alsoKeys = "", long also = 0) const
    {
        *offset = integer("--line-offset", 0);
        *lines = integer("--lines", 0);
        if (also < 0 || *offset < 0 || *lines < 0) throw cli_error(105, alsoKeys + "--line-offset, --lines: non-negative values expected");
    }
};

Parsed parse(const Spec &sp, const std::vector<std::string> &args)
{
    Parsed p;
    for (size_t i = 0; i < args.size(); ++i) {
        std::string a = args[i], v;
        bool has_v = false;
        auto eq = a.find('=');
        if (a.rfind("--", 0) == 0 && eq != std::string::npos) { v = a.substr(eq + 1); a = a.substr(0, eq); has_v = true; }
        auto al = sp.alias.find(a);
        if (al != sp.alias.end()) a = al->second;
        if (sp.flags.count(a)) { p.flag.insert(a); continue; }
        if (sp.valued.count(a)) {
            if (!has_v) {
                if (i + 1 >= args.size()) throw cli_error(114, a + ": 1 required value missing");
                v = args[++i];
            }
            p.val[a] = v;
            continue;
        }
        throw cli_error(109, "The following argument was not expected: " + args[i]);
    }
    return p;
}

// The tools with one positional argument (quicklook, mtfc, despike, denoise, noise, mask, wallis, mtf, overviews, cog, rescale; regcheck, regfix and pansharpen name their
// images by options): IMAGE, an existing regular file, is the first argument that is neither an option nor the value of one (an
// option's value stays with it, alias or not); the rest is parsed as usual.
Parsed parse_with_image(const Spec &sp, const std::vector<std::string> &args, std::string *image)
{
    std::vector<std::string> rest;
    for (size_t i = 0; i < args.size(); ++i) {
        const std::string &a = args[i];
        if (!a.empty() && a[0] != '-' && image->empty()) { *image = a; continue; }
        rest.push_back(a);
        auto al = sp.alias.find(a);
        if (sp.valued.count(al != sp.alias.end() ? al->second : a) && i + 1 < args.size()) rest.push_back(args[++i]);
    }
    Parsed p = parse(sp, rest);
    if (image->empty()) throw cli_error(106, "IMAGE is required");
    struct stat st;
    if (stat(image->c_str(), &st) != 0 || !S_ISREG(st.st_mode)) throw cli_error(105, "IMAGE: File does not exist: " + *image);
    return p;
}

void require(const Parsed &p, const std::string &k)
{
    if (!p.has(k)) throw cli_error(106, k + " is required");
}

void existing_file(const Parsed &p, const std::string &k)
{
    if (!p.val.count(k)) return;
    struct stat st;
    if (stat(p.val.at(k).c_str(), &st) != 0 || !S_ISREG(st.st_mode))
        throw cli_error(105, k + ": File does not exist: " + p.val.at(k));
}

// --fit reference|lstsq (not in the reference): which solver fits the shift polynomials.  `reference` (default)
// restates NumCpp's Poly1d::fit operation by operation (preproc.h:535-536) so the maps are the reference's;
// `lstsq` solves the same least-squares problem by Householder QR on a scaled abscissa.
int fit_mode(const Parsed &p)
{
    const std::string f = p.str("--fit", "reference");
    if (f == "reference") return OIP_FIT_REFERENCE;
    if (f == "lstsq") return OIP_FIT_LSTSQ;
    throw cli_error(105, "--fit: reference or lstsq expected");
}

void usage()
{
    puts("Optical Satellite Image Pre-Processing/Processing Utility (MI355X build)\n"
         "Usage: oip [OPTIONS] [SUBCOMMAND]\n\n"
         "Options:\n"
         "  -h,--help  -v,--version  --width N  --tiff-compress reference|none|lzw|deflate\n"
         "  --pan FILE --mss FILE [--do-rrc4pan --rrc-pan FILE --write-rrcpan/--no-rrcpan] [--no-rrc4mss]\n"
         "  --rrc-msb1 FILE --rrc-msb2 FILE --rrc-msb3 FILE --rrc-msb4 FILE\n"
         "  --slices N --ibc-sections N --ibc-threshold X --line-offset N --lines-section N --overlap-lines N -k,--keep-leading\n"
         "  --fit reference|lstsq   (polynomial fit: the reference's NumCpp formulation [default] or QR least squares)\n\n"
         "Subcommands:\n"
         "  prestitch  --pan1 FILE --pan2 FILE [--rrc1 FILE --rrc2 FILE -s N -l N --stitch-overlap N\n"
         "             --stt-threshold X --stt-maxdeltay X -e N -r,--rrc/--no-rrc -c,--only-calculate --fp16-accumulate]\n"
         "  stitch     --image1 FILE --image2 FILE -c,--fold-cols N [-o,--out FILE] [-g,--GDAL -m,--band-map a,b,c,d]\n"
         "             [--balance none|offset|gain|moments] image 2's gain / offset relative to image 1, fitted on the overlap\n"
         "             [--balance-lines N] with --balance: a fit per block of N lines (N >= 1), interpolated to a gain / offset per line\n"
         "             [--feather N] blend the images over N columns around the seam (even, 0 <= N <= fold-cols)\n"
         "             [--valid-min N] [--valid-max N] (samples outside are no data; default 1, 65535) [--min-count N]\n"
         "             [--overviews] [--levels N] also write the product's pyramid to <output>.ovr, as `overviews` does (--valid-min applies)\n"
         "  --gpus N   (default action and prestitch) scan-line blocks over the N GPUs of the node, RCCL exchanges\n"
         "  plan       strip|ccd --width W --lines L --gpus N ...: print the multi-GPU row plan as JSON\n"
         "  task       prestitch + stitch + default action x2 + stitch in one process (intermediates stay on the GPU;\n"
         "             --pan-only: the stitched PAN product alone, RRC and resampling written straight into it):\n"
         "             --pan1 --pan2 --rrc1 --rrc2 --mss1 --mss2 --rrc-mss{1,2}-b{1..4} FILE --fold-cols-pan N --fold-cols-mss N\n"
         "             --out-pan FILE.TIFF --out-mss FILE.TIFF [prestitch, default-action and stitch options]\n"
         "             [--balance M --balance-lines N --valid-min N --valid-max N --min-count N] as for stitch, applied to both stitches,\n"
         "             [--feather-pan N] [--feather-mss N] (even, 0 <= N <= the stitch's --fold-cols-*); none of these with --pan-only\n"
         "  rrc-calib  derive RRC coefficient files from a strip (moment matching of the per-column statistics); the --rrc-* files\n"
         "             are OUTPUTS here, and the same arguments given to the default action apply them:\n"
         "             [--pan FILE --rrc-pan OUT] [--mss FILE --rrc-msb1 OUT --rrc-msb2 OUT --rrc-msb3 OUT --rrc-msb4 OUT]\n"
         "             [--mode moments|gain] [--valid-min N] [--valid-max N] [--min-count N]\n"
         "             [--line-offset N] [--lines N] (of each image's own lines) [--force] (replace existing OUT files)\n"
         "             [--bad-pan OUT] [--bad-mss OUT] the columns without usable statistics (dead detectors), as despike --bad-columns reads them\n"
         "  quicklook  IMAGE.RAW|IMAGE.TIFF: an 8-bit browse image, box-decimated by --factor and contrast-stretched per band\n"
         "             between two percentiles of its valid samples; written to <stem>.QL.TIFF in the working directory:\n"
         "             [--format tiff|jpeg] (default tiff, uncompressed; jpeg: a baseline JFIF file, <stem>.QL.JPG, its scan encoded on\n"
         "             the GPU, at most 65535 x 65535 pixels) [--quality Q] (with --format jpeg; 1 <= Q <= 100, default 90)\n"
         "             [-o,--out FILE] [--factor 2|4|8|16|32|64] [--clip-low P] [--clip-high P] [--valid-min N] [--valid-max N]\n"
         "             [--bands A | A,B,C] [--bil] (RAW: the MSS line layout) [--width N] [--line-offset N] [--lines N] [--force]\n"
         "  mtfc       IMAGE.RAW|IMAGE.TIFF: MTF compensation, a fixed-point restoration filter of up to 9 x 9 taps; the output has\n"
         "             the container of the input and is written to <stem>.MTFC.<ext> in the working directory:\n"
         "             [-o,--out FILE] --kernel FILE (text: `ky kx', then ky rows of kx coefficients summing to 1)\n"
         "             | --mtf-x M --mtf-y M (the MTF at Nyquist across / along the lines, 0 < M <= 1) [--max-gain G] (default 2.0)\n"
         "             | --mtf REPORT (the report of `oip mtf`: M of either axis from its `# all' lines) [--mtf-stat median|p75|p90]\n"
         "             (default median; p75 / p90 where soft natural edges pull the median down)\n"
         "             [--valid-min N] (samples below are no data and pass through; default 1) [--width N] [--force]\n"
         "  despike    IMAGE.RAW|IMAGE.TIFF: repair of a raw strip ahead of RRC; the output has the container of the input and is\n"
         "             written to <stem>.DSPK.<ext> in the working directory.  At least one of --threshold, --noise and --bad-columns:\n"
         "             [-o,--out FILE] [--threshold N] a sample further than N (0..65535) + R * median from the median of its 3 x 3\n"
         "             neighbourhood is replaced by it (there is no default: measure the sensor's noise) [--relative R] (0..1, default 0)\n"
         "             [--noise REPORT] (in place of --threshold / --relative) N and R from the report of `oip noise`: the tangent at the\n"
         "             report's reference level to K times its noise model, the largest over its bands [--k-sigma K] (1..100; default 5,\n"
         "             the usual convention, nothing measured)\n"
         "             [--bad-columns FILE] (RAW; text: 0-based columns, # comments) interpolated from their good neighbours\n"
         "             [--bil] (RAW: the MSS line layout, bands never mix) [--valid-min N] (samples below are no data; default 1)\n"
         "             [--width N] [--report FILE] (`column count' of the replaced samples) [--force]\n"
         "  denoise    IMAGE.RAW|IMAGE.TIFF: noise reduction behind RRC / prestitch and ahead of mtfc, Lee's sigma filter with a pilot\n"
         "             estimate: a sample becomes the mean of the neighbours of its (2 R + 1)^2 window that lie within K sigma of the\n"
         "             pilot (the same mean over 3 x 3), sigma taken at the pilot's signal level; edges and impulses stay.  The output\n"
         "             has the container of the input and is written to <stem>.DNS.<ext> in the working directory:\n"
         "             [-o,--out FILE] --noise REPORT (the report of `oip noise` on the same file: sigma^2 = a + b * level per band; its\n"
         "             bands must be the image's samples per pixel) | --sigma S (one sigma > 0 at every level of every band)\n"
         "             [--k-sigma K] (0 < K <= 100; default 2) [--radius 1|2|3] (default 2) [--min-members M] (a sample with fewer\n"
         "             neighbours in range stays as it is; 1..(2 R + 1)^2, default 2 R + 1) [--valid-min N] (samples below are no\n"
         "             data: they pass through and enter no mean; default 1) [--width N] [--force]\n"
         "  noise      IMAGE.RAW|IMAGE.TIFF: the noise-level function of a strip or product, measured on the image itself: the standard\n"
         "             deviation of every B x B block without an edge or a ramp in it, per signal level the mode of those, and the fit\n"
         "             sigma^2 = a + b * level; level_lo,level_hi,blocks,sigma,snr per band and level and the fit per band are written\n"
         "             to <stem>.NOISE.CSV in the working directory, which `despike --noise` reads:\n"
         "             [-o,--out FILE] [--block 8|16] (default 8) [--bits N] (8..16, the sensor's depth: 256 levels of 2^(N-8); default 12)\n"
         "             [--valid-min N] [--valid-max N] (a block with a sample outside is no data; default 1, 65535)\n"
         "             [--min-blocks N] (blocks a level needs; default 100) [--bil] (RAW: the MSS line layout, bands measured apart)\n"
         "             [--width N] [--line-offset N] (a multiple of the block) [--lines N] [--force]\n"
         "  mask       IMAGE.TIFF|IMAGE.RAW: which parts of a product (TIFF of 1 or 4 samples) or a single-band strip are usable, one byte\n"
         "             per C x C cell: 1 no data (a channel below --valid-min), 2 saturated (a channel at or above --saturation), and with 4\n"
         "             samples 16 cloud candidate (bright, white, hazy, not vegetation), 4 cloud (the opening of the candidates by A\n"
         "             cells), 8 buffer (within D cells of cloud); written to <stem>.MASK.TIFF (8-bit) with the counters and the shares\n"
         "             nodata_pct, saturated_pct, cloud_pct, cloud_or_buffer_pct in <stem>.MASK.CSV in the working directory:\n"
         "             [-o,--out FILE] [--report FILE] [--cell 4|8|16] (default 8) [--bits N] (8..16, full scale 2^N - 1; default 12)\n"
         "             [--saturation DN] (default: full scale) [--valid-min N] (default 1)\n"
         "             [--bands B,G,R,N] (1-based channels of blue, green, red, nir; default 3,2,1,4, the product's R, G, B, alpha order)\n"
         "             [--bright F] [--white F] [--hot F] [--ndvi F] (fractions 0..1: mean of B, G, R of full scale at least F; spread of\n"
         "             B, G, R at most F of their mean; blue - red / 2 at least F of full scale; NDVI at most F; defaults 0.30, 0.15,\n"
         "             0.08, 0.20: conventions for top-of-atmosphere-like DN, nothing was measured on real imagery)\n"
         "             [--no-cloud] (no cloud stage) [--open A] (0..32 cells; default 1) [--buffer D] (0..64 cells; default 2)\n"
         "             [--width N] [--force]\n"
         "  wallis     IMAGE.TIFF|IMAGE.RAW: the Wallis filter (dodging) on a product (TIFF of 1 or 4 samples) or a single-band strip: every\n"
         "             sample gets a gain and an offset that pull the mean and standard deviation of its B x B block toward the image's own\n"
         "             (or --mean / --std), interpolated between the blocks' centres; removes uneven illumination, haze and vignetting;\n"
         "             written to <stem>.WAL.<ext> with the figures per band and the clamp counters in <stem>.WAL.CSV:\n"
         "             [-o,--out FILE] [--report FILE] [--block 32|64|128|256] (default 128) [--contrast C] (0 < C <= 1; default 0.8)\n"
         "             [--brightness B] (0..1; default 0.6) [--mean M[,M,M,M]] [--std S[,S,S,S]] (targets; default: the image's own)\n"
         "             [--min-gain G] [--max-gain G] (0 < min <= 1 <= max <= 16; default 0.25, 4) [--min-count N] (samples a block needs)\n"
         "             [--valid-min DN] [--valid-max DN] (samples outside pass through; default 1, 65535) [--max-value DN] (results are cut\n"
         "             there; default 65535) (the defaults are conventions, nothing was measured on real imagery)\n"
         "             [--width N] [--line-offset N] [--lines N] (the selected lines are the raster) [--force]\n"
         "  mtf        IMAGE.RAW|IMAGE.TIFF: the MTF at Nyquist across (x) and along (y) the lines, measured on the image itself by the\n"
         "             slanted-edge method: every 32 x 32 tile with one straight edge of at least --contrast-min DN that crosses 1 to 8\n"
         "             samples gives a value; band,axis,ty,tx,polarity,slope_q,contrast,mtf per tile and count, median, p75 and p90 per\n"
         "             band and axis are written to <stem>.MTF.CSV in the working directory, which `mtfc --mtf` reads:\n"
         "             [-o,--out FILE] [--axis x|y|both] (default both) [--contrast-min DN] (1..65535; default 200)\n"
         "             [--tv-slack DN] (0..65535; what a profile may vary beyond its edge; default 256) | [--noise REPORT] (48 times\n"
         "             the sigma_ref of each band of a report of `oip noise`) [--valid-min N] [--valid-max N] (a tile with a sample\n"
         "             outside is no data; default 1, 65535) [--width N] [--line-offset N] [--lines N] [--force]\n"
         "  overviews  IMAGE.RAW|IMAGE.TIFF: the reduced-resolution pyramid of a strip or product, every band at 16 bits, each level\n"
         "             the 2 x 2 average of the one before; written to IMAGE.ovr beside the image, where GDAL-based viewers look for it:\n"
         "             [-o,--out FILE] [--levels N] (1..16; default: until a level fits 256 x 256) [--valid-min N] (samples below are\n"
         "             no data and do not enter an average; default 1) [--width N] [--force]\n"
         "  cog        IMAGE.TIFF|IMAGE.RAW: a product (TIFF of 1 or 4 samples, strips or tiles) or a single-band strip as a tiled TIFF\n"
         "             with its pyramid inside, the levels of `overviews` as further directories, every directory ahead of the pixels;\n"
         "             written to <stem>.COG.TIFF in the working directory:\n"
         "             [-o,--out FILE] [--tile T] (a multiple of 16, 16..1024; default 256, at 4 samples 128) [--levels N] (0..16, 0: none; default: until\n"
         "             a level fits 256 x 256) [--valid-min N] (as for overviews; default 1) [--width N] [--force]\n"
         "  rescale    IMAGE.TIFF|IMAGE.RAW: a product (TIFF of 1 or 4 samples) or a single-band strip on another pixel grid, by a separable\n"
         "             polyphase filter that is stretched on reduction (antialiasing) and replicates the border; a line-rate correction\n"
         "             (--scale-y), a fixed ground sample distance (--scale 0.8), the MSS product on the PAN grid (--scale 4); written to\n"
         "             <stem>.RSC.<ext>; -o with the other extension (.TIFF / .RAW) changes the container:\n"
         "             [-o,--out FILE] (--scale S | --scale-x SX | --scale-y SY | --to-width N | --to-lines N) (S: a decimal such as 0.8, read\n"
         "             as 8/10, or a fraction p/q; 1/4 .. 16 per axis; an axis that is not named keeps its size; --scale excludes the other\n"
         "             four, --scale-x excludes --to-width, --scale-y excludes --to-lines) [--kernel lanczos|cubic|linear] (default lanczos,\n"
         "             Lanczos-3) [--valid-min V] (an output sample whose footprint holds a sample below V takes the nearest source sample:\n"
         "             no data stays no data; 0: off; default 1) (Lanczos-3 and Q14 taps are conventions, nothing was measured on real\n"
         "             imagery) [--width N] [--force]\n"
         "  regcheck   --image1 A [--image2 B]: how well B is registered to A (TIFF of 1 or 4 samples, or single-band RAW), measured by\n"
         "             template matching (zero-mean normalised cross-correlation from exact integer sums) on a grid of tiles; writes\n"
         "             x,y,dx,dy,score,flags per tile and a summary (count, mean, std, RMS, CE90, max) to <stem of A>.REG.CSV:\n"
         "             [--band1 k] [--band2 k] (1-based; B defaults to A: band against band of one aligned product)\n"
         "             [--scale F] (2..64: box-decimate A first; PAN against an MSS band is --scale 4)\n"
         "             [--shift-x N] [--shift-y N] (B's origin in (decimated) A coordinates; the CCD overlap is --shift-x W-fold)\n"
         "             [--tile T] (multiple of 8, 8..128; default 64) [--search S] (1..16; default 4) [--step N] (default T)\n"
         "             [--valid-min N] [--valid-max N] (samples outside are no data; default 1, 65535) [--min-score X] (default 0.5)\n"
         "             flags: 1 no data in the tile, 2 flat, 4 peak on the border of the search range, 8 score below --min-score\n"
         "             [--mask FILE --mask-cell C] (the mask `oip mask --cell C` wrote for A) [--mask-bits B] (default 12: cloud or\n"
         "             buffer) flag 16: the tile's template touches a cell with a bit of B set; `regfix` leaves such tiles out\n"
         "             [--width N] [--width2 N] (RAW: samples per line of A / B) [-o,--out report.csv] [--force]\n"
         "  regfix     --report R.CSV --image B: resamples B, the image 2 of the regcheck report R.CSV (TIFF of 1 or 4 samples, or\n"
         "             single-band RAW), by the shift field the report's tiles hold, so that it lands on the report's image 1; flagged\n"
         "             tiles are filled from their neighbours, the field is bilinear between tiles, the resampling the product's\n"
         "             bicubic; the output has the container of the input and is written to <stem>.REGFIX.<ext>:\n"
         "             [--bands k[,k...]|all] (1-based; default: the report's band2; the other bands are copied)\n"
         "             [--smooth N] (0..16 passes of [1 2 1] over the field; default 0) [--width N] [-o,--out FILE] [--force]\n"
         "  pansharpen --pan P --mss M: fuses the PAN strip P (TIFF of 1 sample, or single-band RAW) and the aligned MSS product M (TIFF\n"
         "             of 4 samples, a quarter of P's line) into a 4-band product at PAN resolution: every band up-sampled by 4 (cubic)\n"
         "             and multiplied by PAN / up-sampled 4 x 4 mean of PAN; written to <stem of M>.PSH.TIFF:\n"
         "             [--line-offset N] (first PAN line used; default 0) [--max-gain G] (1..64, the ratio is cut there; default 4)\n"
         "             [--width N] (RAW: samples per PAN line) [-o,--out FILE] [--force]\n"
         "             [--overviews] [--levels N] also write the product's pyramid to <output>.ovr, as `overviews` does");
}

int run_prestitch(const std::vector<std::string> &args, int width)
{
    Spec sp;
    sp.valued = {"--pan1", "--pan2", "--rrc1", "--rrc2", "--sections", "--section-lines", "--stitch-overlap", "--stt-threshold",
                 "--stt-maxdeltay", "--edge-cols", "--width", "--gpus"};
    sp.flags = {"--rrc", "--no-rrc", "--only-calculate", "--fp16-accumulate"};
    sp.alias = {{"-s", "--sections"}, {"-l", "--section-lines"}, {"-e", "--edge-cols"}, {"-r", "--rrc"}, {"-c", "--only-calculate"}};
    Parsed p = parse(sp, args);
    require(p, "--pan1");
    require(p, "--pan2");
    for (auto k : {"--pan1", "--pan2", "--rrc1", "--rrc2"}) existing_file(p, k);
    width = p.integer("--width", width);
    const int sections = p.integer("--sections", OIP_STT_DEF_SECTIONS);
    const int sectionLines = p.integer("--section-lines", OIP_STT_DEF_SECLINES);
    const int overlapCols = p.integer("--stitch-overlap", OIP_STT_DEF_OVERLAPPX);
    const int edgeCols = p.integer("--edge-cols", 0);
    if (edgeCols < 0 || edgeCols > overlapCols / 2) throw cli_error(105, "--edge-cols: invalid edge cols");      // main.cpp:135-141
    const double thr = p.real("--stt-threshold", OIP_STT_DEF_PHCTHRHLD), maxdy = p.real("--stt-maxdeltay", 0.0);
    const bool doRRC = !p.flag.count("--no-rrc");
    const bool onlyCalc = p.flag.count("--only-calculate") != 0;
    const int gpus = p.integer("--gpus", 1);
    if (gpus < 1 || gpus > 64) throw cli_error(105, "--gpus: GPU count expected");
    if (p.has("--gpus")) {                        // scan-line blocks over the GPUs of the node (oip_multigpu.hpp); --gpus 1 included
        MultiGpuPrestitchOptions mo;
        mo.width = width; mo.gpus = gpus; mo.sections = sections; mo.sectionLines = sectionLines; mo.overlapCols = overlapCols;
        mo.edgeCols = edgeCols; mo.threshold = thr; mo.maxDeltaY = maxdy; mo.doRRC = doRRC; mo.onlyCalc = onlyCalc;
        mo.fp16acc = p.flag.count("--fp16-accumulate") != 0;
        RunPrestitchMultiGpu(p.str("--pan1"), p.str("--pan2"), p.str("--rrc1"), p.str("--rrc2"), mo);
        return 0;
    }
    // main.cpp:270-286
    Stitcher stt(p.str("--pan1"), p.str("--pan2"), p.str("--rrc1"), p.str("--rrc2"), sections, sectionLines, overlapCols, width);
    stt.CalcSttParameters(thr, maxdy, edgeCols);
    if (!onlyCalc) {
        if (doRRC) stt.DoRRC();
        stt.PreStitch(p.flag.count("--fp16-accumulate") != 0);      // not in the reference: BASELINE config 5's resampling variant
    }
    stt.Finish();                                                   // the products' writer threads
    return 0;
}

// The seam options `stitch` and `task` share (not in the reference): --balance, --balance-lines, --valid-min, --valid-max,
// --min-count.  The blend width is per stitch (seam_feather).  Without any of them a stitch is the reference's hard cut.
const char *const kSeamValued[] = {"--balance", "--balance-lines", "--valid-min", "--valid-max", "--min-count"};

SeamOptions seam_options(const Parsed &p)
{
    SeamOptions seam;
    const std::string balance = p.str("--balance", "none");
    if (balance == "moments") seam.balance = OIP_SEAM_MOMENTS;
    else if (balance == "gain") seam.balance = OIP_SEAM_GAIN;
    else if (balance == "offset") seam.balance = OIP_SEAM_OFFSET;
    else if (balance != "none") throw cli_error(105, "--balance: none, offset, gain or moments expected");
    if (p.has("--balance-lines")) {
        seam.blockLines = p.integer("--balance-lines", 0);
        if (seam.blockLines < 1) throw cli_error(105, "--balance-lines: a line count of at least 1 expected");
        if (seam.balance < 0) throw cli_error(107, "--balance-lines requires --balance");
    }
    seam.validMin = p.integer("--valid-min", 1);
    seam.validMax = p.integer("--valid-max", 65535);
    if (seam.validMin < 0 || seam.validMax > 65535 || seam.validMin > seam.validMax) throw cli_error(105, "--valid-min/--valid-max: 0 <= min <= max <= 65535 expected");
    seam.minCount = p.integer("--min-count", 0);
    if (seam.minCount < 0) throw cli_error(105, "--min-count: a non-negative value expected");
    return seam;
}

// --feather / --feather-pan / --feather-mss: the blend width in columns, halved like the fold columns it is bounded by
int seam_feather(const Parsed &p, const std::string &key, int foldCols, const std::string &foldKey)
{
    const int feather = p.integer(key, 0);
    if (feather < 0 || feather % 2 != 0 || feather > foldCols) throw cli_error(105, key + ": an even value, 0 <= N <= " + foldKey + ", expected");
    return feather / 2;
}

// --levels N of `overviews` and `stitch --overviews`: 1..16; 0 without one (the default count, oip_overview_levels)
int overview_levels(const Parsed &p)
{
    if (!p.has("--levels")) return 0;
    const int n = p.integer("--levels", 0);
    if (n < 1 || n > 16) throw cli_error(105, "--levels: 1 <= N <= 16 expected");
    return n;
}

int run_stitch(const std::vector<std::string> &args, int width)
{
    Spec sp;
    sp.valued = {"--image1", "--image2", "--out", "--fold-cols", "--band-map", "--width", "--feather"};
    sp.valued.insert(std::begin(kSeamValued), std::end(kSeamValued));
    sp.valued.insert("--levels");
    sp.flags = {"--GDAL", "--overviews"};
    sp.alias = {{"-o", "--out"}, {"-c", "--fold-cols"}, {"-g", "--GDAL"}, {"-m", "--band-map"}};
    Parsed p = parse(sp, args);
    require(p, "--image1");
    require(p, "--image2");
    require(p, "--fold-cols");
    width = p.integer("--width", width);
    const int foldCols = p.integer("--fold-cols", 0);
    if (foldCols < 2) throw cli_error(105, "--fold-cols: fold column value too small");                           // main.cpp:166-170
    if (p.has("--band-map") && !p.has("--GDAL")) throw cli_error(107, "--band-map requires --GDAL");              // ->needs(gdal)
    int map[MSS_BANDS] = {0, 0, 0, 0};
    const std::string bandMap = p.str("--band-map");
    if (!bandMap.empty()) {                                                                                      // main.cpp:177-188
        if (sscanf(bandMap.c_str(), "%d,%d,%d,%d", map, map + 1, map + 2, map + 3) != 4) throw cli_error(105, "-m: need 4 band indices");
        for (int i = 0; i < MSS_BANDS; ++i)
            if (map[i] <= 0 || map[i] > MSS_BANDS) throw cli_error(105, "-m: invalid band index");
    }
    SeamOptions seam = seam_options(p);
    seam.feather = seam_feather(p, "--feather", foldCols, "fold-cols");
    // --overviews [--levels N] (not in the reference): the product's pyramid beside it, with the seam options' --valid-min
    if (p.has("--levels") && !p.has("--overviews")) throw cli_error(107, "--levels requires --overviews");
    OverviewOptions ovr;
    ovr.levels = overview_levels(p);
    ovr.validMin = seam.validMin;
    Stitcher::Stitch(p.str("--image1"), p.str("--image2"), p.str("--out"), foldCols / 2, width, p.has("--GDAL"),
                     bandMap.empty() ? nullptr : map, &seam, p.has("--overviews") ? &ovr : nullptr);             // main.cpp:189
    return 0;
}

int run_default(const std::vector<std::string> &args, int width)
{
    Spec sp;
    sp.valued = {"--pan", "--mss", "--rrc-pan", "--rrc-msb1", "--rrc-msb2", "--rrc-msb3", "--rrc-msb4", "--slices", "--ibc-sections",
                 "--ibc-threshold", "--line-offset", "--lines-section", "--overlap-lines", "--width", "--fit", "--gpus"};
    sp.flags = {"--do-rrc4pan", "--write-rrcpan", "--no-rrcpan", "--no-rrc4mss", "--keep-leading"};
    sp.alias = {{"-k", "--keep-leading"}};
    Parsed p = parse(sp, args);
    for (auto k : {"--pan", "--mss", "--rrc-msb1", "--rrc-msb2", "--rrc-msb3", "--rrc-msb4"}) existing_file(p, k);
    width = p.integer("--width", width);
    const double thr = p.real("--ibc-threshold", OIP_IBCV_DEF_THRESHOLD);
    if (thr < 0.0 || thr >= 1.0) throw cli_error(105, "--ibc-threshold: invalid threshold value");               // main.cpp:233-239
    if ((p.has("--rrc-pan") || p.has("--write-rrcpan") || p.has("--no-rrcpan")) && !p.has("--do-rrc4pan"))
        throw cli_error(107, "--rrc-pan requires --do-rrc4pan");                                                  // ->needs(rrc4pan)
    const bool doRRC4PAN = p.flag.count("--do-rrc4pan") != 0;
    const bool doRRC4MSS = !p.flag.count("--no-rrc4mss");
    // main.cpp:288-299
    if (doRRC4PAN && p.str("--rrc-pan").empty()) throw usage_error("RRC parameter file of PAN needed");
    std::string msb[MSS_BANDS] = {p.str("--rrc-msb1"), p.str("--rrc-msb2"), p.str("--rrc-msb3"), p.str("--rrc-msb4")};
    if (doRRC4MSS && (msb[0].empty() || msb[1].empty() || msb[2].empty() || msb[3].empty()))
        throw usage_error("RRC parameter file of all MSS Bands needed");
    if (p.has("--gpus")) {                        // scan-line blocks over the GPUs of the node (oip_multigpu.hpp); --gpus 1 included
        MultiGpuDefaultOptions mo;
        mo.width = width; mo.gpus = p.integer("--gpus", 1);
        if (mo.gpus < 1 || mo.gpus > 64) throw cli_error(105, "--gpus: GPU count expected");
        if (p.flag.count("--write-rrcpan")) throw cli_error(105, "--write-rrcpan is not available with --gpus");
        require(p, "--pan");
        require(p, "--mss");
        mo.doRRC4PAN = doRRC4PAN; mo.doRRC4MSS = doRRC4MSS; mo.keepLeading = p.flag.count("--keep-leading") != 0;
        mo.slices = p.integer("--slices", OIP_IBCV_DEF_SLICES); mo.sections = p.integer("--ibc-sections", OIP_IBCV_DEF_SECTIONS);
        mo.linesSection = p.integer("--lines-section", OIP_IBPA_DEFAULT_BATCHLINES); mo.lineOffset = p.integer("--line-offset", 0);
        mo.overlapLines = p.integer("--overlap-lines", OIP_IBPA_DEFAULT_LINEOVERLAP); mo.fitMode = fit_mode(p); mo.threshold = thr;
        RunDefaultActionMultiGpu(p.str("--pan"), p.str("--mss"), p.str("--rrc-pan"), msb, mo);
        return 0;
    }
    // main.cpp:301-316
    PreProcessor pp(p.str("--pan"), p.str("--mss"), p.str("--rrc-pan"), msb, width);
    pp.SetFitMode(fit_mode(p));
    const char *pl = getenv("OIP_PIPELINE");
    if (!(pl && atoi(pl) == 0)) {
        // the same steps as one pipeline: read || RRC || correlation || product writes (PreProcessor::RunPipelined);
        // OIP_PIPELINE=0 runs them one after the other as the reference does -- the products are the same bytes
        PreProcessor::DefaultActionOptions o;
        o.doRRC4PAN = doRRC4PAN; o.writeRrcPan = doRRC4PAN && p.flag.count("--write-rrcpan") != 0; o.doRRC4MSS = doRRC4MSS;
        o.keepLeading = p.flag.count("--keep-leading") != 0;
        o.slices = p.integer("--slices", OIP_IBCV_DEF_SLICES); o.sections = p.integer("--ibc-sections", OIP_IBCV_DEF_SECTIONS); o.threshold = thr;
        o.linesSection = p.integer("--lines-section", OIP_IBPA_DEFAULT_BATCHLINES); o.lineOffset = p.integer("--line-offset", 0);
        o.overlapLines = p.integer("--overlap-lines", OIP_IBPA_DEFAULT_LINEOVERLAP);
        pp.RunPipelined(o);
        return 0;
    }
    pp.LoadPAN();
    pp.LoadMSS();
    if (doRRC4PAN) {
        pp.DoRRC4PAN();
        if (p.flag.count("--write-rrcpan")) pp.WriteRRCedPAN();      // RAW instead of the reference's TIFF
    }
    pp.DoRRC4MSS(doRRC4MSS);
    pp.CalcInterBandCorrelation(p.integer("--slices", OIP_IBCV_DEF_SLICES), p.integer("--ibc-sections", OIP_IBCV_DEF_SECTIONS), thr);
    pp.DoInterBandAlignment(p.integer("--lines-section", OIP_IBPA_DEFAULT_BATCHLINES), p.integer("--line-offset", 0),
                            p.integer("--overlap-lines", OIP_IBPA_DEFAULT_LINEOVERLAP), p.flag.count("--keep-leading") != 0);
    return 0;
}

// oip plan strip|ccd ...: prints the multi-GPU row plan as JSON (no device is touched) -- what each rank computes,
// which window pieces and halo lines move.  tests/test_cli_cpu.py compares it with dist.py's plan.
int run_plan(const std::vector<std::string> &args)
{
    if (args.empty() || (args[0] != "strip" && args[0] != "ccd")) throw cli_error(105, "plan: strip or ccd expected");
    Spec sp;
    sp.valued = {"--width", "--lines", "--gpus", "--slices", "--ibc-sections", "--corr-lines", "--lines-section", "--line-offset", "--overlap-lines",
                 "--min-lines", "--halo-cap", "--cy", "--sections", "--section-lines", "--stitch-overlap", "--edge-cols", "--dy", "--section-rows"};
    sp.flags = {"--keep-leading"};
    Parsed p = parse(sp, {args.begin() + 1, args.end()});
    const int W = p.integer("--width", OIP_PIXELS_PER_LINE), gpus = p.integer("--gpus", 1);
    const long L = (long)p.real("--lines", 0);
    if (args[0] == "strip") {
        StripPlanC plan(W, L, gpus, p.integer("--slices", OIP_IBCV_DEF_SLICES), p.integer("--ibc-sections", OIP_IBCV_DEF_SECTIONS),
                        p.integer("--corr-lines", OIP_CORRELATION_LINES), p.integer("--lines-section", OIP_IBPA_DEFAULT_BATCHLINES),
                        p.integer("--line-offset", 0), p.integer("--overlap-lines", OIP_IBPA_DEFAULT_LINEOVERLAP), p.flag.count("--keep-leading") != 0,
                        p.integer("--min-lines", OIP_IBPA_MIN_PROCESSLINES), p.integer("--halo-cap", 64));
        double cy[12] = {0};
        const std::string c = p.str("--cy", "0,0,0");
        double a = 0, b = 0, d = 0;
        if (sscanf(c.c_str(), "%lf,%lf,%lf", &a, &b, &d) != 3) throw cli_error(105, "--cy: three coefficients expected");
        for (int k = 0; k < 4; ++k) { cy[3 * k] = a; cy[3 * k + 1] = b; cy[3 * k + 2] = d; }
        PrintStripPlan(plan, cy);
    } else {
        CcdPlanC plan(W, L, gpus, p.integer("--sections", OIP_STT_DEF_SECTIONS), p.integer("--section-lines", OIP_STT_DEF_SECLINES),
                      p.integer("--stitch-overlap", OIP_STT_DEF_OVERLAPPX), p.integer("--edge-cols", 0),
                      p.integer("--section-rows", OIP_REMAP_SECTION_ROWS));
        PrintCcdPlan(plan, p.real("--dy", 0.0));
    }
    return 0;
}

// oip task: DOC/sample-task.sh's five commands in one process, intermediates resident on the GPU
int run_task(const std::vector<std::string> &args, int width)
{
    Spec sp;
    sp.valued = {"--pan1", "--pan2", "--rrc1", "--rrc2", "--mss1", "--mss2", "--out-pan", "--out-mss", "--fold-cols-pan", "--fold-cols-mss",
                 "--sections", "--section-lines", "--stitch-overlap", "--stt-threshold", "--stt-maxdeltay", "--edge-cols", "--band-map",
                 "--slices", "--ibc-sections", "--ibc-threshold", "--line-offset", "--lines-section", "--overlap-lines", "--width", "--fit",
                 "--feather-pan", "--feather-mss"};
    sp.valued.insert(std::begin(kSeamValued), std::end(kSeamValued));
    for (int c = 1; c <= 2; ++c)
        for (int b = 1; b <= MSS_BANDS; ++b) sp.valued.insert("--rrc-mss" + std::to_string(c) + "-b" + std::to_string(b));
    sp.flags = {"--GDAL", "--keep-leading", "--fp16-accumulate", "--pan-only"};
    sp.alias = {{"-s", "--sections"}, {"-l", "--section-lines"}, {"-e", "--edge-cols"}, {"-g", "--GDAL"}, {"-m", "--band-map"}, {"-k", "--keep-leading"}};
    Parsed p = parse(sp, args);
    std::string msb[2][MSS_BANDS];
    // --pan-only: the stitched PAN product alone (steps 1-2 of DOC/sample-task.sh).  No corrected strip is needed afterwards,
    // so RRC of CCD 1 and the resampled CCD-2 lines are written straight into the stitched raster (one pass each).
    const bool panOnly = p.flag.count("--pan-only") != 0;
    // The seam options of the two stitches.  In the --pan-only flow the resampling kernel writes the right half of the product
    // itself and has no (G, O) to apply on store, so any of them is refused there -- here, before a file or the device is touched.
    if (panOnly) {
        for (auto k : kSeamValued)
            if (p.has(k)) throw cli_error(107, std::string(k) + " is not available with --pan-only");
        for (auto k : {"--feather-pan", "--feather-mss"})
            if (p.has(k)) throw cli_error(107, std::string(k) + " is not available with --pan-only");
    }
    const SeamOptions seam = seam_options(p);
    // (a missing --fold-cols-* is reported below, as before)
    const int featherPAN = seam_feather(p, "--feather-pan", p.integer("--fold-cols-pan", INT_MAX), "fold-cols-pan");
    const int featherMSS = seam_feather(p, "--feather-mss", p.integer("--fold-cols-mss", INT_MAX), "fold-cols-mss");
    for (auto k : {"--pan1", "--pan2", "--rrc1", "--rrc2", "--out-pan", "--fold-cols-pan"}) require(p, k);
    if (!panOnly)
        for (auto k : {"--mss1", "--mss2", "--out-mss", "--fold-cols-mss"}) require(p, k);
    for (int c = 0; c < 2 && !panOnly; ++c)
        for (int b = 0; b < MSS_BANDS; ++b) {
            const std::string k = "--rrc-mss" + std::to_string(c + 1) + "-b" + std::to_string(b + 1);
            require(p, k);
            existing_file(p, k);
            msb[c][b] = p.str(k);
        }
    for (auto k : {"--pan1", "--pan2", "--rrc1", "--rrc2", "--mss1", "--mss2"}) existing_file(p, k);
    TaskOptions o;
    o.width = p.integer("--width", width);
    o.sections = p.integer("--sections", o.sections);
    o.sectionLines = p.integer("--section-lines", o.sectionLines);
    o.overlapCols = p.integer("--stitch-overlap", o.overlapCols);
    o.edgeCols = p.integer("--edge-cols", 0);
    if (o.edgeCols < 0 || o.edgeCols > o.overlapCols / 2) throw cli_error(105, "--edge-cols: invalid edge cols");
    o.sttThreshold = p.real("--stt-threshold", o.sttThreshold);
    o.sttMaxDeltaY = p.real("--stt-maxdeltay", 0.0);
    o.foldColsPAN = p.integer("--fold-cols-pan", 0);
    o.foldColsMSS = p.integer("--fold-cols-mss", panOnly ? 2 : 0);
    o.panOnly = panOnly;
    if (o.foldColsPAN < 2 || o.foldColsMSS < 2) throw cli_error(105, "--fold-cols: fold column value too small");
    o.useGDAL = p.has("--GDAL");
    if (p.has("--band-map") && !o.useGDAL) throw cli_error(107, "--band-map requires --GDAL");
    int map[MSS_BANDS] = {0, 0, 0, 0};
    const std::string bandMap = p.str("--band-map");
    if (!bandMap.empty()) {
        if (sscanf(bandMap.c_str(), "%d,%d,%d,%d", map, map + 1, map + 2, map + 3) != 4) throw cli_error(105, "-m: need 4 band indices");
        for (int i = 0; i < MSS_BANDS; ++i)
            if (map[i] <= 0 || map[i] > MSS_BANDS) throw cli_error(105, "-m: invalid band index");
        o.bandMap = map;
    }
    o.slices = p.integer("--slices", o.slices);
    o.ibcSections = p.integer("--ibc-sections", o.ibcSections);
    o.ibcThreshold = p.real("--ibc-threshold", o.ibcThreshold);
    if (o.ibcThreshold < 0.0 || o.ibcThreshold >= 1.0) throw cli_error(105, "--ibc-threshold: invalid threshold value");
    o.linesSection = p.integer("--lines-section", o.linesSection);
    o.lineOffset = p.integer("--line-offset", 0);
    o.overlapLines = p.integer("--overlap-lines", o.overlapLines);
    o.keepLeading = p.flag.count("--keep-leading") != 0;
    o.fitMode = fit_mode(p);
    o.fp16acc = p.flag.count("--fp16-accumulate") != 0;
    o.seamPAN = o.seamMSS = seam;
    o.seamPAN.feather = featherPAN;
    o.seamMSS.feather = featherMSS;
    for (auto k : {"--out-pan", "--out-mss"})
        if (p.has(k) && to_lower(std::filesystem::path(p.str(k)).extension().string()) != ".tiff") throw std::invalid_argument("Output file should be a tiff image");
    RunFusedTask(p.str("--pan1"), p.str("--pan2"), p.str("--rrc1"), p.str("--rrc2"), p.str("--mss1"), p.str("--mss2"), msb[0], msb[1],
                 p.str("--out-pan"), p.str("--out-mss"), o);
    return 0;
}

// oip rrc-calib: the "k , b" files that prestitch (--rrc1/--rrc2), the default action (--rrc-pan, --rrc-msb1..4) and task
// read, derived from a strip.  The option names are the default action's on purpose -- here the --rrc-* values are outputs.
int run_rrc_calib(const std::vector<std::string> &args, int width)
{
    Spec sp;
    sp.valued = {"--pan", "--mss", "--rrc-pan", "--rrc-msb1", "--rrc-msb2", "--rrc-msb3", "--rrc-msb4", "--width", "--mode", "--valid-min",
                 "--valid-max", "--min-count", "--line-offset", "--lines", "--bad-pan", "--bad-mss"};
    sp.flags = {"--force"};
    Parsed p = parse(sp, args);
    if (p.has("--bad-pan") && !p.has("--pan")) throw cli_error(107, "--bad-pan requires --pan");             // a list comes with its image
    if (p.has("--bad-mss") && !p.has("--mss")) throw cli_error(107, "--bad-mss requires --mss");
    const char *msbKeys[MSS_BANDS] = {"--rrc-msb1", "--rrc-msb2", "--rrc-msb3", "--rrc-msb4"};
    bool anyMsb = false;
    for (auto k : msbKeys) anyMsb = anyMsb || p.has(k);
    if (!p.has("--pan") && !p.has("--mss") && !p.has("--rrc-pan") && !anyMsb) throw cli_error(106, "--pan or --mss is required");
    if (p.has("--pan") || p.has("--rrc-pan")) { require(p, "--pan"); require(p, "--rrc-pan"); }    // an image and its outputs come together
    if (p.has("--mss") || anyMsb) {
        require(p, "--mss");
        for (auto k : msbKeys) require(p, k);
    }
    for (auto k : {"--pan", "--mss"}) existing_file(p, k);
    RrcCalibOptions o;
    o.width = p.integer("--width", width);
    const std::string mode = p.str("--mode", "moments");
    if (mode == "moments") o.mode = OIP_RRCFIT_MOMENTS;
    else if (mode == "gain") o.mode = OIP_RRCFIT_GAIN;
    else throw cli_error(105, "--mode: moments or gain expected");
    p.valid_range(0, &o.validMin, &o.validMax);
    o.minCount = p.integer("--min-count", 0);
    p.line_range(&o.lineOffset, &o.lines, "--min-count, ", o.minCount);
    o.force = p.has("--force");
    o.badPan = p.str("--bad-pan");
    o.badMss = p.str("--bad-mss");
    if ((p.has("--bad-pan") && o.badPan.empty()) || (p.has("--bad-mss") && o.badMss.empty())) throw cli_error(105, "--bad-pan, --bad-mss: a file name expected");
    const std::string msb[MSS_BANDS] = {p.str(msbKeys[0]), p.str(msbKeys[1]), p.str(msbKeys[2]), p.str(msbKeys[3])};
    RunRrcCalib(p.str("--pan"), p.str("--mss"), p.str("--rrc-pan"), msb, o);
    return 0;
}

// oip quicklook IMAGE: the browse image of a strip (.RAW, with --bil the MSS line layout) or a product (.TIFF of 1 or 4
// samples), an uncompressed TIFF or with --format jpeg a baseline JPEG.  IMAGE is the one positional argument of the tool.
int run_quicklook(const std::vector<std::string> &args, int width)
{
    Spec sp;
    sp.valued = {"--out", "--factor", "--clip-low", "--clip-high", "--valid-min", "--valid-max", "--bands", "--width", "--line-offset", "--lines", "--format",
                 "--quality"};
    sp.flags = {"--bil", "--force"};
    sp.alias = {{"-o", "--out"}};
    std::string image;
    Parsed p = parse_with_image(sp, args, &image);
    QuicklookOptions o;
    const std::string format = p.str("--format", "tiff");
    if (format != "tiff" && format != "jpeg") throw cli_error(105, "--format: tiff or jpeg expected");
    o.jpeg = format == "jpeg";
    if (p.has("--quality") && !o.jpeg) throw cli_error(107, "--quality requires --format jpeg");
    o.quality = p.integer("--quality", OIP_JPEG_DEF_QUALITY);
    if (o.quality < 1 || o.quality > 100) throw cli_error(105, "--quality: 1 <= Q <= 100 expected");
    o.width = p.integer("--width", width);
    o.bil = p.has("--bil");
    o.factor = p.integer("--factor", OIP_QUICKLOOK_DEF_FACTOR);
    o.clipLow = p.real("--clip-low", OIP_QUICKLOOK_DEF_CLIPLOW);
    o.clipHigh = p.real("--clip-high", OIP_QUICKLOOK_DEF_CLIPHIGH);
    if (!(o.clipLow >= 0.0 && o.clipLow <= o.clipHigh && o.clipHigh <= 100.0)) throw cli_error(105, "--clip-low/--clip-high: 0 <= low <= high <= 100 expected");
    p.valid_range(1, &o.validMin, &o.validMax);
    p.line_range(&o.lineOffset, &o.lines);
    o.force = p.has("--force");
    if (p.has("--bands")) {
        const std::string b = p.str("--bands");
        int v[4] = {0, 0, 0, 0};
        char junk = 0;
        const int n = sscanf(b.c_str(), "%d,%d,%d%c", v, v + 1, v + 2, &junk);
        const bool one = n == 1 && b.find(',') == std::string::npos;
        if (!one && n != 3) throw usage_error("--bands: one band index (grey) or three (RGB) expected");
        o.bands.assign(v, v + (one ? 1 : 3));
    }
    RunQuicklook(image, p.str("--out"), o);
    return 0;
}

// oip mtfc IMAGE: the MTF-compensation filter of a strip (.RAW, --width samples per line) or a product (.TIFF of 1 or 4
// samples).  IMAGE is the one positional argument, as for quicklook.
int run_mtfc(const std::vector<std::string> &args, int width)
{
    Spec sp;
    sp.valued = {"--out", "--kernel", "--mtf-x", "--mtf-y", "--max-gain", "--valid-min", "--width", "--mtf", "--mtf-stat"};
    sp.flags = {"--force"};
    sp.alias = {{"-o", "--out"}};
    std::string image;
    Parsed p = parse_with_image(sp, args, &image);
    // --mtf REPORT stands in for --mtf-x / --mtf-y: the two numbers come from the report of `oip mtf`
    if (p.has("--mtf") && (p.has("--kernel") || p.has("--mtf-x") || p.has("--mtf-y"))) throw cli_error(107, "--mtf excludes --kernel and --mtf-x/--mtf-y");
    if (p.has("--mtf-stat") && !p.has("--mtf")) throw cli_error(107, "--mtf-stat requires --mtf");
    const std::string stat = p.str("--mtf-stat", "median");
    if (stat != "median" && stat != "p75" && stat != "p90") throw cli_error(105, "--mtf-stat: median, p75 or p90 expected");
    const bool design = p.has("--mtf-x") || p.has("--mtf-y") || p.has("--max-gain") || p.has("--mtf");
    if (p.has("--kernel") && design) throw usage_error("--kernel and --mtf-x/--mtf-y/--max-gain exclude each other");
    if (!p.has("--kernel") && !design) throw usage_error("--kernel FILE or --mtf-x M --mtf-y M expected");
    MtfcOptions o;
    o.width = p.integer("--width", width);
    if (design) {
        if (p.has("--mtf")) {
            existing_file(p, "--mtf");
            MtfAxisSummary s[2];
            std::string err;
            if (!ParseMtfReport(p.str("--mtf"), s, &err)) throw std::runtime_error(err);
            if (!MtfcValueOf(s[0], 0, stat, &o.mtfX, &err) || !MtfcValueOf(s[1], 1, stat, &o.mtfY, &err))
                throw cli_error(105, "--mtf: MTF report [" + p.str("--mtf") + "]: " + err);
            OLOG("mtfc: %s of the MTF report [%s]: mtf-x %.17g, mtf-y %.17g", stat.c_str(), p.str("--mtf").c_str(), o.mtfX, o.mtfY);
        } else {
            require(p, "--mtf-x");
            require(p, "--mtf-y");
            o.mtfX = p.real("--mtf-x", 0.0);
            o.mtfY = p.real("--mtf-y", 0.0);
        }
        o.maxGain = p.real("--max-gain", OIP_MTFC_DEF_MAXGAIN);
        if (!(o.mtfX > 0.0 && o.mtfX <= 1.0) || !(o.mtfY > 0.0 && o.mtfY <= 1.0)) throw cli_error(105, "--mtf-x/--mtf-y: 0 < M <= 1 expected");
        if (!(o.maxGain >= 1.0)) throw cli_error(105, "--max-gain: G >= 1 expected");
    } else {
        existing_file(p, "--kernel");
        o.kernelFile = p.str("--kernel");
    }
    o.validMin = p.valid_min();
    o.force = p.has("--force");
    RunMtfc(image, p.str("--out"), o);
    return 0;
}

// oip despike IMAGE: column repair and the conditional 3 x 3 median of a strip (.RAW, --width samples per line, with --bil the
// MSS line layout) or a product (.TIFF of 1 or 4 samples).  IMAGE is the one positional argument, as for mtfc.
int run_despike(const std::vector<std::string> &args, int width)
{
    Spec sp;
    sp.valued = {"--out", "--threshold", "--relative", "--bad-columns", "--valid-min", "--width", "--report", "--noise", "--k-sigma"};
    sp.flags = {"--bil", "--force"};
    sp.alias = {{"-o", "--out"}};
    std::string image;
    Parsed p = parse_with_image(sp, args, &image);
    // there is no default threshold: it is given, or follows from the noise `oip noise` measured (--noise), and without one only
    // the listed columns are repaired
    if (p.has("--noise") && (p.has("--threshold") || p.has("--relative"))) throw cli_error(107, "--noise excludes --threshold and --relative");
    if (p.has("--k-sigma") && !p.has("--noise")) throw cli_error(107, "--k-sigma requires --noise");
    if (!p.has("--threshold") && !p.has("--noise") && !p.has("--bad-columns")) throw usage_error("--threshold N, --noise REPORT or --bad-columns FILE expected");
    if (p.has("--relative") && !p.has("--threshold")) throw cli_error(107, "--relative requires --threshold");
    DespikeOptions o;
    o.width = p.integer("--width", width);
    o.bil = p.has("--bil");
    o.hasThreshold = p.has("--threshold");
    o.thrAbs = p.within("--threshold", 65535, 0, 65535, "0 <= N <= 65535 expected");
    const double rel = p.real("--relative", 0.0);
    if (!(rel >= 0.0 && rel <= 1.0)) throw cli_error(105, "--relative: 0 <= R <= 1 expected");
    o.thrRelQ8 = (int)std::rint(rel * 256.0);
    o.validMin = p.valid_min();
    existing_file(p, "--bad-columns");
    o.badColumns = p.str("--bad-columns");
    if (p.has("--bad-columns") && o.badColumns.empty()) throw cli_error(105, "--bad-columns: a file name expected");
    o.report = p.str("--report");
    o.force = p.has("--force");
    existing_file(p, "--noise");
    // --k-sigma 5 is the usual convention for an impulse, nothing measured
    const double kSigma = p.real("--k-sigma", 5.0);
    if (!(kSigma >= 1.0 && kSigma <= 100.0)) throw cli_error(105, "--k-sigma: 1 <= K <= 100 expected");
    if (p.has("--noise")) DespikeNoiseThreshold(p.str("--noise"), kSigma, &o);
    RunDespike(image, p.str("--out"), o);
    return 0;
}

// oip denoise IMAGE: the sigma filter of a strip (.RAW, --width samples per line) or a product (.TIFF of 1 or 4 samples), its
// thresholds from the report of `oip noise` on the same file (--noise) or from one --sigma (RunDenoise).  IMAGE is the one
// positional argument, as for mtfc.  Bad values end in 105 before any file is read.
int run_denoise(const std::vector<std::string> &args, int width)
{
    Spec sp;
    sp.valued = {"--out", "--noise", "--sigma", "--k-sigma", "--radius", "--min-members", "--valid-min", "--width"};
    sp.flags = {"--force"};
    sp.alias = {{"-o", "--out"}};
    std::string image;
    Parsed p = parse_with_image(sp, args, &image);
    if (p.has("--noise") && p.has("--sigma")) throw usage_error("--noise and --sigma exclude each other");
    if (!p.has("--noise") && !p.has("--sigma")) throw usage_error("--noise REPORT or --sigma S expected");
    DenoiseOptions o;
    o.width = p.integer("--width", width);
    o.radius = p.within("--radius", 2, 1, 3, "1, 2 or 3 expected");
    const int side = 2 * o.radius + 1;
    o.minMembers = p.within("--min-members", side, 1, side * side, "1 <= M <= (2 * radius + 1)^2 expected");
    o.validMin = p.valid_min();
    // --k-sigma 2 is Lee's choice (95 % of a Gaussian): a wider range keeps more of an edge's other side
    o.kSigma = p.real("--k-sigma", 2.0);
    if (!(o.kSigma > 0.0 && o.kSigma <= 100.0)) throw cli_error(105, "--k-sigma: 0 < K <= 100 expected");
    if (p.has("--sigma")) {
        o.sigma = p.real("--sigma", 0.0);
        if (!(o.sigma > 0.0) || !std::isfinite(o.sigma)) throw cli_error(105, "--sigma: a finite S > 0 expected");
    }
    existing_file(p, "--noise");
    o.noiseReport = p.str("--noise");
    if (p.has("--noise") && o.noiseReport.empty()) throw cli_error(105, "--noise: a file name expected");
    o.force = p.has("--force");
    RunDenoise(image, p.str("--out"), o);
    return 0;
}

// oip noise IMAGE: the noise-level function of a strip (.RAW, --width samples per line, with --bil the MSS line layout) or a
// product (.TIFF of 1 or 4 samples) as <stem>.NOISE.CSV (RunNoise).  IMAGE is the one positional argument, as for mtfc.  Bad
// values end in 105 before any file is read.
int run_noise(const std::vector<std::string> &args, int width)
{
    Spec sp;
    sp.valued = {"--out", "--block", "--bits", "--valid-min", "--valid-max", "--min-blocks", "--width", "--line-offset", "--lines"};
    sp.flags = {"--bil", "--force"};
    sp.alias = {{"-o", "--out"}};
    std::string image;
    Parsed p = parse_with_image(sp, args, &image);
    NoiseOptions o;
    o.width = p.integer("--width", width);
    o.bil = p.has("--bil");
    o.block = p.integer("--block", 8);
    if (o.block != 8 && o.block != 16) throw cli_error(105, "--block: 8 or 16 expected");
    o.bits = p.within("--bits", 12, 8, 16, "8 <= N <= 16 expected");
    p.valid_range(1, &o.validMin, &o.validMax);
    o.minBlocks = p.within("--min-blocks", 100, 0, INT_MAX, "N >= 0 expected");
    p.line_range(&o.lineOffset, &o.lines);
    if (o.lineOffset % o.block != 0) throw cli_error(105, "--line-offset: a multiple of --block expected");
    o.force = p.has("--force");
    char buf[256];
    snprintf(buf, sizeof buf, " block=%d bits=%d valid-min=%d valid-max=%d min-blocks=%ld bil=%d line-offset=%ld lines=%ld", o.block, o.bits, o.validMin,
             o.validMax, o.minBlocks, o.bil ? 1 : 0, o.lineOffset, o.lines);
    o.params = "oip noise image=" + image + buf + " columns=band,level_lo,level_hi,blocks,sigma,snr";
    RunNoise(image, p.str("--out"), o);
    return 0;
}

// oip mask IMAGE: the no-data / saturation / cloud mask of a strip (.RAW, --width samples per line) or a product (.TIFF of 1 or 4
// samples) as <stem>.MASK.TIFF and <stem>.MASK.CSV (RunMask).  IMAGE is the one positional argument, as for mtfc.  Bad values
// end in 105 before any file is read.
int run_mask(const std::vector<std::string> &args, int width)
{
    Spec sp;
    sp.valued = {"--out", "--report", "--cell", "--bits", "--saturation", "--valid-min", "--bands", "--bright", "--white", "--hot", "--ndvi",
                 "--open", "--buffer", "--width"};
    sp.flags = {"--no-cloud", "--force"};
    sp.alias = {{"-o", "--out"}};
    std::string image;
    Parsed p = parse_with_image(sp, args, &image);
    MaskOptions o;
    o.width = p.positive_width(width);
    o.cell = p.integer("--cell", 8);
    if (o.cell != 4 && o.cell != 8 && o.cell != 16) throw cli_error(105, "--cell: 4, 8 or 16 expected");
    o.bits = p.within("--bits", 12, 8, 16, "8 <= N <= 16 expected");
    const int full = (1 << o.bits) - 1;
    o.saturation = p.within("--saturation", full, 1, 65535, "1 <= DN <= 65535 expected");
    o.validMin = p.valid_min();
    const std::string bands = p.str("--bands", "3,2,1,4");
    {
        int v[4] = {0, 0, 0, 0}, seen = 0;
        char junk = 0;
        const bool four = sscanf(bands.c_str(), "%d,%d,%d,%d%c", v, v + 1, v + 2, v + 3, &junk) == 4;
        for (int k = 0; k < 4 && four; ++k)
            if (v[k] >= 1 && v[k] <= 4) seen |= 1 << (v[k] - 1);
        if (!four || seen != 15) throw cli_error(105, "--bands: B,G,R,N, a permutation of the channels 1,2,3,4, expected");
        for (int k = 0; k < 4; ++k) o.band[k] = v[k] - 1;
    }
    const char *keys[4] = {"--bright", "--white", "--hot", "--ndvi"};
    const double defs[4] = {0.30, 0.15, 0.08, 0.20};
    for (int k = 0; k < 4; ++k) {
        const double F = p.real(keys[k], defs[k]);
        if (!(F >= 0.0 && F <= 1.0)) throw cli_error(105, std::string(keys[k]) + ": a fraction 0 <= F <= 1 expected");
        o.q8[k] = MaskQ8(F);
    }
    o.noCloud = p.has("--no-cloud");
    o.open = p.within("--open", 1, 0, 32, "0 <= A <= 32 expected");
    o.buffer = p.within("--buffer", 2, 0, 64, "0 <= D <= 64 expected");
    o.force = p.has("--force");
    o.report = p.str("--report");
    if ((p.has("--report") && o.report.empty()) || (p.has("--out") && p.str("--out").empty())) throw cli_error(105, "--out, --report: a file name expected");
    RunMask(image, p.str("--out"), o);
    return 0;
}

// oip wallis IMAGE: the Wallis filter on a strip (.RAW, --width samples per line) or a product (.TIFF of 1 or 4 samples), as
// <stem>.WAL.<ext> and <stem>.WAL.CSV (RunWallis).  IMAGE is the one positional argument, as for mtfc.  Bad values end in 105
// before any file is read.
int run_wallis(const std::vector<std::string> &args, int width)
{
    Spec sp;
    sp.valued = {"--out", "--report", "--block", "--contrast", "--brightness", "--mean", "--std", "--min-gain", "--max-gain", "--min-count",
                 "--valid-min", "--valid-max", "--max-value", "--width", "--line-offset", "--lines"};
    sp.flags = {"--force"};
    sp.alias = {{"-o", "--out"}};
    std::string image;
    Parsed p = parse_with_image(sp, args, &image);
    WallisOptions o;
    o.width = p.positive_width(width);
    o.block = p.integer("--block", 128);
    if (o.block != 32 && o.block != 64 && o.block != 128 && o.block != 256) throw cli_error(105, "--block: 32, 64, 128 or 256 expected");
    o.contrast = p.real("--contrast", 0.8);
    if (!(o.contrast > 0.0 && o.contrast <= 1.0)) throw cli_error(105, "--contrast: 0 < C <= 1 expected");
    o.brightness = p.real("--brightness", 0.6);
    if (!(o.brightness >= 0.0 && o.brightness <= 1.0)) throw cli_error(105, "--brightness: 0 <= B <= 1 expected");
    o.gMin = p.real("--min-gain", 0.25);
    o.gMax = p.real("--max-gain", 4.0);
    if (!(o.gMin > 0.0 && o.gMin <= 1.0 && o.gMax >= 1.0 && o.gMax <= 16.0)) throw cli_error(105, "--min-gain/--max-gain: 0 < min <= 1 <= max <= 16 expected");
    p.valid_range(1, &o.validMin, &o.validMax);
    o.maxValue = p.integer("--max-value", 65535);
    if (o.maxValue < o.validMin || o.maxValue > 65535) throw cli_error(105, "--max-value: --valid-min <= DN <= 65535 expected");
    o.minCount = p.integer("--min-count", 0);
    p.line_range(&o.lineOffset, &o.lines, "--min-count, ", o.minCount);
    // --mean / --std: one value for every channel or one per channel; a mean in 0..65535, a std in (0, 65535]
    auto targets = [&](const char *key, bool positive, std::vector<double> *out) {
        if (!p.has(key)) return;
        const std::string s = p.str(key);
        size_t at = 0;
        while (at <= s.size()) {
            const size_t comma = std::min(s.find(',', at), s.size());
            const std::string item = s.substr(at, comma - at);
            char *e = nullptr;
            const double v = strtod(item.c_str(), &e);
            if (item.empty() || !e || *e || !(v >= 0.0 && v <= 65535.0) || (positive && !(v > 0.0)))
                throw cli_error(105, std::string(key) + (positive ? ": 0 < S <= 65535 expected, one value or one per channel" : ": 0 <= M <= 65535 expected, one value or one per channel"));
            out->push_back(v);
            at = comma + 1;
        }
        if (out->size() != 1 && out->size() != 4) throw cli_error(105, std::string(key) + ": one value, or four (one per channel) expected");
    };
    targets("--mean", false, &o.mean);
    targets("--std", true, &o.std);
    o.force = p.has("--force");
    o.report = p.str("--report");
    if ((p.has("--report") && o.report.empty()) || (p.has("--out") && p.str("--out").empty())) throw cli_error(105, "--out, --report: a file name expected");
    RunWallis(image, p.str("--out"), o);
    return 0;
}

// oip mtf IMAGE: the MTF at Nyquist of a strip (.RAW, --width samples per line) or a product (.TIFF of 1 or 4 samples) from its
// slanted edges, as <stem>.MTF.CSV (RunMtf).  IMAGE is the one positional argument, as for mtfc.  Bad values end in 105 before
// any file is read.
int run_mtf(const std::vector<std::string> &args, int width)
{
    Spec sp;
    sp.valued = {"--out", "--axis", "--contrast-min", "--tv-slack", "--noise", "--valid-min", "--valid-max", "--width", "--line-offset", "--lines"};
    sp.flags = {"--force"};
    sp.alias = {{"-o", "--out"}};
    std::string image;
    Parsed p = parse_with_image(sp, args, &image);
    if (p.has("--noise") && p.has("--tv-slack")) throw cli_error(107, "--noise excludes --tv-slack");
    MtfOptions o;
    o.width = p.integer("--width", width);
    const std::string axis = p.str("--axis", "both");
    if (axis != "x" && axis != "y" && axis != "both") throw cli_error(105, "--axis: x, y or both expected");
    o.axes = axis == "x" ? 1 : axis == "y" ? 2 : 3;
    o.contrastMin = p.within("--contrast-min", 200, 1, 65535, "1 <= DN <= 65535 expected");
    o.tvSlack = p.within("--tv-slack", 256, 0, 65535, "0 <= DN <= 65535 expected");
    p.valid_range(1, &o.validMin, &o.validMax);
    p.line_range(&o.lineOffset, &o.lines);
    o.force = p.has("--force");
    existing_file(p, "--noise");
    o.noiseReport = p.str("--noise");
    char buf[256];
    snprintf(buf, sizeof buf, " axis=%s contrast-min=%d tv-slack=%s valid-min=%d valid-max=%d line-offset=%ld lines=%ld", axis.c_str(), o.contrastMin,
             p.has("--noise") ? "noise" : std::to_string(o.tvSlack).c_str(), o.validMin, o.validMax, o.lineOffset, o.lines);
    o.params = "oip mtf image=" + image + buf + " columns=band,axis,ty,tx,polarity,slope_q,contrast,mtf";
    RunMtf(image, p.str("--out"), o);
    return 0;
}

// oip overviews IMAGE: the pyramid of a strip (.RAW, --width samples per line) or a product (.TIFF of 1 or 4 samples) as
// IMAGE.ovr.  IMAGE is the one positional argument, as for mtfc.
int run_overviews(const std::vector<std::string> &args, int width)
{
    Spec sp;
    sp.valued = {"--out", "--levels", "--valid-min", "--width"};
    sp.flags = {"--force"};
    sp.alias = {{"-o", "--out"}};
    std::string image;
    Parsed p = parse_with_image(sp, args, &image);
    OverviewsOptions o;
    o.width = p.integer("--width", width);
    o.pyramid.levels = overview_levels(p);
    o.pyramid.validMin = p.valid_min();
    o.force = p.has("--force");
    RunOverviews(image, p.str("--out"), o);
    return 0;
}

// oip cog IMAGE: a product (.TIFF of 1 or 4 samples, strips or tiles) or a single-band strip (.RAW, --width samples per line)
// as <stem>.COG.TIFF, tiled and with its pyramid inside (RunCog).  IMAGE is the one positional argument, as for mtfc.  Bad
// values end in 105 before any file is read.
int run_cog(const std::vector<std::string> &args, int width)
{
    Spec sp;
    sp.valued = {"--out", "--tile", "--levels", "--valid-min", "--width"};
    sp.flags = {"--force"};
    sp.alias = {{"-o", "--out"}};
    std::string image;
    Parsed p = parse_with_image(sp, args, &image);
    CogOptions o;
    o.width = p.integer("--width", width);
    o.tile = p.has("--tile") ? p.within("--tile", 0, 16, 1024, "a multiple of 16, 16 <= T <= 1024, expected") : 0;      // 0: by the samples per pixel
    if (o.tile % 16 != 0) throw cli_error(105, "--tile: a multiple of 16, 16 <= T <= 1024, expected");
    o.levels = p.has("--levels") ? p.within("--levels", 0, 0, 16, "0 <= N <= 16 expected") : -1;
    o.validMin = p.valid_min();
    o.force = p.has("--force");
    RunCog(image, p.str("--out"), o);
    return 0;
}

// oip rescale IMAGE: a strip (.RAW, --width samples per line) or a product (.TIFF of 1 or 4 samples) on another pixel grid, as
// <stem>.RSC.<ext> (RunRescale).  IMAGE is the one positional argument, as for mtfc.  A scale is a rational: bad syntax and bad
// values end in 105, options that exclude each other in 107, none of the five in 106, before any file is read.
int run_rescale(const std::vector<std::string> &args, int width)
{
    Spec sp;
    sp.valued = {"--out", "--scale", "--scale-x", "--scale-y", "--to-width", "--to-lines", "--kernel", "--valid-min", "--width"};
    sp.flags = {"--force"};
    sp.alias = {{"-o", "--out"}};
    std::string image;
    Parsed p = parse_with_image(sp, args, &image);
    RescaleOptions o;
    o.width = p.positive_width(width);
    for (const char *k : {"--scale-x", "--scale-y", "--to-width", "--to-lines"})
        if (p.has("--scale") && p.has(k)) throw cli_error(107, std::string("--scale excludes ") + k);
    if (p.has("--scale-x") && p.has("--to-width")) throw cli_error(107, "--scale-x excludes --to-width");
    if (p.has("--scale-y") && p.has("--to-lines")) throw cli_error(107, "--scale-y excludes --to-lines");
    if (!p.has("--scale") && !p.has("--scale-x") && !p.has("--scale-y") && !p.has("--to-width") && !p.has("--to-lines"))
        throw cli_error(106, "--scale, --scale-x, --scale-y, --to-width or --to-lines is required");
    auto scale = [&](const char *key, long *num, long *den) {
        if (p.has(key) && !oip_rescale_parse_scale(p.str(key).c_str(), num, den))
            throw cli_error(105, std::string(key) + ": a positive decimal such as 0.8 or a fraction p/q expected (at most 9 digits)");
    };
    scale("--scale", &o.px, &o.qx);
    if (p.has("--scale")) o.py = o.px, o.qy = o.qx;
    scale("--scale-x", &o.px, &o.qx);
    scale("--scale-y", &o.py, &o.qy);
    o.toWidth = p.has("--to-width") ? p.within("--to-width", 0, 1, INT_MAX, "a positive number of pixels expected") : 0;
    o.toLines = p.has("--to-lines") ? p.within("--to-lines", 0, 1, INT_MAX, "a positive number of lines expected") : 0;
    const std::string kernel = p.str("--kernel", "lanczos");
    if (kernel == "lanczos") o.kind = OIP_RESCALE_LANCZOS;
    else if (kernel == "cubic") o.kind = OIP_RESCALE_CUBIC;
    else if (kernel == "linear") o.kind = OIP_RESCALE_LINEAR;
    else throw cli_error(105, "--kernel: lanczos, cubic or linear expected");
    o.validMin = p.valid_min();
    o.force = p.has("--force");
    if (p.has("--out") && p.str("--out").empty()) throw cli_error(105, "--out: a file name expected");
    RunRescale(image, p.str("--out"), o);
    return 0;
}

// oip regcheck --image1 A [--image2 B]: the registration check of two rasters (RunRegcheck).  Bad values end in 105, an
// option that needs another in 107, before any file is read.
int run_regcheck(const std::vector<std::string> &args, int width)
{
    Spec sp;
    sp.valued = {"--image1", "--image2", "--band1", "--band2", "--scale", "--shift-x", "--shift-y", "--tile", "--search", "--step",
                 "--valid-min", "--valid-max", "--min-score", "--width", "--width2", "--out", "--mask", "--mask-cell", "--mask-bits"};
    sp.flags = {"--force", "--bil"};
    sp.alias = {{"-o", "--out"}};
    Parsed p = parse(sp, args);
    require(p, "--image1");
    existing_file(p, "--image1");
    existing_file(p, "--image2");
    existing_file(p, "--mask");
    if (p.has("--mask") && !p.has("--mask-cell")) throw cli_error(107, "--mask requires --mask-cell");
    if ((p.has("--mask-cell") || p.has("--mask-bits")) && !p.has("--mask")) throw cli_error(107, "--mask-cell / --mask-bits require --mask");
    if (p.has("--width2") && !p.has("--image2")) throw cli_error(107, "--width2 requires --image2");
    if ((p.has("--shift-x") || p.has("--shift-y")) && !p.has("--image2")) throw cli_error(107, "--shift-x / --shift-y require --image2");
    RegcheckOptions o;
    o.image2 = p.str("--image2");
    o.band1 = p.integer("--band1", 1);
    o.band2 = p.integer("--band2", 1);
    if (o.band1 < 1 || o.band1 > MSS_BANDS || o.band2 < 1 || o.band2 > MSS_BANDS) throw cli_error(105, "--band1/--band2: 1 <= k <= 4 expected");
    o.scale = p.integer("--scale", 1);
    if (p.has("--scale") && o.scale != 2 && o.scale != 4 && o.scale != 8 && o.scale != 16 && o.scale != 32 && o.scale != 64)
        throw cli_error(105, "--scale: one of 2, 4, 8, 16, 32, 64 expected");
    o.shiftX = p.integer("--shift-x", 0);
    o.shiftY = p.integer("--shift-y", 0);
    o.tile = p.integer("--tile", 64);
    if (o.tile < OIP_MATCH_MIN_T || o.tile > OIP_MATCH_MAX_T || o.tile % 8 != 0) throw cli_error(105, "--tile: a multiple of 8, 8 <= T <= 128 expected");
    o.search = p.within("--search", 4, 1, OIP_MATCH_MAX_S, "1 <= S <= 16 expected");
    o.step = p.within("--step", o.tile, 1, INT_MAX, "N >= 1 expected");
    p.valid_range(1, &o.validMin, &o.validMax);
    o.minScore = p.real("--min-score", 0.5);
    if (!(o.minScore >= -1.0 && o.minScore <= 1.0)) throw cli_error(105, "--min-score: -1 <= X <= 1 expected");
    o.width = p.integer("--width", width);
    o.width2 = p.integer("--width2", 0);
    if (o.width <= 0 || (p.has("--width2") && o.width2 <= 0)) throw cli_error(105, "--width/--width2: a positive line width expected");
    o.bil = p.has("--bil");
    o.force = p.has("--force");
    o.mask = p.str("--mask");
    if (p.has("--mask") && o.mask.empty()) throw cli_error(105, "--mask: a file name expected");
    o.maskCell = p.integer("--mask-cell", 8);
    if (o.maskCell != 4 && o.maskCell != 8 && o.maskCell != 16) throw cli_error(105, "--mask-cell: 4, 8 or 16 expected");
    o.maskBits = p.within("--mask-bits", OIP_MASK_CLOUD | OIP_MASK_BUFFER, 1, 255, "1 <= B <= 255 expected");
    char buf[256];
    snprintf(buf, sizeof buf, " band1=%d band2=%d scale=%d shift-x=%ld shift-y=%ld tile=%d search=%d step=%d valid-min=%d valid-max=%d min-score=%g",
             o.band1, o.band2, o.scale, o.shiftX, o.shiftY, o.tile, o.search, o.step, o.validMin, o.validMax, o.minScore);
    // (a report without --mask is what it was before the option existed)
    const std::string maskBits = p.has("--mask") ? " mask-bits=" + std::to_string(o.maskBits) : "";
    o.params = "oip regcheck image1=" + p.str("--image1") + " image2=" + (o.image2.empty() ? p.str("--image1") : o.image2) + buf + maskBits +
               " columns=x,y,dx,dy,score,flags";
    RunRegcheck(p.str("--image1"), p.str("--out"), o);
    return 0;
}

// oip regfix --report R.CSV --image B: resampling of the image 2 of a regcheck report by the report's shift field (RunRegfix).
// Bad option values end in 105, a missing --report or --image in 106, a report that cannot be used in 2, all before a device
// is touched.
int run_regfix(const std::vector<std::string> &args, int width)
{
    Spec sp;
    sp.valued = {"--report", "--image", "--bands", "--smooth", "--width", "--out"};
    sp.flags = {"--force", "--bil"};
    sp.alias = {{"-o", "--out"}};
    Parsed p = parse(sp, args);
    require(p, "--report");
    require(p, "--image");
    existing_file(p, "--report");
    existing_file(p, "--image");
    RegfixOptions o;
    o.report = p.str("--report");
    o.smooth = p.within("--smooth", 0, 0, OIP_REGFIX_MAX_SMOOTH, "0 <= N <= 16 expected");
    o.width = p.positive_width(width);
    if (p.has("--bands")) {
        const std::string b = p.str("--bands");
        if (b == "all") {
            o.allBands = true;
        } else {
            size_t a = 0;
            while (a <= b.size()) {
                size_t c = b.find(',', a);
                if (c == std::string::npos) c = b.size();
                const std::string t = b.substr(a, c - a);
                if (t.empty() || t.size() > 1 || t[0] < '1' || t[0] > '0' + MSS_BANDS) throw cli_error(105, "--bands: band indices 1..4 separated by commas, or all, expected");
                o.bands.push_back(t[0] - '0');
                a = c + 1;
            }
        }
    }
    o.bil = p.has("--bil");
    o.force = p.has("--force");
    RunRegfix(p.str("--image"), p.str("--out"), o);
    return 0;
}

// oip pansharpen --pan P --mss M: the 4-band product at PAN resolution (RunPansharpen).  Bad option values end in 105, a missing
// --pan or --mss in 106, inputs that cannot be used (sample counts, W != 4 w, too few lines) in 2, all before a device is touched.
int run_pansharpen(const std::vector<std::string> &args, int width)
{
    Spec sp;
    sp.valued = {"--pan", "--mss", "--line-offset", "--max-gain", "--width", "--out", "--levels"};
    sp.flags = {"--force", "--overviews"};
    sp.alias = {{"-o", "--out"}};
    Parsed p = parse(sp, args);
    require(p, "--pan");
    require(p, "--mss");
    existing_file(p, "--pan");
    existing_file(p, "--mss");
    PansharpenOptions o;
    o.pan = p.str("--pan");
    o.mss = p.str("--mss");
    o.lineOffset = p.within("--line-offset", 0, 0, INT_MAX, "N >= 0 expected");
    o.maxGain = p.within("--max-gain", OIP_PANSHARPEN_DEF_GAIN, 1, OIP_PANSHARPEN_MAX_GAIN, "1 <= G <= 64 expected");
    o.width = p.positive_width(width);
    if (p.has("--levels") && !p.has("--overviews")) throw cli_error(107, "--levels requires --overviews");
    o.overviews = p.has("--overviews");
    o.pyramid.levels = overview_levels(p);
    o.force = p.has("--force");
    RunPansharpen(p.str("--out"), o);
    return 0;
}

}  // namespace

static int oip_main(int argc, const char *argv[]);

// The products are on disk and the log is flushed when oip_main returns; what is left is tear-down -- hipFree of ~10 GB,
// un-pinning the staging ring, the HIP runtime's own shutdown (measured: DESIGN.md 4.5) -- which the kernel does faster
// for a process that simply leaves.  OIP_FAST_EXIT=0 runs the destructors.
int main(int argc, const char *argv[])
{
    process_start();
    const int rc = oip_main(argc, argv);
    fflush(stdout);
    if (log_file()) fflush(log_file());
    const char *fe = getenv("OIP_FAST_EXIT");
    if (!(fe && atoi(fe) == 0)) _exit(rc);
    return rc;
}

static int oip_main(int argc, const char *argv[])
{
    try {
        const char *lf = getenv("LOGFILE");                             // main.cpp:322-329
        log_file() = fopen(lf ? lf : "oip.log", "a");
        std::vector<std::string> args(argv + 1, argv + argc);
        int width = OIP_PIXELS_PER_LINE;
        try {
            for (auto &a : args) {
                if (a == "-h" || a == "--help") { usage(); return 255; }
                if (a == "-v" || a == "--version") { puts("1.1"); return 255; }
            }
            // --tiff-compress reference|none|lzw|deflate (not in the reference; anywhere on the line)
            for (size_t i = 0; i < args.size(); ++i) {
                std::string v;
                if (args[i] == "--tiff-compress" && i + 1 < args.size()) { v = args[i + 1]; args.erase(args.begin() + i, args.begin() + i + 2); }
                else if (args[i].rfind("--tiff-compress=", 0) == 0) { v = args[i].substr(16); args.erase(args.begin() + i); }
                else continue;
                if (v == "reference") tiff_policy() = -1;
                else if (v == "none") tiff_policy() = TIFF_NONE;
                else if (v == "lzw") tiff_policy() = TIFF_LZW;
                else if (v == "deflate") tiff_policy() = TIFF_DEFLATE;
                else throw cli_error(105, "--tiff-compress: reference, none, lzw or deflate expected");
                break;
            }
            if (!args.empty() && args[0] == "prestitch") return run_prestitch({args.begin() + 1, args.end()}, width);
            if (!args.empty() && args[0] == "stitch") return run_stitch({args.begin() + 1, args.end()}, width);
            if (!args.empty() && args[0] == "task") return run_task({args.begin() + 1, args.end()}, width);
            if (!args.empty() && args[0] == "plan") return run_plan({args.begin() + 1, args.end()});
            if (!args.empty() && args[0] == "rrc-calib") return run_rrc_calib({args.begin() + 1, args.end()}, width);
            if (!args.empty() && args[0] == "quicklook") return run_quicklook({args.begin() + 1, args.end()}, width);
            if (!args.empty() && args[0] == "mtfc") return run_mtfc({args.begin() + 1, args.end()}, width);
            if (!args.empty() && args[0] == "despike") return run_despike({args.begin() + 1, args.end()}, width);
            if (!args.empty() && args[0] == "denoise") return run_denoise({args.begin() + 1, args.end()}, width);
            if (!args.empty() && args[0] == "noise") return run_noise({args.begin() + 1, args.end()}, width);
            if (!args.empty() && args[0] == "mask") return run_mask({args.begin() + 1, args.end()}, width);
            if (!args.empty() && args[0] == "wallis") return run_wallis({args.begin() + 1, args.end()}, width);
            if (!args.empty() && args[0] == "mtf") return run_mtf({args.begin() + 1, args.end()}, width);
            if (!args.empty() && args[0] == "overviews") return run_overviews({args.begin() + 1, args.end()}, width);
            if (!args.empty() && args[0] == "cog") return run_cog({args.begin() + 1, args.end()}, width);
            if (!args.empty() && args[0] == "rescale") return run_rescale({args.begin() + 1, args.end()}, width);
            if (!args.empty() && args[0] == "regcheck") return run_regcheck({args.begin() + 1, args.end()}, width);
            if (!args.empty() && args[0] == "regfix") return run_regfix({args.begin() + 1, args.end()}, width);
            if (!args.empty() && args[0] == "pansharpen") return run_pansharpen({args.begin() + 1, args.end()}, width);
            if (!args.empty() && args[0] == "auxsep")
                throw std::invalid_argument("auxsep (down-link de-framing) is outside this build: run the reference's auxsep, then this tool");
            if (args.empty()) { usage(); return 0; }
            return run_default(args, width);
        } catch (const cli_error &e) {
            fprintf(stderr, "%s\nRun with --help for more information.\n", e.what());
            return e.code;
        }
    } catch (usage_error &ex) {
        printf("USAGE ERROR: %s.\n", ex.what());
        return 254;
    } catch (std::exception &ex) {
        OLOG("[ERROR] %s.", ex.what());
        return 2;
    } catch (...) {
        OLOG("[FATAL] UNKOWN FATAL ERROR OCCURED.");
        return 1;
    }
}
