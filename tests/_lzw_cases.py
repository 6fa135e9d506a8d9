"""Inputs that put a TIFF LZW coder into the states where such coders are historically wrong, and the search that found them.

A case is one image row (one strip: predictor 2, one row per strip) of 12-bit sensor-like noise, or of such noise followed by a
constant run, whose predictor-2 byte stream makes the independent coder (tests/_tiff.py::lzw_trace) produce one named event:

  end<N>        the strip ends with next == N after the last code's increment (libtiff's LZWPostEncode): at 512 / 1024 / 2048
                EndOfInformation goes out one bit wider than the last code, at 4094 a ClearCode precedes it; N - 1 and N + 1 bracket
  clear_last    the LAST byte of the strip fills the table inside the loop: ClearCode, the last code at 9 bits, end next 259
  widen<W>_last the LAST byte of the strip widens the code inside the loop: the last code is the first of W bits
  kwkwk<N>      a code equal to the decoder's own next, N, goes out (the entry the previous miss assigned): at 510 .. 512,
                1022 .. 1024, 2046 .. 2048 around the decoder's early width change; 4092 is the highest that can occur, the
                ClearCode follows it
  kwkwk_last    such a code is the very last data code of the strip

CASES is the table, as literals; find_cases() regenerates it (python tests/_lzw_cases.py prints it).  Every test asserts through
has_event that its input still produces the event before it looks at a coder of the product."""
import numpy as np

import _tiff

SPPS = (1, 4)
EVENTS = (["end%d" % n for n in (511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4093, 4094)] +
          ["clear_last", "widen10_last", "widen11_last", "widen12_last"] +
          ["kwkwk%d" % n for n in (510, 511, 512, 1022, 1023, 1024, 2046, 2047, 2048, 4092)] + ["kwkwk_last"])

# (seed, width, samples per pixel, kind, event, prefix): `width` pixels; kind "noise": all of them noise (prefix == width);
# kind "run": `prefix` pixels of noise, then the constant 4242 in every sample
CASES = [
    (2, 132, 1, "noise", "end511", 132),
    (1, 132, 1, "noise", "end512", 132),
    (1, 133, 1, "noise", "end513", 133),
    (1, 426, 1, "noise", "end1023", 426),
    (3, 424, 1, "noise", "end1024", 424),
    (1, 427, 1, "noise", "end1025", 427),
    (1, 1104, 1, "noise", "end2047", 1104),
    (1, 1105, 1, "noise", "end2048", 1105),
    (3, 1109, 1, "noise", "end2049", 1109),
    (1, 2730, 1, "noise", "end4093", 2730),
    (1, 2731, 1, "noise", "end4094", 2731),
    (1, 2732, 1, "noise", "clear_last", 2732),
    (2, 133, 1, "noise", "widen10_last", 133),
    (1, 427, 1, "noise", "widen11_last", 427),
    (3, 1109, 1, "noise", "widen12_last", 1109),
    (1, 248, 1, "run", "kwkwk510", 120),
    (1, 249, 1, "run", "kwkwk511", 121),
    (1, 249, 1, "run", "kwkwk512", 121),
    (1, 541, 1, "run", "kwkwk1022", 413),
    (1, 541, 1, "run", "kwkwk1023", 413),
    (1, 542, 1, "run", "kwkwk1024", 414),
    (1, 1218, 1, "run", "kwkwk2046", 1090),
    (1, 1219, 1, "run", "kwkwk2047", 1091),
    (1, 1219, 1, "run", "kwkwk2048", 1091),
    (1, 2842, 1, "run", "kwkwk4092", 2714),
    (1, 249, 1, "run", "kwkwk_last", 121),
    (4, 33, 4, "noise", "end511", 33),
    (3, 33, 4, "noise", "end512", 33),
    (1, 712, 4, "noise", "end513", 712),
    (5, 108, 4, "noise", "end1023", 108),
    (18, 105, 4, "noise", "end1024", 105),
    (8, 107, 4, "noise", "end1025", 107),
    (10, 279, 4, "noise", "end2047", 279),
    (1, 277, 4, "noise", "end2048", 277),
    (5, 277, 4, "noise", "end2049", 277),
    (17, 679, 4, "noise", "end4093", 679),
    (8, 675, 4, "noise", "end4094", 675),
    (1, 679, 4, "noise", "clear_last", 679),
    (1, 712, 4, "noise", "widen10_last", 712),
    (8, 107, 4, "noise", "widen11_last", 107),
    (5, 277, 4, "noise", "widen12_last", 277),
    (1, 62, 4, "run", "kwkwk510", 30),
    (1, 62, 4, "run", "kwkwk511", 30),
    (1, 62, 4, "run", "kwkwk512", 30),
    (1, 136, 4, "run", "kwkwk1022", 104),
    (1, 136, 4, "run", "kwkwk1023", 104),
    (1, 136, 4, "run", "kwkwk1024", 104),
    (1, 335, 4, "run", "kwkwk2046", 271),
    (1, 335, 4, "run", "kwkwk2047", 271),
    (1, 335, 4, "run", "kwkwk2048", 271),
    (1, 704, 4, "run", "kwkwk4092", 672),
    (1, 56, 4, "run", "kwkwk_last", 40),
]

# Streams that are legal TIFF LZW but that libtiff's encoder never writes (the knobs of _tiff.lzw_trace).  A variant is here only
# if _tiff.lzw_decode returns the input for it AND libtiff (through Pillow; 4.7.1 / 12.2.0 when this was written) reads a one-strip
# file that holds it: tests/test_tifflzw_cpu.py asserts both.  Left out because libtiff refuses it ("Using code not yet in
# table", decoder error -2): leading_clear=False, a strip that does not start with ClearCode.  The product's decoders happen to
# read such a strip; nothing tests or promises that.
VARIANTS = {
    "clear_at_4095": dict(clear_at=4095),
    "clear_at_4096": dict(clear_at=4096),                      # the table really full before ClearCode (TIFF 6.0's text)
    "extra_clears": dict(extra_clear_every=700),               # ClearCodes in the middle of a half-filled table
    "double_clear": dict(double_clear=True),                   # every ClearCode twice
    "trailing_bytes": dict(trailing_bytes=5),                  # junk after EndOfInformation
}
VARIANT_WIDTH = {1: 8000, 4: 2000}                             # 16000-byte noise strips: the table fills three times


def variant_row(spp):
    return noise_row(7, VARIANT_WIDTH[spp], spp)


def variant_reaches_its_state(t, knobs):
    """the trace of a variant stream shows what the variant is about"""
    if "clear_at" in knobs:
        return t.max_next == knobs["clear_at"] and len(t.clears) >= 3
    if "extra_clear_every" in knobs:
        return len(t.clears) > 10 and t.max_next < 4094
    if "double_clear" in knobs:
        return any(b == a + 1 for a, b in zip(t.clears, t.clears[1:])) and t.max_next == 4094
    return t.stream.endswith(b"\xa5" * knobs["trailing_bytes"]) and t.codes[-1][0] == 257


def noise_row(seed, pixels, spp):
    rng = np.random.default_rng(seed)
    return np.clip(rng.normal(1800.0, 300.0, pixels * spp), 64, 4095).astype(np.uint16)


def row_of(seed, width, spp, kind, prefix):
    """the image row of a case: width * spp samples (also of a case's generator at another width: noise is noise all along, a
    run starts after `prefix` pixels where the row is that long)"""
    prefix = width if kind == "noise" else min(prefix, width)
    a = noise_row(seed, prefix, spp)
    if kind == "run":
        a = np.concatenate([a, np.full((width - prefix) * spp, 4242, dtype=np.uint16)])
    assert kind in ("noise", "run") and a.size == width * spp
    return a


def case_row(case):
    seed, width, spp, kind, _, prefix = case
    return row_of(seed, width, spp, kind, prefix)


def predict2(block, spp):
    """TIFF predictor 2 on 16-bit samples, row by row, as the little-endian byte stream the coder sees; block: rows x (width * spp)"""
    block = np.atleast_2d(block)
    d = block.astype(np.uint16).copy()
    d[:, spp:] = (block[:, spp:].astype(np.int32) - block[:, :-spp].astype(np.int32)).astype(np.uint16)
    return d.astype("<u2").tobytes()


def case_bytes(case):
    return predict2(case_row(case), case[2])


def case_id(case):
    return "%s-spp%d" % (case[4], case[2])


def has_event(t, event):
    """does the trace of a strip show the event"""
    if event == "kwkwk_last":
        return bool(t.last_data_code()[2])
    if event.startswith("kwkwk"):
        return int(event[5:]) in t.kwkwk_values()
    if event == "clear_last":
        return t.last_byte == "clear" and t.end_next == 259 and t.last_data_code()[1] == 9
    if event.startswith("widen"):
        w = int(event[5:7])
        return t.last_byte == "widen%d" % w and t.end_next == (1 << (w - 1)) + 1 and t.last_data_code()[1] == w
    n = int(event[3:])
    if t.end_next != n:
        return False
    if n == 4094:                                # ClearCode between the last data code and EndOfInformation, which is 9 bits again
        return t.codes[-2][0] == 256 and t.eoi_width == 9
    if n in (512, 1024, 2048):                   # EndOfInformation one bit wider than the last data code
        return t.eoi_width == t.last_data_code()[1] + 1
    return t.eoi_width == t.last_data_code()[1]


def input_key(case):
    """what the input of a case depends on: cases that differ only in the event share it"""
    return case[:4] + (case[5],)


def distinct_inputs(cases=None):
    """the cases without those that share an input with an earlier one"""
    seen, out = set(), []
    for c in (CASES if cases is None else cases):
        key = input_key(c)
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


def _states(seed, spp, pixels):
    """one trace of a long noise row: next after every input byte, and the bytes that missed.  A coder's state after a prefix of
    its input does not depend on what follows, so this is the state every shorter row of this seed ends its loop in (given that the
    generator's shorter draws are prefixes of its longer ones: each candidate is confirmed by a trace of its own afterwards)."""
    data = predict2(noise_row(seed, pixels, spp), spp)
    t = _tiff.lzw_trace(data)
    nxt_after = np.zeros(len(data), dtype=np.int64)
    miss = np.zeros(len(data), dtype=bool)
    nxt, at = 258, 0
    for v, _, _, pos in t.codes:
        if v in (256, 257) or pos >= len(data):
            continue
        nxt_after[at:pos] = nxt
        nxt += 1
        if nxt == 4094:
            nxt = 258
        nxt_after[pos] = nxt
        miss[pos] = True
        at = pos + 1
    nxt_after[at:] = nxt
    return nxt_after, miss


def find_cases(max_seed=64, log=None):
    """The table, searched again: per samples-per-pixel value and event the first (seed, width) -- seeds 1 .. max_seed, widths upward --
    whose trace shows the event; an input already in the table is taken where it shows a further event.  Raises when a target stays
    without a case: extend the seed range then."""
    found = []
    for spp in SPPS:
        pixels = 2800 if spp == 1 else 720
        bpp = 2 * spp
        states = {}

        def st(seed):
            if seed not in states:
                states[seed] = _states(seed, spp, pixels)
            return states[seed]

        def confirm(seed, width, kind, event, prefix):
            case = (seed, width, spp, kind, event, prefix)
            return case if has_event(_tiff.lzw_trace(case_bytes(case)), event) else None

        def search(event):
            for c in found:                      # an input we already have
                if c[2] == spp:
                    hit = confirm(c[0], c[1], c[3], event, c[5])
                    if hit:
                        return hit
            for seed in range(1, max_seed + 1):
                nxt_after, miss = st(seed)
                ends = np.arange(1, pixels + 1) * bpp - 1            # last byte of a row of 1 .. pixels pixels
                if event == "kwkwk_last":
                    cands = [(40, 40 + r) for r in range(1, 120)]
                elif event.startswith("kwkwk"):
                    n = int(event[5:])
                    pre = np.nonzero((nxt_after[ends] >= n - 30) & (nxt_after[ends] <= n - 2))[0] + 1
                    cands = [(int(p), int(p) + r) for p in pre for r in (8, 16, 32, 64, 128)]
                elif event == "clear_last":
                    cands = [(int(w), int(w)) for w in np.nonzero(miss[ends] & (nxt_after[ends] == 258))[0] + 1 if w > 1]
                elif event.startswith("widen"):
                    n = 1 << (int(event[5:7]) - 1)
                    cands = [(int(w), int(w)) for w in np.nonzero(miss[ends] & (nxt_after[ends] == n))[0] + 1]
                else:
                    n = int(event[3:])
                    cands = [(int(w), int(w)) for w in np.nonzero(nxt_after[ends] == n - 1)[0] + 1]
                for prefix, width in cands:
                    hit = confirm(seed, width, "noise" if prefix == width else "run", event, prefix)
                    if hit:
                        return hit
            raise LookupError("no case for %s at %d samples per pixel within seeds 1..%d" % (event, spp, max_seed))

        for event in EVENTS:
            found.append(search(event))
            if log:
                log(found[-1])
    return found


if __name__ == "__main__":
    print("CASES = [")
    find_cases(log=lambda c: print("    %r," % (c,), flush=True))
    print("]")
