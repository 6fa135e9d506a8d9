"""What the launch-boundary tests of the two device strip encoders share (tests/test_gpu_tifflzw.py, tests/test_gpu_deflate_encode.py).
A launch of either encoder takes 32768 streams; an image of 32770 one-row strips takes two, the second with two streams whose slots
start again at 0 while their lengths and offsets go on at 32768.  The rows are a few distinct patterns, so the reference coder runs
once per pattern and the expected payload is put together from its streams.  Tests only."""
import numpy as np
import torch

PER_LAUNCH = 32768      # csrc/oip_tiffstreams.h: streams per encode launch of both codecs
NSTRIPS = PER_LAUNCH + 2
GUARD = 4096            # bytes behind the payload, pre-filled, that no encode may touch
PATTERN = 0xA5


WIDTH = 7               # pixels of a row, one sample each: streams of 8 to 23 bytes, odd and even ones with either coder


def rows_named(names):
    """(len(names), WIDTH) uint16: one row of every named kind"""
    rng = np.random.default_rng(1)
    kinds = {
        "noise16": rng.integers(0, 65536, WIDTH, dtype=np.uint16),
        "noise12": rng.integers(64, 4096, WIDTH).astype(np.uint16),
        "const": np.full(WIDTH, 4242, np.uint16),
        "zero": np.zeros(WIDTH, np.uint16),
        "ramp": (np.arange(WIDTH) * 257).astype(np.uint16),
        "small": rng.integers(0, 4, WIDTH).astype(np.uint16),
    }
    return np.stack([kinds[n] for n in names])


def predict2(row):
    """TIFF predictor 2 of a one-sample row, as the little-endian bytes the coder sees"""
    d = row.copy()
    d[1:] = row[1:] - row[:-1]
    return d.astype("<u2").tobytes()


def pattern_of_rows(npatterns):
    """which pattern row r holds: neighbours differ, and the sequence does not repeat with a short period"""
    r = np.arange(NSTRIPS)
    return (r * 3 + (r >> 4) + (r >> 9)) % npatterns


def expected_payload(idx, streams):
    """(offsets, lengths, total, bytes) of streams[idx[k]] one behind the other at even offsets, pad bytes zero"""
    lens = np.array([len(s) for s in streams], dtype=np.int64)[idx]
    ends = np.cumsum(lens + (lens & 1))                      # every stream plus its pad
    offs = ends - (lens + (lens & 1))
    total = int(offs[-1] + lens[-1])
    buf = np.zeros(int(ends[-1]), dtype=np.uint8)
    for p, s in enumerate(streams):
        at = offs[idx == p]
        buf[at[:, None] + np.arange(len(s))[None, :]] = np.frombuffer(s, dtype=np.uint8)[None, :]
    return offs, lens, total, buf


def check_two_launches(ctx, encode, worst_bytes, scratch_bytes, rows_u16, width, spp, idx, streams, own_scratch):
    """rows_u16: (npatterns, width * spp) uint16; streams: the reference coder's stream of every pattern's predictor-2 bytes.
    Offsets, lengths, bytes, zero pad bytes and the total over all 32770 strips, and the guard behind worst_bytes untouched."""
    lens = [len(s) for s in streams]
    assert lens[idx[PER_LAUNCH - 1]] % 2 == 1, "the last stream of the first launch must be odd: its pad byte straddles the boundary"
    assert {n % 2 for n in lens} == {0, 1}, "odd and even streams"
    img = np.ascontiguousarray(rows_u16[idx])
    d_img = torch.from_numpy(img.view(np.int16)).cuda()
    worst = worst_bytes(NSTRIPS, width, spp, 1)
    payload = torch.full((worst + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
    scratch = None if own_scratch else torch.zeros(scratch_bytes(NSTRIPS, width, spp, 1), dtype=torch.uint8, device="cuda")
    off, ln, total = encode(d_img, NSTRIPS, width, spp, 1, payload, scratch=scratch, payload_cap=worst)
    host = payload.cpu().numpy()
    want_off, want_len, want_total, want = expected_payload(idx, streams)
    assert len(off) == len(ln) == NSTRIPS
    assert np.array_equal(ln.astype(np.int64), want_len), np.flatnonzero(ln.astype(np.int64) != want_len)[:8]
    assert np.array_equal(off.astype(np.int64), want_off), np.flatnonzero(off.astype(np.int64) != want_off)[:8]
    assert off[PER_LAUNCH] == off[PER_LAUNCH - 1] + ln[PER_LAUNCH - 1] + 1          # the pad byte across the boundary
    assert total == want_total and total <= worst
    bad = np.flatnonzero(host[:total] != want[:total])                                # streams and the zero pad bytes between them
    assert bad.size == 0, ("first differing byte", int(bad[0]), "in strip", int(np.searchsorted(want_off, bad[0], side="right") - 1))
    assert (host[worst:] == PATTERN).all()
    assert np.array_equal(d_img.cpu().numpy().view(np.uint16), img)                   # the image is read, never written
