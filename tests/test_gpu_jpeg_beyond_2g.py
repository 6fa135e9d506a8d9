"""The device JPEG coder on an image of more than 2^31 bytes: grey, 40000 x 53720.  The largest legal height is 65535, so the width
carries the size.  In the manner of tests/_bigraster.py every line holds one constant, except a head band (lines 0..15) and a tail
band (lines 53680..53719) of seeded noise.  Byte 2^31 lies in line 53687, so interval 6710 (lines 53680..53687) straddles it and
intervals 6711..6714 lie wholly beyond it: a 32-bit byte offset would read them from lines 0..32 of the image, the head band and the
constant.  The intervals of both bands are compared with the restatement (tests/_jpeg_ref.py), every other one with the one interval
of the constant, on the device.  No Pillow decode at this size."""
import numpy as np
import pytest
import torch

import _jpeg_ref as J

pytestmark = pytest.mark.gpu

W, H, Q, CONST = 40000, 53720, 50, 137
HEAD, TAIL0 = 16, 53680


def _band(lines, seed):
    """narrow noise (100..139): a dozen symbols a block, so that the restatement of seven 5000-block intervals takes a second"""
    return np.random.default_rng(seed).integers(100, 140, (lines, W), dtype=np.uint8)


def test_intervals_beyond_2_31_bytes(ctx):
    assert W * (TAIL0 + 7) < 2 ** 31 < W * (TAIL0 + 8) and W * H > 2 ** 31
    head, tail = _band(HEAD, 1), _band(H - TAIL0, 2)
    img = torch.full((H, W), CONST, dtype=torch.uint8, device="cuda")
    img[:HEAD] = torch.from_numpy(head).cuda()
    img[TAIL0:] = torch.from_numpy(tail).cuda()
    n = H // 8
    payload = torch.empty(ctx.jpeg_worst_bytes(W, H, 1), dtype=torch.uint8, device="cuda")
    off, ln, total = ctx.jpeg_scan(img, W, W, H, 1, Q, payload)
    assert len(off) == n and off[0] == 0 and np.array_equal(off[1:], np.cumsum(ln)[:-1]) and total == int(off[-1] + ln[-1])

    def got(k):
        return payload[int(off[k]):int(off[k] + ln[k])].cpu().numpy().tobytes()

    for k, want in enumerate(J.encode(head, Q).intervals):
        assert got(k) == want, "interval %d (head band)" % k
    for k, want in enumerate(J.encode(tail, Q).intervals, TAIL0 // 8):
        assert got(k) == want, "interval %d (%s byte 2^31)" % (k, "straddles" if k == TAIL0 // 8 else "beyond")
    const = J.encode(np.full((8, W), CONST, np.uint8), Q).intervals[0]
    a, b = HEAD // 8, TAIL0 // 8
    assert (ln[a:b] == len(const)).all()
    block = payload[int(off[a]):int(off[b])].view(b - a, len(const))
    row = torch.from_numpy(np.frombuffer(const, dtype=np.uint8).copy()).cuda()
    wrong = (block != row).any(dim=1)
    assert not bool(wrong.any()), "interval %d is not the interval of the constant" % (a + int(torch.nonzero(wrong)[0]))
