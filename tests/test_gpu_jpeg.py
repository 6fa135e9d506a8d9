"""The device JPEG coder (csrc/jpeg.hip, oip_jpeg_scan_u8: a restart interval per wave, the coder of csrc/oip_jpeg.h) through the C
ABI against the restatement (tests/_jpeg_ref.py): payload, offsets and lengths interval for interval, the assembled file byte for
byte, and Pillow's libjpeg opens and fully decodes it.  The host build of this code has been through the same inputs under ASan +
UBSan (tests/test_jpeg_cpu.py)."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

import opticalimageprocessor_amd as oip
import _jpeg_ref as J

pytestmark = pytest.mark.gpu

GUARD = 4096            # bytes behind the payload's capacity, pre-filled, that no encode may touch
PATTERN = 0xA5


@pytest.fixture(scope="module")
def restated():
    """{name: (image, quality, Encoded)} of J.CASES, computed once"""
    out = {}
    for name, *_ in J.CASES:
        img, q = J.case_image(name)
        out[name] = (img, q, J.encode(img, q))
    return out


def _device_image(img, pad, odd):
    """the image on the device with lines `pad` bytes longer than they need be, from byte `odd` of its buffer on"""
    h, w = img.shape[:2]
    nch = 1 if img.ndim == 2 else 3
    pitch = w * nch + pad
    rows = np.full((h, pitch), 0xEE, dtype=np.uint8)
    rows[:, :w * nch] = img.reshape(h, w * nch)
    buf = torch.full((odd + h * pitch,), 0x11, dtype=torch.uint8, device="cuda")
    buf[odd:] = torch.from_numpy(rows.reshape(-1)).cuda()
    return buf, pitch


@pytest.mark.parametrize("pad,odd", [(0, 0), (5, 1)], ids=["packed", "pitch_and_odd_base"])
@pytest.mark.parametrize("name", [c[0] for c in J.CASES])
def test_the_scan_is_the_restatements(ctx, restated, tmp_path, name, pad, odd):
    img, q, e = restated[name]
    J.assert_case_preconditions(name, e.trace)
    h, w = img.shape[:2]
    nch = 1 if img.ndim == 2 else 3
    buf, pitch = _device_image(img, pad, odd)
    worst = ctx.jpeg_worst_bytes(w, h, nch)
    assert worst == oip.jpeg_worst_bytes(w, h, nch) == -(-h // 8) * -(-w // 8) * nch * 416
    payload = torch.full((worst + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
    off, ln, total = ctx.jpeg_scan(buf, pitch, w, h, nch, q, payload, payload_cap=worst, byte_offset=odd)
    host = payload.cpu().numpy()
    assert (host[total:] == PATTERN).all(), "a store behind the scan's last byte"
    assert len(off) == len(e.intervals)
    pos = 0
    for k, want in enumerate(e.intervals):
        assert off[k] == pos and ln[k] == len(want), (k, off[k], ln[k], pos, len(want))
        assert host[pos:pos + len(want)].tobytes() == want, "interval %d differs" % k
        assert want == oip.jpeg_interval_host(img, q, k), "interval %d: device and host bytes differ" % k
        pos += len(want)
    assert total == pos
    # the file: the restatement's, and libjpeg decodes all of it
    path = str(tmp_path / "x.jpg")
    oip.write_jpeg_u8(path, host[:total], off, ln, w, h, nch, q)
    with open(path, "rb") as f:
        data = f.read()
    assert data == e.file
    with Image.open(io.BytesIO(data)) as im:
        im.load()
        assert im.mode == ("L" if nch == 1 else "RGB") and im.size == (w, h)
    # a caller's scratch buffer gives the same payload
    scratch = torch.zeros(ctx.jpeg_scratch_bytes(w, h, nch), dtype=torch.uint8, device="cuda")
    payload2 = torch.full((worst + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
    off2, ln2, total2 = ctx.jpeg_scan(buf, pitch, w, h, nch, q, payload2, scratch=scratch, payload_cap=worst, byte_offset=odd)
    assert total2 == total and np.array_equal(off2, off) and np.array_equal(ln2, ln) and np.array_equal(payload2.cpu().numpy(), host)
    # the image is read, never written
    assert (buf[:odd].cpu().numpy() == 0x11).all()
    back = buf[odd:].cpu().numpy().reshape(h, pitch)
    assert np.array_equal(back[:, :w * nch].reshape(img.shape), img) and (back[:, w * nch:] == 0xEE).all()


@pytest.mark.parametrize("name", ["grey_520x24_noise_q100", "rgb_13x67_noise_q50"])
def test_an_interval_is_a_function_of_its_own_lines(ctx, restated, name):
    """lines 8..15 of an image, encoded as an 8-line image of their own, give the bytes of interval 1"""
    img, q, e = restated[name]
    w = img.shape[1]
    nch = 1 if img.ndim == 2 else 3
    part = np.ascontiguousarray(img[8:16])
    d = torch.from_numpy(part.reshape(-1)).cuda()
    payload = torch.zeros(ctx.jpeg_worst_bytes(w, 8, nch), dtype=torch.uint8, device="cuda")
    off, ln, total = ctx.jpeg_scan(d, w * nch, w, 8, nch, q, payload)
    assert len(off) == 1 and off[0] == 0 and payload[:total].cpu().numpy().tobytes() == e.intervals[1]


def test_refusals_launch_nothing(ctx):
    w, h, nch, q = 24, 16, 3, 75
    img = J.noise(h, w, nch, 3)
    d = torch.from_numpy(img.reshape(-1)).cuda()
    worst = ctx.jpeg_worst_bytes(w, h, nch)
    payload = torch.full((worst,), PATTERN, dtype=torch.uint8, device="cuda")
    need = ctx.jpeg_scratch_bytes(w, h, nch)
    scratch = torch.zeros(need + 8, dtype=torch.uint8, device="cuda")
    bad = [
        dict(img=None), dict(payload=None),                                    # a null pointer
        dict(w=0), dict(w=65536), dict(h=0), dict(h=65536),
        dict(nch=2), dict(nch=4),
        dict(quality=0), dict(quality=101),
        dict(pitch=w * nch - 1),
        dict(payload_cap=worst - 1),
        dict(scratch=scratch, scratch_bytes=need - 1),
        dict(scratch=scratch[4:], scratch_bytes=need),                         # misaligned
    ]
    for kw in bad:
        a = dict(img=d, pitch=w * nch, w=w, h=h, nch=nch, quality=q, payload=payload, scratch=None, payload_cap=worst, scratch_bytes=None)
        a.update(kw)
        with pytest.raises(ValueError):
            ctx.jpeg_scan(a["img"], a["pitch"], a["w"], a["h"], a["nch"], a["quality"], a["payload"], scratch=a["scratch"],
                          payload_cap=a["payload_cap"], scratch_bytes=a["scratch_bytes"])
    assert ctx.jpeg_worst_bytes(0, h, nch) == 0 and ctx.jpeg_worst_bytes(w, 65536, nch) == 0 and ctx.jpeg_scratch_bytes(w, h, 2) == 0
    assert oip.jpeg_interval_host(img, 0, 0) == b"" and oip.jpeg_interval_host(img, q, 2) == b"" and oip.jpeg_interval_host(img, q, 0, cap=3) == b""
    ctx.sync()
    assert (payload.cpu().numpy() == PATTERN).all()
    off, ln, total = ctx.jpeg_scan(d, w * nch, w, h, nch, q, payload, scratch=scratch)
    assert payload[:int(ln[0])].cpu().numpy().tobytes() == J.encode(img, q).intervals[0]
