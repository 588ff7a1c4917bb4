"""The numpy restatement of the thumbnail pipeline (tests/thumb_ref.py) against Pillow 12 (libjpeg-turbo), an independent decoder
and the nearest stand-in for cv2's encoder on a machine without cv2: every stream decodes at the right size and mode, the DQT and
DHT segments are those Pillow writes, and against Pillow's own encode of the same resized pixels the stream costs at most
thumb_ref.GAP_PSNR_DB of PSNR and thumb_ref.GAP_SCAN of entropy-coded bytes - twice the largest gap measured,
inside the 0.5 dB / 3 % a rounding difference in the DCT could cost.  The coder's hard cases are counted, and the shared inputs
reach each of them."""
import io

import numpy as np
import pytest

import thumb_ref as R

Image = pytest.importorskip("PIL.Image")


def _segments(jpeg):
    """[(marker, payload)] up to and including SOS"""
    out, i = [], 2
    assert jpeg[:2] == b"\xff\xd8"
    while True:
        assert jpeg[i] == 0xFF
        n = int.from_bytes(jpeg[i + 2:i + 4], "big")
        out.append((jpeg[i + 1], jpeg[i + 4:i + 2 + n]))
        i += 2 + n
        if out[-1][0] == 0xDA:
            return out


def _pillow(img, quality):
    return R.pillow_jpeg(img, quality)


ALL = [(name, img, wh, q) for name, img, wh, q in R.hard_inputs()] + \
      [(f"natural_{w}x{h}_c{c}_q{q}", R.natural(h, w, c), wh, q) for h, w, c, wh, q in R.GAP_IMAGES] + \
      [("one_pixel", np.full((1, 1, 3), 90, np.uint8), (1, 1), 70), ("upscale_bgra", R.natural(4, 5, 4), (23, 19), 70)]


@pytest.fixture(scope="module")
def encoded():
    hard = {}
    return {name: R.encode(img, wh, q, hard) for name, img, wh, q in ALL}, hard


def test_every_stream_decodes_at_the_right_size_and_mode(encoded):
    streams, _ = encoded
    for name, img, wh, q in ALL:
        e = streams[name]
        im = R.decode(e["jpeg"])
        assert im.size == wh and im.mode == ("L" if np.asarray(img).ndim == 2 else "RGB"), name
        assert e["jpeg"][:2] == b"\xff\xd8" and e["jpeg"][-2:] == b"\xff\xd9"
        scan = e["jpeg"][len(e["header"]):-2]
        assert b"\xff" not in scan.replace(b"\xff\x00", b""), name                    # no marker inside the scan
        assert [m for m, _ in _segments(e["jpeg"])] == ([0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDA] if e["g"]["ncomp"] == 3
                                                        else [0xE0, 0xDB, 0xC0, 0xC4, 0xC4, 0xDA]), name


@pytest.mark.parametrize("quality", [1, 25, 50, 70, 75, 95, 100])
def test_quantisation_tables_are_pillows(quality):
    img = R.natural(16, 16, 3)
    ours = R.encode(img, (16, 16), quality)["jpeg"]
    theirs = Image.open(io.BytesIO(_pillow(img, quality))).quantization                # natural order
    zz_inv = np.argsort(R.ZIGZAG)
    dqt = [(p[0], np.frombuffer(p[1:], np.uint8)[zz_inv]) for m, p in _segments(ours) if m == 0xDB]     # stored in zigzag order
    assert [i for i, _ in dqt] == [0, 1]
    for i, table in dqt:
        assert table.tolist() == list(theirs[i]), (quality, i)
    assert {k: list(v) for k, v in Image.open(io.BytesIO(ours)).quantization.items()} == {k: list(v) for k, v in theirs.items()}
    grey = R.encode(img[:, :, 0], (16, 16), quality)["jpeg"]
    assert [p for m, p in _segments(grey) if m == 0xDB] == [p for m, p in _segments(_pillow(img[:, :, 0], quality)) if m == 0xDB]


def test_huffman_tables_and_frame_header_are_pillows():
    for img in (R.natural(16, 24, 3), R.natural(16, 24, 1)):
        ours, theirs = _segments(R.encode(img, (24, 16), 70)["jpeg"]), _segments(_pillow(img, 70))      # (without `optimize`)
        assert b"".join(p for m, p in ours if m == 0xC4) == b"".join(p for m, p in theirs if m == 0xC4)  # one segment or several
        for marker in (0xE0, 0xC0, 0xDA):
            assert [p for m, p in ours if m == marker] == [p for m, p in theirs if m == marker], hex(marker)


def test_psnr_and_scan_length_against_pillows_encode(encoded):
    streams, _ = encoded
    assert R.GAP_PSNR_DB <= 0.5 and R.GAP_SCAN <= 0.03
    worst_db, worst_scan = -1.0, -1.0
    for h, w, c, wh, q in R.GAP_IMAGES:
        e = streams[f"natural_{w}x{h}_c{c}_q{q}"]
        d_db, d_scan, ours_db = R.gaps(e["jpeg"], e["resized"], q)
        print(f"{w}x{h} c{c} -> {wh[0]}x{wh[1]} q{q}: PSNR {ours_db:.3f} dB, Pillow's minus ours {d_db:+.3f} dB, scan bytes over Pillow's {100 * d_scan:+.2f} %")
        worst_db, worst_scan = max(worst_db, d_db), max(worst_scan, d_scan)
        assert d_db <= R.GAP_PSNR_DB and d_scan <= R.GAP_SCAN, (h, w, c, wh, q, d_db, d_scan)
    print(f"largest: {worst_db:+.3f} dB, {100 * worst_scan:+.2f} %")


def test_the_inputs_reach_every_hard_case(encoded):
    _, hard = encoded
    assert set(hard) <= set(R.HARD_CASES)
    assert all(hard.get(k, 0) > 0 for k in R.HARD_CASES), hard
    own = {}
    for name, img, wh, q in R.hard_inputs():                   # the shared inputs alone (what the GPU test encodes)
        R.encode(img, wh, q, own)
    assert all(own.get(k, 0) > 0 for k in R.HARD_CASES), own
    two = {}
    R.encode(R.hard_inputs()[4][1], (16, 16), 1, two)
    assert two["zrl"] == 8                                      # two ZRLs in a row in each of four blocks


def test_stage_shapes_capacity_and_the_unconfirmed_list(encoded):
    streams, _ = encoded
    e = streams["natural_1241x376_c3_q70"]
    g = e["g"]
    assert (g["yw"], g["yh"], g["cw"], g["ch"], g["blocks"]) == (640, 368, 320, 184, 5520)
    assert e["y"].shape == (368, 640) and e["cb"].shape == e["cr"].shape == (184, 320) and e["coef"].shape == (5520, 64)
    assert np.array_equal(e["y"][360:], np.repeat(e["y"][359:360], 8, 0))             # the last row replicated
    assert e["bitoff"][0] == 0 and np.all(np.diff(e["bitoff"]) >= 4) and e["bits"] > e["bitoff"][-1]
    assert len(e["jpeg"]) <= R.capacity(640, 360) == 623 + 416 * 5520 + 2
    assert len(R.UNCONFIRMED) >= 3 and any("resize" in u for u in R.UNCONFIRMED) and any("4:2:0" in u for u in R.UNCONFIRMED) \
        and any("APP0" in u for u in R.UNCONFIRMED)
    # the identity resize, and the ends of the tap table
    img = R.natural(9, 7, 3)
    assert np.array_equal(R.resize(img, (7, 9)), img)
    s0, s1, a0, a1 = R.resize_coords(23, 5)
    assert s0.min() == 0 and s1.max() == 4 and (a0 + a1 == 2048).all() and a1[0] == 0 and a1[-1] == 0
