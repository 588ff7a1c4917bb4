"""Numpy restatement of the keyframe-thumbnail pipeline (csrc/thumb_kernels.hip, csrc/thumb_plan.hpp): cv2.resize (INTER_LINEAR,
uint8) -> libjpeg's integer colour conversion and 4:2:0 subsampling -> an exactly defined integer forward DCT and quantisation ->
baseline Huffman coding with the Annex K tables -> the JFIF byte stream.  Every stage is a function of its own, so the GPU tests
compare stage by stage and then byte for byte.  `encode` also counts the coder's hard cases (`HARD_CASES`), so a test can show that
its inputs reach each of them.

UNCONFIRMED (cv2 is not installed where this was written; the items are restated from memory of OpenCV 4.x / libjpeg and compared
only with Pillow's libjpeg-turbo, see tests/test_thumb_ref.py):"""
import numpy as np

UNCONFIRMED = [
    "resize: the source coordinate (d + 0.5) * (src / dst) - 0.5 is taken in double and floored (OpenCV may hold it in float32)",
    "resize: an index below 0 or at / above src - 1 is clamped and its fraction set to 0",
    "resize: weights are float32 1 - f and f times 2048 rounded half to even to int16",
    "resize: the vertical pass is (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2 on horizontal sums at scale 2^11",
    "cv2.imencode's default chroma layout is 4:2:0 (OpenCV >= 4.7 has IMWRITE_JPEG_SAMPLING_FACTOR; its default is 4:2:0)",
    "APP0: JFIF 1.01, density units 0, Xdensity = Ydensity = 1, no thumbnail (what libjpeg writes by default; Pillow writes the same)",
    "the forward DCT is this file's own exact integer definition, not libjpeg's jfdctint: coefficients differ from cv2's by rounding",
]

MAX_DST, MAX_SRC = 4096, 16384

LUMA_Q = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                   14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                   49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64)
CHROMA_Q = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                     47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, np.int64)
# ZIGZAG[i] = natural (row-major) index of the i-th coefficient in zigzag order
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

DC_BITS = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
DC_VALS = (list(range(12)), list(range(12)))
AC_BITS = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119])
AC_VALS = (
    [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
     0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a,
     0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53,
     0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79,
     0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
     0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9,
     0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2,
     0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa],
    [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
     0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17,
     0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a,
     0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78,
     0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7,
     0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2,
     0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])

HARD_CASES = ("zrl", "coef63", "stuffed_ff", "dummy_row", "dummy_col", "eob_only", "dc_cat11", "ac_cat10")
BLOCK_BYTES = 416            # 2 * ceil((20 + 63 * 26) / 8): the worst block, every byte stuffed
STAGES = {"resized": 0, "y": 1, "cb": 2, "cr": 3, "coef": 4, "bitoff": 5}


def check_create(max_src_w, max_src_h, dst_w, dst_h, quality):
    """The refusals of thumb_plan.hpp's thumb_check_create -> message or None."""
    if not 1 <= quality <= 100:
        return f"quality {quality} outside 1..100"
    if not (1 <= dst_w <= MAX_DST and 1 <= dst_h <= MAX_DST):
        return f"thumbnail size {dst_w}x{dst_h} outside 1..{MAX_DST}"
    if not (1 <= max_src_w <= MAX_SRC and 1 <= max_src_h <= MAX_SRC):
        return f"source size {max_src_w}x{max_src_h} outside 1..{MAX_SRC}"
    return None


def check_image(ws, hs, c, max_w, max_h):
    if c not in (1, 3, 4):
        return f"{c} channels (want 1, 3 or 4)"
    if not (1 <= ws <= MAX_SRC and 1 <= hs <= MAX_SRC):
        return f"source size {ws}x{hs} outside 1..{MAX_SRC}"
    if ws > max_w or hs > max_h:
        return f"source {ws}x{hs} is larger than the instance's {max_w}x{max_h}"
    return None


# ---------------------------------------------------------------------------------------------------------------- resize
def resize_coords(dst, src):
    """-> (index int64 [dst], second index, weight of the first int64, weight of the second): taps of one axis."""
    d = np.arange(dst, dtype=np.float64)
    f = (d + 0.5) * (np.float64(src) / np.float64(dst)) - 0.5
    s = np.floor(f)
    f = f - s
    s = s.astype(np.int64)
    lo, hi = s < 0, s >= src - 1
    f = np.where(lo | hi, 0.0, f)
    s = np.where(lo, 0, np.where(hi, src - 1, s))
    f32 = f.astype(np.float32)
    a1 = np.rint(f32 * np.float32(2048)).astype(np.int64)
    a0 = np.rint((np.float32(1) - f32) * np.float32(2048)).astype(np.int64)
    return s, np.minimum(s + 1, src - 1), a0, a1


def resize(img, wh):
    """cv2.resize(img, (w, h)) for uint8, INTER_LINEAR; every channel (an alpha plane included) is interpolated."""
    w, h = wh
    img = np.asarray(img)
    src = img.reshape(img.shape[0], img.shape[1], -1).astype(np.int64)
    x0, x1, a0, a1 = resize_coords(w, src.shape[1])
    y0, y1, b0, b1 = resize_coords(h, src.shape[0])
    hor = src[:, x0] * a0[None, :, None] + src[:, x1] * a1[None, :, None]           # [Hs, w, C] at scale 2^11
    out = (((b0[:, None, None] * (hor[y0] >> 4)) >> 16) + ((b1[:, None, None] * (hor[y1] >> 4)) >> 16) + 2) >> 2
    out = np.clip(out, 0, 255).astype(np.uint8)
    return out[:, :, 0] if img.ndim == 2 else out


# ------------------------------------------------------------------------------------------------- geometry and planes
def geometry(w, h, c):
    """c: channels of the SOURCE (1: one component, 8 x 8 MCUs; 3 / 4: Y Cb Cr at 4:2:0, 16 x 16 MCUs)."""
    ncomp = 1 if c == 1 else 3
    mcu = 8 if ncomp == 1 else 16
    mcux, mcuy = -(-w // mcu), -(-h // mcu)
    g = dict(w=w, h=h, ncomp=ncomp, mcu=mcu, mcux=mcux, mcuy=mcuy, yw=mcux * mcu, yh=mcuy * mcu, bw=-(-w // 8), bh=-(-h // 8))
    g["cw"], g["ch"] = (0, 0) if ncomp == 1 else (mcux * 8, mcuy * 8)
    g["blocks"] = mcux * mcuy * (1 if ncomp == 1 else 6)
    return g


def is_dummy(g, bx, by):
    """a Y block (in 8-pixel units of the padded plane) wholly beyond the image's own block grid"""
    return bx >= g["bw"] or by >= g["bh"]


def block_info(g, b):
    """scan-order block b -> (component, bx, by, dummy, bx / by of the block whose DC a dummy carries, preceding block of the
    same component or -1)"""
    if g["ncomp"] == 1:
        return 0, b % g["mcux"], b // g["mcux"], False, b % g["mcux"], b // g["mcux"], b - 1
    m, i = divmod(b, 6)
    mx, my = m % g["mcux"], m // g["mcux"]
    if i >= 4:
        return i - 3, mx, my, False, mx, my, (b - 6 if m else -1)
    bx, by = 2 * mx + (i & 1), 2 * my + (i >> 1)
    j = i
    while is_dummy(g, 2 * mx + (j & 1), 2 * my + (j >> 1)):
        j -= 1                                               # (block 0 of an MCU is never a dummy)
    prev = b - 1 if i else (b - 3 if m else -1)
    return 0, bx, by, j != i, 2 * mx + (j & 1), 2 * my + (j >> 1), prev


def planes(small, g):
    """small: the resized image [h, w] or [h, w, 3 | 4] in cv2's B G R (A) order -> (Y [yh, yw], Cb, Cr [ch, cw] or None)."""
    a = np.asarray(small)
    a = a.reshape(a.shape[0], a.shape[1], -1).astype(np.int64)
    a = np.pad(a, ((0, g["yh"] - g["h"]), (0, g["yw"] - g["w"]), (0, 0)), mode="edge")
    if g["ncomp"] == 1:
        return a[:, :, 0].astype(np.uint8), None, None
    B, G, R = a[:, :, 0], a[:, :, 1], a[:, :, 2]
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16

    def sub(p):
        s = p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
        bias = 1 + (np.arange(s.shape[1]) & 1)                # 1, 2, 1, 2 along a row
        return ((s + bias[None, :]) >> 2).astype(np.uint8)
    return Y.astype(np.uint8), sub(Cb), sub(Cr)


# --------------------------------------------------------------------------------------------------- DCT and quantisation
def dct_matrix():
    k, n = np.mgrid[0:8, 0:8]
    ck = np.where(k == 0, 1 / np.sqrt(2.0), 1.0)
    return np.rint(8192.0 * ck / 2 * np.cos((2 * n + 1) * k * np.pi / 16)).astype(np.int64)


def quant_tables(quality):
    """libjpeg's jpeg_quality_scaling + jpeg_add_quant_table (force_baseline) -> (luma, chroma) int64 [64], natural order."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((t * s + 50) // 100, 1, 255) for t in (LUMA_Q, CHROMA_Q))


def coefficients(Y, Cb, Cr, g, quality):
    """-> int16 [blocks, 64]: zigzag order, blocks in scan order, dummy blocks by the dummy-block rule."""
    M = dct_matrix()
    ql, qc = quant_tables(quality)
    out = np.zeros((g["blocks"], 64), np.int16)
    pl = (Y, Cb, Cr)
    for b in range(g["blocks"]):
        comp, bx, by, dummy, sx, sy, _ = block_info(g, b)
        B = pl[comp][8 * sy:8 * sy + 8, 8 * sx:8 * sx + 8].astype(np.int64) - 128
        D = (M @ B @ M.T).reshape(64)
        Q = ql if comp == 0 else qc
        q = np.sign(D) * ((np.abs(D) + (Q << 25)) // (Q << 26))
        if dummy:
            q[1:] = 0
        out[b] = q[ZIGZAG]
    return out


# ---------------------------------------------------------------------------------------------------------- entropy coding
def huff_codes(bits, vals):
    """Annex C: -> {symbol: (code, length)}"""
    out, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            out[vals[k]] = (code, ln)
            code += 1
            k += 1
        code <<= 1
    return out


DC_CODES = tuple(huff_codes(b, v) for b, v in zip(DC_BITS, DC_VALS))
AC_CODES = tuple(huff_codes(b, v) for b, v in zip(AC_BITS, AC_VALS))


def _cat_bits(v):
    cat = int(abs(v)).bit_length()
    return cat, (v if v >= 0 else v - 1) & ((1 << cat) - 1)


def block_code(z, diff, tsel, hard=None):
    """z: the block's 64 zigzag coefficients, diff: its DC difference -> (code as an int, length in bits)."""
    hard = hard if hard is not None else {}
    cat, vb = _cat_bits(diff)
    c, ln = DC_CODES[tsel][cat]
    code, n = (c << cat) | vb, ln + cat
    if cat == 11:
        hard["dc_cat11"] = hard.get("dc_cat11", 0) + 1
    run = 0
    nz = np.flatnonzero(z[1:]) + 1
    last = 0
    for i in nz:
        run = int(i) - 1 - last
        last = int(i)
        while run > 15:
            c, ln = AC_CODES[tsel][0xF0]
            code, n = (code << ln) | c, n + ln
            run -= 16
            hard["zrl"] = hard.get("zrl", 0) + 1
        cat, vb = _cat_bits(int(z[i]))
        assert 1 <= cat <= 10
        if cat == 10:
            hard["ac_cat10"] = hard.get("ac_cat10", 0) + 1
        c, ln = AC_CODES[tsel][(run << 4) | cat]
        code, n = (((code << ln) | c) << cat) | vb, n + ln + cat
    if z[63] == 0:
        c, ln = AC_CODES[tsel][0x00]
        code, n = (code << ln) | c, n + ln
        if len(nz) == 0:
            hard["eob_only"] = hard.get("eob_only", 0) + 1
    else:
        hard["coef63"] = hard.get("coef63", 0) + 1
    return code, n


def entropy(coef, g, hard=None):
    """-> (bit offsets int64 [blocks] (exclusive), total bits, the unstuffed scan bytes, the last one padded with 1-bits)"""
    hard = hard if hard is not None else {}
    offs = np.zeros(g["blocks"], np.int64)
    acc, total = 0, 0
    for b in range(g["blocks"]):
        comp, bx, by, dummy, _, _, prev = block_info(g, b)
        if dummy:
            key = "dummy_row" if by >= g["bh"] else "dummy_col"
            hard[key] = hard.get(key, 0) + 1
        diff = int(coef[b, 0]) - (int(coef[prev, 0]) if prev >= 0 else 0)
        code, n = block_code(coef[b], diff, 0 if comp == 0 else 1, hard)
        offs[b] = total
        acc, total = (acc << n) | code, total + n
    pad = -total % 8
    acc = (acc << pad) | ((1 << pad) - 1)
    return offs, total, acc.to_bytes((total + pad) // 8, "big")


def stuff(scan, hard=None):
    if hard is not None:
        hard["stuffed_ff"] = hard.get("stuffed_ff", 0) + scan.count(b"\xff")
    return scan.replace(b"\xff", b"\xff\x00")


# -------------------------------------------------------------------------------------------------------------- the stream
def _seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def header(w, h, ncomp, quality):
    ql, qc = quant_tables(quality)
    out = b"\xff\xd8" + _seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    out += _seg(0xDB, bytes([0]) + bytes(ql[ZIGZAG].astype(np.uint8)))
    if ncomp == 3:
        out += _seg(0xDB, bytes([1]) + bytes(qc[ZIGZAG].astype(np.uint8)))
    comps = [(1, 0x22 if ncomp == 3 else 0x11, 0)] + ([(2, 0x11, 1), (3, 0x11, 1)] if ncomp == 3 else [])
    out += _seg(0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([ncomp]) + b"".join(bytes(c) for c in comps))
    for t in range(2 if ncomp == 3 else 1):
        out += _seg(0xC4, bytes([t]) + bytes(DC_BITS[t]) + bytes(DC_VALS[t]))
        out += _seg(0xC4, bytes([0x10 | t]) + bytes(AC_BITS[t]) + bytes(AC_VALS[t]))
    out += _seg(0xDA, bytes([ncomp]) + b"".join(bytes([i + 1, 0x11 if i else 0x00]) for i in range(ncomp)) + bytes([0, 63, 0]))
    return out


def capacity(w, h):
    """bytes no encode at this size can exceed (the colour layout: the larger of the two)"""
    return len(header(w, h, 3, 50)) + BLOCK_BYTES * geometry(w, h, 3)["blocks"] + 2


def encode(img, wh, quality, hard=None):
    """-> dict of every stage and `jpeg`: the whole byte stream.  `hard` (a dict) collects the hard-case counts."""
    img = np.asarray(img)
    c = 1 if img.ndim == 2 else img.shape[2]
    w, h = wh
    g = geometry(w, h, c)
    small = resize(img, wh)
    Y, Cb, Cr = planes(small, g)
    coef = coefficients(Y, Cb, Cr, g, quality)
    offs, total, scan = entropy(coef, g, hard)
    hdr = header(w, h, g["ncomp"], quality)
    jpeg = hdr + stuff(scan, hard) + b"\xff\xd9"
    assert len(jpeg) <= len(hdr) + BLOCK_BYTES * g["blocks"] + 2
    return dict(g=g, resized=small, y=Y, cb=Cb, cr=Cr, coef=coef, bitoff=offs, bits=total, scan=scan, header=hdr, jpeg=jpeg)


# ------------------------------------------------------------------------------------------------------ the shared inputs
def hard_inputs():
    """[(name, image, (w, h), quality)]: small inputs that between them reach every hard case of the coder."""
    rng = np.random.default_rng(7)
    noise = rng.integers(0, 256, (24, 40, 3), dtype=np.uint8)
    noise[1::2] = 255 - noise[1::2]                                      # every second row inverted: energy up to coefficient 63
    yy, xx = np.mgrid[0:16, 0:16]
    pix = (((yy + xx) & 1) * 255).astype(np.uint8)                        # a one-pixel checker: coefficient 63, AC category 10
    yy, xx = np.mgrid[0:32, 0:48]
    sq = ((((yy >> 3) + (xx >> 3)) & 1) * 255).astype(np.uint8)           # 8 x 8 squares: DC differences of category 11
    return [("noise_rows_inverted_40x24", noise, (40, 24), 100),
            ("noise_rows_inverted_24x40", np.ascontiguousarray(noise.transpose(1, 0, 2)), (24, 40), 100),
            ("pixel_checker", pix, (16, 16), 100),
            ("square_checker", sq, (48, 32), 100),
            ("pixel_checker_q10", pix, (16, 16), 10),                     # few survivors, far apart: one ZRL per block
            ("pixel_checker_q1", pix, (16, 16), 1),                       # ... and two in a row
            ("constant_0", np.zeros((16, 16, 3), np.uint8), (16, 16), 70),
            ("constant_255", np.full((16, 16, 3), 255, np.uint8), (16, 16), 70)]


# ------------------------------------------------------------------------------------- measures against an independent codec
# Pillow (libjpeg-turbo) encodes the same resized pixels at the same quality and 4:2:0; both streams are decoded by Pillow.  A gap
# is what this pipeline COSTS against it: PSNR it loses, scan bytes it adds (where it is better the gap is negative).  The bounds
# tests/test_thumb_ref.py asserts are twice the largest gap measured over GAP_IMAGES when the arithmetic was written (DESIGN.md
# section 5 has the table): +0.084 dB on the 8 x 8 image (at most +0.009 dB on the others), +0.12 % of scan bytes (one byte in 805;
# the 8 x 8 image's scan is one byte SHORTER than Pillow's 17).  Inputs and arithmetic are deterministic, so the figures repeat.
GAP_PSNR_DB = 0.17           # PSNR to the resized source: Pillow's minus ours
GAP_SCAN = 0.0024            # entropy-coded bytes: ours over Pillow's, minus 1
# (source h, w, channels, thumbnail (w, h), quality)
GAP_IMAGES = [(8, 8, 3, (8, 8), 70), (60, 100, 3, (50, 30), 70), (60, 100, 1, (50, 30), 70), (60, 100, 3, (50, 30), 25),
              (60, 100, 3, (50, 30), 95), (17, 33, 3, (33, 17), 70), (376, 1241, 3, (640, 360), 70), (376, 1241, 1, (640, 360), 70)]


def natural(h, w, c, seed=0):
    """a smooth scene with sensor-like noise (a photograph's statistics, roughly), uint8 [h, w] or [h, w, c]"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    a = (128 + 60 * np.sin(xx / 7.0) + 50 * np.cos(yy / 5.0))[:, :, None] + rng.normal(0, 12, (h, w, max(c, 1))) + np.arange(max(c, 1)) * 10
    a = np.clip(a, 0, 255).astype(np.uint8)
    return a[:, :, 0] if c == 1 else a


def psnr(a, b):
    m = float(((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2).mean())
    return 10 * np.log10(255.0 ** 2 / m) if m else 99.0


def scan_length(jpeg):
    """bytes between the SOS segment and EOI"""
    i = jpeg.index(b"\xff\xda")
    return len(jpeg) - (i + 2 + int.from_bytes(jpeg[i + 2:i + 4], "big")) - 2


def as_rgb(small):
    """cv2's B G R (A) or grey -> what Pillow calls the same picture"""
    small = np.asarray(small)
    return small if small.ndim == 2 else np.ascontiguousarray(small[:, :, 2::-1])


def pillow_jpeg(small, quality):
    import io
    from PIL import Image
    buf = io.BytesIO()
    rgb = as_rgb(small)
    # (a grey image has one component and no subsampling; asked for 4:2:0 Pillow would write sampling factors 2 x 2 for it)
    Image.fromarray(rgb).save(buf, "JPEG", quality=quality, **({} if rgb.ndim == 2 else {"subsampling": 2}))
    return buf.getvalue()


def decode(jpeg):
    import io
    from PIL import Image
    im = Image.open(io.BytesIO(jpeg))
    im.load()
    return im


def gaps(jpeg, small, quality):
    """-> (PSNR of Pillow's encode minus ours, our scan bytes over Pillow's minus 1, our PSNR) for one stream of `small`"""
    theirs = pillow_jpeg(small, quality)
    ref = as_rgb(small)
    ours_db, theirs_db = psnr(np.asarray(decode(jpeg)), ref), psnr(np.asarray(decode(theirs)), ref)
    return theirs_db - ours_db, scan_length(jpeg) / scan_length(theirs) - 1, ours_db
