"""numpy statement of the baseline JPEG encode (csrc/jpeg_enc_math.h) and a Python writer of the file (csrc/jpeg_enc_host.h):
libjpeg's default encoder - jccolor, jcsample without smoothing, jfdctint, jcdctmgr, jccoefct's dummy blocks, jchuff with the
Annex K.3 tables.  tests/test_jpeg_enc_host.py pins it to PIL's files byte for byte (g20_jpeg_enc.npz, and live PIL when it
imports); the GPU tests and the tight-allocation tool compare the kernels with it."""
import numpy as np

S444, S422, S420 = 0, 1, 2
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
BASE_QT = np.array([
    [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99],
    [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32])
DC_COUNTS = [[0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]]
DC_SYMBOLS = list(range(12))
AC_COUNTS = [[0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]]
AC_SYMBOLS = [
    [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa],
    [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa]]
assert all(len(s) == 162 and sorted(s) == sorted([0x00, 0xf0] + [r * 16 + v for r in range(16) for v in range(1, 11)]) for s in AC_SYMBOLS)


def to8b(x, divisor=None):
    """the reference's to8b: (255 * np.clip(x, 0, 1)).astype(np.uint8) of x [/ divisor]; NaN gives 0"""
    x = np.asarray(x, np.float32)
    if divisor:
        x = x / np.float32(divisor)
    with np.errstate(invalid="ignore"):
        c = np.where(x > 0, np.where(x < 1, x, np.float32(1)), np.float32(0)).astype(np.float32)
        return (np.float32(255) * c).astype(np.uint8)


def quant_tables(quality):
    quality = min(max(int(quality), 1), 100)
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((BASE_QT * scale + 50) // 100, 1, 255).astype(np.uint16)


def geometry(H, W, ncomp, sampling):
    """-> hs, vs, mx, my"""
    hs = 2 if ncomp == 3 and sampling != S444 else 1
    vs = 2 if ncomp == 3 and sampling == S420 else 1
    return hs, vs, -(-W // (8 * hs)), -(-H // (8 * vs))


def coef_count(H, W, ncomp, sampling):
    hs, vs, mx, my = geometry(H, W, ncomp, sampling)
    return 64 * mx * my * (hs * vs + (2 if ncomp == 3 else 0))


def planes(img, ncomp, sampling):
    """img: uint8 [H,W,3] (or [H,W] / [H,W,1]: R = G = B) -> the padded uint8 planes, [Y] or [Y, Cb, Cr]"""
    img = np.asarray(img)
    if img.ndim == 2:
        img = img[..., None]
    H, W = img.shape[:2]
    hs, vs, mx, my = geometry(H, W, ncomp, sampling)
    rgb = np.repeat(img, 3, -1) if img.shape[-1] == 1 else img[..., :3]
    r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
    if ncomp == 1:
        full = [img[..., 0].astype(np.int64)]
    else:
        full = [(19595 * r + 38470 * g + 7471 * b + 32768) >> 16,
                (-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16,
                (32768 * r - 27439 * g - 5329 * b + 8388608 + 32767) >> 16]
    out = []
    for c, p in enumerate(full):
        p = np.pad(p, ((0, (-H) % vs), (0, mx * hs * 8 - W)), mode="edge")        # columns in full, rows to a multiple of vs
        ph = my * vs * 8
        if c and (hs, vs) != (1, 1):
            x = np.arange(p.shape[1] // 2)
            if vs == 1:
                p = (p[:, 0::2] + p[:, 1::2] + (x & 1)) >> 1
            else:
                p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 1 + (x & 1)) >> 2
            ph = my * 8
        p = np.pad(p, ((0, ph - p.shape[0]), (0, 0)), mode="edge")                   # the rest of the rows AFTER the down-sampling
        out.append(p.astype(np.uint8))
    return out


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_1d(d, rows):
    """d: [..., 8] int64 -> [..., 8]"""
    s = 11 if rows else 15
    d = [d[..., k] for k in range(8)]
    t0, t1, t2, t3 = d[0] + d[7], d[1] + d[6], d[2] + d[5], d[3] + d[4]
    t7, t6, t5, t4 = d[0] - d[7], d[1] - d[6], d[2] - d[5], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = [None] * 8
    o[0] = (t10 + t11) << 2 if rows else _descale(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if rows else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2] = _descale(z1 + t13 * 6270, s)
    o[6] = _descale(z1 - t12 * 15137, s)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7], o[5], o[3], o[1] = _descale(t4 + z1 + z3, s), _descale(t5 + z2 + z4, s), _descale(t6 + z2 + z3, s), _descale(t7 + z1 + z4, s)
    return np.stack(o, -1)


def fdct(blocks):
    """blocks: [..., 8, 8] samples 0..255 -> [..., 8, 8] coefficients (8 x the DCT), natural order"""
    v = _fdct_1d(np.asarray(blocks, np.int64) - 128, True)
    return np.swapaxes(_fdct_1d(np.swapaxes(v, -1, -2), False), -1, -2)


def quantise(c, q):
    d = 8 * np.asarray(q, np.int64)
    return np.sign(c) * ((np.abs(c) + (d >> 1)) // d)


def coefficients(img, qt, ncomp, sampling):
    """img as planes() takes it, qt [2][64] natural order -> int16 [coef_count] in the layout of swnerf_jpeg_entropy"""
    img = np.asarray(img)
    H, W = img.shape[:2]
    hs, vs, mx, my = geometry(H, W, ncomp, sampling)
    qt = np.asarray(qt, np.int64).reshape(-1, 64)
    out = []
    for c, p in enumerate(planes(img, ncomp, sampling)):
        pby, pbx = p.shape[0] // 8, p.shape[1] // 8
        q = quantise(fdct(p.reshape(pby, 8, pbx, 8).transpose(0, 2, 1, 3)), qt[min(c, 1)].reshape(8, 8)).reshape(pby, pbx, 64)
        wc, hc = (W, H) if c == 0 else (-(-W // hs), -(-H // vs))
        rbx, rby = -(-wc // 8), -(-hc // 8)
        mw = hs if c == 0 else 1
        for by in range(pby):
            for bx in range(pbx):
                if by < rby and bx < rbx:
                    continue
                sy, sx = by, bx
                if by >= rby:
                    sy, sx = rby - 1, bx // mw * mw + mw - 1
                sx = min(sx, rbx - 1)
                dc = q[sy, sx, 0]
                q[by, bx] = 0
                q[by, bx, 0] = dc
        out.append(q.reshape(-1))
    return np.concatenate(out).astype(np.int16)


def _codes(counts, symbols):
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            table[symbols[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return table


class _Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, bits, length):
        self.acc = (self.acc << length) | (bits & ((1 << length) - 1))
        self.n += length
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 255
            self.out.append(b)
            if b == 255:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1


def _block(w, blk, pred, dc, ac):
    diff = int(blk[0]) - pred
    s = abs(diff).bit_length()
    w.put(*dc[s])
    if s:
        w.put(diff - 1 if diff < 0 else diff, s)
    run = 0
    for k in range(1, 64):
        v = int(blk[ZIGZAG[k]])
        if v == 0:
            run += 1
            continue
        while run > 15:
            w.put(*ac[0xF0])
            run -= 16
        s = abs(v).bit_length()
        w.put(*ac[run << 4 | s])
        w.put(v - 1 if v < 0 else v, s)
        run = 0
    if run:
        w.put(*ac[0])
    return int(blk[0])


def write(coef, qt, H, W, ncomp, sampling):
    """coef: int16 [coef_count], qt [2][64] natural order -> the bytes of the file"""
    hs, vs, mx, my = geometry(H, W, ncomp, sampling)
    qt = np.asarray(qt).reshape(-1, 64)
    tables = 2 if ncomp == 3 else 1
    o = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t in range(tables):
        o += b"\xff\xdb\x00\x43" + bytes([t]) + bytes(int(v) for v in qt[t][ZIGZAG])
    o += b"\xff\xc0" + (8 + 3 * ncomp).to_bytes(2, "big") + b"\x08" + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([ncomp])
    for c in range(ncomp):
        o += bytes([c + 1, 0x11 if c else hs << 4 | vs, 1 if c else 0])
    for t in range(tables):
        o += b"\xff\xc4" + (19 + 12).to_bytes(2, "big") + bytes([t]) + bytes(DC_COUNTS[t]) + bytes(DC_SYMBOLS)
        o += b"\xff\xc4" + (19 + 162).to_bytes(2, "big") + bytes([0x10 | t]) + bytes(AC_COUNTS[t]) + bytes(AC_SYMBOLS[t])
    o += b"\xff\xda" + (6 + 2 * ncomp).to_bytes(2, "big") + bytes([ncomp])
    for c in range(ncomp):
        o += bytes([c + 1, 0x11 if c else 0])
    o += b"\x00\x3f\x00"
    dc = [_codes(DC_COUNTS[t], DC_SYMBOLS) for t in range(2)]
    ac = [_codes(AC_COUNTS[t], AC_SYMBOLS[t]) for t in range(2)]
    n0, n1 = mx * hs * my * vs * 64, mx * my * 64
    coef = np.asarray(coef)
    plane = [coef[:n0].reshape(my * vs, mx * hs, 64)]
    if ncomp == 3:
        plane += [coef[n0:n0 + n1].reshape(my, mx, 64), coef[n0 + n1:].reshape(my, mx, 64)]
    w, pred = _Bits(), [0, 0, 0]
    for y in range(my):
        for x in range(mx):
            for c in range(ncomp):
                nh, nv = (hs, vs) if c == 0 else (1, 1)
                for v in range(nv):
                    for h in range(nh):
                        pred[c] = _block(w, plane[c][y * nv + v, x * nh + h], pred[c], dc[min(c, 1)], ac[min(c, 1)])
    if w.n:
        w.put(0x7F, 8 - w.n)
    return bytes(o + w.out + b"\xff\xd9")


def encode(img, quality, sampling, ncomp=3):
    """img: uint8 [H,W,3|4], [H,W,1] or [H,W] -> the bytes libjpeg writes at this quality and sampling"""
    img = np.asarray(img)
    qt = quant_tables(quality)
    return write(coefficients(img, qt, ncomp, sampling), qt, img.shape[0], img.shape[1], ncomp, sampling)


# ---- the fixtures of g20_jpeg_enc.npz (tests/golden/make_golden_jpeg_enc.py) -------------------------------------------------
SAMPLING_OF = {"444": S444, "422": S422, "420": S420, "gray": S444}
SUBSAMPLING_OF = {"444": "4:4:4", "422": "4:2:2", "420": "4:2:0", "gray": "4:4:4"}


def golden_files(g):
    """{name: the bytes of PIL's file}"""
    blob = g["files"]
    return {str(n): blob[o:o + l].tobytes() for n, (o, l) in zip(g["names"], g["offsets"])}


def golden_cases(g):
    """the single-frame fixtures: [(name, pixels - [H,W,3], or [H,W] for a grey file -, components, sampling name, quality)]"""
    out = []
    for n in (str(n) for n in g["names"]):
        if n.startswith(("stack_", "float_", "disp_")):
            continue
        hw, kind, s, q = n.split("_")
        px = g[f"px_{hw}_{kind}"]
        out.append((n, px[..., 1] if s == "gray" else px, 1 if s == "gray" else 3, s, int(q[1:])))
    return out


def tight_cases():
    """the inputs tools/tight_buffer_check_jpeg_enc.py runs on the GPU: (name, frames [2,H,W,c], sampling name)"""
    out = []
    for (H, W) in ((1, 1), (17, 23), (257, 9)):
        for s in ("420", "444"):
            for dtype in ("u8", "f32"):
                for c in (3, 4):
                    rng = np.random.default_rng(H * 1000 + W * 10 + c + (dtype == "u8"))
                    px = rng.integers(0, 256, (2, H, W, c), dtype=np.uint8) if dtype == "u8" else (rng.random((2, H, W, c), dtype=np.float32) * np.float32(1.5) - np.float32(0.25))
                    out.append((f"{H}x{W}_{s}_{dtype}_c{c}", px, s))
    return out
