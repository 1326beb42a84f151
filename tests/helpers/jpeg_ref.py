"""numpy model of the device JPEG decoder (openibl_amd/csrc/jpeg.hip, jpeg_entropy.h): baseline JPEG from the
file's bytes to RGB with the arithmetic of libjpeg-turbo as Pillow uses it — T.81 F.2.2 entropy decoding, 8-bit
dequantisation, the "islow" integer IDCT, "fancy" chroma upsampling and the 16-bit fixed-point colour conversion.
The model has its own marker walk (nothing of openibl_amd is imported), reads the stream bit by bit and is the
specification the kernels are held to; tests/test_jpeg_decode_cpu.py holds it to the installed Pillow.

    decode(data) -> Decoded(rgb [H][W][3] uint8, status, coefs [per component: [bh][bw][64] int16, natural order])

status: 0 ok, 1 bad code, 2 coefficient overrun, 3 ran out of bytes, 4 restart marker missing or wrong (or data
left in front of the marker that ends a segment).  A damaged stream still yields pixels, from what was decoded."""
import io
from collections import namedtuple

import numpy as np

OK, BAD_CODE, OVERRUN, OUT_OF_BYTES, BAD_RESTART = 0, 1, 2, 3, 4
Decoded = namedtuple("Decoded", "rgb status coefs")

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20,
                   13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52,
                   45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


class _Stream:
    """What the model needs of a file: frame, tables, the scan's bytes."""

    def __init__(self, data):
        b = bytes(data)
        assert b[:2] == b"\xff\xd8", "not a JPEG"
        self.qt, self.dc, self.ac, self.dri = {}, {}, {}, 0
        pos = 2
        while True:
            assert b[pos] == 0xFF
            m = b[pos + 1]
            L = (b[pos + 2] << 8) | b[pos + 3]
            seg = b[pos + 4:pos + 2 + L]
            if m == 0xDB:
                while seg:
                    assert seg[0] >> 4 == 0
                    q = np.zeros(64, np.int32)
                    q[ZIGZAG] = np.frombuffer(seg[1:65], np.uint8)
                    self.qt[seg[0] & 15] = q
                    seg = seg[65:]
            elif m == 0xC4:
                while seg:
                    counts = list(seg[1:17])
                    n = sum(counts)
                    (self.ac if seg[0] >> 4 else self.dc)[seg[0] & 15] = (counts, list(seg[17:17 + n]))
                    seg = seg[17 + n:]
            elif m == 0xC0:
                assert seg[0] == 8
                self.H, self.W = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4]
                self.comps = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i])
                              for i in range(seg[5])]
            elif m == 0xDD:
                self.dri = (seg[0] << 8) | seg[1]
            elif m == 0xDA:
                assert seg[0] == len(self.comps)
                self.tables = [(seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15) for i in range(seg[0])]
                self.scan = b[pos + 2 + L:]
                return
            else:
                assert m not in (0xC1, 0xC2, 0xC9, 0xCA), "not baseline"
            pos += 2 + L


class _Bits:
    """The scan's bits, one at a time; FF 00 is the data byte FF; a marker or the end of the data ends the bits."""

    def __init__(self, data):
        self.d, self.pos, self.cur, self.left, self.starved = data, 0, 0, 0, False

    def bit(self):
        if self.left == 0:
            d, p = self.d, self.pos
            if p >= len(d) or (d[p] == 0xFF and (p + 1 >= len(d) or d[p + 1] != 0)):
                self.starved = True
                return 0
            self.cur, self.left = d[p], 8
            self.pos = p + (2 if d[p] == 0xFF else 1)
        self.left -= 1
        return (self.cur >> self.left) & 1

    def receive(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v

    def restart(self, k):
        """Discard to the byte boundary and take the marker RST(k mod 8); False if it is not there."""
        self.left = 0
        d, p = self.d, self.pos
        if p + 1 < len(d) and d[p] == 0xFF and d[p + 1] == 0xD0 + (k & 7):
            self.pos = p + 2
            return True
        return False

    def at_marker(self):
        d, p = self.d, self.pos
        return p >= len(d) or (d[p] == 0xFF and p + 1 < len(d) and d[p + 1] != 0)


def _codes(counts, values):
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            if k < len(values):
                table[(length, code)] = values[k]
            code, k = code + 1, k + 1
        code <<= 1
    return table


def _symbol(bits, table):
    code = 0
    for length in range(1, 17):
        code = (code << 1) | bits.bit()
        v = table.get((length, code))
        if v is not None:
            return v
    return -1


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def _block(bits, dc, ac, pred, out):
    s = _symbol(bits, dc)
    if s < 0 or s > 15:
        return BAD_CODE, pred
    pred += _extend(bits.receive(s), s)
    out[0] = np.int16(((pred + 32768) & 0xFFFF) - 32768)
    k = 1
    while k < 64:
        rs = _symbol(bits, ac)
        if rs < 0:
            return BAD_CODE, pred
        r, s = rs >> 4, rs & 15
        if s == 0:
            if r != 15:
                break
            k += 16
            continue
        k += r
        if k > 63:
            return OVERRUN, pred
        out[ZIGZAG[k]] = _extend(bits.receive(s), s)
        k += 1
    return OK, pred


def geometry(H, W, comps):
    """Per component (blocks across, blocks down) of the MCU-padded planes, and the MCU grid."""
    hm, vm = max(c[1] for c in comps), max(c[2] for c in comps)
    if len(comps) == 1:
        return [((W + 7) // 8, (H + 7) // 8)], (W + 7) // 8, (H + 7) // 8, 1, 1
    mx, my = -(-W // (8 * hm)), -(-H // (8 * vm))
    return [(mx * c[1], my * c[2]) for c in comps], mx, my, hm, vm


def entropy(s):
    """-> coefs (list per component of [bh][bw][64] int16, natural order), status."""
    dims, mx, my, hm, vm = geometry(s.H, s.W, s.comps)
    single = len(s.comps) == 1
    coefs = [np.zeros((bh, bw, 64), np.int16) for bw, bh in dims]
    dc = [_codes(*s.dc[t[0]]) for t in s.tables]
    ac = [_codes(*s.ac[t[1]]) for t in s.tables]
    bits = _Bits(s.scan)
    pred = [0] * len(s.comps)
    status, total = OK, mx * my
    for m in range(total):
        if s.dri and m and m % s.dri == 0:
            if bits.left >= 8 or not bits.restart(m // s.dri - 1):
                return coefs, BAD_RESTART
            pred = [0] * len(s.comps)
        for c, comp in enumerate(s.comps):
            h, v = (1, 1) if single else (comp[1], comp[2])
            for y in range(v):
                for x in range(h):
                    st, pred[c] = _block(bits, dc[c], ac[c], pred[c], coefs[c][(m // mx) * v + y, (m % mx) * h + x])
                    if st:
                        return coefs, st
        if bits.starved:
            return coefs, OUT_OF_BYTES
    bits.left = 0
    if not bits.at_marker():
        status = BAD_RESTART          # data left in front of the marker that ends the scan
    return coefs, status


# ---- IDCT ------------------------------------------------------------------------------------------------------
def _idct_pass(x, shift):
    """x [..., 8] int64 along the last axis -> the eight outputs, descaled by `shift`."""
    x0, x1, x2, x3, x4, x5, x6, x7 = [x[..., i] for i in range(8)]
    z1 = (x2 + x6) * 4433
    t2, t3 = z1 - x6 * 15137, z1 + x2 * 6270
    t0, t1 = (x0 + x4) << 13, (x0 - x4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    u0, u1, u2, u3 = x7, x5, x3, x1
    z1, z2, z3, z4 = u0 + u3, u1 + u2, u0 + u2, u1 + u3
    z5 = (z3 + z4) * 9633
    u0, u1, u2, u3 = u0 * 2446, u1 * 16819, u2 * 25172, u3 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    u0, u1, u2, u3 = u0 + z1 + z3, u1 + z2 + z4, u2 + z2 + z3, u3 + z1 + z4
    out = np.stack([t10 + u3, t11 + u2, t12 + u1, t13 + u0, t13 - u0, t12 - u1, t11 - u2, t10 - u3], -1)
    return (out + (1 << (shift - 1))) >> shift


def idct(coefs, q):
    """coefs [bh][bw][64] int16, q [64] (natural order) -> the plane [bh * 8][bw * 8] uint8."""
    bh, bw, _ = coefs.shape
    x = (coefs.astype(np.int64) * q.astype(np.int64)).reshape(bh, bw, 8, 8)
    ws = _idct_pass(x.swapaxes(-1, -2), 11).swapaxes(-1, -2)        # columns first
    px = np.clip(_idct_pass(ws, 18) + 128, 0, 255).astype(np.uint8)
    return px.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


# ---- upsampling and colour -------------------------------------------------------------------------------------
def _h2(t, r1, r2, shift):
    """Fancy horizontal doubling of rows t: out[2c] = (3 t[c] + t[c-1] + r1) >> shift, out[2c+1] with t[c+1], r2."""
    left = np.concatenate([t[:, :1], t[:, :-1]], 1)
    right = np.concatenate([t[:, 1:], t[:, -1:]], 1)
    out = np.empty((t.shape[0], t.shape[1] * 2), np.int64)
    out[:, 0::2] = (3 * t + left + r1) >> shift
    out[:, 1::2] = (3 * t + right + r2) >> shift
    return out


def upsample(plane, h, v, hm, vm, H, W):
    p = plane[:-(-H * v // vm), :-(-W * h // hm)].astype(np.int64)
    if (h, v) == (hm, vm):
        return p[:H, :W]
    if (hm // h, vm // v) == (2, 1):
        return _h2(p, 1, 2, 2)[:H, :W]
    assert (hm // h, vm // v) == (2, 2)
    up = np.concatenate([p[:1], p[:-1]], 0)
    down = np.concatenate([p[1:], p[-1:]], 0)
    t = np.empty((p.shape[0] * 2, p.shape[1]), np.int64)
    t[0::2], t[1::2] = 3 * p + up, 3 * p + down
    return _h2(t, 8, 7, 4)[:H, :W]


def colour(y, cb, cr):
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def decode(data):
    s = _Stream(data)
    coefs, status = entropy(s)
    _, _, _, hm, vm = geometry(s.H, s.W, s.comps)
    planes = [idct(c, s.qt[comp[3]]) for c, comp in zip(coefs, s.comps)]
    if len(planes) == 1:
        y = planes[0][:s.H, :s.W]
        return Decoded(np.stack([y, y, y], -1), status, coefs)
    full = [upsample(p, comp[1], comp[2], hm, vm, s.H, s.W) for p, comp in zip(planes, s.comps)]
    return Decoded(colour(*full), status, coefs)


# ---- the installed Pillow, for the tests that compare against it -------------------------------------------------
def make_image(seed, h, w, kind="smooth"):
    """Deterministic test content: 'smooth' gradients with a few edges, 'noise' uniform bytes, 'flat' one colour,
    'photo' low-pass noise over gradients."""
    rng = np.random.RandomState(seed)
    if kind == "noise":
        return rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    if kind == "flat":
        return np.broadcast_to(np.array([200, 60, 90], np.uint8), (h, w, 3)).copy()
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([128 + 100 * np.sin(xx / (3.0 + seed % 5) + c) * np.cos(yy / (4.0 + c)) for c in range(3)], -1)
    img[h // 3:h // 2, w // 4:w // 2] = rng.randint(0, 256, 3)
    if kind == "photo":
        img += rng.normal(0, 12, (h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def pil_encode(img, mode="RGB", **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img if mode != "L" else img[..., 0], mode).save(buf, "JPEG", **kw)
    return np.frombuffer(buf.getvalue(), np.uint8).copy()


def pil_decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(bytes(data))).convert("RGB"))
