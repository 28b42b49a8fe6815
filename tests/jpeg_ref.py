"""numpy restatement of the baseline JPEG decode of mvlpt_amd/csrc/jpeg_core.h (libjpeg's integer arithmetic as Pillow drives it):
parser with the same routes, Huffman decode with the same status bits, jidctint "islow", fancy h2v1 / h2v2 upsampling, YCbCr -> RGB.
Written for clarity and for small images: the entropy decode is a Python loop over a bit string.  tests/test_jpeg_ref.py holds it `==`
against Pillow; the GPU tests hold each device stage against it."""
from __future__ import annotations

import numpy as np

(ROUTE_DEVICE, ROUTE_MALFORMED, ROUTE_FRAME, ROUTE_SCANS, ROUTE_COLOUR, ROUTE_SAMPLING, ROUTE_TABLES, ROUTE_RESTART,
 ROUTE_SIZE) = range(9)
ST_BAD_CODE, ST_COEF_INDEX, ST_ENDED_EARLY, ST_BAD_SIZE = 1, 2, 4, 8

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                   62, 63])


class Parsed:
    def __init__(self):
        self.route = ROUTE_MALFORMED
        self.height = self.width = self.components = self.h_samp = self.v_samp = self.restart_interval = self.n_segments = 0
        self.q = {}          # id -> int array [64], natural order
        self.huff = {}       # (class, id) -> (bits[17], vals)
        self.tq, self.td, self.ta = [], [], []
        self.segs = []       # (begin, end) of the entropy bytes of each restart segment

    @property
    def hs(self):
        return 1 if self.components == 1 else self.h_samp

    @property
    def vs(self):
        return 1 if self.components == 1 else self.v_samp

    @property
    def mcux(self):
        return -(-self.width // (8 * self.hs))

    @property
    def mcuy(self):
        return -(-self.height // (8 * self.vs))


def parse(blob: bytes) -> Parsed:
    p, n, P = blob, len(blob), Parsed()

    def verdict(route):
        P.route = route
        return P

    if n < 4 or p[0] != 0xFF or p[1] != 0xD8:
        return verdict(ROUTE_MALFORMED)
    pos, jfif, adobe, bad_tables, sof, q_wide = 2, False, False, False, None, set()
    comps = []
    while True:
        if pos + 2 > n or p[pos] != 0xFF:
            return verdict(ROUTE_MALFORMED)
        while pos < n and p[pos] == 0xFF:
            pos += 1
        if pos >= n:
            return verdict(ROUTE_MALFORMED)
        m = p[pos]
        pos += 1
        if m in (0, 1) or 0xD0 <= m <= 0xD9 or pos + 2 > n:
            return verdict(ROUTE_MALFORMED)
        ln = (p[pos] << 8) | p[pos + 1]
        if ln < 2 or pos + ln > n:
            return verdict(ROUTE_MALFORMED)
        s = p[pos + 2:pos + ln]
        if m == 0xE0:
            jfif = jfif or s[:5] == b"JFIF\0"
        elif m == 0xEE:
            adobe = adobe or (len(s) >= 12 and s[:5] == b"Adobe")
        elif m == 0xDB:
            while s:
                pq, t = s[0] >> 4, s[0] & 15
                need = 1 + (128 if pq else 64)
                if pq > 1 or t > 3 or len(s) < need:
                    return verdict(ROUTE_MALFORMED)
                if pq == 0:
                    q = np.zeros(64, np.int64)
                    q[ZIGZAG] = np.frombuffer(s[1:65], np.uint8)
                    P.q[t] = q
                    q_wide.discard(t)
                else:
                    P.q[t] = None
                    q_wide.add(t)
                s = s[need:]
        elif m == 0xC4:
            while s:
                if len(s) < 17:
                    return verdict(ROUTE_MALFORMED)
                tc, th = s[0] >> 4, s[0] & 15
                count = sum(s[1:17])
                if tc > 1 or th > 3 or count > 256 or len(s) < 17 + count:
                    return verdict(ROUTE_MALFORMED)
                if th < 2:
                    ok, code = True, 0
                    for l in range(1, 17):
                        code += s[l]
                        ok = ok and code <= (1 << l)
                        code <<= 1
                    vals = list(s[17:17 + count])
                    if tc == 0 and any(v > 15 for v in vals):
                        ok = False
                    if ok:
                        P.huff[(tc, th)] = ([0] + list(s[1:17]), vals)
                    else:
                        P.huff.pop((tc, th), None)
                        bad_tables = True
                s = s[17 + count:]
        elif m == 0xDD:
            if len(s) < 2:
                return verdict(ROUTE_MALFORMED)
            P.restart_interval = (s[0] << 8) | s[1]
        elif m == 0xDC:
            return verdict(ROUTE_SCANS)
        elif 0xC0 <= m <= 0xCF and m not in (0xC8, 0xCC):
            if sof is not None or len(s) < 6:
                return verdict(ROUTE_MALFORMED)
            sof, precision = m, s[0]
            P.height, P.width, nf = (s[1] << 8) | s[2], (s[3] << 8) | s[4], s[5]
            P.components = nf
            if len(s) < 6 + 3 * nf:
                return verdict(ROUTE_MALFORMED)
            comps = [(s[6 + 3 * c], s[7 + 3 * c] >> 4, s[7 + 3 * c] & 15, s[8 + 3 * c]) for c in range(min(nf, 4))]
            if comps:
                P.h_samp, P.v_samp = comps[0][1], comps[0][2]
        elif m == 0xDA:
            if sof is None or len(s) < 1:
                return verdict(ROUTE_MALFORMED)
            ns = s[0]
            if ns < 1 or ns > 4 or len(s) < 4 + 2 * ns:
                return verdict(ROUTE_MALFORMED)
            scan_c = [(s[1 + 2 * c], s[2 + 2 * c]) for c in range(ns)]
            ss, se, ahal = s[1 + 2 * ns], s[2 + 2 * ns], s[3 + 2 * ns]
            scan = pos + ln
            break
        pos += ln
    nf = P.components
    if sof != 0xC0 or precision != 8:
        return verdict(ROUTE_FRAME)
    if P.height <= 0 or P.width <= 0 or P.height * P.width > 1 << 26:
        return verdict(ROUTE_SIZE)
    if nf not in (1, 3):
        return verdict(ROUTE_COLOUR)
    if nf == 3:
        if adobe or (not jfif and [c[0] for c in comps] != [1, 2, 3]):
            return verdict(ROUTE_COLOUR)
        if (comps[0][1], comps[0][2]) not in ((1, 1), (2, 1), (2, 2)) or any((c[1], c[2]) != (1, 1) for c in comps[1:]):
            return verdict(ROUTE_SAMPLING)
    elif not (1 <= comps[0][1] <= 4 and 1 <= comps[0][2] <= 4):
        return verdict(ROUTE_MALFORMED)
    if ns != nf or ss != 0 or se != 63 or ahal != 0:
        return verdict(ROUTE_SCANS)
    for c in range(nf):
        if scan_c[c][0] != comps[c][0]:
            return verdict(ROUTE_SCANS)
        td, ta, tq = scan_c[c][1] >> 4, scan_c[c][1] & 15, comps[c][3]
        if td > 1 or ta > 1 or tq > 3 or bad_tables:
            return verdict(ROUTE_TABLES)
        if (0, td) not in P.huff or (1, ta) not in P.huff or P.q.get(tq) is None:
            return verdict(ROUTE_TABLES)
        P.tq.append(tq), P.td.append(td), P.ta.append(ta)
    i, seg_begin, expected, closed = scan, scan, 0, False
    while i < n:
        if p[i] != 0xFF:
            i += 1
            continue
        j = i
        while j < n and p[j] == 0xFF:
            j += 1
        if j >= n:
            break
        m = p[j]
        if m == 0:
            if j - i != 1:
                return verdict(ROUTE_RESTART)
            i = j + 1
            continue
        if 0xD0 <= m <= 0xD7:
            if m - 0xD0 != expected & 7:
                return verdict(ROUTE_RESTART)
            expected += 1
            P.segs.append((seg_begin, i))
            seg_begin = i = j + 1
            continue
        if m != 0xD9:
            return verdict(ROUTE_SCANS)
        P.segs.append((seg_begin, i))
        closed = True
        break
    if not closed:
        P.segs.append((seg_begin, n))
    P.n_segments = len(P.segs)
    mcus = P.mcux * P.mcuy
    want = -(-mcus // P.restart_interval) if P.restart_interval > 0 else 1
    return verdict(ROUTE_DEVICE if len(P.segs) == want else ROUTE_RESTART)


# ---------------------------------------------------------------------------------------------------- entropy decode
def _code_table(bits, vals):
    """{(length, code): symbol}"""
    table, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(bits[l]):
            table[(l, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return table


def _segment_bits(data: bytes) -> str:
    out, i, n = [], 0, len(data)
    while i < n:
        b = data[i]
        i += 1
        if b == 0xFF:
            if i < n and data[i] == 0:
                i += 1
            else:
                break            # a marker, or the file's last byte: the data stops here
        out.append(b)
    return "".join(f"{b:08b}" for b in out)


def extend(v, s):
    return v if v >= 1 << (s - 1) else v - (1 << s) + 1


def decode_coefficients(blob: bytes, P: Parsed):
    """([int16 [blocks_c, 64] natural order, raster over the component's whole-MCU block grid] per component, status)"""
    hs, vs, mcux, mcuy = P.hs, P.vs, P.mcux, P.mcuy
    shape = [(mcuy * (vs if c == 0 else 1), mcux * (hs if c == 0 else 1)) for c in range(P.components)]
    coefs = [np.zeros((h * w, 64), np.int16) for h, w in shape]
    dc = [_code_table(*P.huff[(0, t)]) for t in P.td]
    ac = [_code_table(*P.huff[(1, t)]) for t in P.ta]
    mcus, status = mcux * mcuy, 0
    restart = P.restart_interval if P.restart_interval > 0 else mcus

    class Stop(Exception):
        pass

    for s, (b, e) in enumerate(P.segs):
        bits = _segment_bits(blob[b:max(b, e)])
        real = len(bits)
        pos = 0

        def symbol(table):
            nonlocal pos, bits
            if len(bits) < pos + 32:
                bits = bits + "0" * 64
            for l in range(1, 17):
                sym = table.get((l, int(bits[pos:pos + l], 2)))
                if sym is not None:
                    pos += l
                    return sym
            raise Stop(ST_BAD_CODE)

        def receive(k):
            nonlocal pos
            v = int(bits[pos:pos + k], 2)
            pos += k
            return v

        pred = [0] * P.components
        try:
            for m in range(s * restart, min(mcus, (s + 1) * restart)):
                my, mx = divmod(m, mcux)
                for c in range(P.components):
                    hb, vb = (hs, vs) if c == 0 else (1, 1)
                    for by in range(vb):
                        for bx in range(hb):
                            blk = coefs[c][(my * vb + by) * shape[c][1] + mx * hb + bx]
                            k = symbol(dc[c])
                            if k > 15:
                                raise Stop(ST_BAD_SIZE)
                            if k:
                                pred[c] += extend(receive(k), k)
                            blk[0] = np.int64(pred[c]).astype(np.int16)
                            k = 1
                            while k < 64:
                                rs = symbol(ac[c])
                                run, size = rs >> 4, rs & 15
                                if size == 0:
                                    if run != 15:
                                        break
                                    k += 16
                                    continue
                                k += run
                                if k > 63:
                                    raise Stop(ST_COEF_INDEX)
                                blk[ZIGZAG[k]] = extend(receive(size), size)
                                k += 1
            if pos > real:
                status |= ST_ENDED_EARLY
        except Stop as stop:
            status |= stop.args[0]
    return coefs, status


# ---------------------------------------------------------------------------------------------------- IDCT
def _wrap32(x):
    return ((x + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def _idct_1d(v, shift):
    """jpeg_idct_islow, one pass along the last axis of an int64 array; 32-bit wrap where the C code shifts."""
    i0, i1, i2, i3, i4, i5, i6, i7 = [v[..., k] for k in range(8)]
    z1 = (i2 + i6) * 4433
    tmp2 = z1 - i6 * 15137
    tmp3 = z1 + i2 * 6270
    tmp0 = (i0 + i4) << 13
    tmp1 = (i0 - i4) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    t0, t1, t2, t3 = i7, i5, i3, i1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    rnd = 1 << (shift - 1)
    outs = [tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3]
    return np.stack([_wrap32(_wrap32(o) + rnd) >> shift for o in outs], axis=-1)


def idct_blocks(coefs, q):
    """coefs int [n, 64] natural order, q int [64] -> uint8 [n, 8, 8]"""
    x = (np.asarray(coefs, np.int64) * np.asarray(q, np.int64)).reshape(-1, 8, 8)
    x = _wrap32(x)
    ws = _idct_1d(x.transpose(0, 2, 1), 11).transpose(0, 2, 1)      # columns
    out = _idct_1d(ws, 18)                                          # rows
    return np.clip(out + 128, 0, 255).astype(np.uint8)


def planes_from_blocks(px, blocks_h, blocks_w):
    """uint8 [blocks_h * blocks_w, 8, 8] -> plane [blocks_h * 8, blocks_w * 8]"""
    return px.reshape(blocks_h, blocks_w, 8, 8).transpose(0, 2, 1, 3).reshape(blocks_h * 8, blocks_w * 8)


# ---------------------------------------------------------------------------------------------------- upsample + colour
def upsample(plane, cw, ch, hs, vs, W, H):
    """fancy upsampling of the component's real samples plane[:ch, :cw] to [H, W] (int64)"""
    c = plane[:ch, :cw].astype(np.int64)
    if hs == 1:
        return c[:H, :W]
    if cw <= 2:                                                      # jinit_upsampler: replicated when at most two samples wide
        return np.repeat(np.repeat(c, vs, axis=0), 2, axis=1)[:H, :W]
    left, right = np.concatenate([c[:, :1], c[:, :-1]], 1), np.concatenate([c[:, 1:], c[:, -1:]], 1)
    if vs == 1:
        out = np.empty((ch, 2 * cw), np.int64)
        out[:, 0::2] = (3 * c + left + 1) >> 2
        out[:, 1::2] = (3 * c + right + 2) >> 2
        out[:, 0], out[:, -1] = c[:, 0], c[:, -1]
        return out[:H, :W]
    above, below = np.concatenate([c[:1], c[:-1]], 0), np.concatenate([c[1:], c[-1:]], 0)
    rows = np.empty((2 * ch, cw), np.int64)
    rows[0::2], rows[1::2] = 3 * c + above, 3 * c + below
    left, right = np.concatenate([rows[:, :1], rows[:, :-1]], 1), np.concatenate([rows[:, 1:], rows[:, -1:]], 1)
    out = np.empty((2 * ch, 2 * cw), np.int64)
    out[:, 0::2] = (3 * rows + left + 8) >> 4
    out[:, 1::2] = (3 * rows + right + 7) >> 4
    out[:, 0], out[:, -1] = (4 * rows[:, 0] + 8) >> 4, (4 * rows[:, -1] + 7) >> 4
    return out[:H, :W]


def colour(planes, W, H, hs, vs):
    """component planes (whole MCUs) -> uint8 [H, W, 3]"""
    y = planes[0][:H, :W].astype(np.int64)
    if len(planes) == 1:
        return np.repeat(y[:, :, None], 3, axis=2).astype(np.uint8)
    cw, ch = -(-W // hs), -(-H // vs)
    cb = upsample(planes[1], cw, ch, hs, vs, W, H) - 128
    cr = upsample(planes[2], cw, ch, hs, vs, W, H) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


def decode_stages(blob: bytes):
    """(Parsed, coefficient blocks per component, planes per component, RGB [H, W, 3], status) of a device-route file"""
    P = parse(blob)
    if P.route != ROUTE_DEVICE:
        raise ValueError(f"route {P.route}: not a file the device decodes")
    coefs, status = decode_coefficients(blob, P)
    planes = []
    for c in range(P.components):
        bh, bw = P.mcuy * (P.vs if c == 0 else 1), P.mcux * (P.hs if c == 0 else 1)
        planes.append(planes_from_blocks(idct_blocks(coefs[c], P.q[P.tq[c]]), bh, bw))
    return P, coefs, planes, colour(planes, P.width, P.height, P.hs, P.vs), status


def decode(blob: bytes):
    """(RGB uint8 [H, W, 3], status)"""
    _, _, _, rgb, status = decode_stages(blob)
    return rgb, status
