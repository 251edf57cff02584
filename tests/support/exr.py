"""An independent restatement of the OpenEXR scan-line layout in numpy + zlib: a writer (with PIZ and PXR24 encoders) and a reader, which
the ExrInterface tests and the tools' end-to-end test hold the C++ reader / writer to."""
import struct
import zlib

import numpy as np


def attr(name, typ, payload):
    return name.encode() + b"\0" + typ.encode() + b"\0" + struct.pack("<i", len(payload)) + payload


# ---- PIZ and PXR24 ENCODERS, restated here from the published scheme (wavelet + LUT + Huffman with run-length symbol;
# ---- byte-plane delta + zlib).  Test infrastructure: the C++ reader has the decoders, nothing ships an encoder.

def _wenc14(a, b):
    as_ = a - 65536 if a >= 32768 else a
    bs = b - 65536 if b >= 32768 else b
    return ((as_ + bs) >> 1) & 0xFFFF, (as_ - bs) & 0xFFFF


def _wenc16(a, b):
    ao = (a + 0x8000) & 0xFFFF
    m = (ao + b) >> 1
    d = ao - b
    if d < 0:
        m = (m + 0x8000) & 0xFFFF
    return m, d & 0xFFFF


def _wav2_encode(a, base, nx, ox, ny, oy, mx):
    wenc = _wenc14 if mx < (1 << 14) else _wenc16
    n = min(nx, ny)
    p, p2 = 1, 2
    while p2 <= n:
        py, ey = base, base + oy * (ny - p2)
        oy1, oy2, ox1, ox2 = oy * p, oy * p2, ox * p, ox * p2
        while py <= ey:
            px, ex = py, py + ox * (nx - p2)
            while px <= ex:
                p01, p10 = px + ox1, px + oy1
                p11 = p10 + ox1
                i00, i01 = wenc(a[px], a[p01])
                i10, i11 = wenc(a[p10], a[p11])
                a[px], a[p10] = wenc(i00, i10)
                a[p01], a[p11] = wenc(i01, i11)
                px += ox2
            if nx & p:
                p10 = px + oy1
                i00, a[p10] = wenc(a[px], a[p10])
                a[px] = i00
            py += oy2
        if ny & p:
            px, ex = py, py + ox * (nx - p2)
            while px <= ex:
                p01 = px + ox1
                i00, a[p01] = wenc(a[px], a[p01])
                a[px] = i00
                px += ox2
        p, p2 = p2, p2 << 1


class _BitWriter:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0
        self.bits = 0

    def put(self, nbits, value):
        self.acc = (self.acc << nbits) | (value & ((1 << nbits) - 1))
        self.n += nbits
        self.bits += nbits
        while self.n >= 8:
            self.n -= 8
            self.out.append((self.acc >> self.n) & 0xFF)
        self.acc &= (1 << self.n) - 1

    def finish(self):
        if self.n:
            self.out.append((self.acc << (8 - self.n)) & 0xFF)
            self.acc = self.n = 0
        return bytes(self.out)


def _huf_compress_py(words):
    import heapq
    freq = {}
    for wv in words:
        freq[wv] = freq.get(wv, 0) + 1
    im, iM = min(freq), max(freq) + 1
    freq[iM] = 1                                        # the run-length pseudo-symbol
    # Huffman code lengths (any valid tree will do: the stream carries the lengths)
    heap = [(f, i, (s,)) for i, (s, f) in enumerate(sorted(freq.items()))]
    heapq.heapify(heap)
    length = {s: 0 for s in freq}
    cnt = len(heap)
    while len(heap) > 1:
        f1, _, s1 = heapq.heappop(heap)
        f2, _, s2 = heapq.heappop(heap)
        for x in s1 + s2:
            length[x] += 1
        heapq.heappush(heap, (f1 + f2, cnt, s1 + s2))
        cnt += 1
    assert max(length.values()) <= 58
    # canonical codes: longest codes first
    n = [0] * 59
    for l in length.values():
        n[l] += 1
    c = 0
    for i in range(58, 0, -1):
        nc = (c + n[i]) >> 1
        n[i] = c
        c = nc
    code = {}
    for s_ in sorted(length):
        code[s_] = n[length[s_]]
        n[length[s_]] += 1
    # packed table: 6-bit lengths with zero-run escapes
    tb = _BitWriter()
    s_ = im
    while s_ <= iM:
        l = length.get(s_, 0)
        if l == 0:
            run = 1
            while s_ + run <= iM and run < 255 + 6 and length.get(s_ + run, 0) == 0:
                run += 1
            if run >= 2:
                if run >= 6:
                    tb.put(6, 63)
                    tb.put(8, run - 6)
                else:
                    tb.put(6, 59 + run - 2)
                s_ += run
                continue
        tb.put(6, l)
        s_ += 1
    table = tb.finish()
    # data with run-length coding where it is shorter
    db = _BitWriter()

    def send(sym, run):
        if run and length[sym] + length[iM] + 8 < length[sym] * run:
            db.put(length[sym], code[sym])
            db.put(length[iM], code[iM])
            db.put(8, run)
        else:
            for _ in range(run + 1):
                db.put(length[sym], code[sym])

    cur, run = words[0], 0
    for wv in words[1:]:
        if wv == cur and run < 255:
            run += 1
        else:
            send(cur, run)
            cur, run = wv, 0
    send(cur, run)
    nbits = db.bits
    data = db.finish()
    return struct.pack("<IIIII", im, iM, len(table), nbits, 0) + table + data


def piz_compress_py(chan_rows):
    """chan_rows: list (channel order) of 2-D arrays (rows of this block) -> PIZ chunk payload"""
    words, layout = [], []
    for a in chan_rows:
        w16 = np.ascontiguousarray(a.astype(a.dtype.newbyteorder("<"))).view("<u2")     # (rows, width * size)
        size = a.dtype.itemsize // 2
        layout.append((len(words), a.shape[1], size, a.shape[0]))
        words.extend(int(x) for x in w16.reshape(-1))
    bitmap = bytearray(8192)
    for wv in set(words):
        bitmap[wv >> 3] |= 1 << (wv & 7)
    bitmap[0] &= ~1 & 0xFF
    nz = [i for i in range(8192) if bitmap[i]]
    min_nz, max_nz = (nz[0], nz[-1]) if nz else (8191, 0)
    lut, k = {}, 0
    for i in range(65536):
        if i == 0 or bitmap[i >> 3] & (1 << (i & 7)):
            lut[i] = k
            k += 1
    mx = k - 1
    words = [lut[wv] for wv in words]
    for start, nx, size, ny in layout:
        for j in range(size):
            _wav2_encode(words, start + j, nx, size, ny, nx * size, mx)
    huf = _huf_compress_py(words)
    out = struct.pack("<HH", min_nz, max_nz)
    if min_nz <= max_nz:
        out += bytes(bitmap[min_nz:max_nz + 1])
    return out + struct.pack("<i", len(huf)) + huf


def pxr24_compress_py(chan_rows):
    """byte planes of horizontally delta-coded samples, scan line by scan line, channel by channel; FLOAT as 24 bits"""
    out = bytearray()
    rows = chan_rows[0].shape[0]
    for y in range(rows):
        for a in chan_rows:
            if a.dtype == np.float16:
                v = a[y].view(np.uint16).astype(np.int64)
                d = np.diff(np.concatenate([[0], v])) & 0xFFFF
                planes = [(d >> 8) & 0xFF, d & 0xFF]
            elif a.dtype == np.float32:
                v = (a[y].view(np.uint32).astype(np.int64) >> 8)        # the caller passes values that fit 24 bits
                d = np.diff(np.concatenate([[0], v])) & 0xFFFFFF
                planes = [(d >> 16) & 0xFF, (d >> 8) & 0xFF, d & 0xFF]
            else:
                v = a[y].astype(np.int64)
                d = np.diff(np.concatenate([[0], v])) & 0xFFFFFFFF
                planes = [(d >> 24) & 0xFF, (d >> 16) & 0xFF, (d >> 8) & 0xFF, d & 0xFF]
            for pl in planes:
                out += pl.astype(np.uint8).tobytes()
    return zlib.compress(bytes(out))


def write_exr_py(path, chans, comp, x0=0, y0=0):
    """chans: dict name -> 2-D array (float16 / float32 / uint32).  comp: 0 none, 2 zips, 3 zip, 4 piz, 5 pxr24."""
    names = sorted(chans)
    h, w = chans[names[0]].shape
    tcode = {np.dtype("uint32"): 0, np.dtype("float16"): 1, np.dtype("float32"): 2}
    chl = b"".join(n.encode() + b"\0" + struct.pack("<iB3xii", tcode[chans[n].dtype], 0, 1, 1) for n in names) + b"\0"
    box = struct.pack("<4i", x0, y0, x0 + w - 1, y0 + h - 1)
    hdr = struct.pack("<ii", 20000630, 2) + attr("channels", "chlist", chl) + attr("compression", "compression", bytes([comp]))
    hdr += attr("dataWindow", "box2i", box) + attr("displayWindow", "box2i", box) + attr("lineOrder", "lineOrder", b"\0")
    hdr += attr("pixelAspectRatio", "float", struct.pack("<f", 1.0)) + attr("screenWindowCenter", "v2f", struct.pack("<2f", 0, 0))
    hdr += attr("screenWindowWidth", "float", struct.pack("<f", 1.0)) + b"\0"
    lpb = {3: 16, 4: 32, 5: 16}.get(comp, 1)
    nblk = (h + lpb - 1) // lpb
    chunks = []
    for b in range(nblk):
        rows = range(b * lpb, min(h, (b + 1) * lpb))
        raw = b"".join(chans[n][y].astype(chans[n].dtype.newbyteorder("<")).tobytes() for y in rows for n in names)
        if comp == 4:
            z = piz_compress_py([chans[n][rows.start:rows.stop] for n in names])
            data = z if len(z) < len(raw) else raw
        elif comp == 5:
            z = pxr24_compress_py([chans[n][rows.start:rows.stop] for n in names])
            data = z if len(z) < len(raw) else raw
        elif comp in (2, 3):
            a = np.frombuffer(raw, dtype=np.uint8)
            t = np.concatenate([a[0::2], a[1::2]]).astype(np.int32)
            p = t.copy()
            p[1:] = (t[1:] - t[:-1] + 128) & 0xFF
            z = zlib.compress(p.astype(np.uint8).tobytes())
            data = z if len(z) < len(raw) else raw
        else:
            data = raw
        chunks.append(struct.pack("<ii", y0 + b * lpb, len(data)) + data)
    pos = len(hdr) + 8 * nblk
    table = b""
    for c in chunks:
        table += struct.pack("<Q", pos)
        pos += len(c)
    open(path, "wb").write(hdr + table + b"".join(chunks))


def read_exr_py(path):
    d = open(path, "rb").read()
    assert struct.unpack_from("<i", d, 0)[0] == 20000630, "not an OpenEXR file: " + path
    p = 8
    info = {}
    while d[p] != 0:
        e = d.index(b"\0", p)
        name = d[p:e].decode()
        p = e + 1
        e = d.index(b"\0", p)
        p = e + 1
        size = struct.unpack_from("<i", d, p)[0]
        p += 4
        info[name] = d[p:p + size]
        p += size
    p += 1
    chans = []
    c = info["channels"]
    q = 0
    while c[q] != 0:
        e = c.index(b"\0", q)
        nm = c[q:e].decode()
        t = struct.unpack_from("<i", c, e + 1)[0]
        chans.append((nm, t))
        q = e + 1 + 16
    x0, y0, x1, y1 = struct.unpack("<4i", info["dataWindow"])
    w, h = x1 - x0 + 1, y1 - y0 + 1
    comp = info["compression"][0]
    lpb = 16 if comp == 3 else 1
    nblk = (h + lpb - 1) // lpb
    offs = struct.unpack_from("<%dQ" % nblk, d, p)
    sz = {0: 4, 1: 2, 2: 4}
    dt = {0: "<u4", 1: "<f2", 2: "<f4"}
    line = sum(w * sz[t] for _, t in chans)
    out = {n: np.zeros((h, w), dtype=np.float32) for n, _ in chans}
    for o in offs:
        yy, n = struct.unpack_from("<ii", d, o)
        data = d[o + 8:o + 8 + n]
        lines = min(lpb, y1 - yy + 1)
        if comp in (2, 3) and n != line * lines:
            t = np.frombuffer(zlib.decompress(data), dtype=np.uint8).astype(np.int32)
            t = (np.cumsum(t - 128) + 128) & 0xFF   # inverse predictor
            t = t.astype(np.uint8)
            half = (t.size + 1) // 2
            a = np.empty(t.size, dtype=np.uint8)
            a[0::2] = t[:half]
            a[1::2] = t[half:]
            data = a.tobytes()
        q = 0
        for l in range(lines):
            for nm, tt in chans:
                out[nm][yy - y0 + l] = np.frombuffer(data, dtype=dt[tt], count=w, offset=q).astype(np.float32)
                q += w * sz[tt]
    return out, comp
