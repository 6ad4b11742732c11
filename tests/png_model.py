"""The PNG encoder's format contract stated a second time, in numpy and plain Python, independent of
mvlm_amd/csrc/png_encode.hip and png_pack.cpp: filter, tokens, Huffman lengths, block header, block choice, segment framing,
file.  tests/test_png_model_cpu.py holds it against zlib and Pillow; the GPU tests hold the device's files against it byte for
byte.  Nothing here is shared with the code under test."""
from __future__ import annotations

import struct
import zlib

import numpy as np

SEGMENT = 32768
MAX_DIM = 4096
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)


def png_bound(height: int, width: int) -> int:
    """Bytes that hold any file of this size: per segment its length + 5 (stored header) + 5 (flush); per file the signature (8),
    IHDR (25), the IDAT framing (12), the zlib header (2), Adler-32 (4) and IEND (12)."""
    if not (1 <= height <= MAX_DIM and 1 <= width <= MAX_DIM):
        raise ValueError("png: height and width must be 1..4096")
    total = height * (1 + 3 * width)
    return total + 10 * ((total + SEGMENT - 1) // SEGMENT) + 63


# ---- filter (PNG specification, section 9) --------------------------------------------------------------------------------
def filter_rows(rgb: np.ndarray, filter_mode: int = -1) -> np.ndarray:
    """u8[H,W,3] -> the filtered stream u8[H,1+3W].  Adaptive (-1): per row the type with the smallest sum of
    b < 128 ? b : 256 - b over its filtered bytes, the lowest type on a tie."""
    H, W, _ = rgb.shape
    a = rgb.astype(np.int32).reshape(H, 3 * W)
    left = np.zeros_like(a)
    left[:, 3:] = a[:, :-3]
    up = np.zeros_like(a)
    up[1:] = a[:-1]
    ul = np.zeros_like(a)
    ul[1:, 3:] = a[:-1, :-3]
    p = left + up - ul
    pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - ul)
    paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
    cand = [((a - x) & 255).astype(np.uint8) for x in (np.zeros_like(a), left, up, (left + up) >> 1, paeth)]
    if filter_mode == -1:
        cost = np.stack([np.where(f < 128, f.astype(np.int64), 256 - f.astype(np.int64)).sum(axis=1) for f in cand])
        types = np.argmin(cost, axis=0)  # (the first minimum: the lowest type)
    elif 0 <= filter_mode <= 4:
        types = np.full(H, filter_mode)
    else:
        raise ValueError("png: filter_mode must be -1..4")
    out = np.empty((H, 1 + 3 * W), np.uint8)
    out[:, 0] = types
    for k in range(5):
        out[types == k, 1:] = cand[k][types == k]
    return out


# ---- tokens: literals and distance-1 matches ------------------------------------------------------------------------------
def tokenize(seg: np.ndarray):
    """A segment's bytes -> (positions, lengths): lengths[k] == 0 is the literal seg[positions[k]], otherwise a match of that
    length at distance 1.  A run's first byte is a literal; the rest is cut into pieces of 258 from the front; a piece of 3 or
    more is one match, a shorter one is literals."""
    n = len(seg)
    idx = np.arange(n)
    brk = np.ones(n, bool)
    brk[1:] = seg[1:] != seg[:-1]
    start = np.maximum.accumulate(np.where(brk, idx, 0))
    starts = np.flatnonzero(brk)
    ends = np.append(starts[1:], n)
    end = ends[np.cumsum(brk) - 1]
    k = idx - start
    rest = end - start - 1  # the bytes behind the run's first
    j = k - 1
    j0 = j // 258 * 258
    piece = np.minimum(258, rest - j0)
    literal = (k == 0) | (piece < 3)
    match = (k > 0) & (piece >= 3) & (j == j0)
    keep = literal | match
    return idx[keep], np.where(match, piece, 0)[keep]


def length_symbol(length: int):
    for c in range(28, -1, -1):
        if length >= LEN_BASE[c]:
            return 257 + c, LEN_EXTRA[c], length - LEN_BASE[c]
    raise AssertionError(length)


# ---- Huffman code lengths -------------------------------------------------------------------------------------------------
def unlimited_depths(freq):
    """Depth of every used symbol in the Huffman tree the two-queue construction builds: leaves ascending by (count, symbol) in
    one queue, internal nodes in creation order in the other, the smaller head first and the leaf on a tie."""
    order = sorted((f, s) for s, f in enumerate(freq) if f > 0)
    n = len(order)
    if n == 0:
        return {}
    if n == 1:
        return {order[0][1]: 1}
    weight = [f for f, _ in order]
    parent = [0] * (2 * n - 1)
    a, b = 0, n  # heads of the leaf queue and of the internal queue
    for node in range(n, 2 * n - 1):
        w = 0
        for _ in range(2):
            if a < n and (b >= node or weight[a] <= weight[b]):
                pick, a = a, a + 1
            else:
                pick, b = b, b + 1
            parent[pick] = node
            w += weight[pick]
        weight.append(w)
    depth = [0] * (2 * n - 1)
    for node in range(2 * n - 3, -1, -1):
        depth[node] = depth[parent[node]] + 1
    return {order[i][1]: depth[i] for i in range(n)}


def code_lengths(freq, limit: int):
    """Lengths limited to `limit` bits.  The tree's depths are counted per length with everything deeper counted at the limit;
    while the Kraft sum is too large one code leaves the limit and the deepest shorter code becomes two codes one bit longer.
    The counts are then dealt out over the symbols ascending by (count, symbol), the longest first."""
    depths = unlimited_depths(freq)
    lens = [0] * len(freq)
    if not depths:
        return lens
    count = [0] * (limit + 1)
    for d in depths.values():
        count[min(d, limit)] += 1
    total = sum(count[l] << (limit - l) for l in range(1, limit + 1))
    while total > (1 << limit):
        count[limit] -= 1
        for l in range(limit - 1, 0, -1):
            if count[l]:
                count[l] -= 1
                count[l + 1] += 2
                break
        total -= 1
    order = sorted((f, s) for s, f in enumerate(freq) if f > 0)
    l = limit
    for _, s in order:
        while count[l] == 0:
            l -= 1
        lens[s] = l
        count[l] -= 1
    return lens


def canonical_codes(lens):
    """RFC 1951 3.2.2, each code bit-reversed so that it can be written least significant bit first."""
    mx = max(lens) if lens else 0
    count = [0] * (mx + 2)
    for l in lens:
        if l:
            count[l] += 1
    nxt, code = [0] * (mx + 2), 0
    for l in range(1, mx + 1):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = [0] * len(lens)
    for s, l in enumerate(lens):
        if l:
            out[s] = int(format(nxt[l], f"0{l}b")[::-1], 2)
            nxt[l] += 1
    return out


FIXED_LENS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_CODES = canonical_codes(FIXED_LENS)


def rle_code_lengths(seq):
    """The literal/length lengths followed by the distance lengths as code-length symbols (sym, extra bits, extra value): a
    run of zeros is cut into pieces of 138 from the front, 18 for 11 and more, 17 for 3..10, single zeros below; a run of
    another value sends the value once, then pieces of 6 as 16, the value itself below 3."""
    out, i, n = [], 0, len(seq)
    while i < n:
        v, r = seq[i], 1
        while i + r < n and seq[i + r] == v:
            r += 1
        i += r
        if v == 0:
            while r >= 3:
                m = min(r, 138)
                out.append((18, 7, m - 11) if m >= 11 else (17, 3, m - 3))
                r -= m
        else:
            out.append((v, 0, 0))
            r -= 1
            while r >= 3:
                m = min(r, 6)
                out.append((16, 2, m - 3))
                r -= m
        out.extend([(v, 0, 0)] * r)
    return out


class BitWriter:
    def __init__(self):
        self.vals, self.lens = [], []

    def put(self, value, nbits):
        self.vals.append(int(value))
        self.lens.append(int(nbits))

    def extend(self, values, nbits):
        self.vals.extend(int(v) for v in values)
        self.lens.extend(int(b) for b in nbits)

    def nbits(self):
        return sum(self.lens)

    def tobytes(self) -> bytes:
        vals = np.asarray(self.vals, np.uint64)
        lens = np.asarray(self.lens, np.int64)
        off = np.concatenate(([0], np.cumsum(lens)))
        bits = np.zeros((int(off[-1]) + 7) // 8 * 8, np.uint8)
        for k in range(int(lens.max()) if len(lens) else 0):
            m = lens > k
            bits[off[:-1][m] + k] = (vals[m] >> np.uint64(k)) & np.uint64(1)
        return np.packbits(bits, bitorder="little").tobytes()


# ---- one segment ----------------------------------------------------------------------------------------------------------
def deflate_segment(seg: bytes, last: bool, info: dict | None = None) -> bytes:
    """One segment's DEFLATE bytes: one block (stored, fixed or dynamic: the form whose segment is smallest in bytes with its
    framing, that order on a tie); a compressed block that is not the image's last is followed by an empty stored block."""
    data = np.frombuffer(seg, np.uint8)
    n = len(data)
    pos, mlen = tokenize(data)
    ll_freq, d_freq = [0] * 286, [0] * 30
    syms, ebits, evals = [], [], []
    lit = data[pos]
    for p, m in zip(lit.tolist(), mlen.tolist()):
        if m == 0:
            syms.append(p), ebits.append(0), evals.append(0)
        else:
            s, eb, ev = length_symbol(m)
            syms.append(s), ebits.append(eb), evals.append(ev)
    for s in syms:
        ll_freq[s] += 1
    ll_freq[256] = 1
    n_match = int((mlen > 0).sum())
    d_freq[0] = n_match
    ll_lens = code_lengths(ll_freq, 15)
    d_len0 = 1 if n_match else 0
    hlit = max(257, max(s for s in range(286) if ll_lens[s]) + 1)
    cl_syms = rle_code_lengths(ll_lens[:hlit] + [d_len0])
    cl_freq = [0] * 19
    for s, _, _ in cl_syms:
        cl_freq[s] += 1
    cl_lens = code_lengths(cl_freq, 7)
    hclen = max(4, max(k for k in range(19) if cl_lens[CL_ORDER[k]]) + 1)
    header_bits = 3 + 14 + 3 * hclen + sum(cl_lens[s] + eb for s, eb, _ in cl_syms)
    dyn_bits = header_bits + sum(ll_lens[s] + eb for s, eb in zip(syms, ebits)) + n_match * 1 + ll_lens[256]
    fix_bits = 3 + sum(FIXED_LENS[s] + eb for s, eb in zip(syms, ebits)) + n_match * 5 + 7

    def framed(bits):
        return (bits + 7) // 8 if last else (bits + 3 + 7) // 8 + 4

    sizes = (n + 5, framed(fix_bits), framed(dyn_bits))
    kind = min(range(3), key=lambda k: (sizes[k], k))
    if info is not None:
        info.update(kind=kind, sizes=sizes, ll_lens=ll_lens, cl_lens=cl_lens, ll_freq=ll_freq, cl_freq=cl_freq,
                    n_tokens=len(syms))
    if kind == 0:
        return bytes([1 if last else 0]) + struct.pack("<HH", n & 0xFFFF, ~n & 0xFFFF) + bytes(seg)
    w = BitWriter()
    w.put(1 if last else 0, 1)
    if kind == 1:
        w.put(1, 2)
        lens, codes, dist_bits = FIXED_LENS, FIXED_CODES, 5
    else:
        w.put(2, 2)
        w.put(hlit - 257, 5), w.put(0, 5), w.put(hclen - 4, 4)
        for k in range(hclen):
            w.put(cl_lens[CL_ORDER[k]], 3)
        cl_codes = canonical_codes(cl_lens)
        for s, eb, ev in cl_syms:
            w.put(cl_codes[s] | (ev << cl_lens[s]), cl_lens[s] + eb)
        lens, codes, dist_bits = ll_lens, canonical_codes(ll_lens), 1
    lens_a, codes_a = np.asarray(lens, np.int64), np.asarray(codes, np.int64)
    s_a, eb_a, ev_a = np.asarray(syms, np.int64), np.asarray(ebits, np.int64), np.asarray(evals, np.int64)
    is_match = s_a > 256
    vals = codes_a[s_a] | (ev_a << lens_a[s_a])  # (the distance code is 0 in either form: zeros above the extra bits)
    nb = lens_a[s_a] + eb_a + np.where(is_match, dist_bits, 0)
    w.extend(vals, nb)
    w.put(codes[256], lens[256])
    if not last:
        w.put(0, 3)
        w.put(0, -w.nbits() % 8)
        w.put(0xFFFF0000, 32)
    out = w.tobytes()
    assert len(out) == sizes[kind], (len(out), sizes, kind)
    return out


# ---- file -----------------------------------------------------------------------------------------------------------------
def chunk(tag: bytes, body: bytes) -> bytes:
    return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body))


def encode(rgb: np.ndarray, filter_mode: int = -1, info: list | None = None):
    """u8[H,W,3] (or [H,W,4], alpha dropped) -> (file, filtered stream, the segments' DEFLATE bytes)."""
    rgb = np.ascontiguousarray(rgb[..., :3])
    H, W, _ = rgb.shape
    png_bound(H, W)
    stream = filter_rows(rgb, filter_mode).tobytes()
    segs = []
    for o in range(0, len(stream), SEGMENT):
        rec = {}
        segs.append(deflate_segment(stream[o:o + SEGMENT], o + SEGMENT >= len(stream), rec))
        if info is not None:
            info.append(rec)
    idat = b"\x78\x01" + b"".join(segs) + struct.pack(">I", zlib.adler32(stream))
    png = (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)) + chunk(b"IDAT", idat)
           + chunk(b"IEND", b""))
    return png, stream, segs


def idat_of(png: bytes) -> bytes:
    out, p = b"", 8
    while p < len(png):
        n, = struct.unpack(">I", png[p:p + 4])
        if png[p + 4:p + 8] == b"IDAT":
            out += png[p + 8:p + 8 + n]
        p += 12 + n
    return out
