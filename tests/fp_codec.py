"""A model of chromaprint 1.5's fingerprint codec (FingerprintCompressor / FingerprintDecompressor), written from the
format's description and independent of the product: a sequential encoder, a sequential decoder with its four refusals,
and the URL-safe unpadded base64 text form.  The tests hold the device codec against it byte for byte.

Format.  x[i] = item[i] ^ item[i-1], item[-1] = 0.  The set bits of x from bit 0 up, at 1-based positions p: gap = p - last
(last = 0, then the previous p); gap < 7 -> the normal symbol gap, gap >= 7 -> the normal symbol 7 and the exceptional symbol
gap - 7; behind the last set bit the normal symbol 0.  Bytes: [algorithm & 0xFF] [n >> 16] [n >> 8] [n], the normal symbols
(3 bits each, LSB first, little-endian bit string, ceil(3 S / 8) bytes), the exceptional ones (5 bits each, the same way,
ceil(5 E / 8) bytes), padding bits 0."""
import base64 as _b64

OK, SHORT_HEADER, NORMAL_ENDS, EXCEPTIONAL_ENDS, BIT_POSITION = 0, 1, 2, 3, 4

# the ten vectors of the format's description: (items, algorithm, bytes)
VECTORS = [
    ([], 0, [0, 0, 0, 0]),
    ([1], 0, [0, 0, 0, 1, 1]),
    ([7], 0, [0, 0, 0, 1, 73, 0]),
    ([1 << 6], 0, [0, 0, 0, 1, 7, 0]),
    ([1 << 8], 0, [0, 0, 0, 1, 7, 2]),
    ([1, 0], 0, [0, 0, 0, 2, 65, 0]),
    ([1, 1], 0, [0, 0, 0, 2, 1, 0]),
    ([1 << 31], 0, [0, 0, 0, 1, 7, 25]),
    ([0x80000001], 0, [0, 0, 0, 1, 57, 0, 24]),
]
SILENCE_ITEMS, SILENCE_ALGORITHM, SILENCE_TEXT = [627964279] * 3, 1, "AQAAA0mUaEkSRZEGAA"


def symbols(items):
    """The normal and the exceptional symbols of a fingerprint."""
    normal, exceptional, prev = [], [], 0
    for item in items:
        x, last = (int(item) ^ prev) & 0xFFFFFFFF, 0
        prev = int(item)
        for p in range(1, 33):
            if x >> (p - 1) & 1:
                gap, last = p - last, p
                if gap < 7:
                    normal.append(gap)
                else:
                    normal.append(7)
                    exceptional.append(gap - 7)
        normal.append(0)
    return normal, exceptional


def _pack(values, width):
    acc = 0
    for k, v in enumerate(values):
        acc |= v << (width * k)
    return acc.to_bytes((width * len(values) + 7) // 8, "little")


def compress(items, algorithm=1):
    n = len(items)
    assert n < 1 << 24
    normal, exceptional = symbols(items)
    return bytes([algorithm & 0xFF, n >> 16 & 0xFF, n >> 8 & 0xFF, n & 0xFF]) + _pack(normal, 3) + _pack(exceptional, 5)


def decompress(blob):
    """-> (items, algorithm, status); the items of a refused blob are []."""
    blob = bytes(blob)
    if len(blob) < 4:
        return [], (blob[0] if blob else 0), SHORT_HEADER
    algorithm, n = blob[0], blob[1] << 16 | blob[2] << 8 | blob[3]
    body = int.from_bytes(blob[4:], "little")
    available = 8 * (len(blob) - 4) // 3
    normal, zeros, j = [], 0, 0
    while zeros < n:
        if j >= available:
            return [], algorithm, NORMAL_ENDS
        normal.append(body >> (3 * j) & 7)
        zeros += normal[-1] == 0
        j += 1
    S, E = len(normal), sum(1 for s in normal if s == 7)
    start = 4 + (3 * S + 7) // 8
    if len(blob) - start < (5 * E + 7) // 8:
        return [], algorithm, EXCEPTIONAL_ENDS
    tail = int.from_bytes(blob[start:], "little")
    items, x, pos, e, prev = [], 0, 0, 0, 0
    for s in normal:
        if s == 0:
            prev ^= x
            items.append(prev)
            x, pos = 0, 0
            continue
        gap = s
        if s == 7:
            gap += tail >> (5 * e) & 31
            e += 1
        pos += gap
        if pos > 32:
            return [], algorithm, BIT_POSITION
        x |= 1 << (pos - 1)
    return items, algorithm, OK


def b64encode(data):
    return _b64.urlsafe_b64encode(bytes(data)).rstrip(b"=").decode()


def b64decode(text):
    """None for a character outside the alphabet or a length of 1 mod 4."""
    if isinstance(text, bytes):
        text = text.decode("latin-1")
    if len(text) % 4 == 1 or any(c not in "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789-_" for c in text):
        return None
    return _b64.urlsafe_b64decode(text + "=" * (-len(text) % 4))
