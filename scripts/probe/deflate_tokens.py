"""What the inflate has to walk (host only): literals, matches, match lengths and codes longer than
the 11-bit primary table in one synthetic 480 x 640 depth map as a bare zlib stream of its u16
samples (a .sens depth frame) and as the IDAT payload of the PNG PIL writes of it, both at level 6.
usage: python scripts/probe/deflate_tokens.py [frame]"""
import io
import os
import sys
import zlib

from PIL import Image

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


class Bits:
    def __init__(self, data):
        self.d, self.p = data + b"\0" * 16, 0

    def get(self, n):
        i = self.p >> 3
        r = (int.from_bytes(self.d[i:i + 8], "little") >> (self.p & 7)) & ((1 << n) - 1)
        self.p += n
        return r


def build(lens):
    """canonical code (RFC 1951 3.2.2) -> {(length, code): symbol}"""
    cnt = [0] * 16
    for n in lens:
        cnt[n] += 1
    cnt[0] = 0
    nxt, c = [0] * 16, 0
    for b in range(1, 16):
        c = (c + cnt[b - 1]) << 1
        nxt[b] = c
    codes = {}
    for s, n in enumerate(lens):
        if n:
            codes[(n, nxt[n])] = s
            nxt[n] += 1
    return codes


def symbol(br, codes):
    c = 0
    for n in range(1, 16):
        c = (c << 1) | br.get(1)
        if (n, c) in codes:
            return codes[(n, c)], n
    raise ValueError("no such code")


def stats(z):
    br = Bits(z[2:])
    st = dict(blocks=0, stored_bytes=0, literals=0, matches=0, match_bytes=0, codes_over_11_bits=0)
    last = 0
    while not last:
        last, kind = br.get(1), br.get(2)
        st["blocks"] += 1
        if kind == 0:
            br.p = (br.p + 7) & ~7
            n = br.get(16)
            br.p += 16 + 8 * n
            st["stored_bytes"] += n
            continue
        if kind == 1:
            lit, dist = build([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), build([5] * 30)
        else:
            nl, nd, nc = br.get(5) + 257, br.get(5) + 1, br.get(4) + 4
            cl = [0] * 19
            for i in range(nc):
                cl[[16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15][i]] = br.get(3)
            cc, lens = build(cl), []
            while len(lens) < nl + nd:
                s, _ = symbol(br, cc)
                if s < 16:
                    lens.append(s)
                elif s == 16:
                    lens += [lens[-1]] * (3 + br.get(2))
                else:
                    lens += [0] * ((3 + br.get(3)) if s == 17 else (11 + br.get(7)))
            lit, dist = build(lens[:nl]), build(lens[nl:])
        while True:
            s, n = symbol(br, lit)
            st["codes_over_11_bits"] += n > 11
            if s == 256:
                break
            if s < 256:
                st["literals"] += 1
                continue
            length = LEN_BASE[s - 257] + br.get(LEN_EXTRA[s - 257])
            d, n = symbol(br, dist)
            st["codes_over_11_bits"] += n > 11
            br.get(DIST_EXTRA[d])
            st["matches"] += 1
            st["match_bytes"] += length
    return st


def main():
    from scripts.sens_bench import depth_images
    img = depth_images(2)[int(sys.argv[1]) if len(sys.argv) > 1 else 1]
    raw = img.tobytes()
    z = zlib.compress(raw, 6)
    b = io.BytesIO()
    Image.fromarray(img).save(b, format="PNG", compress_level=6)
    png = b.getvalue()
    pos, idat = 8, b""
    while pos < len(png):
        n = int.from_bytes(png[pos:pos + 4], "big")
        if png[pos + 4:pos + 8] == b"IDAT":
            idat += png[pos + 8:pos + 8 + n]
        pos += 12 + n
    assert zlib.decompress(z) == raw
    for name, s in (("bare zlib stream of the u16 samples", z), ("PNG IDAT payload (PIL, adaptive filters)", idat)):
        st = stats(s)
        tok = st["literals"] + st["matches"]
        print(f"{name}: {len(s)} bytes, {tok} tokens, {st}, "
              f"mean match {st['match_bytes'] / max(st['matches'], 1):.1f} bytes", flush=True)


if __name__ == "__main__":
    main()
