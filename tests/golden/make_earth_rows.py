"""Generate tests/golden/reference/earth-map_rows64.png from raysnail's examples/earth-map.png.

usage: python tests/golden/make_earth_rows.py <path to examples/earth-map.png>

The whole map (1920x960 RGB, 1.3 MB) is too large a fixture, so the first ROWS rows are kept: the IDAT stream is
inflated, cut after ROWS filtered scanlines and deflated again under an IHDR with height ROWS. A scanline's
filter only looks at the rows above it, so the kept rows hold the encoder's own filter bytes (Sub, Up and Paeth
occur) and decode to the same pixels as in the full file.
"""
import os
import struct
import sys
import zlib

ROWS = 64
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference", "earth-map_rows64.png")


def chunk(t, d):
    return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xFFFFFFFF)


def main():
    data = open(sys.argv[1], "rb").read()
    pos, idat, hdr = 8, b"", None
    while pos < len(data):
        n = struct.unpack(">I", data[pos:pos + 4])[0]
        t = data[pos + 4:pos + 8]
        if t == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", data[pos + 8:pos + 21])
        elif t == b"IDAT":
            idat += data[pos + 8:pos + 8 + n]
        pos += 12 + n
    w, h, depth, ctype, comp, flt, interlace = hdr
    assert (depth, ctype, interlace) == (8, 2, 0) and h >= ROWS
    raw = zlib.decompress(idat)[:ROWS * (1 + 3 * w)]
    print("filter types in the kept rows:", sorted({raw[y * (1 + 3 * w)] for y in range(ROWS)}))
    png = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, ROWS, depth, ctype, comp, flt, interlace))
    png += chunk(b"IDAT", zlib.compress(raw, 9)) + chunk(b"IEND", b"")
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    open(OUT, "wb").write(png)
    print(OUT, len(png), "bytes")


if __name__ == "__main__":
    main()
