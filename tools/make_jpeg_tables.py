#!/usr/bin/env python
"""Write gscream_amd/jpeg_tables.json and gscream_amd/csrc/jpeg_tables.h: the constant tables of the baseline JPEG encoder
(gscream_amd/jpeg.py, gscream_amd/csrc/jpeg.hip; the rules are in include/gsraster.h, "JPEG encoding").

    python tools/make_jpeg_tables.py [--check]

    quant       the two base quantisation tables (Annex K.1 luminance, K.2 chrominance), natural order: read out of a file the
                installed PIL writes at quality 50, where libjpeg's scaling is the identity
    huffman     the four "typical" Huffman tables (Annex K.3: DC / AC, luminance / chrominance) as {bits[16], values}: read out of the
                DHT segments of the same file (optimize=False)
    zigzag      zigzag[i] = the natural (row-major) index of the i-th coefficient in coding order: computed
    dct         C[k][n] = rint(8192 s_k cos((2n + 1) k pi / 16)), s_0 = 1 / sqrt(8), s_k = 1 / 2: computed
The header also carries the canonical codes of the Huffman tables as code | length << 16 per symbol.
--check compares the committed files with what this would write and changes nothing."""
import io
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JSON_PATH = os.path.join(ROOT, "gscream_amd", "jpeg_tables.json")
HEADER_PATH = os.path.join(ROOT, "gscream_amd", "csrc", "jpeg_tables.h")


def zigzag():
    order = sorted(range(64), key=lambda i: (i // 8 + i % 8, (i // 8) if (i // 8 + i % 8) % 2 else (i % 8)))
    return order


def dct_matrix():
    return [[int(round(8192.0 * (1.0 / math.sqrt(8.0) if k == 0 else 0.5) * math.cos((2 * n + 1) * k * math.pi / 16.0))) for n in range(8)]
            for k in range(8)]


def segments(data):
    """(marker, payload) of every segment in front of the scan."""
    assert data[:2] == b"\xff\xd8"
    at, out = 2, []
    while True:
        assert data[at] == 0xFF
        marker, n = data[at + 1], int.from_bytes(data[at + 2:at + 4], "big")
        out.append((marker, data[at + 4:at + 2 + n]))
        at += 2 + n
        if marker == 0xDA:
            return out


def from_pil():
    from PIL import Image
    buf = io.BytesIO()
    Image.new("RGB", (16, 16)).save(buf, format="JPEG", quality=50, optimize=False, subsampling=0)
    zz = zigzag()
    quant, huffman = {}, {}
    for marker, p in segments(buf.getvalue()):
        if marker == 0xDB:
            while p:
                assert p[0] >> 4 == 0, "8-bit tables"
                nat = [0] * 64
                for i in range(64):
                    nat[zz[i]] = p[1 + i]
                quant[p[0] & 15] = nat
                p = p[65:]
        if marker == 0xC4:
            while p:
                bits = list(p[1:17])
                n = sum(bits)
                huffman[("dc", "ac")[p[0] >> 4] + str(p[0] & 15)] = {"bits": bits, "values": list(p[17:17 + n])}
                p = p[17 + n:]
    assert sorted(quant) == [0, 1] and sorted(huffman) == ["ac0", "ac1", "dc0", "dc1"]
    return {"quant": [quant[0], quant[1]], "huffman": huffman, "zigzag": zz, "dct": dct_matrix()}


def codes(table):
    """{symbol: (code, length)}: the canonical codes of a {bits, values} table (Annex C)."""
    out, code, at = {}, 0, 0
    for length in range(1, 17):
        for _ in range(table["bits"][length - 1]):
            out[table["values"][at]] = (code, length)
            code += 1
            at += 1
        code <<= 1
    return out


def rows(values, per, fmt="%d"):
    values = list(values)
    return ",\n".join("    " + ", ".join(fmt % v for v in values[i:i + per]) for i in range(0, len(values), per))


def header_text(t):
    parts = ["// jpeg_tables.h -- written by tools/make_jpeg_tables.py (do not edit): the constant tables of jpeg.hip.",
             "// Quantisation (natural order) and Huffman tables as the installed PIL writes them at quality 50, optimize=False (Annex K.1 .. K.3).",
             "#pragma once", "#include <stdint.h>", ""]
    for i, name in enumerate(("luminance", "chrominance")):
        parts += [f"static const uint8_t JPEG_QUANT_BASE_{i}[64] = {{  // {name}", rows(t["quant"][i], 8, "%3d"), "};"]
    parts += ["#define JPEG_ZIGZAG_LIST /* coding position -> natural index */ \\", rows(t["zigzag"], 8, "%2d").replace("\n", " \\\n"), "",
              "static const uint8_t JPEG_ZIGZAG[64] = { JPEG_ZIGZAG_LIST };"]
    flat = [v for row in t["dct"] for v in row]
    parts += ["#define JPEG_DCT_ROWS \\", rows(flat, 8, "%5d").replace("\n", " \\\n"), ""]
    for key in ("dc0", "ac0", "dc1", "ac1"):
        h = t["huffman"][key]
        parts += [f"static const uint8_t JPEG_{key.upper()}_BITS[16] = {{ {', '.join(map(str, h['bits']))} }};",
                  f"static const uint8_t JPEG_{key.upper()}_VALUES[{len(h['values'])}] = {{", rows(h["values"], 16, "0x%02x"), "};"]
    for key in ("dc0", "dc1"):
        c = codes(t["huffman"][key])
        parts += [f"#define JPEG_{key.upper()}_CODES \\", rows((c[s][0] | c[s][1] << 16 for s in range(12)), 6, "0x%06xu").replace("\n", " \\\n"), ""]
    for key in ("ac0", "ac1"):
        c = codes(t["huffman"][key])
        parts += [f"#define JPEG_{key.upper()}_CODES \\",
                  rows(((c[s][0] | c[s][1] << 16) if s in c else 0 for s in range(256)), 8, "0x%06xu").replace("\n", " \\\n"), ""]
    return "\n".join(parts) + "\n"


def json_text(t):
    return json.dumps(t, indent=None, separators=(", ", ": ")).replace('], "', '],\n "').replace('}, "', '},\n "') + "\n"


def main():
    import PIL
    t = from_pil()
    outputs = ((JSON_PATH, json_text(t)), (HEADER_PATH, header_text(t)))
    print(f"PIL {PIL.__version__}: {sum(len(h['values']) for h in t['huffman'].values())} Huffman symbols, 2 quantisation tables")
    if "--check" in sys.argv:
        bad = [p for p, text in outputs if not os.path.exists(p) or open(p).read() != text]
        print("differs: " + ", ".join(bad) if bad else "committed tables match")
        return 1 if bad else 0
    for p, text in outputs:
        with open(p, "w") as f:
            f.write(text)
        print("wrote", os.path.relpath(p, ROOT))
    return 0


if __name__ == "__main__":
    sys.exit(main())
