// png_inflate_check -- the decoder core of gscream_amd/csrc/png_inflate.h on the host, one lane, for a sanitizer build:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/png_inflate_check.cpp -o png_inflate_check
//     png_inflate_check a.png b.png ...
// Per file one line:  <path> status=<code> path=<parallel|serial> segments=<n> digest=<CRC-32 of the picture's bytes, hex>
// (digest 0 when the status is not 0), or  <path> rejected: <reason>  for a file outside the accepted subset.  The stages and their
// order are the device's: inflate, size, Adler-32, filter bytes, CRC-32; a file of several segments is measured segment by segment
// first, exactly as the device's measuring pass does, and decoded with all IDATs joined.  tests/test_png_decode.py runs this over the
// whole corpus, corrupt files included: the codes must be the expected ones and the sanitizers must stay silent.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../gscream_amd/csrc/png_inflate.h"

struct BufferSink {
    uint8_t* out;
    uint64_t pos, limit;
    bool lit(uint8_t b)
    {
        if (pos >= limit) return false;
        out[pos++] = b;
        return true;
    }
    bool match(int len, uint32_t dist)  // dist <= pos: checked by the caller
    {
        if ((uint64_t)len > limit - pos) return false;
        for (int i = 0; i < len; i++, pos++) out[pos] = out[pos - dist];
        return true;
    }
};

static uint32_t be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | (uint32_t)p[3]; }

static uint32_t crc32(const uint8_t* p, size_t n)
{
    uint32_t c = 0xffffffffu;
    for (size_t i = 0; i < n; i++) {
        c ^= p[i];
        for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
    }
    return c ^ 0xffffffffu;
}

static int decode_file(const char* path)
{
    std::vector<uint8_t> data;
    {
        FILE* f = fopen(path, "rb");
        if (!f) { printf("%s rejected: cannot open\n", path); return 0; }
        uint8_t buf[65536];
        size_t n;
        while ((n = fread(buf, 1, sizeof buf, f)) > 0) data.insert(data.end(), buf, buf + n);
        fclose(f);
    }
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    if (data.size() < 8 || memcmp(data.data(), sig, 8) != 0) { printf("%s rejected: bad signature\n", path); return 0; }
    std::vector<PngiPiece> pieces;
    int H = 0, W = 0, C = 0;
    bool ihdr = false, iend = false, idat = false, restart = false;
    int segments = 0;
    for (size_t at = 8; at < data.size() && !iend;) {
        if (data.size() - at < 12) { printf("%s rejected: truncated chunk\n", path); return 0; }
        const uint32_t len = be32(&data[at]);
        if ((size_t)len > data.size() - at - 12) { printf("%s rejected: truncated chunk\n", path); return 0; }
        const uint8_t* type = &data[at + 4];
        PngiPiece pc = {(uint64_t)at + 8, len, 0u, 0u, 0u};
        if (pieces.empty()) {
            static const int channels[7] = {1, 0, 3, 0, 2, 0, 4};
            if (memcmp(type, "IHDR", 4) != 0 || len != 13) { printf("%s rejected: bad IHDR\n", path); return 0; }
            const uint8_t* h = &data[at + 8];
            const uint32_t w = be32(h), hh = be32(h + 4);
            if (!w || !hh || w >= (1u << 24) || hh >= (1u << 24) || h[10] || h[11]) { printf("%s rejected: bad IHDR\n", path); return 0; }
            if (h[8] != 8) { printf("%s rejected: bit depth %d\n", path, h[8]); return 0; }
            if (h[9] > 6 || !channels[h[9]]) { printf("%s rejected: colour type %d\n", path, h[9]); return 0; }
            if (h[12]) { printf("%s rejected: interlaced\n", path); return 0; }
            W = (int)w; H = (int)hh; C = channels[h[9]];
            if ((uint64_t)H * (1 + (uint64_t)W * C) >= 0x70000000ull) { printf("%s rejected: too large\n", path); return 0; }
            ihdr = true;
        } else if (memcmp(type, "IDAT", 4) == 0) {
            pc.flags = PNGI_PIECE_IDAT;
            if (!idat || restart) { pc.flags |= 2u; segments++; }
            idat = true;
            restart = len >= 4 && memcmp(&data[at + 8 + len - 4], "\x00\x00\xff\xff", 4) == 0;
        } else if (memcmp(type, "IEND", 4) == 0) {
            iend = true;
        }
        pieces.push_back(pc);
        at += 12 + (size_t)len;
    }
    if (!ihdr || !idat || !iend) { printf("%s rejected: missing IHDR, IDAT or IEND\n", path); return 0; }
    {
        PngiReader r;
        r.init(data.data(), data.size(), pieces.data(), 0, (int)pieces.size());
        uint32_t v;
        if (!r.take(16, v)) { printf("%s rejected: zlib header\n", path); return 0; }
        const uint32_t cmf = v & 255u, flg = v >> 8;
        if ((cmf & 15u) != 8 || (cmf >> 4) > 7 || (flg & 32u) || ((cmf << 8) | flg) % 31u) { printf("%s rejected: zlib header\n", path); return 0; }
    }
    const uint64_t row = 1 + (uint64_t)W * C, stream_bytes = (uint64_t)H * row;
    const int np = (int)pieces.size();
    PngiHostTeam tm;
    static PngiShared sh;
    // the measuring pass
    bool parallel = segments > 1;
    uint64_t total = 0;
    int seen = 0;
    for (int p = 0; p < np && parallel; p++) {
        if ((pieces[p].flags & 3u) != 3u) continue;
        int end = p + 1;
        while (end < np && (pieces[end].flags & 3u) != 3u) end++;
        seen++;
        PngiReader r;
        r.init(data.data(), data.size(), pieces.data(), p, end);
        PngiCountSink sink = {0, stream_bytes};
        uint32_t trailer = 0;
        const int rc = pngi_inflate(tm, r, sh, sink, (seen == 1 ? PNGI_HEAD : 0) | (seen == segments ? PNGI_TAIL : 0), &trailer);
        if (rc != PNGI_OK) parallel = false;
        total += sink.pos;
    }
    // the decode, all IDATs joined (what a segment-wise decode writes is the same bytes when no segment is flagged)
    std::vector<uint8_t> stream(stream_bytes);
    PngiReader r;
    r.init(data.data(), data.size(), pieces.data(), 0, np);
    BufferSink sink = {stream.data(), 0, stream_bytes};
    uint32_t trailer = 0;
    int status = pngi_inflate(tm, r, sh, sink, PNGI_HEAD | PNGI_TAIL, &trailer);
    if (status == PNGI_OK && sink.pos < stream_bytes) status = PNGI_TOO_SHORT;
    if (status == PNGI_OK && parallel && total != stream_bytes) status = 99;  // the two passes disagree: a defect of the measuring pass
    if (status == PNGI_OK) {
        uint32_t a = 1, b = 0;
        for (uint64_t i = 0; i < stream_bytes; i++) {
            a = (a + stream[i]) % PNGI_ADLER_MOD;
            b = (b + a) % PNGI_ADLER_MOD;
        }
        if (((b << 16) | a) != trailer) status = PNGI_ADLER;
    }
    std::vector<uint8_t> picture((size_t)H * W * C);
    if (status == PNGI_OK) {
        const size_t wc = (size_t)W * C;
        for (int y = 0; y < H && status == PNGI_OK; y++) {
            const uint8_t* s = &stream[(size_t)y * row];
            const int type = s[0];
            if (type > 4) { status = PNGI_FILTER; break; }
            uint8_t* cur = &picture[(size_t)y * wc];
            const uint8_t* up = y ? cur - wc : nullptr;
            for (size_t x = 0; x < wc; x++) {
                const int a = x >= (size_t)C ? cur[x - C] : 0, b = up ? up[x] : 0, c = (up && x >= (size_t)C) ? up[x - C] : 0;
                cur[x] = (uint8_t)pngi_unfilter(type, s[1 + x], a, b, c);
            }
        }
    }
    if (status == PNGI_OK)
        for (const PngiPiece& pc : pieces)
            if (crc32(&data[pc.offset - 4], 4 + (size_t)pc.length) != be32(&data[pc.offset + pc.length])) { status = PNGI_CRC; break; }
    const uint32_t digest = status == PNGI_OK ? crc32(picture.data(), picture.size()) : 0u;
    printf("%s status=%d path=%s segments=%d digest=%08x\n", path, status, parallel ? "parallel" : "serial", segments, digest);
    return 0;
}

int main(int argc, char** argv)
{
    for (int i = 1; i < argc; i++) decode_file(argv[i]);
    return 0;
}
