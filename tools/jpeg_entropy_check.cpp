// jpeg_entropy_check -- the entropy core of gscream_amd/csrc/jpeg_entropy.h on the host, one lane, for a sanitizer build:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_entropy_check.cpp -o jpeg_entropy_check
//     jpeg_entropy_check a.jpg b.jpg ...
// Per file one line:  <path> status=<code> intervals=<n> digest=<CRC-32 of the int16 coefficients, natural order, blocks in scan order, hex>
// (digest 0 when the status is not 0), or  <path> rejected: <reason>  for a file outside the accepted subset.  The stages and their
// order are the device's: the Huffman tables, the walk over the scan's markers, the intervals in scan order.  tests/test_jpeg_decode.py
// runs this over the whole corpus, corrupt files included: the codes must be the expected ones and the sanitizers must stay silent.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../gscream_amd/csrc/jpeg_entropy.h"

struct HostTeam {
    int lane = 0, lanes = 1;
    void sync() {}
};
struct HostFetch {
    const uint8_t* scan;
    uint8_t operator()(uint32_t at) const { return scan[at]; }
};
struct HostSink {
    int16_t block[64];
    std::vector<int16_t>* out;
    void put(int k, int16_t v) { block[jpge_natural(k)] = v; }
    void flush(size_t b)
    {
        memcpy(out->data() + 64 * b, block, sizeof block);
        memset(block, 0, sizeof block);
    }
};

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
    const size_t N = data.size();
    if (N < 4 || data[0] != 0xFF || data[1] != 0xD8) { printf("%s rejected: no SOI\n", path); return 0; }
    JpgeHuffman huff[8];
    bool have_huff[8] = {};
    memset(huff, 0, sizeof huff);
    int H = 0, W = 0, C = 0, hs = 0, vs = 0, dri = 0, dc[3] = {}, ac[3] = {};
    size_t at = 2, scan = 0;
    while (!scan) {
        if (at + 4 > N || data[at] != 0xFF) { printf("%s rejected: marker expected\n", path); return 0; }
        const int marker = data[at + 1];
        if (marker == 0xFF) { at++; continue; }
        const size_t n = (size_t)data[at + 2] << 8 | data[at + 3];
        if (n < 2 || at + 2 + n > N) { printf("%s rejected: a segment runs past the file\n", path); return 0; }
        const uint8_t* p = &data[at + 4];
        const size_t len = n - 2;
        if (marker == 0xC4) {
            for (size_t q = 0; q < len;) {
                if (len - q < 17) { printf("%s rejected: DHT\n", path); return 0; }
                const int id = p[q], slot = (id >> 4) * 4 + (id & 15);
                size_t total = 0;
                for (int i = 0; i < 16; i++) total += p[q + 1 + i];
                if ((id >> 4) > 1 || (id & 15) > 3 || total > 256 || len - q - 17 < total) { printf("%s rejected: DHT\n", path); return 0; }
                memset(&huff[slot], 0, sizeof huff[slot]);
                memcpy(huff[slot].bits, p + q + 1, 16);
                memcpy(huff[slot].values, p + q + 17, total);
                have_huff[slot] = true;
                q += 17 + total;
            }
        } else if (marker == 0xDD) {
            if (len != 2) { printf("%s rejected: DRI\n", path); return 0; }
            dri = p[0] << 8 | p[1];
        } else if (marker == 0xC0) {
            if (len < 6 || p[0] != 8 || (p[5] != 1 && p[5] != 3) || len != 6 + 3 * (size_t)p[5]) { printf("%s rejected: SOF0\n", path); return 0; }
            H = p[1] << 8 | p[2]; W = p[3] << 8 | p[4]; C = p[5];
            hs = p[7] >> 4; vs = p[7] & 15;
            const bool sampling = C == 1 ? (hs == 1 && vs == 1) : ((hs == 1 || hs == 2) && (vs == 1 || vs == 2) && !(hs == 1 && vs == 2) && p[10] == 0x11 && p[13] == 0x11);
            if (!H || !W || !sampling) { printf("%s rejected: sizes or sampling\n", path); return 0; }
        } else if (marker == 0xDA) {
            if (!C || len != 4 + 2 * (size_t)C || p[0] != C) { printf("%s rejected: SOS\n", path); return 0; }
            for (int c = 0; c < C; c++) {
                dc[c] = p[2 + 2 * c] >> 4; ac[c] = 4 + (p[2 + 2 * c] & 15);
                if (dc[c] > 3 || ac[c] > 7 || !have_huff[dc[c]] || !have_huff[ac[c]]) { printf("%s rejected: SOS names a missing table\n", path); return 0; }
            }
            scan = at + 2 + n;
        } else if ((marker >= 0xC1 && marker <= 0xCF) || marker == 0xD9) {
            printf("%s rejected: marker %02x\n", path, marker);
            return 0;
        }
        at += 2 + n;
    }
    const uint32_t mcux = (uint32_t)(W + 8 * hs - 1) / (8 * hs), mcuy = (uint32_t)(H + 8 * vs - 1) / (8 * vs), mcus = mcux * mcuy;
    const int ny = hs * vs, bpm = ny + C - 1;
    const uint32_t intervals = dri ? (mcus + dri - 1) / dri : 1u, per = dri ? (uint32_t)dri : mcus;
    const uint8_t* S = data.data() + scan;
    const uint32_t L = (uint32_t)(N - scan);

    HostTeam tm;
    static JpgeCode codes[6];
    const JpgeCode* use[6] = {};
    int status = JPGE_OK;
    for (int c = 0; c < C && status == JPGE_OK; c++) {
        if (!jpge_build(tm, codes[2 * c], &huff[dc[c]]) || !jpge_build(tm, codes[2 * c + 1], &huff[ac[c]])) status = JPGE_TABLE;
        use[2 * c] = &codes[2 * c];
        use[2 * c + 1] = &codes[2 * c + 1];
    }
    // rule 2: the walk over the scan
    std::vector<uint32_t> marks;
    uint32_t closing = L;
    bool closed = false, numbered = true;
    for (uint32_t i = 0; i + 1 < L && !closed && status == JPGE_OK; i++) {
        const int cls = jpge_marker_class(S[i], S[i + 1]);
        if (cls == JPGE_CLOSING) { closed = true; closing = i; }
        else if (cls == JPGE_RST) {
            if (!jpge_marker_numbered(S[i + 1], (uint32_t)marks.size())) numbered = false;
            marks.push_back(i);
        }
    }
    if (status == JPGE_OK) status = jpge_marker_verdict(closed, (uint32_t)marks.size(), numbered, intervals);
    std::vector<int16_t> coef((size_t)mcus * bpm * 64);
    HostSink sink;
    memset(sink.block, 0, sizeof sink.block);
    sink.out = &coef;
    const HostFetch in = {S};
    for (uint32_t k = 0; k < intervals && status == JPGE_OK; k++) {
        const uint32_t start = k ? marks[k - 1] + 2 : 0u, end = k + 1 < intervals ? marks[k] : closing;
        const uint32_t first = k * per, count = mcus - first < per ? mcus - first : per;
        status = jpge_interval(in, start, end, k + 1 < intervals, use, ny, bpm, first, count, sink);
    }
    const uint32_t digest = status == JPGE_OK ? crc32((const uint8_t*)coef.data(), coef.size() * 2) : 0u;
    printf("%s status=%d intervals=%u digest=%08x\n", path, status, intervals, digest);
    return 0;
}

int main(int argc, char** argv)
{
    for (int i = 1; i < argc; i++) decode_file(argv[i]);
    return 0;
}
