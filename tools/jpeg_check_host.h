// jpeg_check_host.h -- what tools/jpeg_entropy_check.cpp and tools/jpeg_split_check.cpp share: the host's Team, Fetch and Sink for the cores
// of gscream_amd/csrc/jpeg_entropy.h and jpeg_split.h, the digest, and the walk over a file up to its restart intervals.  The stages and
// their order are the device's: the Huffman tables, the walk over the scan's markers (rule 2), the intervals in scan order.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../gscream_amd/csrc/jpeg_entropy.h"

struct HostTeam {
    int lane = 0, lanes = 1;
    void sync() {}
};
struct HostFetch {
    const uint8_t* scan;
    uint32_t length;
    uint8_t operator()(uint32_t at) const
    {
        if (at >= length) abort();  // the core asked for a byte outside the scan
        return scan[at];
    }
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
// the digest of a file's coefficients (int16, natural order, blocks in scan order); 0 when the status is not 0
static uint32_t host_digest(int status, const std::vector<int16_t>& coef)
{
    return status == JPGE_OK ? crc32((const uint8_t*)coef.data(), coef.size() * 2) : 0u;
}

// A file of the accepted subset, up to its intervals.
struct HostFile {
    int verdict;  // rules 1 and 2: JPGE_OK, or the status the file ends with (then no interval is listed)
    int ny, bpm;
    uint32_t mcus, per, intervals;
    JpgeCode codes[6];
    const JpgeCode* use[6];          // use[2c], use[2c + 1]: component c's DC and AC tables
    std::vector<uint8_t> scan;       // of its exact size: a read past it is the sanitizer's to report
    std::vector<uint32_t> start, end;  // interval k: the bytes [start[k], end[k]) of the scan
    uint32_t first_mcu(uint32_t k) const { return k * per; }
    uint32_t count(uint32_t k) const { return mcus - k * per < per ? mcus - k * per : per; }  // interval k's MCUs
};
// -> false: the file lies outside the accepted subset, and its line  <path> rejected: <reason>  is printed
static bool host_walk(const char* path, HostFile& out)
{
    std::vector<uint8_t> data;
    {
        FILE* f = fopen(path, "rb");
        if (!f) { printf("%s rejected: cannot open\n", path); return false; }
        uint8_t buf[65536];
        size_t n;
        while ((n = fread(buf, 1, sizeof buf, f)) > 0) data.insert(data.end(), buf, buf + n);
        fclose(f);
    }
    const size_t N = data.size();
    if (N < 4 || data[0] != 0xFF || data[1] != 0xD8) { printf("%s rejected: no SOI\n", path); return false; }
    JpgeHuffman huff[8];
    bool have_huff[8] = {};
    memset(huff, 0, sizeof huff);
    int H = 0, W = 0, C = 0, hs = 0, vs = 0, dri = 0, dc[3] = {}, ac[3] = {};
    size_t at = 2, scan = 0;
    while (!scan) {
        if (at + 4 > N || data[at] != 0xFF) { printf("%s rejected: marker expected\n", path); return false; }
        const int marker = data[at + 1];
        if (marker == 0xFF) { at++; continue; }
        const size_t n = (size_t)data[at + 2] << 8 | data[at + 3];
        if (n < 2 || at + 2 + n > N) { printf("%s rejected: a segment runs past the file\n", path); return false; }
        const uint8_t* p = &data[at + 4];
        const size_t len = n - 2;
        if (marker == 0xC4) {
            for (size_t q = 0; q < len;) {
                if (len - q < 17) { printf("%s rejected: DHT\n", path); return false; }
                const int id = p[q], slot = (id >> 4) * 4 + (id & 15);
                size_t total = 0;
                for (int i = 0; i < 16; i++) total += p[q + 1 + i];
                if ((id >> 4) > 1 || (id & 15) > 3 || total > 256 || len - q - 17 < total) { printf("%s rejected: DHT\n", path); return false; }
                memset(&huff[slot], 0, sizeof huff[slot]);
                memcpy(huff[slot].bits, p + q + 1, 16);
                memcpy(huff[slot].values, p + q + 17, total);
                have_huff[slot] = true;
                q += 17 + total;
            }
        } else if (marker == 0xDD) {
            if (len != 2) { printf("%s rejected: DRI\n", path); return false; }
            dri = p[0] << 8 | p[1];
        } else if (marker == 0xC0) {
            if (len < 6 || p[0] != 8 || (p[5] != 1 && p[5] != 3) || len != 6 + 3 * (size_t)p[5]) { printf("%s rejected: SOF0\n", path); return false; }
            H = p[1] << 8 | p[2]; W = p[3] << 8 | p[4]; C = p[5];
            hs = p[7] >> 4; vs = p[7] & 15;
            const bool sampling = C == 1 ? (hs == 1 && vs == 1) : ((hs == 1 || hs == 2) && (vs == 1 || vs == 2) && !(hs == 1 && vs == 2) && p[10] == 0x11 && p[13] == 0x11);
            if (!H || !W || !sampling) { printf("%s rejected: sizes or sampling\n", path); return false; }
        } else if (marker == 0xDA) {
            if (!C || len != 4 + 2 * (size_t)C || p[0] != C) { printf("%s rejected: SOS\n", path); return false; }
            for (int c = 0; c < C; c++) {
                dc[c] = p[2 + 2 * c] >> 4; ac[c] = 4 + (p[2 + 2 * c] & 15);
                if (dc[c] > 3 || ac[c] > 7 || !have_huff[dc[c]] || !have_huff[ac[c]]) { printf("%s rejected: SOS names a missing table\n", path); return false; }
            }
            scan = at + 2 + n;
        } else if ((marker >= 0xC1 && marker <= 0xCF) || marker == 0xD9) {
            printf("%s rejected: marker %02x\n", path, marker);
            return false;
        }
        at += 2 + n;
    }
    const uint32_t mcux = (uint32_t)(W + 8 * hs - 1) / (8 * hs), mcuy = (uint32_t)(H + 8 * vs - 1) / (8 * vs);
    out.mcus = mcux * mcuy;
    out.ny = hs * vs;
    out.bpm = out.ny + C - 1;
    out.intervals = dri ? (out.mcus + dri - 1) / dri : 1u;
    out.per = dri ? (uint32_t)dri : out.mcus;
    out.scan.assign(data.begin() + scan, data.end());
    const uint8_t* S = out.scan.data();
    const uint32_t L = (uint32_t)out.scan.size();

    HostTeam tm;
    out.verdict = JPGE_OK;
    for (int e = 0; e < 6; e++) out.use[e] = nullptr;
    for (int c = 0; c < C && out.verdict == JPGE_OK; c++) {
        if (!jpge_build(tm, out.codes[2 * c], &huff[dc[c]]) || !jpge_build(tm, out.codes[2 * c + 1], &huff[ac[c]])) out.verdict = JPGE_TABLE;
        out.use[2 * c] = &out.codes[2 * c];
        out.use[2 * c + 1] = &out.codes[2 * c + 1];
    }
    // rule 2: the walk over the scan
    std::vector<uint32_t> marks;
    uint32_t closing = L;
    bool closed = false, numbered = true;
    for (uint32_t i = 0; i + 1 < L && !closed && out.verdict == JPGE_OK; i++) {
        const int cls = jpge_marker_class(S[i], S[i + 1]);
        if (cls == JPGE_CLOSING) { closed = true; closing = i; }
        else if (cls == JPGE_RST) {
            if (!jpge_marker_numbered(S[i + 1], (uint32_t)marks.size())) numbered = false;
            marks.push_back(i);
        }
    }
    if (out.verdict == JPGE_OK) out.verdict = jpge_marker_verdict(closed, (uint32_t)marks.size(), numbered, out.intervals);
    out.start.clear();
    out.end.clear();
    for (uint32_t k = 0; k < out.intervals && out.verdict == JPGE_OK; k++) {
        out.start.push_back(k ? marks[k - 1] + 2 : 0u);
        out.end.push_back(k + 1 < out.intervals ? marks[k] : closing);
    }
    return true;
}
