// jpeg_split_check -- the split decode of gscream_amd/csrc/jpeg_split.h on the host, for a sanitizer build:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_split_check.cpp -o jpeg_split_check
//     jpeg_split_check [-b subsequence_bytes] [-s chunk] a.jpg b.jpg ...          (defaults: 16 and 4)
// The lanes of a chunk are emulated one after another with the device's round structure kept (jpeg_split.hip: round 0 cold, round r
// through subsequence i + r, a lane stops when it meets the stored state), then the walk across chunks, the scan, the write pass from
// the final entry states with the checks of rule 6, the DC prefix.  An interval of fewer than two subsequences, or one marked for
// repair, is decoded by the serial core (jpeg_entropy.h) as on the device.  Beside it the serial core decodes the whole file.
// Per file one line:
//     <path> status=<code> serial=<code> digest=<CRC-32 of the split path's int16 coefficients> serial_digest=<the serial core's>
//            split=<intervals split> repaired=<of those, repaired> subsequences=<n>
// (digests 0 when the status is not 0), or  <path> rejected: <reason>.  tests/test_jpeg_split.py runs this over the corpus and the corrupt
// files: status and digest equal the serial core's on every file, repaired = 0 on every valid file, and the sanitizers stay silent.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../gscream_amd/csrc/jpeg_split.h"

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
struct HostStore {
    int16_t* out;  // the interval's first block
    void operator()(uint32_t block, int k, int32_t v) { out[(size_t)block * 64 + jpge_natural(k)] = (int16_t)v; }
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

static uint32_t B = 16, S = 4;

// -> true: the interval's coefficients are in `out`; false: repair
static bool split_interval(HostFetch& in, const JpsInterval& iv, int16_t* out, uint32_t& subsequences)
{
    const uint32_t n = iv.cut.count;
    subsequences = n;
    std::vector<uint32_t> entry(n, 0xdeadbeefu), blocks(n, 0xdeadbeefu), first(n);
    std::vector<JpsState> lane(n);
    std::vector<char> active(n);
    // sync within a chunk
    for (uint32_t c0 = 0; c0 < n; c0 += S) {
        const uint32_t c1 = n - c0 < S ? n : c0 + S;
        for (uint32_t i = c0; i < c1; i++) active[i] = jps_cold(in, iv, i, lane[i], entry.data(), blocks.data());
        for (uint32_t r = 1; r < S; r++) {
            bool any = false;
            for (uint32_t i = c0; i < c1; i++) {  // (a slot is touched by one lane per round: the order of the lanes does not matter)
                if (!active[i]) continue;
                if (i + r >= c1) { active[i] = 0; continue; }
                active[i] = jps_through(in, iv, i + r, lane[i], false, entry.data(), blocks.data());
                any = any || active[i];
            }
            if (!any) break;
        }
    }
    jps_walk(in, iv, S, entry.data(), blocks.data());
    uint32_t run = 0;
    for (uint32_t i = 0; i < n; i++) { first[i] = run; run += blocks[i]; }
    memset(out, 0, (size_t)iv.total * 128);
    HostStore store = {out};
    bool sound = true;
    for (uint32_t i = 0; i < n; i++) sound = jps_write(in, iv, i, entry.data(), blocks.data(), first.data(), store) && sound;
    if (!sound) return false;
    uint32_t pred[3] = {0u, 0u, 0u};
    for (uint32_t b = 0; b < iv.total; b++) {
        const int j = (int)(b % (uint32_t)iv.bpm), c = j < iv.ny ? 0 : j - iv.ny + 1;
        pred[c] += (uint32_t)(int32_t)out[(size_t)b * 64];
        out[(size_t)b * 64] = (int16_t)(uint16_t)pred[c];
    }
    return true;
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
    // the scan in a buffer of its exact size: a read past it is the sanitizer's to report
    std::vector<uint8_t> bytes(data.begin() + scan, data.end());
    const uint8_t* Sc = bytes.data();
    const uint32_t L = (uint32_t)bytes.size();

    HostTeam tm;
    static JpgeCode codes[6];
    const JpgeCode* use[6] = {};
    int verdict = JPGE_OK;
    for (int c = 0; c < C && verdict == JPGE_OK; c++) {
        if (!jpge_build(tm, codes[2 * c], &huff[dc[c]]) || !jpge_build(tm, codes[2 * c + 1], &huff[ac[c]])) verdict = JPGE_TABLE;
        use[2 * c] = &codes[2 * c];
        use[2 * c + 1] = &codes[2 * c + 1];
    }
    std::vector<uint32_t> marks;
    uint32_t closing = L;
    bool closed = false, numbered = true;
    for (uint32_t i = 0; i + 1 < L && !closed && verdict == JPGE_OK; i++) {
        const int cls = jpge_marker_class(Sc[i], Sc[i + 1]);
        if (cls == JPGE_CLOSING) { closed = true; closing = i; }
        else if (cls == JPGE_RST) {
            if (!jpge_marker_numbered(Sc[i + 1], (uint32_t)marks.size())) numbered = false;
            marks.push_back(i);
        }
    }
    if (verdict == JPGE_OK) verdict = jpge_marker_verdict(closed, (uint32_t)marks.size(), numbered, intervals);
    std::vector<int16_t> serial((size_t)mcus * bpm * 64), coef((size_t)mcus * bpm * 64);
    HostSink sink;
    memset(sink.block, 0, sizeof sink.block);
    HostFetch in = {Sc, L};
    int status = verdict, serial_status = verdict;
    uint32_t split = 0, repaired = 0, subsequences = 0;
    for (uint32_t k = 0; k < intervals && verdict == JPGE_OK; k++) {
        const uint32_t start = k ? marks[k - 1] + 2 : 0u, end = k + 1 < intervals ? marks[k] : closing;
        const uint32_t first = k * per, count = mcus - first < per ? mcus - first : per;
        if (serial_status == JPGE_OK) {
            sink.out = &serial;
            serial_status = jpge_interval(in, start, end, k + 1 < intervals, use, ny, bpm, first, count, sink);
        }
        if (status != JPGE_OK) continue;  // (the device decodes the later intervals too; the first failing one decides)
        const JpsInterval iv = {jps_cut(in, start, end, B), JpsTables{codes, 0x543210u}, ny, bpm, count * (uint32_t)bpm};
        bool done = false;
        if (iv.cut.count >= 2) {
            uint32_t n = 0;
            split++;
            done = split_interval(in, iv, coef.data() + (size_t)first * bpm * 64, n);
            subsequences += n;
            if (!done) repaired++;
        }
        if (!done) {
            sink.out = &coef;
            memset(sink.block, 0, sizeof sink.block);
            status = jpge_interval(in, start, end, k + 1 < intervals, use, ny, bpm, first, count, sink);
        }
    }
    const uint32_t digest = status == JPGE_OK ? crc32((const uint8_t*)coef.data(), coef.size() * 2) : 0u;
    const uint32_t serial_digest = serial_status == JPGE_OK ? crc32((const uint8_t*)serial.data(), serial.size() * 2) : 0u;
    printf("%s status=%d serial=%d digest=%08x serial_digest=%08x split=%u repaired=%u subsequences=%u\n", path, status, serial_status, digest,
           serial_digest, split, repaired, subsequences);
    return 0;
}

int main(int argc, char** argv)
{
    int i = 1;
    for (; i + 1 < argc && argv[i][0] == '-'; i += 2) {
        const long v = strtol(argv[i + 1], nullptr, 10);
        if (!strcmp(argv[i], "-b") && jps_bytes_allowed((int)v)) B = (uint32_t)v;
        else if (!strcmp(argv[i], "-s") && v >= 1 && v <= 1024) S = (uint32_t)v;
        else { fprintf(stderr, "jpeg_split_check: bad option %s %s\n", argv[i], argv[i + 1]); return 2; }
    }
    for (; i < argc; i++) decode_file(argv[i]);
    return 0;
}
