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
#include "jpeg_check_host.h"

#include "../gscream_amd/csrc/jpeg_split.h"

struct HostStore {
    int16_t* out;  // the interval's first block
    void operator()(uint32_t block, int k, int32_t v) { out[(size_t)block * 64 + jpge_natural(k)] = (int16_t)v; }
};

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
        const int c = jpge_component((int)(b % (uint32_t)iv.bpm), iv.ny);
        pred[c] += (uint32_t)(int32_t)out[(size_t)b * 64];
        out[(size_t)b * 64] = (int16_t)(uint16_t)pred[c];
    }
    return true;
}

static int decode_file(const char* path)
{
    static HostFile file;
    if (!host_walk(path, file)) return 0;
    const int ny = file.ny, bpm = file.bpm;
    std::vector<int16_t> serial((size_t)file.mcus * bpm * 64), coef((size_t)file.mcus * bpm * 64);
    HostSink serial_sink = {{}, &serial}, sink = {{}, &coef};
    HostFetch in = {file.scan.data(), (uint32_t)file.scan.size()};
    int status = file.verdict, serial_status = file.verdict;
    uint32_t split = 0, repaired = 0, subsequences = 0;
    for (uint32_t k = 0; k < file.start.size(); k++) {
        const uint32_t start = file.start[k], end = file.end[k], first = file.first_mcu(k), count = file.count(k);
        if (serial_status == JPGE_OK) serial_status = jpge_interval(in, start, end, k + 1 < file.intervals, file.use, ny, bpm, first, count, serial_sink);
        if (status != JPGE_OK) continue;  // (the device decodes the later intervals too; the first failing one decides)
        const JpsInterval iv = {jps_cut(in, start, end, B), JpsTables{file.codes, 0x543210u}, ny, bpm, count * (uint32_t)bpm};
        bool done = false;
        if (iv.cut.count >= 2) {
            uint32_t n = 0;
            split++;
            done = split_interval(in, iv, coef.data() + (size_t)first * bpm * 64, n);
            subsequences += n;
            if (!done) repaired++;
        }
        if (!done) status = jpge_interval(in, start, end, k + 1 < file.intervals, file.use, ny, bpm, first, count, sink);
    }
    printf("%s status=%d serial=%d digest=%08x serial_digest=%08x split=%u repaired=%u subsequences=%u\n", path, status, serial_status,
           host_digest(status, coef), host_digest(serial_status, serial), split, repaired, subsequences);
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
