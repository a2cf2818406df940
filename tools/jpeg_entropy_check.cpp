// jpeg_entropy_check -- the entropy core of gscream_amd/csrc/jpeg_entropy.h on the host, one lane, for a sanitizer build:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_entropy_check.cpp -o jpeg_entropy_check
//     jpeg_entropy_check a.jpg b.jpg ...
// Per file one line:  <path> status=<code> intervals=<n> digest=<CRC-32 of the int16 coefficients, natural order, blocks in scan order, hex>
// (digest 0 when the status is not 0), or  <path> rejected: <reason>  for a file outside the accepted subset.  The stages and their
// order are the device's: the Huffman tables, the walk over the scan's markers, the intervals in scan order.  tests/test_jpeg_decode.py
// runs this over the whole corpus, corrupt files included: the codes must be the expected ones and the sanitizers must stay silent.
#include "jpeg_check_host.h"

static int decode_file(const char* path)
{
    static HostFile file;
    if (!host_walk(path, file)) return 0;
    int status = file.verdict;
    std::vector<int16_t> coef((size_t)file.mcus * file.bpm * 64);
    HostSink sink = {{}, &coef};
    const HostFetch in = {file.scan.data(), (uint32_t)file.scan.size()};
    for (uint32_t k = 0; k < file.start.size() && status == JPGE_OK; k++)
        status = jpge_interval(in, file.start[k], file.end[k], k + 1 < file.intervals, file.use, file.ny, file.bpm, file.first_mcu(k), file.count(k), sink);
    printf("%s status=%d intervals=%u digest=%08x\n", path, status, file.intervals, host_digest(status, coef));
    return 0;
}

int main(int argc, char** argv)
{
    for (int i = 1; i < argc; i++) decode_file(argv[i]);
    return 0;
}
