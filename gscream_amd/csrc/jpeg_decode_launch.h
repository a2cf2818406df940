// jpeg_decode_launch.h -- what jpeg_decode.hip shares with jpeg_split.hip (the split decode of include/gsraster_jpeg_split.h, which runs
// jpeg_decode.hip's own launch sequence with its launches put between markers and entropy): the workspace's tables, a file's geometry,
// the team, a scan's dwords, an interval's owner and piece, the build of a file's lookup tables, and the launcher.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gsr_api.h"
#include "jpeg_entropy.h"

struct JdWorkspace {
    uint8_t* area;
    unsigned long long area_bytes;
    uint32_t *ivl_start, *ivl_end;
    int32_t *ivl_status, *ivl_owner;
};

// what the sizes and the sampling of a file make
struct JdGeometry {
    uint32_t mcux, mcuy, mcus, blocks, per;  // per: MCUs in an interval (all of them without DRI)
    int ny, bpm;                             // component 0's blocks per MCU, all blocks per MCU
};
__host__ __device__ __forceinline__ JdGeometry jd_geometry(const gsr_jpeg_file& f)  // of a validated file
{
    JdGeometry g;
    g.mcux = ((uint32_t)f.W + 8u * f.hs - 1u) / (8u * f.hs);
    g.mcuy = ((uint32_t)f.H + 8u * f.vs - 1u) / (8u * f.vs);
    g.mcus = g.mcux * g.mcuy;  // <= 8192^2
    g.ny = f.hs * f.vs;
    g.bpm = g.ny + f.C - 1;
    g.blocks = g.mcus * (uint32_t)g.bpm;  // < 2^29
    g.per = f.restart_interval ? (uint32_t)f.restart_interval : g.mcus;
    return g;
}

// ---- what the kernels of both files that read a scan start from ----
struct JdTeam {  // jpeg_entropy.h's Team: a workgroup of `lanes` threads
    int lane, lanes;
    __device__ void sync() { __syncthreads(); }
};

// A file's scan as aligned dwords of `bytes`: it starts at aligned + shift and ends at aligned + limit.
struct JdScan {
    const uint8_t* aligned;  // the scan's first byte, rounded down to a dword
    uint32_t shift, limit;
    // the dword at offset o (a multiple of 4); one that reaches over the scan's end is read byte by byte, zeros behind the end
    __device__ uint32_t dword(uint32_t o) const
    {
        if (o < limit && limit - o >= 4u) return *(const uint32_t*)(aligned + o);
        uint32_t v = 0;
        for (uint32_t j = 0; j < 4u && o < limit && j < limit - o; j++) v |= (uint32_t)aligned[o + j] << (8u * j);
        return v;
    }
};
__device__ __forceinline__ JdScan jd_scan(const uint8_t* bytes, const gsr_jpeg_file& fl)
{
    const uint8_t* scan = bytes + fl.scan_offset;
    const uint32_t shift = (uint32_t)((uintptr_t)scan & 3u);
    return JdScan{scan - shift, shift, shift + fl.scan_length};
}

// the file that owns interval i and is sound so far, or -1
__device__ __forceinline__ int jd_owner(int i, const gsr_jpeg_file* files, int nfiles, const JdWorkspace& ws, const int32_t* status)
{
    const int f = ws.ivl_owner[i];
    if ((uint32_t)f >= (uint32_t)nfiles || status[2 * f] != GSR_JPEG_DECODE_OK) return -1;
    if (i < files[f].first_interval || i >= files[f].first_interval + files[f].intervals) return -1;  // (an entry no sound file owns)
    return f;
}
// interval i of its owner fl: the bytes [start, end) of the scan, the MCUs [first_mcu, first_mcu + mcus); last: the closing marker ends it
struct JdPiece {
    uint32_t start, end, first_mcu, mcus;
    bool last;
};
__device__ __forceinline__ JdPiece jd_piece(const gsr_jpeg_file& fl, const JdGeometry& g, int i, const JdWorkspace& ws)
{
    const uint32_t k = (uint32_t)(i - fl.first_interval);
    JdPiece p;
    // [start, end) lies in the scan: the markers kernel wrote positions of bytes it read
    p.start = min(ws.ivl_start[i], fl.scan_length);
    p.end = min(ws.ivl_end[i], fl.scan_length);
    p.first_mcu = k * g.per;
    p.mcus = min(g.per, g.mcus - p.first_mcu);
    p.last = k + 1u >= (uint32_t)fl.intervals;
    return p;
}

// The file's lookup tables, built by the team together (all its threads call) into codes[0 .. 5]: a table two components share is built
// once.  Entry 2c is component c's DC table, 2c + 1 its AC table; slot e of `slots` (four bits each) is the entry's place in `codes`.
// false: a table is unsound.
__device__ __forceinline__ bool jd_build(JdTeam tm, JpgeCode* codes, const gsr_jpeg_file& fl, const JpgeHuffman* huffman, uint32_t& slots)
{
    bool sound = true;
    slots = 0;
    for (int c = 0; c < fl.C; c++) {
        const bool dc_again = c > 0 && fl.dc[c] == fl.dc[c - 1], ac_again = c > 0 && fl.ac[c] == fl.ac[c - 1];
        uint32_t dc = 2u * (uint32_t)c, ac = dc + 1u;
        if (dc_again) dc = (slots >> (8 * (c - 1))) & 15u;
        else sound = jpge_build(tm, codes[dc], huffman + fl.dc[c]) && sound;
        if (ac_again) ac = (slots >> (8 * (c - 1) + 4)) & 15u;
        else sound = jpge_build(tm, codes[ac], huffman + fl.ac[c]) && sound;
        slots |= (dc | ac << 4) << (8 * c);
    }
    return sound;
}

// Launches that run between markers and entropy, on the same stream.  only[i] != 0: the entropy kernel decodes interval i; the
// workgroup of any other interval reads the word and leaves.
struct JdBetween {
    hipError_t (*launch)(void* self, const JdWorkspace& ws, hipStream_t stream);
    void* self;
    const int32_t* only;
};
// the six launches of gsr_jpeg_decode; between = nullptr: exactly those, every interval decoded by the entropy kernel
__attribute__((visibility("hidden"))) hipError_t jpeg_launch_decode(const uint8_t* bytes, size_t nbytes, const gsr_jpeg_file* files, int nfiles, int nintervals, const uint16_t* quant, int nquant,
                              const gsr_jpeg_huffman* huffman, int nhuffman, uint8_t* out, size_t out_bytes, int32_t* status, void* workspace,
                              size_t workspace_bytes, hipStream_t stream, const JdBetween* between);
__attribute__((visibility("hidden"))) size_t jd_tables_bytes(int nintervals);  // the tables' part alone: the least workspace a call is taken with
