// jpeg_decode_launch.h -- what jpeg_decode.hip shares with jpeg_split.hip (the split decode of include/gsraster_jpeg_split.h, which runs
// jpeg_decode.hip's own launch sequence with its launches put between markers and entropy): the workspace's tables, a file's geometry,
// and the launcher.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gsr_api.h"

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
