/*
 * gsraster_jpeg_split.h -- an extension family of the C ABI of include/gsraster.h: baseline JPEG decoding on the device with the
 * scan of an interval split at self-synchronisation points.  The functions are exported by the same libgsraster.so; GSR_ABI_VERSION
 * stays what gsraster.h says (additions only).  include/gsraster_jpeg_decode.h is the family this one stands beside: its structs, its
 * six rules, its status codes and its rejection rules hold here unchanged, and gsr_jpeg_decode is what it was.  gscream_amd/_abi.py
 * reads this file with the main header's constants in scope (`_abi.extension`).
 *
 * ---- why (jpeg_split.hip, jpeg_split.h) -----------------------------------------------------------------------------------------
 * In gsr_jpeg_decode a restart interval is one instruction stream, decoded by one wavefront; a file without restart markers -- what
 * PIL and cameras write -- is one interval.  Huffman streams synchronise themselves (Klein & Wiseman): a decoder started at a wrong
 * place in a wrong state falls into step with the right one after a few symbols.  So the interval's bytes are cut into subsequences,
 * every subsequence is decoded speculatively by a lane of its own, and the lanes run into their neighbours until the states agree
 * (Weissenberger & Schmidt, "Accelerating JPEG Decompression on GPUs").  Everything here keeps the module's rules: nothing is read
 * back, no global atomics, no workgroup waits for another except by launch order, every loop has a bound known at launch, the
 * same input gives the same bytes, and a corrupt file ends in a status code.
 *
 * The rules.  `start`, `end`: the interval's data is the bytes [start, end) of the scan that rule 2 of gsraster_jpeg_decode.h finds.
 *   1 subsequences  B = subsequence_bytes, a power of two from 16 to 1024.  An interval of n = end - start bytes has ceil(n / B)
 *              subsequences.  Subsequence i nominally begins at byte start + i B; when i > 0 and the byte in front of that position is
 *              FF, the nominal byte is the stuffed 00 of an FF 00 pair and the subsequence begins one byte later (inside an interval
 *              FF only ever opens a pair); a last subsequence that would then begin at `end` does not exist.  Subsequence i ends
 *              where subsequence i + 1 begins, the last one at `end`; none is empty.  A decoding unit
 *              is a Huffman symbol together with its value bits, at most 16 + 11 = 27 bits: every subsequence holds the start of one.
 *   2 state    Between two units a decoder's state is the triple (bit, j, k): bit = its position in the interval's de-stuffed bit
 *              stream (FF 00 counts 8 bits), j = the block's number within its MCU, 0 .. bpm - 1 (bpm = hs vs + C - 1), k = the zigzag
 *              position the next unit codes, 0 .. 63; k = 0: a DC unit comes next.  j selects the tables, k says what EOB (k = 0, the
 *              next j) and ZRL (k + 16) do; behind coefficient 63 the state is (j + 1 mod bpm, 0).  Two decoders in the same state
 *              decode the same from there on: that is the whole argument.
 *   3 entry    Subsequence 0 enters at (0, 0, 0).  The entry state of subsequence i > 0 is the state of the serial decoder (rule 1 of
 *              gsraster_jpeg_decode.h, run from the interval's first bit) in front of the first unit whose first bit lies at or
 *              beyond the subsequence's beginning; when no unit begins there, the state behind the interval's last unit.  The rule
 *              fixes this result, not the route to it: the device's final entry states are exactly these.
 *   4 counting blocks[i] = the DC units among the units that begin in subsequence i (the blocks begun there), decoded from its entry
 *              state.  first_block[i] = the exclusive sum of blocks[] over the interval's subsequences in order (gsr_scan.h): the
 *              number within the interval, in scan order, of the first block begun in subsequence i.  With k it places every
 *              coefficient: a unit at k > 0 that begins in subsequence i in front of its first DC unit belongs to block first_block[i] - 1.
 *              The interval is complete when the chain has decoded MCUs bpm blocks.
 *   5 DC       The write pass stores the DC differences.  Then, per component, an ordered integer prefix sum over the interval's blocks
 *              in scan order, wrapping at 16 bits as the serial decoder's (int16_t)(uint16_t)pred does: exact.
 *   6 repair   An interval is decoded again by the one-wave kernel of gsr_jpeg_decode, whose picture and status code then stand, if
 *              the write pass finds any of: an entry state that is no state; a unit that fails (any code of rule 1); a subsequence
 *              whose exit state is not the next one's entry state, or whose blocks[] is not the recorded one; a block number that is
 *              not j modulo bpm or lies beyond the interval's blocks; at the end of the data, first_block + blocks other than MCUs bpm,
 *              an unfinished block, or a whole byte left.  If none holds, the chain from subsequence 0 has been checked link by link
 *              and the coefficients are the serial decoder's.  Errors met while decoding from a speculative state are never reported.
 *              On a valid stream the chain converges, so nothing is repaired.
 * The output is gsr_jpeg_decode's: int16 coefficients in natural order, blocks in scan order, then its own idct and colour launches.
 *
 * gsr_jpeg_split_workspace_bytes(area_bytes, nfiles, nintervals, scan_bytes, subsequence_bytes): area_bytes as for
 * gsr_jpeg_decode_workspace_bytes; scan_bytes = the `nbytes` the decode will be called with.  gsr_jpeg_decode's tables follow the
 * area, then this family's: per interval seven words, per subsequence (at most scan_bytes / B + nintervals) four.
 * 0 for counts <= 0, an area of 2^40 bytes or more, scan_bytes of 2^32 or more, or a B that rule 1 does not allow.
 *
 * gsr_jpeg_decode_split: the arguments of gsr_jpeg_decode, `stream` staying the last one as in every launching entry point; in front of it
 *   subsequence_bytes  B of rule 1
 *   min_bytes          an interval takes the split path when end - start >= min_bytes and it holds at least two subsequences; every
 *                      other interval is decoded by the one-wave kernel as in gsr_jpeg_decode (min_bytes >= 0)
 *   trace              NULL, or device memory for one gsr_jpeg_split_trace per subsequence the workspace has room for (scan_bytes / B +
 *                      nintervals): the final entry state and the counts of rules 3 and 4, the split intervals in table order, each
 *                      one's subsequences in order, densely.  Written only when given.
 *   info               device, four int32 per file: {intervals split, intervals repaired, subsequences, chunks}
 * All pointers are device pointers (trace and info 4-byte aligned).  The launches, all on `stream`: validate and markers of
 * gsr_jpeg_decode; classify (one workgroup: which intervals are split, where their subsequences and chunks lie: two scans);
 * sync within a chunk (a workgroup of 256 lanes per chunk of 256 consecutive subsequences, the file's six lookup tables in LDS: round 0
 * decodes every subsequence cold from (its beginning, 0, 0), in round r a lane that has not matched goes on through subsequence i + r
 * and compares its state at that subsequence's end with the one stored there by the round before; equal: it stops; else it stores
 * its own; a barrier between rounds, at most 256 rounds); sync across chunks (one lane per split interval walks the chunks in order:
 * from the verified exit of chunk c - 1 into chunk c until its state is the stored one); scan (a workgroup per split interval:
 * first_block); clear (the coefficients of the split intervals' blocks); write (a lane per subsequence, from its final entry state:
 * DC differences and AC values, two bytes a store, and the checks of rule 6); DC prefix (a workgroup per split interval, rule 5);
 * info; then gsr_jpeg_decode's entropy kernel for exactly the intervals that are not split or marked for repair -- a workgroup of any
 * other interval reads its flag and leaves -- and its status, idct and colour launches unchanged.  A slot is written by one lane per
 * round and read in the next, so the result does not depend on scheduling.
 * Rejected before launching (GSR_ERR_INVALID_ARGUMENT): everything gsr_jpeg_decode rejects, by the same rules; subsequence_bytes not a
 * power of two in 16 .. 1024; min_bytes < 0; info NULL; trace or info misaligned; a workspace below its tables' part.
 */
#ifndef GSRASTER_JPEG_SPLIT_H
#define GSRASTER_JPEG_SPLIT_H

#include <stddef.h>
#include <stdint.h>

#include "gsraster_jpeg_decode.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gsr_jpeg_split_trace {
    int32_t bit, j, k, first_block, blocks;
} gsr_jpeg_split_trace;
size_t gsr_jpeg_split_workspace_bytes(size_t area_bytes, int nfiles, int nintervals, size_t scan_bytes, int subsequence_bytes);
int gsr_jpeg_decode_split(const uint8_t* bytes, size_t nbytes, const gsr_jpeg_file* files, int nfiles, int nintervals, const uint16_t* quant,
                          int nquant, const gsr_jpeg_huffman* huffman, int nhuffman, uint8_t* out, size_t out_bytes, int32_t* status,
                          void* workspace, size_t workspace_bytes, int subsequence_bytes, int min_bytes, gsr_jpeg_split_trace* trace,
                          int32_t* info, void* stream /* hipStream_t */);

#ifdef __cplusplus
}
#endif
#endif
