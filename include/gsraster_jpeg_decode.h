/*
 * gsraster_jpeg_decode.h -- an extension family of the C ABI of include/gsraster.h: baseline JPEG decoding on the device.
 * The functions are exported by the same libgsraster.so; GSR_ABI_VERSION stays what gsraster.h says (additions only).  The family has
 * a header of its own because the main header's declarations are counted by its tests.  gscream_amd/_abi.py reads this file with the
 * main header's constants in scope (`_abi.extension`), and gscream_amd/jpeg_decode.py types its calls from that reading.
 *
 * ---- JPEG decoding (jpeg_decode.hip, jpeg_entropy.h): the bytes of .jpg files -> uint8 [H, W, C] pictures, on the device ----------
 * The other half of gsr_jpeg_encode (the frames of gscream_amd/video.py's Motion-JPEG AVI) and of Image.open + to_tensor + upload
 * for scenes whose pictures are .jpg (scene/dataset_readers.py:171-172).  The host reads the marker segments up to SOS and nothing
 * of the entropy-coded data; the device finds the restart markers, decodes the Huffman data, and does everything behind it.  The
 * picture is the one libjpeg-turbo's default decoder gives (JDCT_ISLOW, fancy upsampling; what PIL's Image.open returns), byte for
 * byte, for files made by encoding pictures; tests/jpeg_decode_helpers.py states the rules below in numpy.
 *
 *   accepted   SOF0, precision 8; one scan holding all components, Ss 0, Se 63, Ah/Al 0; C = 1 with sampling 1x1; C = 3 with
 *              component 0 sampled 1x1, 2x1 or 2x2 and both others 1x1 (4:4:4, 4:2:2, 4:2:0); 8-bit DQT; up to two DC and two AC
 *              Huffman tables of any conforming shape; DRI of any value, or none; APPn and COM segments (skipped); bytes behind EOI
 *              (ignored).  Everything else -- progressive, arithmetic, lossless, 12-bit, several scans, four components, 16-bit
 *              DQT, sampling 1x2; three components with an Adobe APP14 segment, or with the ids 'R' 'G' 'B' and no JFIF APP0 (libjpeg
 *              does not take those as YCbCr) -- is the host parser's to reject: the device is never given such a file.
 *   bytes      the files' bytes, unmodified, back to back in one device buffer of `nbytes`.
 *   files      one gsr_jpeg_file per file: where its scan lies in `bytes` (scan_offset = the first byte behind the SOS segment,
 *              scan_length = everything from there to the end of the file, EOI and what follows included); H, W, C; hs, vs = the
 *              sampling factors of component 0; restart_interval = DRI's value in MCUs (0 = none); intervals = ceil(MCUs /
 *              restart_interval), 1 without DRI, and first_interval = the file's first entry in the call's interval tables (the
 *              files' ranges do not overlap and lie in 0 .. nintervals); out_offset = the byte offset of its picture in `out` (H W C
 *              bytes, dense); coef_offset and plane_offset = byte offsets into the workspace of its coefficients (128 bytes a
 *              block) and of its component planes (64 bytes a block), multiples of 16, the areas of a call not overlapping;
 *              quant[c], dc[c], ac[c] = component c's entries in `quant` and `huffman`.
 *              With MCUs = ceil(W / 8 hs) ceil(H / 8 vs) and blocks = MCUs (hs vs + C - 1).
 *   quant      nquant tables of 64 uint16 in NATURAL order (row-major in the block), the values of the DQT segment.
 *   huffman    nhuffman tables as a DHT segment holds them: bits[16] (the number of codes of length 1 .. 16), values[256] (the
 *              symbols in code order; entries behind the last code are not read).
 *   status     two int32 per file: {code, intervals decoded}.
 *   out        the pictures, uint8 [H, W, C] each at its out_offset.
 *
 * The rules.  All arithmetic is int32 with arithmetic shifts.
 *   1 entropy  Baseline Huffman, MSB first; FF 00 is a data byte FF.  Canonical codes (Annex C): the codes of a length are
 *              consecutive, and the first code of a length is twice (the last code of the previous length + 1).  Per block: the
 *              DC symbol is a category s <= 11, followed by s bits v; diff = v when v >= 2^(s-1), else v - 2^s + 1; DC = the DC of the
 *              previous block of the same component + diff, 0 standing for the previous DC at the start of every interval.  AC
 *              symbols are (run << 4 | size): size 1 .. 10 skips `run` zero coefficients and sets the next from `size` bits as
 *              above; F0 (ZRL) skips 16; 00 (EOB) ends the block; a block also ends behind coefficient 63.  Coefficients are coded
 *              in zigzag order.  The blocks of an MCU: component 0's hs vs blocks in raster order, then Cb, then Cr; MCUs in raster
 *              order.
 *   2 restart  A marker is an FF followed by a byte that is neither 00 nor FF.  The first marker of the scan that is not RSTm
 *              (FF D0 .. FF D7) closes it; nothing behind it is looked at.  The RSTm in front of it, in order, must be exactly
 *              intervals - 1 with m = 0, 1, .. 7, 0, ..; interval k is the bytes between marker k - 1 and marker k and holds the
 *              MCUs k restart_interval .. An FF inside an interval that is not followed by 00 (a fill byte in front of a marker)
 *              ends its data.  Fewer than 8 bits may be left behind an interval's last MCU.  The device finds the markers: a launch
 *              scans the scan's bytes and compacts the positions in order (gsr_scan.h), then checks count and numbering.
 *   3 dequant  coefficient x Q of the same position, moved from zigzag to natural order.
 *   4 IDCT     libjpeg's jidctint.c (islow), constants at 13 bits.  One pass over x0 .. x7:
 *                z1 = (x2 + x6) 4433;  t2 = z1 - x6 15137;  t3 = z1 + x2 6270;  t0 = (x0 + x4) << 13;  t1 = (x0 - x4) << 13
 *                t10 = t0 + t3;  t13 = t0 - t3;  t11 = t1 + t2;  t12 = t1 - t2
 *                a0 = x7, a1 = x5, a2 = x3, a3 = x1;  z1 = a0 + a3;  z2 = a1 + a2;  z3 = a0 + a2;  z4 = a1 + a3;  z5 = (z3 + z4) 9633
 *                a0 = a0 2446;  a1 = a1 16819;  a2 = a2 25172;  a3 = a3 12299
 *                z1 = -z1 7373;  z2 = -z2 20995;  z3 = -z3 16069 + z5;  z4 = -z4 3196 + z5
 *                a0 += z1 + z3;  a1 += z2 + z4;  a2 += z2 + z3;  a3 += z1 + z4
 *                y0 / y7 = t10 +- a3;  y1 / y6 = t11 +- a2;  y2 / y5 = t12 +- a1;  y3 / y4 = t13 +- a0
 *              Columns first: w = (y + 1024) >> 11.  Then rows over w: v = (y + (1 << 17)) >> 18.  Sample = clamp(v + 128, 0, 255).
 *              (libjpeg's shortcuts for columns and rows without AC terms give the same values and are not taken.)
 *   5 chroma   n = ceil(W / hs) and r = ceil(H / vs) are the chroma planes' used width and height; samples of the padded blocks
 *              beyond them are never read.  hs = 1: none.  n <= 2: every chroma sample is replicated hs x vs times (libjpeg does not
 *              use its fancy filter on so narrow a plane).  Otherwise
 *              4:2:0   output row 2k:     s[i] = 3 p[k][i] + p[max(k - 1, 0)][i];   row 2k + 1:  s[i] = 3 p[k][i] + p[min(k + 1, r - 1)][i]
 *                      out[2i] = (3 s[i] + s[max(i - 1, 0)] + 8) >> 4;   out[2i + 1] = (3 s[i] + s[min(i + 1, n - 1)] + 7) >> 4
 *              4:2:2   out[2i] = (3 p[i] + p[i - 1] + 1) >> 2;   out[2i + 1] = (3 p[i] + p[i + 1] + 2) >> 2;   out[0] = p[0];
 *                      out[2n - 1] = p[n - 1]
 *   6 colour   cb, cr = the upsampled samples - 128.   R = Y + ((91881 cr + 32768) >> 16)
 *              G = Y + ((-22554 cb - 46802 cr + 32768) >> 16)      B = Y + ((116130 cb + 32768) >> 16)      each clamped to 0 .. 255.
 *              Grey: the output is Y.
 * Pinned by PIL 12.2 on libjpeg-turbo (tests/test_jpeg_decode.py): all six rules, 4:2:2 included, on files PIL wrote (optimised
 * tables and restart markers included) and on files of gsr_jpeg_encode's rules.  Not pinned: a crafted file whose dequantised values
 * overflow these sums or leave libjpeg's range-limit table gets unspecified pixels (and every bound below).
 *
 *   status codes
 *     0 GSR_JPEG_DECODE_OK
 *     1 GSR_JPEG_DECODE_TRUNCATED    no marker closes the scan, or the scan's last interval ends before its last MCU
 *     2 GSR_JPEG_DECODE_BAD_CODE     a bit pattern of 16 bits with no symbol
 *     3 GSR_JPEG_DECODE_BAD_SYMBOL   a DC category above 11, an AC size above 10, or size 0 with a run other than 0 and 15
 *     4 GSR_JPEG_DECODE_OVERRUN      a run, or a ZRL, that leaves no coefficient up to 63 for a value
 *     5 GSR_JPEG_DECODE_RESTART      wrong count or numbering of the RST markers; a marker inside an interval (its data ends before
 *                                    its last MCU); a whole byte or more left behind an interval's last MCU
 *     6 GSR_JPEG_DECODE_TABLE        an entry of gsr_jpeg_file that points outside `bytes`, `out`, the tables or the workspace, sizes or
 *                                    sampling outside the accepted set, an interval count that is not the geometry's: such a file
 *                                    is not touched.  Also a Huffman table with more codes of a length than a prefix code has
 *                                    room for, or more than 256 codes.
 *   The order: TABLE; then the markers of rule 2 (TRUNCATED when nothing closes the scan, else RESTART); then the intervals, of
 *   which the first failing one in scan order decides.  A failed file's picture is unspecified; the other files of the batch are
 *   not affected.
 *   safety     every read of `bytes` is bounded by the file's scan and by nbytes, every write by the block, plane or picture it
 *              belongs to, every table index is checked before the launch that follows it, and every loop consumes a bit or a
 *              coefficient.  A corrupt file ends in a code.
 *
 * gsr_jpeg_decode_workspace_bytes(area_bytes, nfiles, nintervals): area_bytes = the end of the last coefficient or plane area; the
 * call's own tables (four words per interval) follow it.  0 for counts <= 0 or an area of 2^40 bytes or more.
 * gsr_jpeg_decode: all pointers are device pointers (bytes, out, workspace and quant 16-byte aligned, files 8, status 4); the
 * launches go on `stream`: validate (a workgroup per file), markers (a workgroup per file: a thread per run of 64 bytes, ordered
 * compaction), entropy (a one-wave workgroup per restart interval: lookup tables in LDS, the 64 lanes in lockstep, lane k keeping
 * coefficient k of the block in a register; int16 coefficients in natural order, blocks in scan order), status (a thread per
 * file), idct (a thread per column, then per row, of a block: dequantise, both passes through LDS, range limit -> uint8 planes),
 * colour (a thread per four output pixels of a row: upsampling, conversion, the HWC store).  It allocates nothing, never
 * synchronises, reads nothing back, and uses no global atomics: the same input gives the same bytes.  A file without restart
 * markers is ONE interval: one wavefront decodes its whole scan -- correct, and slow.
 * Rejected before launching (GSR_ERR_INVALID_ARGUMENT): NULL pointers, nfiles, nintervals, nquant or nhuffman <= 0, nfiles > 65535, nbytes or
 * out_bytes of 2^32 or more, a misaligned pointer, a workspace below its tables' part.
 * gsr_jpeg_decode_status_name(code): "ok", "truncated", ...; "?" for any other value.
 */
#ifndef GSRASTER_JPEG_DECODE_H
#define GSRASTER_JPEG_DECODE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gsr_jpeg_huffman {
    uint8_t bits[16];
    uint8_t values[256];
} gsr_jpeg_huffman;
typedef struct gsr_jpeg_file {
    uint64_t scan_offset, out_offset, coef_offset, plane_offset;
    uint32_t scan_length;
    int32_t H, W, C, hs, vs, restart_interval, first_interval, intervals;
    int32_t quant[3];
    int32_t dc[3];
    int32_t ac[3];
} gsr_jpeg_file;
enum {
    GSR_JPEG_DECODE_OK = 0, GSR_JPEG_DECODE_TRUNCATED, GSR_JPEG_DECODE_BAD_CODE, GSR_JPEG_DECODE_BAD_SYMBOL, GSR_JPEG_DECODE_OVERRUN,
    GSR_JPEG_DECODE_RESTART, GSR_JPEG_DECODE_TABLE
};
size_t gsr_jpeg_decode_workspace_bytes(size_t area_bytes, int nfiles, int nintervals);
int gsr_jpeg_decode(const uint8_t* bytes, size_t nbytes, const gsr_jpeg_file* files, int nfiles, int nintervals, const uint16_t* quant,
                    int nquant, const gsr_jpeg_huffman* huffman, int nhuffman, uint8_t* out, size_t out_bytes, int32_t* status,
                    void* workspace, size_t workspace_bytes, void* stream /* hipStream_t */);
const char* gsr_jpeg_decode_status_name(int code);

#ifdef __cplusplus
}
#endif
#endif
