/*
 * ppfs_ecc.h -- C ABI of the MI355X (gfx950) per-block ECC engine.
 *
 * This is the drop-in boundary underneath PPFS's IBlockDevice layer
 * (reference: lib/blockdevice/include/ppfs/blockdevice/iblock_device.hpp:34-97).
 * Each entry point replaces the per-block arithmetic of one reference codec with a batch
 * of blocks processed by hand-written HIP kernels:
 *
 *   ppfs_ecc_encode  <- ReedSolomonBlockDevice::_encodeBlock   rs_block_device.cpp:95-117
 *                       CrcBlockDevice::_calculateAndWrite     crc_block_device.cpp:37-67
 *                       HammingBlockDevice::_encodeData        hamming_block_device.cpp:76-109
 *                       ParityBlockDevice::writeBlock (parity) parity_block_device.cpp:49-54
 *   ppfs_ecc_decode  <- ReedSolomonBlockDevice::_fixBlockAndExtract  rs_block_device.cpp:119-183
 *                       CrcBlockDevice::_readAndCheckRaw             crc_block_device.cpp:12-35
 *                       HammingBlockDevice::_readAndFixBlock/_extractData hamming_block_device.cpp:21-74
 *                       ParityBlockDevice::_checkParity              parity_block_device.cpp:90-97
 *   ppfs_ecc_write   <- IBlockDevice::writeBlock of a full payload at offset 0
 *                       (read-modify-write: check/fix the old block, then encode)
 *   ppfs_ecc_create  <- PpFS::_createAppropriateBlockDevice   lib/filesystem/src/ppfs.cpp:35-70
 *
 * Conventions
 *   - Plain pointers and sizes only; no exceptions cross the ABI.  Return 0 on success or a
 *     negative errno-style code.
 *   - Blocks are packed: raw block i at raw + i*raw_block_size, payload i at
 *     data + i*data_size (the on-disk image layout: IDisk address = index * rawBlockSize()).
 *   - *_device functions take device pointers and a hipStream_t passed as void* (NULL =
 *     the null stream); they enqueue work and return without synchronising.
 *   - *_host functions take host pointers, stage through pinned buffers with overlapped
 *     H2D / kernel / D2H, and return after the results are in host memory.
 *   - Per-block status bytes use FsError values (lib/common/include/ppfs/common/types.hpp):
 *       PPFS_ECC_OK (0), PPFS_ECC_CORRECTED (1: the reference writes the block back and logs
 *       an ErrorCorrectionEvent), PPFS_ECC_CORRECTION_ERROR (5 = BlockDevice_CorrectionError),
 *       PPFS_ECC_OUT_OF_BOUNDS (9 = Disk_OutOfBounds, block-list calls only).
 *   - One context per (host thread, GPU); a context is not internally locked.
 */
#ifndef PPFS_ECC_H
#define PPFS_ECC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ECCType (lib/blockdevice/include/ppfs/blockdevice/ecc_type.hpp:8-14) */
enum ppfs_ecc_type {
    PPFS_ECC_NONE = 0,
    PPFS_ECC_CRC = 1,
    PPFS_ECC_HAMMING = 2,
    PPFS_ECC_PARITY = 3,
    PPFS_ECC_REED_SOLOMON = 4
};

enum ppfs_ecc_status {
    PPFS_ECC_OK = 0,
    PPFS_ECC_CORRECTED = 1,
    PPFS_ECC_CORRECTION_ERROR = 5,
    PPFS_ECC_OUT_OF_BOUNDS = 9 /* FsError::Disk_OutOfBounds: a block-list entry past the image */
};

/* Error codes returned by the entry points. */
#define PPFS_ECC_EINVAL (-22)
#define PPFS_ECC_ENOMEM (-12)
#define PPFS_ECC_EHIP (-5)
#define PPFS_ECC_ENOTSUP (-95)

/* Parameters persisted in the SuperBlock (super_block.hpp:20-23) / FsConfig (types.hpp:47-70). */
typedef struct ppfs_ecc_params {
    uint32_t ecc_type;             /* enum ppfs_ecc_type */
    uint32_t block_size;           /* FS block size in bytes (<= 4096, MAX_BLOCK_SIZE) */
    uint32_t rs_correctable_bytes; /* Reed-Solomon t (clamped to min(block,255)/2 like the reference) */
    uint32_t reserved;
    uint64_t crc_polynomial;       /* CRC polynomial in EXPLICIT form (CrcPolynomial::MsgExplicit) */
} ppfs_ecc_params;

typedef struct ppfs_ecc_ctx ppfs_ecc_ctx;

/* Convert a config-file ("implicit +1") CRC polynomial to the explicit form:
 * CrcPolynomial::MsgImplicit, crc_polynomial.cpp:41-54.  */
uint64_t ppfs_ecc_crc_implicit_to_explicit(uint64_t implicit_poly);

/* Create a codec context on HIP device `device`.  Validates params with the reference's
 * clamping rules; builds and uploads the codec tables.  */
int ppfs_ecc_create(const ppfs_ecc_params* params, int device, ppfs_ecc_ctx** out);
void ppfs_ecc_destroy(ppfs_ecc_ctx* ctx);

/* IBlockDevice::rawBlockSize() / dataSize() of the equivalent reference device. */
size_t ppfs_ecc_raw_block_size(const ppfs_ecc_ctx* ctx);
size_t ppfs_ecc_data_size(const ppfs_ecc_ctx* ctx);

/* Short human-readable name of the kernel path the context dispatches to (for logs/tests). */
const char* ppfs_ecc_kernel_name(const ppfs_ecc_ctx* ctx);
/* The kernel path a device call of ctx on `stream` takes: as ppfs_ecc_kernel_name, except for
 * RS 2t <= 8 and 2t = 32, whose ticket-counter kernels need one of the context's 16 per-stream
 * counter sets: a 17th distinct stream, and any stream capturing a hipGraph, get the static-walk
 * kernels ("rs255-wg-seg4-lds" / "rs255-bs-byte-lds-static").  Engine extension, no reference
 * counterpart. */
const char* ppfs_ecc_stream_kernel_name(ppfs_ecc_ctx* ctx, void* stream);

/*
 * Device pointers of the three contiguous calls below.  A call may name any sub-range of a larger
 * buffer (blocks [first, first + n): d_raw + first * rawBlockSize(), d_data + first * dataSize(),
 * d_status + first); it touches the rows of its nblocks blocks only.  Per codec:
 *   RS, fast paths (rawBlockSize() == 255 and 2t one of 2, 4, 6, 8, 10, 16, 32; ppfs_ecc_kernel_name()
 *       is not "rs-generic-lfsr"): d_raw, and the d_data and d_status the call passes, must be 16-byte
 *       aligned, else PPFS_ECC_EINVAL with nothing queued or written.  The write call is its decode
 *       (d_raw, a caller's d_status) and its encode (d_data, d_raw): a d_status inherits the decode's
 *       rule, a NULL one is replaced by the context's own aligned array.
 *   RS, generic path (shortened codes, every other 2t): any address, d_spill included.
 *   Hamming: d_raw must be 16-byte aligned when rawBlockSize() >= 8, else PPFS_ECC_EINVAL with
 *       nothing queued or written; d_data and d_status may have any address, and for blocks of 1, 2
 *       and 4 bytes d_raw too.
 *   CRC, parity: any address.
 * 1, 2 and 4 KiB CRC (degree <= 32), Hamming and parity contexts run their streaming kernels when
 * d_data and d_raw are 16-byte aligned (a NULL d_data counts as aligned) and the generic
 * wave-per-block kernels otherwise -- same results, lower rate;
 * ppfs_ecc_kernel_name() names the streaming path either way.  d_status may always have any address.
 * hipMalloc and torch allocations are 256-byte aligned; a sub-range is aligned when its offsets are
 * multiples of 16.
 */

/*
 * Encode nblocks full payloads.  raw is read-modify-write: bits the codec does not define
 * (CRC unused tail bits when degree % 8 != 0, Hamming bits after the last data bit) keep
 * raw's previous contents exactly as the reference's writeBlock keeps the old block's.
 */
int ppfs_ecc_encode_device(ppfs_ecc_ctx* ctx, const uint8_t* d_data, uint8_t* d_raw, size_t nblocks,
    void* stream);

/*
 * Decode / check nblocks raw blocks.
 *   d_data    (may be NULL) receives the payloads (undefined for blocks with status 5).
 *   d_status  (may be NULL) receives one status byte per block.
 *   write_back != 0 applies the reference's write-back to d_raw in place (RS: the corrected
 *             bytes of the codeword; Hamming: the one flipped byte).
 *   d_spill   (RS only, may be NULL; meaningful only when rawBlockSize() < 255): per block
 *             (256 - rawBlockSize()) bytes: [0] = bytes the reference's write-back writes
 *             past the end of the block, [1..] = those bytes.  Blocks are decoded
 *             independently; a spill is reported, never applied to the neighbouring block.
 */
int ppfs_ecc_decode_device(ppfs_ecc_ctx* ctx, uint8_t* d_raw, uint8_t* d_data, uint8_t* d_status,
    size_t nblocks, int write_back, uint8_t* d_spill, void* stream);

/*
 * writeBlock(full payload, {i, 0}) for nblocks blocks: check/fix the old block held in
 * d_raw, then encode d_data into it.  d_status (may be NULL): 0, 1 (old block corrected and
 * logged), 5 (old block failed its check: the reference returns CorrectionError and leaves
 * the block untouched -- CRC, parity, uncorrectable Hamming).
 */
int ppfs_ecc_write_device(ppfs_ecc_ctx* ctx, const uint8_t* d_data, uint8_t* d_raw, uint8_t* d_status,
    size_t nblocks, void* stream);

/* Host-memory variants (chunked, H2D/kernel/D2H overlapped on two streams).  Pageable caller
 * buffers go through the context's pinned staging buffers (one CPU copy each way); when every
 * caller buffer of the call is page-locked (hipHostMalloc, or ppfs_ecc_host_register below) the
 * chunks are DMA'd straight between the caller's memory and the device. */
int ppfs_ecc_encode_host(ppfs_ecc_ctx* ctx, const uint8_t* data, uint8_t* raw, size_t nblocks);
int ppfs_ecc_decode_host(ppfs_ecc_ctx* ctx, uint8_t* raw, uint8_t* data, uint8_t* status, size_t nblocks,
    int write_back, uint8_t* spill);
int ppfs_ecc_write_host(ppfs_ecc_ctx* ctx, const uint8_t* data, uint8_t* raw, uint8_t* status,
    size_t nblocks);
/* Blocks per staging chunk of the host calls above (16 MiB of codewords, a multiple of 1 Ki).  A
 * decode with write-back of RS(255, k) or Hamming returns the bytes its write-back changed as a
 * patch list that the host writes into raw; other codecs return the changed codewords whole.
 * Engine extension, no reference counterpart. */
size_t ppfs_ecc_host_chunk_blocks(ppfs_ecc_ctx* ctx);

/*
 * Block lists: "these nblocks block indices of this image, in this order" -- what FileIO::readFile /
 * writeFile get from their BlockIndexIterator (lib/file_io/src/file_io.cpp:27-35, 53-69) for a file
 * whose blocks lie wherever the bitmap allocator put them.  Engine extension of readBlocks /
 * writeBlocks; one call instead of one per contiguous run.
 *   d_image / image   packed raw blocks from block 0, image_blocks of them
 *   d_index / index   nblocks unsigned 32-bit block indices
 * Entry i gets exactly what the contiguous call gives block index[i]; payload i (data + i*dataSize()),
 * status i and spill record i are in LIST order.
 *   decode  the listed blocks are decoded; with write_back != 0 the blocks with status 1 are written
 *           back into the image (RS, Hamming).  With write_back == 0, and for CRC / parity / none, the
 *           image is not written at all.  d_data, d_status, d_spill may be NULL as in
 *           ppfs_ecc_decode_device; a shortened RS code's spill (n < 255) is reported per entry and
 *           never applied.
 *   encode  block index[i] = encode(payload i); the bits the codec leaves undefined (and the parity
 *           byte's bits above bit 0) keep the image's contents, as in ppfs_ecc_encode_device.
 *   write   writeBlock(payload i, {index[i], 0}): status 0 / 1 / 5 as ppfs_ecc_write_device; a block
 *           with status 5 stays untouched.
 * An entry with index[i] >= image_blocks is not an error of the call: it gets status
 * PPFS_ECC_OUT_OF_BOUNDS (9) and a zero payload, and touches nothing of the image.
 * Repeated indices:
 *   - encode and write: the indices of one call must be distinct (device forms).  With a repeated
 *     index the call stays memory-safe, but which payload ends up in the block is unspecified.
 *   - decode may repeat an index: every copy gets the same payload.  With write_back, a repeated
 *     entry's status is that of a read either before or after another copy's write-back (1 or 0).
 *     On the direct path (below) a copy's read may also see another copy's write-back partly applied.
 *     For a block within the code's capability (at most t byte errors), and for one whose
 *     miscorrection lands on a codeword, every such view is within t of the same codeword: every copy
 *     gets the same payload, each status is 1 or 0, at least one copy reports 1 and the image ends
 *     corrected.  Only for a block beyond the capability whose fix lands on no codeword, listed more
 *     than once with write_back, may the copies of one call differ in payload and status (on the
 *     staged path they already differ across pieces).
 *   - the host forms process the list in runs without a repeated index, so their result equals the
 *     per-block calls made in list order: the first entry of a corrupted block reports 1, a later
 *     one reads the written-back block; for encode / write the last payload listed wins.
 * Device forms: the rows are gathered into staging memory the context owns (made at the first list
 * call, ppfs_ecc_host_chunk_blocks(ctx) blocks rounded down to a multiple of 1 Ki; longer lists run
 * in pieces of that many blocks on `stream`), the codec runs on the copy, and the changed rows are
 * scattered back.  d_data / d_status / d_spill keep the alignment rules of the contiguous calls
 * (16 bytes for RS and Hamming).  The staging is shared by all streams of the context: each list
 * call waits for the previous list call of that context, whichever stream it ran on.  A stream that
 * is capturing a hipGraph gets PPFS_ECC_ENOTSUP.  Null ctx or required pointer: -EINVAL, checked
 * before anything touches the GPU; nblocks == 0 returns 0.
 * Direct list decode: a context of RS(255, 255 - 2t) with 2t <= 8 (block_size >= 255, t = 1..4) decodes
 * a list in ONE kernel (ppfs_ecc_list_kernel_name: "rs255-wg-list-lds"): the codec kernel reads each
 * listed row straight from the image, writes corrected bytes in place at image + index[i] * 255 + pos and
 * emits payloads and statuses in list order.  No staging copy, no pieces, and no ordering against the
 * context's other list calls: two such decodes on different streams run side by side like two
 * contiguous calls (that ordering only ever protected the staging, never results).  The image may have
 * any alignment; nothing outside [d_image, d_image + image_blocks * 255) is read or written.
 * Direct list encode and write: the same contexts (ppfs_ecc_list_encode_kernel_name:
 * "rs255-wg-list-store-lds") encode a list in ONE kernel, which stores codeword i at
 * d_image + index[i] * 255 itself: every byte of a listed row is written once, no byte outside the
 * listed rows is written, and nothing of the image is read, so neighbouring rows may be written by
 * other calls at the same time.  A write list is the list decode for the old blocks' statuses (it
 * changes nothing of the image) followed by that encode on `stream`; with d_status == NULL the encode
 * alone, since an RS write needs nothing else of the old block.  Like the direct decode these calls
 * use no staging and no pieces, and direct encode / write lists of one context on different streams
 * are not ordered against each other or against the context's other list calls.  Repeated indices
 * stay memory-safe with an unspecified result: each byte of such a row is the corresponding byte of
 * one of the listed payloads' codewords.
 * Every other codec, and a call whose d_data / d_status break the 16-byte rule, keep the staged path
 * above; so does a context created while PPFS_ECC_LIST_DIRECT=0 is in the environment (A/B
 * measurements).  The extent calls below use the same kernels per piece for such a context.
 * Host forms: same arguments with host pointers and no stream; they return when the results are in
 * host memory.
 */
/* How ctx decodes a device list: "rs255-wg-list-lds" (the direct kernel) or "gather-stage-scatter" (the
 * staged pipeline); "" for a null ctx.  Engine extension, no reference counterpart. */
const char* ppfs_ecc_list_kernel_name(const ppfs_ecc_ctx* ctx);
/* How ctx encodes and writes a device list: "rs255-wg-list-store-lds" (the direct kernel) or
 * "gather-stage-scatter" (the staged pipeline); "" for a null ctx.  Engine extension, no reference
 * counterpart. */
const char* ppfs_ecc_list_encode_kernel_name(const ppfs_ecc_ctx* ctx);
int ppfs_ecc_decode_list_device(ppfs_ecc_ctx* ctx, uint8_t* d_image, size_t image_blocks, const uint32_t* d_index,
    size_t nblocks, uint8_t* d_data, uint8_t* d_status, int write_back, uint8_t* d_spill, void* stream);
int ppfs_ecc_encode_list_device(ppfs_ecc_ctx* ctx, const uint8_t* d_data, uint8_t* d_image, size_t image_blocks,
    const uint32_t* d_index, size_t nblocks, void* stream);
int ppfs_ecc_write_list_device(ppfs_ecc_ctx* ctx, const uint8_t* d_data, uint8_t* d_image, size_t image_blocks,
    const uint32_t* d_index, uint8_t* d_status, size_t nblocks, void* stream);
int ppfs_ecc_decode_list_host(ppfs_ecc_ctx* ctx, uint8_t* image, size_t image_blocks, const uint32_t* index,
    size_t nblocks, uint8_t* data, uint8_t* status, int write_back, uint8_t* spill);
int ppfs_ecc_encode_list_host(ppfs_ecc_ctx* ctx, const uint8_t* data, uint8_t* image, size_t image_blocks,
    const uint32_t* index, size_t nblocks);
int ppfs_ecc_write_list_host(ppfs_ecc_ctx* ctx, const uint8_t* data, uint8_t* image, size_t image_blocks,
    const uint32_t* index, uint8_t* status, size_t nblocks);

/*
 * Byte extents: "these n byte ranges of those blocks" -- a batch of (block, offset, length), the form
 * in which the callers of IBlockDevice really read and write.  FileIO::readFile / writeFile
 * (lib/file_io/src/file_io.cpp:24-42, 50-88) start at offset % dataSize() in their first block and stop
 * mid-block in their last; the inode table, bitmap and directory code write a few bytes at
 * DataLocation{block, offset}.  Entry i is one readBlock({block, offset}, length) or
 * writeBlock(bytes, {block, offset}) of the reference (rs_block_device.cpp:25-93,
 * crc_block_device.cpp:69-122, hamming_block_device.cpp:111-162, parity_block_device.cpp:31-88), the
 * entries taken in list order.  Engine extension; no reference counterpart as a batch.
 *   d_ext / ext    n entries (8-byte aligned); entry i's bytes lie at [pos, pos + len) of the packed
 *                  caller buffer, len = min(length, dataSize() - offset) (the reference's clamp;
 *                  offset == dataSize() is a valid access of zero bytes)
 *   d_out / d_in   the packed caller buffer of out_bytes / in_bytes, any alignment
 *   read   out[pos, pos + len) = payload bytes [offset, offset + len) of the block.  Status 0 / 1 / 5 as
 *          ppfs_ecc_decode_device; with write_back != 0 the blocks with status 1 are written back into
 *          the image (RS, Hamming) exactly as by ppfs_ecc_decode_list_*.  An entry with status 5 gets
 *          len zero bytes.  Bytes of out that no entry covers are not written.
 *   write  the old block is checked and fixed, payload bytes [offset, offset + len) are replaced by
 *          in[pos, pos + len) and the block is encoded again; the bits the codec leaves undefined keep
 *          their contents as in ppfs_ecc_encode_device.  Status 0 / 1 / 5 as ppfs_ecc_write_device; a
 *          block with status 5 stays untouched.  len == 0 is legal: the block is checked and encoded
 *          again with its own payload.
 * An entry is invalid when block >= image_blocks (or block == 0xFFFFFFFF), offset > dataSize(), or
 * pos + len > out_bytes / in_bytes.  It gets status PPFS_ECC_OUT_OF_BOUNDS (9), reads and writes
 * nothing, and does not fail the call.  Whatever the entries say, no call touches memory outside the
 * image and the packed buffer.
 * Repeats: a read may repeat a block under the rules of decode_list; where two read entries overlap
 * in out, which bytes win is unspecified.  Device writes need distinct blocks within one call, as
 * ppfs_ecc_write_list_device does.  The host forms cut the list where a valid block repeats, so their
 * result equals the per-block calls made in list order: two entries that write different byte ranges
 * of one block both land.
 * Device forms: the list calls' pipeline (gather, codec on the staging copy, scatter) in pieces of the
 * same size on `stream`, plus a second staging allocation for the decoded payloads made at the first
 * extent call; they wait for and are waited for by the context's staged list calls.  A context that
 * decodes lists directly (ppfs_ecc_list_kernel_name) reads a piece with that one kernel in place of the
 * gather, decode, scatter and range marks, and writes a piece as that list decode (old payloads and
 * statuses, nothing written back), the overlay of the caller's bytes and the list encode
 * (ppfs_ecc_list_encode_kernel_name) in place of gather, decode, overlay, write, scatter and range
 * marks; the payload staging, the pieces and their ordering stay.
 * A capturing stream gets
 * PPFS_ECC_ENOTSUP.  There is no spill argument: a shortened RS code (n < 255) is decoded as by a list
 * decode with d_spill == NULL.  PPFS_ECC_NONE: plain byte copies under the same validity rules.
 * d_status / status may be NULL.  Null ctx or a required pointer missing: -EINVAL before anything
 * touches the GPU; n == 0 returns 0.
 */
typedef struct ppfs_ecc_extent { /* 16 bytes, no padding */
    uint64_t pos;    /* where this entry's bytes lie in the packed caller buffer */
    uint32_t block;  /* block index in the image */
    uint16_t offset; /* DataLocation::offset: first payload byte */
    uint16_t length; /* bytes asked for */
} ppfs_ecc_extent;

int ppfs_ecc_read_extents_device(ppfs_ecc_ctx* ctx, uint8_t* d_image, size_t image_blocks, const ppfs_ecc_extent* d_ext,
    size_t n, uint8_t* d_out, size_t out_bytes, uint8_t* d_status, int write_back, void* stream);
int ppfs_ecc_write_extents_device(ppfs_ecc_ctx* ctx, const uint8_t* d_in, size_t in_bytes, uint8_t* d_image,
    size_t image_blocks, const ppfs_ecc_extent* d_ext, size_t n, uint8_t* d_status, void* stream);
int ppfs_ecc_read_extents_host(ppfs_ecc_ctx* ctx, uint8_t* image, size_t image_blocks, const ppfs_ecc_extent* ext, size_t n,
    uint8_t* out, size_t out_bytes, uint8_t* status, int write_back);
int ppfs_ecc_write_extents_host(ppfs_ecc_ctx* ctx, const uint8_t* in, size_t in_bytes, uint8_t* image, size_t image_blocks,
    const ppfs_ecc_extent* ext, size_t n, uint8_t* status);

/*
 * Whole-image scrub: the disk-image effect of readBlock(i, 0, dataSize()) for
 * i = 0 .. nblocks-1 in index order, without the payloads -- RS writes back the corrected
 * codeword (rs_block_device.cpp:175-180), Hamming the flipped byte (hamming_block_device.cpp:41-51),
 * CRC and parity only check (crc_block_device.cpp:12-35, parity_block_device.cpp:90-97).
 *   image        packed raw blocks from block 0; image_bytes >= nblocks * rawBlockSize() is the
 *                extent a write-back may touch (a shortened RS code, n < 255, can write up to
 *                255 - n bytes past a block end: into the next blocks, which are then scrubbed as
 *                modified, as the sequential reference reads them; a write-back that would pass
 *                image_bytes is rejected whole, like HeapDisk::write, heap_disk.cpp:21-27).
 *   status       (may be NULL) one status byte per block.
 *   counts       (host form, may be NULL) [blocks ok, blocks corrected, blocks failed].
 * The device form enqueues on `stream`; with n < 255 it synchronises between runs of blocks.
 */
int ppfs_ecc_scrub_host(ppfs_ecc_ctx* ctx, uint8_t* image, size_t image_bytes, size_t nblocks, uint8_t* status,
    size_t* counts);
int ppfs_ecc_scrub_device(ppfs_ecc_ctx* ctx, uint8_t* d_image, size_t image_bytes, size_t nblocks,
    uint8_t* d_status, void* stream);

/*
 * Scrub of named blocks only: a block list, or the blocks an allocation bitmap marks.  After an
 * irradiation run the blocks that matter are the ones the allocator handed out; free blocks may never have
 * been written, cost HBM traffic, and their failures would drown the "failed" count of a sparsely filled
 * CRC or parity device.  Engine extension; the reference has no scrub at all.
 *
 * counts record: 64 bytes, OVERWRITTEN (not accumulated) by each call; may be NULL.  d_counts is 8-byte
 * aligned device memory.
 *
 * ppfs_ecc_scrub_list_*: exactly ppfs_ecc_decode_list_* with data == NULL, write_back = 1 and
 * spill == NULL, plus the counts.  Everything is the list decode's: statuses in list order, status 9 for
 * an entry out of range (it touches nothing), the repeated-index rules, the direct / staged choice and
 * the alignment rule of d_status.  d_status / status and d_counts / counts may each be NULL; when only
 * the counts are wanted the call uses a status scratch of its own (device form: the context's scrub
 * scratch, below).  The device form never synchronises `stream`; a capturing stream gets
 * PPFS_ECC_ENOTSUP.  Every entry counts once, repeated ones included.
 *
 * ppfs_ecc_scrub_allocated_*: the reference's on-disk bitmap (lib/bitmap/src/bitmap.cpp), consumed as it
 * lies in the image.
 *   bitmap_block   first block of the bitmap; it spans B = ceil(ceil(nbits / 8) / dataSize()) blocks
 *                  (Bitmap::blocksSpanned, bitmap.cpp:27-31; integer arithmetic here, float there)
 *   first_block    bit j stands for image block first_block + j
 *   nbits          bits of the bitmap.  Bit j is byte j / 8 of the payloads of the B blocks taken back to
 *                  back, under mask 0x80 >> (j % 8) (bitmap.cpp:8-14, 98-100)
 *   d_status       (may be NULL) nbits bytes, any alignment: 0, 1, 5 or 9 for a set bit,
 *                  PPFS_ECC_NOT_ALLOCATED for a clear one, whose block is not read
 *   d_bitmap_status (may be NULL) B bytes, any alignment: the statuses of the bitmap's own blocks
 * In this order: (1) the B bitmap blocks are decoded with write-back, scrubbed like any read of them
 * (bitmap_* counts); (2) the bits are expanded into the ascending list of allocated blocks, the bits of a
 * bitmap block with status 5 counting as SET: its payload is undefined, so every block it covers is
 * scrubbed; (3) that list is list-scrubbed; (4) the per-bit statuses and the counts are written.  A data
 * block at or past image_blocks gets status 9, as a list entry would.
 * Shortened RS (n < 255): blocks are decoded independently and a spill is never applied, as in every list
 * call.  This DIFFERS from ppfs_ecc_scrub_*, which chains a spill into the following blocks as the
 * sequential reference does.
 * Errors: PPFS_ECC_EINVAL, checked before anything touches the GPU, for a null ctx or image,
 * dataSize() == 0, bitmap_block + B > image_blocks, or first_block + nbits passing 2^32.  nbits == 0
 * returns 0 with zeroed counts.
 * Device form: the bit range runs in pieces of 1 Mi bits, which bounds the scratch (4 bytes of index and
 * 1 byte of status per bit).  The scratch is the context's: stream-ordered pool memory made on the
 * context's own stream at the first scrub call that needs it (a larger one when a later call needs
 * more), kept until ppfs_ecc_destroy and shared by all streams of the context, so a scrub call that uses
 * it waits for the previous one, whichever stream that ran on; no call allocates or frees on the
 * caller's stream.  Per piece the host reads back one 8-byte
 * count to size the list call: the call SYNCHRONISES `stream` once per piece (compare
 * ppfs_ecc_scrub_device, which synchronises between runs for n < 255) and returns with everything
 * queued.  A capturing stream gets PPFS_ECC_ENOTSUP.
 * Host form: ppfs_ecc_decode_host over the bitmap blocks in place, the same expansion on the CPU,
 * ppfs_ecc_decode_list_host, and a CPU tally.
 */
#define PPFS_ECC_NOT_ALLOCATED 255 /* status of a bit that is 0 in the bitmap: block not read (engine extension) */

typedef struct ppfs_ecc_scrub_counts { /* 64 bytes, overwritten (not accumulated) by each call */
    uint64_t ok, corrected, failed; /* data blocks / list entries with status 0, 1, 5 */
    uint64_t out_of_range;          /* status 9 */
    uint64_t not_allocated;         /* bitmap form only: bits that are 0 */
    uint64_t bitmap_ok, bitmap_corrected, bitmap_failed; /* bitmap form only: the bitmap's own blocks */
} ppfs_ecc_scrub_counts;

int ppfs_ecc_scrub_list_device(ppfs_ecc_ctx* ctx, uint8_t* d_image, size_t image_blocks, const uint32_t* d_index,
    size_t nblocks, uint8_t* d_status, ppfs_ecc_scrub_counts* d_counts, void* stream);
int ppfs_ecc_scrub_list_host(ppfs_ecc_ctx* ctx, uint8_t* image, size_t image_blocks, const uint32_t* index,
    size_t nblocks, uint8_t* status, ppfs_ecc_scrub_counts* counts);
int ppfs_ecc_scrub_allocated_device(ppfs_ecc_ctx* ctx, uint8_t* d_image, size_t image_blocks, uint32_t bitmap_block,
    uint32_t first_block, size_t nbits, uint8_t* d_status, uint8_t* d_bitmap_status, ppfs_ecc_scrub_counts* d_counts,
    void* stream);
int ppfs_ecc_scrub_allocated_host(ppfs_ecc_ctx* ctx, uint8_t* image, size_t image_blocks, uint32_t bitmap_block,
    uint32_t first_block, size_t nbits, uint8_t* status, uint8_t* bitmap_status, ppfs_ecc_scrub_counts* counts);

/*
 * Read a file from its inode: the read-only walk of the index-block tree on the GPU.  FileIO::readFile
 * (lib/file_io/src/file_io.cpp:12-44) gets its blocks from BlockIndexIterator (:186-463), which reads the
 * file's singly, doubly and trebly indirect index blocks one readBlock at a time (_readIndexBlock,
 * :465-480), each read depending on the one before.  Here the 64 bytes of the inode that describe the
 * tree are the argument, and the walk is at most three list decodes with an expansion kernel between
 * them.  Engine extension; read-only: nothing allocates or grows.
 *
 * The tree (inode.hpp:18-41): ds = dataSize(), ipb = ds / 4 entries per index block, little-endian
 * uint32 at payload bytes [4 slot, 4 slot + 4); payload bytes past 4 ipb are ignored.  A file occupies
 * ceil(file_size / ds) blocks, the tree holds 12 + ipb + ipb^2 + ipb^3 (its capacity, in 64 bits).  File
 * block j: j < 12 is direct[j]; s = j - 12 < ipb is entry s of `indirect`; s = j - 12 - ipb < ipb^2 is
 * entry s % ipb of the leaf named by entry s / ipb of `doubly_indirect`; s = j - 12 - ipb - ipb^2 < ipb^3
 * is entry s % ipb of the leaf named by entry (s / ipb) % ipb of the mid block named by entry s / ipb^2
 * of `trebly_indirect`.
 *
 * ppfs_ecc_file_span: readFile(offset, nbytes)'s first file block, block count and the bytes it delivers
 * (nbytes clamped to file_size - offset).  -EINVAL for offset >= file_size with nbytes > 0 and for a range
 * whose blocks pass the capacity; nbytes == 0 gives zeros.  Outputs may be NULL.  No GPU.
 * ppfs_ecc_file_tree_blocks: the number T of index blocks a walk over [first_block, first_block + nblocks)
 * visits, or a negative error under the rules below.  No GPU.
 *
 * ppfs_ecc_file_blocks_*: the image blocks of file blocks [first_block, first_block + nblocks).
 *   file          HOST pointer in both forms
 *   index         (may be NULL, 4-byte aligned) index[i] = image block of file block first_block + i;
 *                 0xFFFFFFFF where the path to it failed
 *   path_status   (may be NULL) 0, or the 5 / 9 inherited from the index block that failed above it
 *   tree_index / tree_status  (may be NULL) the T index blocks in LEVEL ORDER -- A: the roots visited, in
 *                 the order indirect, doubly_indirect, trebly_indirect; B: the doubly tree's leaves
 *                 ascending, then the trebly tree's mid blocks ascending; C: the trebly tree's leaves
 *                 ascending -- and their statuses 0 / 1 / 5 / 9
 *   counts        (may be NULL; device form: 8-byte aligned device memory) overwritten: index_* count the T
 *                 tree blocks by status, the first four the file blocks by path status
 *   write_back    applies to the index blocks, as in ppfs_ecc_decode_list_*
 * Each needed index block is decoded exactly once per call, as readBlock({b, 0}, 4 ipb) with the codec's
 * write-back.  An index block with status 5 (payload undefined) or 9 hands that status to everything under
 * it, whose pointer becomes 0xFFFFFFFF; status 1 is not handed down.  A pointer to an index block at or past
 * image_blocks gives that block status 9; it touches nothing.  A data pointer at or past image_blocks is
 * reported as it stands (the read gives it 9).
 * ppfs_ecc_read_file_*: ppfs_ecc_file_span's checks, the walk, then the extent read of FileIO::readFile's
 * shape: the first block from offset % ds, the last one up to where the bytes run out.
 *   out           out[0, clamped_bytes) is the file range; out_bytes >= clamped_bytes (-EINVAL otherwise);
 *                 bytes past clamped_bytes are not written
 *   status        (may be NULL) one byte per file block touched: the path status where that is non-zero,
 *                 else the read's 0 / 1 / 5 / 9.  The range of a block with status 5 is zero-filled (a failed
 *                 read, or a failed index block above it); a block with status 9 is not written
 *   counts        both halves: the file blocks by final status, the tree blocks as above
 *   write_back    applies to index and data blocks
 * Batch semantics: every block of the range is attempted; the reference stops at the first failure (the
 * adapters restore that result).  Shortened RS (n < 255): blocks are decoded independently and a spill is
 * dropped, as in every list call.  Repeated pointers (a corrupt or hand-made tree): the calls stay
 * memory-safe and results follow the repeated-index rules of ppfs_ecc_decode_list_*.
 * Errors: -EINVAL, checked before anything touches the GPU, for a null ctx, file, image or required
 * buffer, a misaligned index array or counts record, and blocks at or past ceil(file_size / ds) or the
 * capacity (so any block >= 12 when ds < 4).  nblocks == 0 / nbytes == 0 returns 0 with zeroed counts.
 * Device forms: up to three ppfs_ecc_decode_list_device calls (levels A, B, C) write payloads and statuses
 * into scratch, an expansion kernel runs after each, and the data blocks go through
 * ppfs_ecc_read_extents_device from extents built on the device, in pieces of 32 Ki file blocks.  The call
 * never synchronises `stream` and reads nothing back.  The scratch is the context's scrub scratch (see
 * ppfs_ecc_scrub_allocated_device: pool memory made on the context's stream, shared by all streams, each
 * call waits for the previous user, nothing is allocated or freed on the caller's stream): per tree block
 * ds + 6 bytes, every level rounded up to 16 entries so that the payload and status pointers keep the
 * 16-byte rule and a context that decodes lists directly keeps doing so -- with T <= about nblocks / ipb
 * that is some 4 + 6 / ipb bytes per file block -- plus 22 bytes per block of a piece (index, path status,
 * extent, read status: 704 KiB).  A capturing stream gets PPFS_ECC_ENOTSUP.
 * Host forms: ppfs_ecc_decode_list_host per level, the same plan on the CPU, ppfs_ecc_read_extents_host, a
 * CPU tally.
 */
typedef struct ppfs_ecc_file { /* 64 bytes: the fields of Inode the walk reads */
    uint32_t direct[12], indirect, doubly_indirect, trebly_indirect, file_size;
} ppfs_ecc_file;
typedef struct ppfs_ecc_file_counts { /* 64 bytes, overwritten by each call */
    uint64_t ok, corrected, failed, out_of_range;                         /* file blocks, inherited path statuses included */
    uint64_t index_ok, index_corrected, index_failed, index_out_of_range; /* the tree's own blocks */
} ppfs_ecc_file_counts;

int ppfs_ecc_file_span(const ppfs_ecc_ctx* ctx, const ppfs_ecc_file* file, uint64_t offset, uint64_t nbytes,
    uint64_t* first_block, uint64_t* nblocks, uint64_t* clamped_bytes);
long long ppfs_ecc_file_tree_blocks(const ppfs_ecc_ctx* ctx, const ppfs_ecc_file* file, uint64_t first_block,
    uint64_t nblocks);
int ppfs_ecc_file_blocks_device(ppfs_ecc_ctx* ctx, uint8_t* d_image, size_t image_blocks, const ppfs_ecc_file* file,
    uint64_t first_block, uint64_t nblocks, uint32_t* d_index, uint8_t* d_path_status, uint32_t* d_tree_index,
    uint8_t* d_tree_status, ppfs_ecc_file_counts* d_counts, int write_back, void* stream);
int ppfs_ecc_file_blocks_host(ppfs_ecc_ctx* ctx, uint8_t* image, size_t image_blocks, const ppfs_ecc_file* file,
    uint64_t first_block, uint64_t nblocks, uint32_t* index, uint8_t* path_status, uint32_t* tree_index,
    uint8_t* tree_status, ppfs_ecc_file_counts* counts, int write_back);
int ppfs_ecc_read_file_device(ppfs_ecc_ctx* ctx, uint8_t* d_image, size_t image_blocks, const ppfs_ecc_file* file,
    uint64_t offset, uint64_t nbytes, uint8_t* d_out, size_t out_bytes, uint8_t* d_status, ppfs_ecc_file_counts* d_counts,
    int write_back, void* stream);
int ppfs_ecc_read_file_host(ppfs_ecc_ctx* ctx, uint8_t* image, size_t image_blocks, const ppfs_ecc_file* file,
    uint64_t offset, uint64_t nbytes, uint8_t* out, size_t out_bytes, uint8_t* status, ppfs_ecc_file_counts* counts,
    int write_back);

/*
 * Read many files in one call: the walk above over a BATCH of inodes.  A
 * filesystem is mostly small files -- a directory is one -- and the single-file calls' cost is almost all
 * fixed.  Level A of all the files is one list, level B one list, level C one list and the data blocks one
 * extent stream, so a batch of any number of files costs the launches of one file.
 *
 * A batch is `nfiles` records (`files`, a HOST pointer in both forms) and `ranges`: NULL, or nfiles
 * (offset, nbytes) pairs, range f being readFile(offset, nbytes) of file f.  NULL means every file whole,
 * (0, file_size); an empty file is then a valid empty range.
 *
 * ppfs_ecc_files_plan: where each file's results lie.  Pure arithmetic, no GPU.  slots (may be NULL):
 * nfiles records; totals (may be NULL).
 *   first_block, blocks, bytes   ppfs_ecc_file_span of the file's range
 *   block_pos    its entries in the per-block arrays are [block_pos, block_pos + blocks), files back to back
 *                in batch order
 *   out_pos      its bytes in `out` are [out_pos, out_pos + bytes), files back to back, no padding
 *   tree_pos[3], tree_n[3]   its entries of levels A, B, C in the tree arrays, which are LEVEL-MAJOR: all
 *                files' level A entries in batch order, then all level B, then all level C; within one
 *                file's level the order is the single-file call's
 *   totals       blocks, bytes, tree entries per level, and their sum tree_blocks
 * -EINVAL, with the file's number in ppfs_ecc_last_error, for any range ppfs_ecc_file_span rejects: an
 * offset at or past the file's end with nbytes > 0, blocks past the tree's capacity.
 *
 * ppfs_ecc_files_blocks_*: ppfs_ecc_file_blocks_* of every file's range.  index / path_status: totals.blocks
 * entries; tree_index / tree_status: totals.tree_blocks entries; counts: ONE record for the whole batch.
 *   file_flags   (may be NULL, 4-byte aligned) one uint32 per file, an OR over its blocks: bit 0 = some
 *                data block corrected (1), bit 1 = failed (5), bit 2 = out of range (9); bits 8-10 the
 *                same for its index blocks.  0 = the file is intact.
 * Every output may be NULL as in the single-file call.
 * ppfs_ecc_read_files_*: the same walk, then the read.  out[out_pos, out_pos + bytes) is file f's range;
 * out_bytes >= totals.bytes (-EINVAL otherwise); status: one byte per file block touched, the path status
 * where non-zero, else the read's; file_flags from those final statuses.  Per block the single-file rules
 * hold: the range of a block under a failed index block (5) is zero-filled, its own range only; a block
 * with status 9 is not written; nothing of `out` outside the files' ranges is written.  A payload above
 * 65,535 bytes is -EINVAL.
 *
 * Semantics: exactly the single-file call applied to each file.  Files whose trees and data blocks are
 * disjoint -- any consistent filesystem -- get bit for bit what one ppfs_ecc_read_file_* /
 * ppfs_ecc_file_blocks_* per file gives: bytes, statuses, the image after write-back, and (summed) the
 * counts.  The same inode listed twice, or trees that share blocks (hard links, a corrupt image), stay
 * memory-safe; a block named more than once in a merged level falls under the repeated-index rules of
 * ppfs_ecc_decode_list_* (identical results for every copy of a clean block; with write-back, which copy's
 * correction lands last is unspecified).
 * One bad range fails the whole call with -EINVAL before anything touches the GPU, as do a null ctx, files
 * (nfiles > 0), image or required buffer and a misaligned index array, flags array or counts record.
 * nfiles == 0, or ranges that are all empty, returns 0 after clearing the counts and the flags.
 * Device forms: never synchronise `stream`, read nothing back, PPFS_ECC_ENOTSUP on a capturing stream.  The
 * host-built tables (128 bytes per file and up to four 16-byte rows) are staged in page-locked memory,
 * copied on `stream` into the call's share of the scrub scratch, and the staging buffer goes back to the
 * cache only after an event behind that copy has completed (checked at later batch calls and at destroy).
 * Per level A, B, C over the whole batch: one expansion kernel, one ppfs_ecc_decode_list_device, one merge
 * kernel; per piece of 32 Ki merged file blocks, cut regardless of file boundaries: expansion, extents,
 * ppfs_ecc_read_extents_device, merge.  The launch count does not depend on nfiles.
 * Host forms: the same merged plan on the CPU around three ppfs_ecc_decode_list_host calls and one
 * ppfs_ecc_read_extents_host.
 */
typedef struct ppfs_ecc_file_range {
    uint64_t offset, nbytes;
} ppfs_ecc_file_range;
typedef struct ppfs_ecc_files_slot { /* 88 bytes */
    uint64_t first_block, blocks, bytes;
    uint64_t block_pos, out_pos;
    uint64_t tree_pos[3], tree_n[3];
} ppfs_ecc_files_slot;
typedef struct ppfs_ecc_files_totals { /* 48 bytes */
    uint64_t blocks, bytes, tree_level[3], tree_blocks;
} ppfs_ecc_files_totals;

int ppfs_ecc_files_plan(const ppfs_ecc_ctx* ctx, const ppfs_ecc_file* files, const ppfs_ecc_file_range* ranges,
    size_t nfiles, ppfs_ecc_files_slot* slots, ppfs_ecc_files_totals* totals);
int ppfs_ecc_files_blocks_device(ppfs_ecc_ctx* ctx, uint8_t* d_image, size_t image_blocks, const ppfs_ecc_file* files,
    const ppfs_ecc_file_range* ranges, size_t nfiles, uint32_t* d_index, uint8_t* d_path_status, uint32_t* d_tree_index,
    uint8_t* d_tree_status, uint32_t* d_file_flags, ppfs_ecc_file_counts* d_counts, int write_back, void* stream);
int ppfs_ecc_files_blocks_host(ppfs_ecc_ctx* ctx, uint8_t* image, size_t image_blocks, const ppfs_ecc_file* files,
    const ppfs_ecc_file_range* ranges, size_t nfiles, uint32_t* index, uint8_t* path_status, uint32_t* tree_index,
    uint8_t* tree_status, uint32_t* file_flags, ppfs_ecc_file_counts* counts, int write_back);
int ppfs_ecc_read_files_device(ppfs_ecc_ctx* ctx, uint8_t* d_image, size_t image_blocks, const ppfs_ecc_file* files,
    const ppfs_ecc_file_range* ranges, size_t nfiles, uint8_t* d_out, size_t out_bytes, uint8_t* d_status,
    uint32_t* d_file_flags, ppfs_ecc_file_counts* d_counts, int write_back, void* stream);
int ppfs_ecc_read_files_host(ppfs_ecc_ctx* ctx, uint8_t* image, size_t image_blocks, const ppfs_ecc_file* files,
    const ppfs_ecc_file_range* ranges, size_t nfiles, uint8_t* out, size_t out_bytes, uint8_t* status,
    uint32_t* file_flags, ppfs_ecc_file_counts* counts, int write_back);

/*
 * Write a file range from its inode: the other half of FileIO's call into the block device (DESIGN.md
 * section 4.12).  FileIO::writeFile (lib/file_io/src/file_io.cpp:46-104) walks the same BlockIndexIterator as
 * readFile, one readBlock per index block, and then issues one writeBlock(bytes, {block, offset}) per data
 * block: offset % dataSize() in the first block, a short last block.  ppfs_ecc_write_file_* is that over ONE
 * existing range, ppfs_ecc_write_files_* over a batch of (file, range).  They write INSIDE the file as the
 * inode describes it: nothing allocates, nothing grows, no inode is updated (PPFS's resizeFile comes first).
 *
 * Range.  offset + nbytes <= file_size, else -EINVAL before anything touches the GPU (the batch call puts the
 * file's number in ppfs_ecc_last_error).  Nothing is clamped, unlike the read: a write that runs past the end
 * would have to grow the file.  Blocks past the tree's capacity and a payload above 65,535 bytes are rejected
 * as by the read calls.  nbytes == 0 is a no-op: 0, zeroed counts, written = 0.  DEVIATION: the reference
 * checks and re-encodes one block for an empty write.  An empty write (the single call with nbytes == 0, a
 * batch whose ranges are all empty) needs neither image nor `in` -- both may be NULL -- in either form; the
 * context, the file records and the alignment of written, flags and counts are still checked, and the device
 * forms still clear counts and flags and set written on `stream`.  ranges == NULL: every file whole.
 * Input.  The single-file call takes in[0, nbytes).  The batch call takes file f's bytes at in[out_pos,
 * out_pos + bytes) of ppfs_ecc_files_plan, files back to back; its slots hold unchanged for every batch the
 * write accepts (only the range rule is stricter).  in_bytes below the total is -EINVAL.
 * Walk.  Exactly the read calls': each needed index block is decoded once; write_back applies to the index
 * blocks only; an index block with status 5 / 9 hands that down and the pointer becomes 0xFFFFFFFF.
 * Write.  Per file block one writeBlock(bytes, {block, offset}) of the reference through
 * ppfs_ecc_write_extents_*, entry i being the read's extent with pos pointing into `in`.
 *   status       (may be NULL) one byte per file block touched: the path status where that is non-zero, else
 *                the write's 0 / 1 / 5 / 9.  A block whose final status is 5 or 9 is NOT TOUCHED: its own old
 *                contents failed, an index block above it failed, or its pointer lies past the image
 *   written      (may be NULL, 8-byte aligned) one uint64 per file (a scalar for the single call): the bytes
 *                of the range that precede the first block whose final status is 5 or 9, or the range's byte
 *                count when there is none -- what FileIO::writeFile had written when it failed
 *   file_flags, counts   as in the read calls, over the final statuses; counts is one record per call and
 *                index_* count the tree blocks
 * Nothing outside the named blocks changes; within a block only the codec's re-encoding of the new payload
 * changes, and the bits the codec leaves undefined keep their contents as in ppfs_ecc_write_extents_*.
 * Batch semantics.  Every block of every range is attempted.  DEVIATION: the reference stops at the first
 * failure, so blocks after a failed one have been written here; `written` and the adapters restore the
 * reference's return value.
 * Repeats.  Device writes need distinct blocks (ppfs_ecc_write_extents_device).  ppfs_ecc_write_files_device
 * therefore refuses, with -EINVAL naming the later file and before anything touches the GPU, two ranges of
 * byte-identical inode records whose file-block spans intersect (found on the host from the plan alone, in
 * O(n log n)); spans that only touch are fine.  ppfs_ecc_write_files_host does not refuse:
 * ppfs_ecc_write_extents_host cuts where a block repeats, so ranges apply in batch order and both land.
 * Different inodes that share blocks (a corrupt image) stay memory-safe; which write lands is unspecified,
 * as for ppfs_ecc_write_list_device.
 * Errors: -EINVAL, before anything touches the GPU, for a null ctx, file(s), image or `in`, a misaligned
 * written, flags or counts.  Device forms: PPFS_ECC_ENOTSUP on a capturing stream; `stream` is never
 * synchronised and nothing is read back; the scratch is the scrub scratch with the read's per-piece layout,
 * 32 Ki file blocks a piece, cut regardless of file boundaries; the batch tables go through the same
 * page-locked staging.  `written` is set on the GPU: one lane per file stores the range's bytes, then the
 * merge kernel lowers it with a 64-bit atomic minimum for failing blocks.  Per piece: expansion, extents,
 * ppfs_ecc_write_extents_device, merge.
 * Host forms: the same plan on the CPU around ppfs_ecc_decode_list_host per level and one
 * ppfs_ecc_write_extents_host.
 */
int ppfs_ecc_write_file_device(ppfs_ecc_ctx* ctx, const uint8_t* d_in, size_t in_bytes, uint8_t* d_image, size_t image_blocks,
    const ppfs_ecc_file* file, uint64_t offset, uint64_t nbytes, uint8_t* d_status, uint64_t* d_written,
    ppfs_ecc_file_counts* d_counts, int write_back, void* stream);
int ppfs_ecc_write_file_host(ppfs_ecc_ctx* ctx, const uint8_t* in, size_t in_bytes, uint8_t* image, size_t image_blocks,
    const ppfs_ecc_file* file, uint64_t offset, uint64_t nbytes, uint8_t* status, uint64_t* written,
    ppfs_ecc_file_counts* counts, int write_back);
int ppfs_ecc_write_files_device(ppfs_ecc_ctx* ctx, const uint8_t* d_in, size_t in_bytes, uint8_t* d_image, size_t image_blocks,
    const ppfs_ecc_file* files, const ppfs_ecc_file_range* ranges, size_t nfiles, uint8_t* d_status, uint32_t* d_file_flags,
    uint64_t* d_written, ppfs_ecc_file_counts* d_counts, int write_back, void* stream);
int ppfs_ecc_write_files_host(ppfs_ecc_ctx* ctx, const uint8_t* in, size_t in_bytes, uint8_t* image, size_t image_blocks,
    const ppfs_ecc_file* files, const ppfs_ecc_file_range* ranges, size_t nfiles, uint8_t* status, uint32_t* file_flags,
    uint64_t* written, ppfs_ecc_file_counts* counts, int write_back);

/*
 * Read inodes from the inode table: a batch of inode numbers per call.  Every file
 * call above starts from a ppfs_ecc_file record; InodeManager::get (lib/inode_manager/src/inode_manager.cpp:
 * 127-138) fetches it with one Bitmap::getBit -- a one-byte readBlock of the inode bitmap (bitmap.cpp:8-25,
 * 87-101) -- and _readInode (:56-89), one or more readBlocks of the inode table.  ppfs_ecc_read_inodes_* is that
 * for n inode numbers of one inode table: records, metadata and statuses.  Engine extension; read-only.
 *
 * On disk.  The packed Inode (inode.hpp:18-41) is 81 bytes: time_creation [0, 8), time_modified [8, 16),
 * direct[12] [16, 64), indirect 64, doubly_indirect 68, trebly_indirect 72, file_size 76, type 80 (0 file,
 * 1 directory); ppfs_ecc_file is bytes [16, 80) of it.  Inode i lies at table byte 81 i (_getInodeLocation,
 * :11-18): block table_block + 81 i / ds at offset 81 i % ds, in 64-bit arithmetic, and is read as a plain cut
 * at block boundaries (readBlock clamps to ds - offset, rs_block_device.cpp:28-48): pieces(i) = (81 i % ds + 80)
 * / ds + 1 pieces, at most K(ds) = 2 + 79 / ds (2 for ds >= 80, 4 at ds = 31, 81 at ds = 1).  Bit i of the inode
 * bitmap is byte i / 8 of the bitmap's payload stream under mask 0x80 >> (i % 8): block bitmap_block + (i / 8) /
 * ds, offset (i / 8) % ds.  In this bitmap 1 means FREE (InodeManager::create / remove / format): get returns
 * InodeManager_NotFound for a set bit, and getBit returns Bitmap_IndexOutOfRange for i >= total_inodes.
 *
 * ppfs_ecc_inode_span: block, offset and piece count of inode `ino`; -EINVAL for a null ctx or table, for
 * ino >= total_inodes and for a first block at or past 2^32 - 1.  Outputs may be NULL.  No GPU.
 *
 * Inode numbers.  Number j is the little-endian uint32 at byte j * ino_stride of `ino`, at any alignment;
 * ino_stride >= 4 (-EINVAL below): 4 for a packed array, 128 for DirectoryEntry records (directory.hpp:8-12) as a
 * ppfs_ecc_read_file(s)_* call left them in its out buffer.
 * Outputs, each may be NULL.  files (4-byte aligned): n ppfs_ecc_file records, which ppfs_ecc_read_files_* takes
 * as its `files` argument once they are in host memory; meta (8-byte aligned): n ppfs_ecc_inode_meta; status: n
 * bytes; piece_status: n * (1 + K(ds)) bytes, per inode slot 0 the bitmap byte's read status and slots 1 ..
 * pieces(i) the table pieces' read statuses, 255 in every slot that is unused or was never read; counts (8-byte
 * aligned): the n statuses tallied.  The status arrays may have any alignment.
 * Status of inode j, in the loop's order of evaluation:
 *   1. ino >= total_inodes: 9, whether or not check_bitmap is set;
 *   2. with check_bitmap: a bitmap read status of 5 or 9 as it stands; a set bit: PPFS_ECC_NOT_ALLOCATED (255);
 *   3. the first piece in order whose status is 5 or 9: that status (a table block at or past image_blocks is 9);
 *   4. otherwise 1 if the bitmap byte or any piece reported 1, else 0.
 * For a status other than 0 or 1 the files and meta records are zero-filled.
 * Blocks touched: exactly those the per-inode loop would touch.  A bitmap block only if an in-range number of the
 * batch has its bit there; a table block only if an inode that passed steps 1-2 has bytes there (all pieces of
 * such an inode are read, also after a failing one); the pieces of every other inode are invalid extents (block
 * 0xFFFFFFFF) and touch nothing.  write_back applies to both regions, as in ppfs_ecc_read_extents_*.
 * Repeats are the norm: three inodes share a table block at ds = 249, eight or more a bitmap byte, and a number
 * may appear twice.  The repeated-index rules of ppfs_ecc_decode_list_* hold: every copy gets the same bytes.  On
 * the device with write_back, the inodes that share a corrected block each report 1 or 0, at least one reports 1,
 * and the image ends corrected; without write_back every sharer reports 1.  (A sharer whose status another rule
 * decides -- a free inode that shares the bitmap block -- reports that status; piece_status shows what its read saw.)  The host form equals the loop: the
 * first toucher reports 1, later ones read the written-back block.
 * Errors: -EINVAL, before anything touches the GPU, for a null ctx, table, image or ino (n > 0), a misaligned
 * files, meta or counts, a stride below 4, a payload of 0 or above 65,535 bytes.  n == 0 returns 0 with zeroed
 * counts.  A capturing stream gets PPFS_ECC_ENOTSUP.  Shortened RS is decoded as by a list decode with no spill.
 * Device form: never synchronises `stream`, reads nothing back, allocates and frees nothing on the caller's
 * stream; its scratch is the context's scrub scratch.  In pieces of PPFS_ECC_INODE_PIECE inodes (2 / K(ds) of
 * that where K > 2): bitmap extents kernel, ppfs_ecc_read_extents_device, table extents kernel,
 * ppfs_ecc_read_extents_device, merge kernel.  `table` is a HOST pointer in both forms.
 * Host form: the same plan on the CPU around two ppfs_ecc_read_extents_host calls and a CPU tally.
 */
#define PPFS_ECC_INODE_PIECE 16384

typedef struct ppfs_ecc_inode_table { /* 16 bytes: the SuperBlock fields InodeManager reads */
    uint32_t table_block, bitmap_block, total_inodes, check_bitmap;
} ppfs_ecc_inode_table;
typedef struct ppfs_ecc_inode_meta { /* 24 bytes */
    uint64_t time_creation, time_modified;
    uint8_t type, pad[7];
} ppfs_ecc_inode_meta;
typedef struct ppfs_ecc_inode_counts { /* 64 bytes, overwritten by each call */
    uint64_t ok, corrected, failed, out_of_range, not_allocated, reserved[3];
} ppfs_ecc_inode_counts;

int ppfs_ecc_inode_span(const ppfs_ecc_ctx* ctx, const ppfs_ecc_inode_table* table, uint32_t ino, uint32_t* block,
    uint32_t* offset, uint32_t* pieces);
int ppfs_ecc_read_inodes_device(ppfs_ecc_ctx* ctx, uint8_t* d_image, size_t image_blocks, const ppfs_ecc_inode_table* table,
    const void* d_ino, size_t ino_stride, size_t n, ppfs_ecc_file* d_files, ppfs_ecc_inode_meta* d_meta, uint8_t* d_status,
    uint8_t* d_piece_status, ppfs_ecc_inode_counts* d_counts, int write_back, void* stream);
int ppfs_ecc_read_inodes_host(ppfs_ecc_ctx* ctx, uint8_t* image, size_t image_blocks, const ppfs_ecc_inode_table* table,
    const void* ino, size_t ino_stride, size_t n, ppfs_ecc_file* files, ppfs_ecc_inode_meta* meta, uint8_t* status,
    uint8_t* piece_status, ppfs_ecc_inode_counts* counts, int write_back);

/*
 * Write inodes into the inode table: a batch of updates per call, the mirror of
 * ppfs_ecc_read_inodes_*.  InodeManager::update (lib/inode_manager/src/inode_manager.cpp:142-159) is one Bitmap::getBit
 * and _writeInode (:20-54), one writeBlock per piece of the 81 bytes.  ppfs_ecc_write_inodes_* is the per-inode loop
 * update(ino[j], inode[j]) for j = 0 .. n-1 in the calls' batch form.  Engine extension.
 *
 * table, ino, ino_stride, status, piece_status (1 + K(ds) slots per inode) and counts keep the meaning, the alignment
 * rules and the error rules of the reads.  files and meta are inputs, both required: inode j's 81 bytes on disk are
 * meta[j].time_creation, meta[j].time_modified, the 64 bytes of files[j], meta[j].type; meta[j].pad is not looked at.
 * Status of inode j.  Steps 1 and 2 are the reads': a number at or past total_inodes gives 9; with check_bitmap a
 * bitmap read status of 5 or 9 stands and a set bit gives PPFS_ECC_NOT_ALLOCATED, and nothing of that inode is
 * written.  Otherwise steps 3 and 4 run over the WRITE statuses of its pieces (ppfs_ecc_write_extents_*): the first
 * piece with 5 or 9 gives that status, else 1 if the bitmap byte or a piece reported 1, else 0.
 * What lands.  A table block whose old contents fail their check (5) stays untouched; one at or past image_blocks
 * gives 9.  Every other block touched ends holding its old payload, corrected, with the bytes of every batch inode
 * that passed steps 1-2 replaced, and the bits the codec leaves undefined kept.
 * The one deviation from the loop is ppfs_ecc_write_files_*'s: every piece of an inode that passed steps 1-2 is
 * written, where the loop stops an inode at its first failing piece.
 * Repeats are the norm and exact for the table.  Where several entries touch one table block the result is the
 * loop's in batch order: all their bytes land; where one number appears twice the later entry's bytes win; a
 * corrected block reports 1 at its first toucher -- the lowest entry, within it the lowest piece -- and 0 at every
 * later one, in both forms.  The bitmap byte is read as by ppfs_ecc_read_inodes_*: write_back applies to it and the
 * device form follows the repeat rule of ppfs_ecc_read_extents_device.  piece_status slot 0 is the bitmap byte's read
 * status, slots 1 .. pieces the pieces' write statuses under the first toucher rule, 255 in every slot that is
 * unused or was never attempted.
 * Errors: the -EINVAL set of the reads, before anything touches the GPU, and a null files or meta with n > 0.
 * n == 0 returns 0 with zeroed counts.  A capturing stream gets PPFS_ECC_ENOTSUP.  Shortened RS is written as
 * ppfs_ecc_write_extents_* writes it.
 * Device form: never synchronises, reads nothing back, allocates nothing on the caller's stream; its scratch is the
 * context's scrub scratch.  Per piece (as the reads', and never more slots than one piece of the extent calls):
 * bitmap extents kernel, ppfs_ecc_read_extents_device (with check_bitmap), election tables cleared, elect kernel,
 * extents kernel (one valid extent of length 0 per distinct block), the extent write with the overlay kernel between
 * "old payloads" and "write", status kernel.
 * Host form: the same plan on the CPU, the blocks grouped with a map: one ppfs_ecc_read_extents_host of the bitmap
 * bytes, one of the per-block hulls of the batch's bytes (without write-back), one ppfs_ecc_write_extents_host with
 * one entry per distinct block.
 */
int ppfs_ecc_write_inodes_device(ppfs_ecc_ctx* ctx, uint8_t* d_image, size_t image_blocks, const ppfs_ecc_inode_table* table,
    const void* d_ino, size_t ino_stride, size_t n, const ppfs_ecc_file* d_files, const ppfs_ecc_inode_meta* d_meta,
    uint8_t* d_status, uint8_t* d_piece_status, ppfs_ecc_inode_counts* d_counts, int write_back, void* stream);
int ppfs_ecc_write_inodes_host(ppfs_ecc_ctx* ctx, uint8_t* image, size_t image_blocks, const ppfs_ecc_inode_table* table,
    const void* ino, size_t ino_stride, size_t n, const ppfs_ecc_file* files, const ppfs_ecc_inode_meta* meta, uint8_t* status,
    uint8_t* piece_status, ppfs_ecc_inode_counts* counts, int write_back);

/*
 * Look up names in directories: a batch of (directory, key) per call.  Every path
 * operation starts with DirectoryManager::getInodeByName (lib/directory_manager/src/directory_manager.cpp:135-163):
 * a loop of readFile over batches of 256 DirectoryEntry records and a strlen / strncmp pass over each
 * (_findEntryByName, :189-199).  The search inside removeEntry (:67-90, _findEntryByInode :201-210) is the same loop
 * with the inode number as the key.  ppfs_ecc_lookup_* is that loop for nq queries over ndirs directories, each
 * directory read ONCE and whole.  Engine extension; read-only apart from the codec's write-back.
 *
 * Entries.  Directory d, a ppfs_ecc_file record, has n_d = file_size / 128 entries; trailing bytes are never read.
 * Entry e is the 128 bytes at 128 e of the payload (directory.hpp:8-12): bytes [0, 4) the little-endian inode
 * number, bytes [4, 128) the 124 name bytes.
 * Queries.  queries[q] = {dir, key}.  mode 0 (name): the key is names[128 q, 128 q + 128), a record at any
 * alignment whose name starts at byte 0 and whose length L is the position of its first NUL; `key` is not read.
 * mode 1 (inode number): the key is `key`; names is not read and may be NULL.
 * Name match.  The entry's name length is the position of the first NUL in its 124 name bytes; the query matches
 * when that length is L and the L bytes are equal.  Bytes behind the entry's NUL are not looked at.  L = 0 matches
 * an entry whose first name byte is NUL.  A query with L >= 124 or with no NUL matches nothing.  DEVIATION: an
 * entry with no NUL in its 124 name bytes matches nothing; the reference's strlen would run on into the next entry.
 * Inode match.  Entry bytes [0, 4) equal the key.
 * First match.  m is the lowest matching entry below n_d: duplicates resolve to the first.
 * Failures, the loop's rule.  The loop reads batch b, entries [256 b, min(256 b + 256, n_d)), with one readFile,
 * which fails as a whole if any file block under those bytes fails -- blocks under entries behind a match in the
 * same batch included.  With B = m / 256 for a match and the last batch otherwise, last(B) is the last file block
 * that batch B's bytes touch.  If a file block j <= last(B) has final read status 5 or 9 (the path status where
 * that is non-zero, as ppfs_ecc_read_files_* reports it), the query's status is that of the lowest such j and it
 * reports no inode.  Otherwise the status is 0 with inode and entry, or PPFS_ECC_NOT_FOUND without a match.  A
 * failing block behind last(B) does not matter.  n_d = 0 is PPFS_ECC_NOT_FOUND, and nothing of that directory is
 * read.  Corrections (status 1) are no per-query result: they are reported per block and per directory.
 *
 * ppfs_ecc_lookup_plan: ppfs_ecc_files_plan over the ranges (0, 128 n_d) -- how large the entries buffer
 * (totals.bytes) and the block status array (totals.blocks) are and where each directory's entries lie (slots[d].
 * out_pos, block_pos).  slots and totals may be NULL.  No GPU work.
 * Buffers.  entries (entries_bytes >= totals.bytes) and block_status (totals.blocks bytes) are the call's working
 * memory and the caller's to keep: after the call they hold every directory's entries and final block statuses
 * exactly as ppfs_ecc_read_files_* over those ranges leaves them, so entries is a ready `ino` source at stride 128
 * for ppfs_ecc_read_inodes_*.  Both are required in the device form; the host form uses buffers of its own where
 * they are NULL.  dir_flags (ndirs words) and file_counts are ppfs_ecc_read_files_*' flags and counts, and may be
 * NULL.  hits: nq records, inode and entry 0xFFFFFFFF unless the status is 0.  counts (may be NULL): the nq statuses
 * tallied; out_of_range counts status 9.
 * Errors: -EINVAL, before anything touches the GPU, for a null ctx, image, dirs, queries or hits, null names in
 * mode 0, a mode other than 0 or 1, a `dir` at or past ndirs (ppfs_ecc_last_error names the query), hits or
 * dir_flags not 4-byte or a counts record not 8-byte aligned, buffers that are short (or, in the device form,
 * null), 2^32 - 1 or more queries, and whatever ppfs_ecc_files_plan rejects.  nq == 0 returns 0 with zeroed counts
 * and reads nothing.  A capturing stream gets PPFS_ECC_ENOTSUP.
 * Device form: never synchronises `stream`, reads nothing back, allocates and frees nothing on the caller's
 * stream.  dirs and queries are HOST pointers.  One ppfs_ecc_read_files_device; then the per-directory table (entry
 * count, out_pos, block_pos, blocks) and the query records go into the context's scrub scratch through the page-
 * locked staging of the file batch's tables, released behind an event; the hit records are set to 0xFF; the match
 * kernel, one wave per (query, 256 entries), lowers each query's `entry` word to its first match with one atomicMin
 * per wave; the finish kernel, one wave per query, applies the failure rule and tallies.
 * Host form: ppfs_ecc_read_files_host, then the same rule on the CPU.
 */
#define PPFS_ECC_NOT_FOUND 2 /* status of a query whose loop ran to its end without a match (engine extension) */

typedef struct ppfs_ecc_lookup_query { /* 8 bytes */
    uint32_t dir, key;
} ppfs_ecc_lookup_query;
typedef struct ppfs_ecc_lookup_hit { /* 16 bytes */
    uint32_t inode, entry, status, reserved;
} ppfs_ecc_lookup_hit;
typedef struct ppfs_ecc_lookup_counts { /* 64 bytes, overwritten by each call */
    uint64_t found, not_found, failed, out_of_range, reserved[4];
} ppfs_ecc_lookup_counts;

int ppfs_ecc_lookup_plan(const ppfs_ecc_ctx* ctx, const ppfs_ecc_file* dirs, size_t ndirs, ppfs_ecc_files_slot* slots,
    ppfs_ecc_files_totals* totals);
int ppfs_ecc_lookup_device(ppfs_ecc_ctx* ctx, uint8_t* d_image, size_t image_blocks, const ppfs_ecc_file* dirs, size_t ndirs,
    const ppfs_ecc_lookup_query* queries, const uint8_t* d_names, size_t nq, int mode, uint8_t* d_entries, size_t entries_bytes,
    uint8_t* d_block_status, uint32_t* d_dir_flags, ppfs_ecc_lookup_hit* d_hits, ppfs_ecc_lookup_counts* d_counts,
    ppfs_ecc_file_counts* d_file_counts, int write_back, void* stream);
int ppfs_ecc_lookup_host(ppfs_ecc_ctx* ctx, uint8_t* image, size_t image_blocks, const ppfs_ecc_file* dirs, size_t ndirs,
    const ppfs_ecc_lookup_query* queries, const uint8_t* names, size_t nq, int mode, uint8_t* entries, size_t entries_bytes,
    uint8_t* block_status, uint32_t* dir_flags, ppfs_ecc_lookup_hit* hits, ppfs_ecc_lookup_counts* counts,
    ppfs_ecc_file_counts* file_counts, int write_back);

/*
 * 2-of-3 bitwise majority of nrec replicated records of rec_bytes each, replacing
 * SuperBlockManager::_performBitVoting (lib/super_block_manager/src/super_block_manager.cpp:133-165):
 *   out[i] = majority(a[i], b[i], c[i]) bit by bit;
 *   damaged (may be NULL) per record: bit k set when copy k+1 differs from the majority
 *   (the reference's damaged1/2/3).
 * The host form runs on HIP device `device` and returns when the outputs are in host memory.
 */
int ppfs_vote3_device(const uint8_t* d_a, const uint8_t* d_b, const uint8_t* d_c, uint8_t* d_out, size_t rec_bytes,
    size_t nrec, uint32_t* d_damaged, void* stream);
int ppfs_vote3_host(int device, const uint8_t* a, const uint8_t* b, const uint8_t* c, uint8_t* out, size_t rec_bytes,
    size_t nrec, uint32_t* damaged);

/*
 * Device-to-device copy of `bytes` (any alignment) on `stream`: the measurement reference for
 * the HBM roofline ("also measure a device-to-device copy kernel on the box and report
 * both fractions").  Not a reference interface: full-grid 16-byte copy, see DESIGN.md section 5.
 */
int ppfs_copy_device(void* d_dst, const void* d_src, size_t bytes, void* stream);

/*
 * Fault injection, one byte per block: block b of the raw image (stride bytes per block) gets
 * byte pos[b] set to val[b] (mode 0) or XORed with val[b] (mode 1); pos[b] >= stride leaves the
 * block alone.  Positions are one byte each, so only the first 256 bytes of a block are
 * reachable.  The device-side counterpart of the reference's bit flipper
 * (usage_simulator/simulation/src/bit_flipper.cpp), which is out of scope as a simulator: this
 * entry exists for bench.py's corrupt-then-decode step and the tests.  Not a reference interface.
 */
int ppfs_inject_device(uint8_t* d_raw, size_t stride, size_t nblocks, const uint8_t* d_pos, const uint8_t* d_val,
    int mode, void* stream);

/*
 * Page-lock / release a caller buffer (hipHostRegister), e.g. the host mirror of a disk image
 * (replacing FileDisk's seekp + fstream I/O, lib/disk/src/file_disk.cpp:56-101,
 * by an mmap'd or resident image the *_host calls then DMA directly).
 */
int ppfs_ecc_host_register(void* ptr, size_t bytes);
int ppfs_ecc_host_unregister(void* ptr);
/* Ranges registered through ppfs_ecc_host_register and not yet unregistered: their number (and
 * their total bytes in *bytes when bytes is non-null).  Diagnostics: tests assert that no range
 * outlives the test that registered it.  Engine extension, no reference counterpart. */
long long ppfs_ecc_host_registered(size_t* bytes);

/*
 * Multi-GPU host path: a group of contexts, one per listed HIP device (a device may
 * repeat), over which the *_host calls shard a batch into contiguous block ranges -- shard g =
 * blocks [g*N/G, (g+1)*N/G), one contiguous range of the packed image -- each run by its own host
 * thread on its context's streams and pinned staging.  Blocks are independent codewords: no data
 * moves between devices and no collective runs; the call returns when every shard's results are in
 * host memory, with the first failing shard's error.  Status / spill are split like the blocks.
 * (Reference: the caller side of IBlockDevice, file_io.cpp:12-104, issues the same per-block work
 * serially on one CPU thread.)
 */
typedef struct ppfs_ecc_group ppfs_ecc_group;
int ppfs_ecc_group_create(const ppfs_ecc_params* params, const int* devices, int ndevices, ppfs_ecc_group** out);
void ppfs_ecc_group_destroy(ppfs_ecc_group* group);
int ppfs_ecc_group_size(const ppfs_ecc_group* group);
ppfs_ecc_ctx* ppfs_ecc_group_ctx(ppfs_ecc_group* group, int index);
int ppfs_ecc_group_encode_host(ppfs_ecc_group* group, const uint8_t* data, uint8_t* raw, size_t nblocks);
int ppfs_ecc_group_decode_host(ppfs_ecc_group* group, uint8_t* raw, uint8_t* data, uint8_t* status, size_t nblocks,
    int write_back, uint8_t* spill);
int ppfs_ecc_group_write_host(ppfs_ecc_group* group, const uint8_t* data, uint8_t* raw, uint8_t* status,
    size_t nblocks);

/* Kernel timing hook (bench.py's roofline, tools): the next RS kernel the calling thread launches
 * through any context records start_event / stop_event (hipEvent_t, created by the caller with
 * timing enabled) from its own dispatch packet (hipExtLaunchKernel) -- the kernel's execution time
 * as rocprofv3 measures it, without the launch gap that events recorded on the stream around the
 * call include.  The hook disarms after one launch; (NULL, NULL) disarms it.  -EINVAL if only one
 * event is given.  Engine extension, no reference counterpart. */
int ppfs_ecc_time_next_launch(void* start_event, void* stop_event);

/* Last HIP error string recorded by this thread (diagnostics). */
const char* ppfs_ecc_last_error(void);

/* Diagnostics of PPFS_ECC_DEBUG builds (csrc/dbg.hpp): the number of out-of-bounds global
 * accesses the kernels detected (and skipped) so far; -1 in normal builds.  Engine extension,
 * no reference counterpart. */
long long ppfs_ecc_debug_faults(void);
/* PPFS_ECC_DEBUG builds: launches one deliberately out-of-range row gather and returns how many
 * accesses the kernel reported (and skipped), >= 1 when the checks work; -1 in normal builds. */
long long ppfs_ecc_debug_selftest(void);
/* PPFS_ECC_DEBUG builds: copies the engine refused because an end was not page-locked host memory /
 * device memory over its whole range (every hipMemcpy the library issues is checked first);
 * -1 in normal builds. */
long long ppfs_ecc_debug_dma_rejects(void);
/* PPFS_ECC_DEBUG builds: positive control of those checks (a pageable source and a device range past
 * its allocation must both be refused): 1 when they are, 0 when not, -1 in normal builds. */
long long ppfs_ecc_debug_dma_selftest(void);

#ifdef __cplusplus
}
#endif

#endif /* PPFS_ECC_H */
