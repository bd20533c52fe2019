// kernels.hpp -- the host-callable launchers of the kernel translation units, declared once:
// rs_kernels.hip (Reed-Solomon and its servers), bit_kernels.hip (CRC, Hamming, parity and the bit
// server) vote.hip (vote, copy, gather, patch list, inject, flag, block lists), alloc_scan.hip (bitmap
// expansion, scrub tally), files_walk.hip (the file walk's expansion, extents and merges),
// inode_walk.hip (the inode reads' extents, the inode writes' election and overlay, their one status kernel) and
// dir_walk.hip (the directory lookups' match and finish).
// The three table-sizing functions are in host_tables.hpp, beside the builders that use them.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ppfs_ecc.h" // ppfs_ecc_extent, ppfs_ecc_file
#include "server_box.hpp"

// Who owns the entries of a launch of the file walk.  A batch: recs, its nfiles filesplan::FileRec, and rows, the nrows
// filesplan::Row of the level the launch works on (sentinel not counted), both in device memory, 8-byte aligned; one
// null.  ONE file: one, a HOST pointer to its filesplan::OneRec (the record and the Tree of its range), which travels
// to the kernel by value; the other fields are not read.
struct ppfs_files_owner {
    const void* recs;
    uint64_t nfiles;
    const void* rows;
    uint64_t nrows;
    const void* one;
};

extern "C" {
int ppfs_rs_fast_supported(int n, int t2);
// res_tiles: the batch's resident prefix in tiles (resident_plan.hpp; the 2t <= 8 ticket encode)
hipError_t ppfs_rs_fast_encode(int t2, const uint8_t* d, uint8_t* r, uint64_t nb, const uint8_t* tab, hipStream_t s,
    uint32_t* ctr, uint32_t* ctr_clear, uint64_t res_tiles);
const char* ppfs_rs_fast_path(int t2);
hipError_t ppfs_flag_launch(uint32_t* flag, uint32_t v, hipStream_t s);
hipError_t ppfs_rs_generic_server_launch(int n, int t2, ppfs::SrvBox* box, uint8_t* zc, uint64_t zc_bytes,
    const uint8_t* tab, uint32_t gen, uint32_t idle_us, hipStream_t s);
hipError_t ppfs_bit_server_launch(int ecc_type, uint32_t bs, uint32_t ds, uint32_t crc_n, uint64_t crc_mask, uint32_t ham_L,
    ppfs::SrvBox* box, uint8_t* zc, uint64_t zc_bytes, const uint8_t* tab, uint32_t gen, uint32_t idle_us, hipStream_t s);
hipError_t ppfs_rs_server_launch(int t2, ppfs::SrvBox* box, uint8_t* zc, uint64_t zc_bytes, const uint8_t* tab,
    uint32_t gen, uint32_t idle_us, hipStream_t s);
hipError_t ppfs_rs_fast_decode(int t2, uint8_t* r, uint8_t* d, uint8_t* st, uint64_t nb, const uint8_t* tab, int wb,
    hipStream_t s, uint32_t* ctr, uint32_t* ctr_clear, uint8_t* wb_dst);
// RS(255, 255-2t), 2t <= 8: the list decode in one kernel (rs_wg_list.hpp); entry i = image row index[i],
// d (16-byte aligned or null) and st (or null) in list order
hipError_t ppfs_rs_list_decode(int t2, uint8_t* image, uint64_t image_blocks, const uint32_t* index, uint8_t* d, uint8_t* st,
    uint64_t nb, const uint8_t* tab, int wb, hipStream_t s);
// the list encode in one kernel: payload i of d (16-byte aligned, list order) -> image row index[i]; an
// entry >= image_blocks stores nothing
hipError_t ppfs_rs_list_encode(int t2, const uint8_t* d, uint8_t* image, uint64_t image_blocks, const uint32_t* index,
    uint64_t nb, const uint8_t* tab, hipStream_t s);
hipError_t ppfs_rs_generic_encode(const uint8_t* d, uint8_t* r, uint64_t nb, int n, int t2, const uint8_t* tab,
    hipStream_t s);
hipError_t ppfs_rs_generic_decode(uint8_t* r, uint8_t* d, uint8_t* st, uint8_t* spill, uint64_t nb, int n, int t2,
    int wb, const uint8_t* tab, hipStream_t s);
int ppfs_crc_fast_supported(uint32_t bs, uint32_t n);
int ppfs_bitfast_supported(uint32_t bs);
hipError_t ppfs_crc_encode(const uint8_t* d, uint8_t* r, const uint8_t* skip, uint64_t nb, uint32_t bs, uint32_t ds,
    uint32_t n, uint64_t mask, const uint8_t* tab, hipStream_t s);
hipError_t ppfs_crc_check(const uint8_t* r, uint8_t* d, uint8_t* st, uint64_t nb, uint32_t bs, uint32_t ds, uint32_t n,
    uint64_t mask, const uint8_t* tab, hipStream_t s);
hipError_t ppfs_ham_encode(const uint8_t* d, uint8_t* r, const uint8_t* skip, uint64_t nb, uint32_t bs, uint32_t ds,
    uint32_t L, hipStream_t s);
hipError_t ppfs_ham_decode(uint8_t* r, uint8_t* d, uint8_t* st, uint64_t nb, int wb, uint32_t bs, uint32_t ds,
    uint32_t L, hipStream_t s);
hipError_t ppfs_parity_encode(const uint8_t* d, uint8_t* r, const uint8_t* skip, uint64_t nb, uint32_t bs,
    hipStream_t s);
hipError_t ppfs_parity_check(const uint8_t* r, uint8_t* d, uint8_t* st, uint64_t nb, uint32_t bs, hipStream_t s);
hipError_t ppfs_gather_rows_launch(const uint8_t* src, uint64_t src_rows, uint8_t* dst, const uint32_t* idx, uint32_t nrows,
    uint32_t row_bytes, hipStream_t s);
hipError_t ppfs_vote3_launch(const uint8_t* a, const uint8_t* b, const uint8_t* c, uint8_t* out, uint64_t rec_bytes,
    uint64_t nrec, uint32_t* damaged, hipStream_t s);
hipError_t ppfs_copy_launch(uint8_t* dst, const uint8_t* src, uint64_t bytes, hipStream_t s);
hipError_t ppfs_patch_list_launch(const uint8_t* cur, const uint8_t* orig, const uint8_t* status, uint32_t n, uint64_t nb,
    uint32_t S, uint32_t* patch, uint8_t* image, hipStream_t s);
hipError_t ppfs_inject_launch(uint8_t* raw, uint64_t stride, uint64_t nblocks, const uint8_t* pos, const uint8_t* val,
    int mode, hipStream_t s);
// block lists, the staged side of a piece of listed rows (list_path.cpp PieceIO: fetch = gather, the
// scatter after decode / encode / write, marks = list_oob; the direct side is the two ppfs_rs_list_*
// calls above): stage is 16-byte aligned with a capacity of nb * raw rounded up to 16;
// scatter mode 0 = every in-range entry (encode), 1 = status 1 (decode), 2 = status other than 5 (write)
hipError_t ppfs_gather_blocks_launch(const uint8_t* img, uint64_t image_blocks, const uint32_t* index, uint32_t nb,
    uint32_t raw, uint8_t* stage, hipStream_t s);
hipError_t ppfs_scatter_blocks_launch(const uint8_t* stage, uint8_t* img, uint64_t image_blocks, const uint32_t* index,
    const uint8_t* status, int mode, uint32_t nb, uint32_t raw, hipStream_t s);
hipError_t ppfs_list_oob_launch(const uint32_t* index, uint32_t nb, uint64_t image_blocks, uint8_t* status, uint8_t* data,
    uint32_t data_bytes, hipStream_t s);
// byte extents (extent_path.cpp): index[i] = entry i's block, or 0xFFFFFFFF when the entry is invalid
// (image_blocks <= 0xFFFFFFFF); copy to_stage 0 = pack payload bytes into buf (zeros for status 5),
// 1 = overlay buf's bytes onto the payloads.  stage: 16-byte aligned, stage_cap a multiple of 16.
hipError_t ppfs_extent_index_launch(const ppfs_ecc_extent* ext, uint32_t nb, uint64_t image_blocks, uint32_t ds,
    uint64_t buf_bytes, uint32_t* index, hipStream_t s);
hipError_t ppfs_extent_copy_launch(int to_stage, const ppfs_ecc_extent* ext, const uint32_t* index, const uint8_t* status,
    uint32_t nb, uint32_t ds, uint8_t* stage, uint64_t stage_cap, uint8_t* buf, uint64_t buf_bytes, hipStream_t s);
// allocated-block and list scrub (scrub_path.cpp; alloc_scan.hip, arithmetic in alloc_plan.hpp).
// expand: piece `piece` of the decoded bitmap (stream: 4-byte aligned, B * ds bytes; bstatus: its blocks'
// statuses) -> the ascending list of first_block + j for its set bits in index, their number in
// *piece_total (8-byte aligned); scratch: 2 * alloc::PIECE_CHUNKS dwords; counts (may be null): the
// 64-byte record whose not_allocated grows by the piece's clear bits.
// iota: index[i] = first + i.  tally: list-order statuses st[k] of entries index[k] -> status_out[index[k] -
// first] (below out_n; null: no scatter, index unused) and counts[slot0 + slot] for the slots below ncat.
hipError_t ppfs_alloc_expand_launch(const uint8_t* stream, const uint8_t* bstatus, uint64_t B, uint64_t ds, uint64_t nbits,
    uint32_t first_block, uint64_t piece, uint32_t* scratch, unsigned long long* piece_total, uint32_t* index,
    unsigned long long* counts, hipStream_t s);
hipError_t ppfs_alloc_iota_launch(uint32_t* index, uint32_t first, uint64_t n, hipStream_t s);
hipError_t ppfs_scrub_tally_launch(const uint8_t* st, const uint32_t* index, uint64_t n, uint32_t first, uint8_t* status_out,
    uint64_t out_n, unsigned long long* counts, int slot0, int ncat, hipStream_t s);
// the file walk (files_path.cpp; files_walk.hip, arithmetic in file_plan.hpp and files_plan.hpp).  owner: who owns the
// launch's entries (ppfs_files_owner above); e0: the merged entry of element 0 of the launch's arrays; payload / st /
// inh: the merged tree scratch of `slots` entries (ds bytes, 1 and 1 byte each).
// expand: merged entries [e0, e0 + n) of a level -> pointer[i] (4-byte aligned) and inherited[i], either may be null.
// extents: the ppfs_ecc_extent entries (8-byte aligned) of the merged file blocks [e0, e0 + n), each at its file's place
// in the call's buffer; NO_BLOCK where path[i] != 0.
// merge: status_out[i] = path[i] ? path[i] : read[i] (read null: 0); pointer_out[i] = pointer_in[i]; out's (out_bytes
// bytes) range of a block with path status 5 zero-filled; flags[file] |= filesplan::flag_of(final status), and the
// counts, in the tree half for a level of the tree and in the data half for LEVEL_DATA.
// written_init: written[f] = file f's bytes (8-byte aligned; null: nothing).
// write_merge: status_out[i] = path[i] ? path[i] : wst[i]; counts' file half; flags[file]; written[file] lowered by a
// 64-bit atomicMin to the position, within the file's bytes, of a block whose final status is 5 or 9.  No payload byte
// is read or written.
hipError_t ppfs_files_expand_launch(const ppfs_files_owner* owner, int level, uint64_t e0, uint64_t n, uint64_t ds,
    const uint8_t* payload, const uint8_t* st, const uint8_t* inh, uint64_t slots, uint32_t* pointer, uint8_t* inherited,
    hipStream_t s);
hipError_t ppfs_files_extents_launch(const ppfs_files_owner* owner, const uint32_t* pointer, const uint8_t* path, uint64_t e0,
    uint64_t n, uint64_t ds, ppfs_ecc_extent* ext, hipStream_t s);
hipError_t ppfs_files_merge_launch(const ppfs_files_owner* owner, int level, const uint8_t* path, const uint8_t* read, uint64_t e0,
    uint64_t n, uint8_t* status_out, const uint32_t* pointer_in, uint32_t* pointer_out, uint8_t* out, uint64_t out_bytes,
    uint64_t ds, uint32_t* flags, unsigned long long* counts, hipStream_t s);
hipError_t ppfs_files_written_init_launch(const ppfs_files_owner* owner, unsigned long long* written, hipStream_t s);
hipError_t ppfs_files_write_merge_launch(const ppfs_files_owner* owner, const uint8_t* path, const uint8_t* wst, uint64_t e0,
    uint64_t n, uint8_t* status_out, uint64_t ds, uint32_t* flags, unsigned long long* written, unsigned long long* counts,
    hipStream_t s);
// the inode reads (inode_path.cpp; inode_walk.hip, arithmetic in inode_plan.hpp) over one piece of n inodes, at most
// inodeplan::piece_inodes(ds); K = inodeplan::max_pieces(ds); table: a HOST pointer, travels by value.
// bitmap_extents: number j = the little-endian uint32 at src + j * stride (any alignment, stride >= 4) -> ino[j]
// (4-byte aligned) and ext[j] (8-byte aligned), the one-byte extent of its bitmap byte with pos = j, invalid when the
// number is out of range or the bitmap is not checked.
// table_extents: bm[j] / bst[j], the bitmap bytes and their read statuses -> ext[j * K + k], the pieces of the inodes
// whose table is read with pos = 81 j + the bytes before piece k, every other one invalid.
// merge: rows (81 n bytes) and pst[j * K + k], the pieces' read statuses -> files, meta, status, piece_status
// (n * (1 + K) bytes) and the counts (five categories), each may be null.  The status kernel on the read's pieces.
hipError_t ppfs_inode_bitmap_extents_launch(const void* src, uint64_t stride, uint64_t n, const ppfs_ecc_inode_table* table,
    uint64_t ds, uint32_t* ino, ppfs_ecc_extent* ext, hipStream_t s);
hipError_t ppfs_inode_table_extents_launch(const uint32_t* ino, const uint8_t* bm, const uint8_t* bst, uint64_t n,
    const ppfs_ecc_inode_table* table, uint64_t ds, ppfs_ecc_extent* ext, hipStream_t s);
hipError_t ppfs_inode_merge_launch(const uint32_t* ino, const uint8_t* bm, const uint8_t* bst, const uint8_t* rows,
    const uint8_t* pst, uint64_t n, const ppfs_ecc_inode_table* table, uint64_t ds, ppfs_ecc_file* files, ppfs_ecc_inode_meta* meta,
    uint8_t* status, uint8_t* piece_status, unsigned long long* counts, hipStream_t s);
// the inode writes (inode_path.cpp; the grouping step of inode_wplan.hpp) over one piece of n inodes, n * K slots, at
// most 2 * inodeplan::PIECE_INODES of them; ino, bm, bst: the scratch the bitmap steps above left; tab: the two
// election tables, inodewplan::table_bytes(cap) bytes cleared to 0xFF on the stream, cap = inodewplan::capacity(n * K).
// elect: the elect kernel, then the extents kernel: ext[slot] (8-byte aligned), the owner slot of each distinct block
// {pos 0, block, 0, 0}, every other slot invalid.
// overlay: the bytes of the winning entries' rows (files: 64 n bytes, meta: 24 n bytes, 8-byte aligned) into their
// blocks' owner rows of P (stride ds, P_cap bytes); idx: the staged indices of the n * K extents.
// write_status: wst[slot], the extents' write statuses -> status, piece_status (n * (1 + K) bytes) and the counts, each
// may be null.  The same status kernel on the write's pieces.
hipError_t ppfs_inode_elect_launch(const uint32_t* ino, const uint8_t* bm, const uint8_t* bst, uint64_t n,
    const ppfs_ecc_inode_table* table, uint64_t ds, uint32_t* tab, uint32_t cap, ppfs_ecc_extent* ext, hipStream_t s);
hipError_t ppfs_inode_overlay_launch(const uint32_t* ino, const uint8_t* bm, const uint8_t* bst, uint64_t n,
    const ppfs_ecc_inode_table* table, uint64_t ds, uint32_t* tab, uint32_t cap, const ppfs_ecc_file* files,
    const ppfs_ecc_inode_meta* meta, const uint32_t* idx, uint8_t* P, uint64_t P_cap, hipStream_t s);
hipError_t ppfs_inode_write_status_launch(const uint32_t* ino, const uint8_t* bm, const uint8_t* bst, const uint8_t* wst,
    uint64_t n, const ppfs_ecc_inode_table* table, uint64_t ds, uint32_t* tab, uint32_t cap, uint8_t* status, uint8_t* piece_status,
    unsigned long long* counts, hipStream_t s);
// the directory lookups (lookup_path.cpp; dir_walk.hip, the rule in lookup_plan.hpp).  dirs: ndirs lookupplan::DirRec,
// queries: nq lookupplan::Query, both in device memory, 8-byte aligned; names: nq records of 128 bytes at any alignment
// (mode 1: not read, may be null); entries (entries_bytes) and block_status (total_blocks) as ppfs_ecc_read_files_*
// left them; hits: nq ppfs_ecc_lookup_hit, 4-byte aligned.
// match: lowers the `entry` word of every query's hit record, set to 0xFFFFFFFF on the stream before, to its first
// matching entry; max_entries: the longest directory's entries (0: no launch).
// finish: the failure rule over the block statuses -> the hit records and the counts (8-byte aligned, may be null).
hipError_t ppfs_lookup_match_launch(const void* dirs, uint64_t ndirs, const void* queries, const uint8_t* names, uint64_t nq,
    int mode, const uint8_t* entries, uint64_t entries_bytes, uint64_t max_entries, void* hits, hipStream_t s);
hipError_t ppfs_lookup_finish_launch(const void* dirs, uint64_t ndirs, const void* queries, uint64_t nq, const uint8_t* entries,
    uint64_t entries_bytes, const uint8_t* block_status, uint64_t total_blocks, uint64_t ds, void* hits, unsigned long long* counts,
    hipStream_t s);
}
