/*
 * pbs_fixed.h -- C ABI of the fixed-size chunk path (.fidx archives, VM images): the index
 * image, a dirty map of two resident images, per-chunk digests and the upload of an image
 * with such a map, and the restore of an archive range.
 *
 * Reference interfaces replaced:
 *  - `FixedChunkStream` (pbs-client/src/chunk_stream.rs:80-134): chunks of exactly
 *    chunk_size bytes, one shorter last chunk;
 *  - the upload with `prefix == "fixed"` (pbs-client/src/backup_writer.rs:272-275, 654, 685:
 *    the client's csum hashes the digests alone, the `!is_fixed_chunk_size` branch is skipped);
 *  - `FixedIndexReader` (pbs-datastore/src/fixed_index.rs:59-215): new (:67-127), index_count /
 *    index_digest / index_bytes / chunk_info (:149-182), compute_csum (:192-203),
 *    chunk_from_offset (:205-214);
 *  - `FixedIndexWriter` (:243-461): create (:245-317), close (:341-362), check_chunk_alignment
 *    (:364-392), add_chunk / add_digest (:394-448), clone_data_from (:450-460), which the
 *    server uses for `reuse-csum` (src/api2/backup/mod.rs:447-514);
 *  - `dump_image` (proxmox-backup-client/src/main.rs:1109-1153): the restore of an image.
 *
 * Conventions are those of pbs_blob.h / pbs_restore.h: offset arrays on the host, byte buffers
 * on the device, every device call synchronous on `hip_stream`, a `timing` struct that may be
 * NULL, the codes of pbs_chunker.h.  Chunk i of an image of `size` bytes is
 * [i * chunk_size, min((i + 1) * chunk_size, size)); there are n = ceil(size / chunk_size).
 * Every device call of this header wants chunk_size a power of two >= 4096: another power of
 * two is PBS_ERR_INVALID, anything else (0 included) PBS_ERR_NOT_POW2.
 */
#ifndef PBS_FIXED_H
#define PBS_FIXED_H

#include <stddef.h>
#include <stdint.h>

#include "pbs_blob.h"
#include "pbs_chunker.h"
#include "pbs_digest.h"
#include "pbs_restore.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- 1. The index image (host) ---- */

/* Header (fixed_index.rs:20-32), 4096 bytes: magic[8] = FIXED_SIZED_CHUNK_INDEX_1_0
 * (file_formats.rs:20-21), uuid[16], ctime (LE i64), index_csum[32] = SHA-256(d1 || d2 || ...)
 * (close, :341-362), size (LE u64), chunk_size (LE u64), zeros; then n digests of 32 bytes. */

/* ceil(size / chunk_size); 0 when chunk_size == 0. */
size_t pbs_fidx_count(uint64_t size, uint64_t chunk_size);
/* 4096 + 32 n. */
size_t pbs_fidx_size(size_t n);

/* The image of an archive of `size` bytes in chunks of `chunk_size` (> 0) with the
 * pbs_fidx_count(size, chunk_size) digests at `digests`, into `out` (cap >= pbs_fidx_size(n),
 * else PBS_ERR_CAPACITY).  `uuid` NULL: zeros.  `csum_out` (may be NULL) receives index_csum,
 * what FixedIndexWriter::close returns. */
int pbs_fidx_build(const uint8_t *digests, uint64_t size, uint64_t chunk_size, const uint8_t uuid[16],
                   int64_t ctime, uint8_t *out, size_t cap, uint8_t csum_out[32]);

/* Reads such an image; fails where FixedIndexReader::new bails (:79-103).  PBS_ERR_INVALID:
 * an image shorter than the header ("index too small"), a wrong magic, chunk_size == 0 (the
 * reference divides by it), n * 32 != len - 4096 ("got unexpected file size"), size == 0 (the
 * reference's zero-length mmap fails).  PBS_ERR_NOT_POW2: a chunk_size that is no power of
 * two -- a deviation: the reference opens such a file, but its own chunk_from_offset (:205-214)
 * and check_chunk_alignment (:387) mask with chunk_size - 1.  PBS_ERR_CAPACITY when the image
 * holds more than `cap` entries (*n is still set).  Every output pointer may be NULL
 * (`digests`, 32 cap bytes, when cap == 0).  `header_csum` is the header's field and
 * `computed_csum` compute_csum (:192-203) over the digests; they are the caller's to compare,
 * the reference does not compare them at open either. */
int pbs_fidx_parse(const uint8_t *image, size_t len, uint8_t uuid[16], int64_t *ctime,
                   uint8_t header_csum[32], uint8_t computed_csum[32], uint64_t *size,
                   uint64_t *chunk_size, uint8_t *digests, size_t cap, size_t *n);

/* chunk_info (:165-182): [start, end) of chunk `pos`, the last one clipped to `size`.
 * pos >= n or chunk_size == 0: PBS_ERR_INVALID. */
int pbs_fidx_chunk_info(uint64_t size, uint64_t chunk_size, size_t pos, uint64_t *start, uint64_t *end);
/* chunk_from_offset (:205-214): offset >= size is PBS_ERR_INVALID (the reference's None);
 * chunk_size no power of two: PBS_ERR_NOT_POW2 (0: PBS_ERR_INVALID). */
int pbs_fidx_chunk_from_offset(uint64_t size, uint64_t chunk_size, uint64_t offset, size_t *idx,
                               uint64_t *within);
/* check_chunk_alignment (:364-392), clause by clause in the reference's order; each bail is
 * PBS_ERR_INVALID, PBS_OK sets *idx.  Its quirks are kept: a short last chunk is legal only
 * with end_offset == size, and a full-length last chunk of an image whose size is no multiple
 * of chunk_size (end_offset == size, chunk_len == chunk_size) passes the length clause and
 * fails as "unaligned".  chunk_size must be a power of two (as in pbs_fidx_chunk_from_offset). */
int pbs_fidx_check_chunk_alignment(uint64_t size, uint64_t chunk_size, uint64_t end_offset,
                                   uint64_t chunk_len, size_t *idx);

/* ---- 2. Dirty map of two resident images ---- */

/* dirty_dev[i] = 1 iff any byte of chunk i differs between the images at `prev_dev` and
 * `cur_dev` (device, `size` bytes each, any alignment, independently), else 0; n bytes of
 * `dirty_dev` (device) are written and nothing else; no byte outside [p, p + size) of either
 * image is read and neither is written.  *n_dirty (may be NULL): the number of ones, counted
 * on the device.  size == 0: PBS_OK, nothing written. */
int pbs_fixed_dirty_device(const uint8_t *prev_dev, const uint8_t *cur_dev, uint64_t size,
                           uint64_t chunk_size, uint8_t *dirty_dev, size_t *n_dirty, void *hip_stream);
/* The same map by memcmp per chunk (every pointer host memory; any chunk_size > 0): the mirror
 * the GPU is compared against. */
int pbs_fixed_dirty_host(const uint8_t *prev, const uint8_t *cur, uint64_t size, uint64_t chunk_size,
                         uint8_t *dirty, size_t *n_dirty);

/* ---- 3. Digests of a resident image ---- */

typedef struct {
    double total_ms;        /* call entry .. digests on the host */
    double gpu_ms;          /* the SHA-256 kernels (HIP events) */
    uint64_t hashed_chunks; /* chunks whose bytes were read */
    uint64_t hashed_bytes;
} pbs_fixed_digest_timing;

/* digests[32 i ..] (host, 32 n) = SHA-256(chunk i || key) of the image at `dev_data` (device).
 * With `dirty` (host, n bytes): a chunk with dirty[i] == 0 takes prev_digests[32 i ..] (host)
 * verbatim and its bytes are not read; `dirty` without `prev_digests` is PBS_ERR_INVALID.
 * `index_csum` (may be NULL): SHA-256 over the n digests.  The chunks to hash go through the
 * kernels of pbs_digest_chunks_async with the list of their indices as the order (chunk_size
 * < 1 MiB) or through pbs_digest_chunks_hybrid (longer chunks: one GPU lane walks a 4 MiB
 * chain for ~120 ms, host cores share them): where they lie when their indices are one run,
 * else packed back to back into device scratch (up to 1 GiB per hybrid call) by the segment
 * copy kernel. */
int pbs_fixed_digests_device(const uint8_t *dev_data, uint64_t size, uint64_t chunk_size,
                             const uint8_t *key, size_t key_len, const uint8_t *dirty,
                             const uint8_t *prev_digests, uint8_t *digests, uint8_t index_csum[32],
                             pbs_fixed_digest_timing *timing, void *hip_stream);

/* ---- 4. Upload of an image from host memory ---- */

typedef struct {
    pbs_upload_timing up;
    uint64_t dirty_chunks; /* chunks hashed and tested (all of them without a map) */
    uint64_t copied_bytes; /* bytes of the pieces copied to the device */
} pbs_upload_fixed_timing;

/* The fixed twin of pbs_upload_stream_host (pbs_digest.h): the same outputs, the same
 * UploadStats, the same per-piece overlap, with the grid instead of the chunker -- `ends` is
 * min((i + 1) * chunk_size, len), cap >= ceil(len / chunk_size).  `index_csum` (may be NULL):
 * SHA-256 over the n digests (the fixed branch of backup_writer.rs:685).
 * With `dirty` (n bytes; needs `prev_digests`, 32 n, else PBS_ERR_INVALID): a clean chunk gets
 * digests[i] = prev_digests[i], is_known[i] = 1 and an empty blob, counts in chunk_reused /
 * size_reused, and is neither hashed nor encoded; a piece that holds no byte of a dirty chunk
 * is not copied to the device.  `known` keeps its meaning: the sorted list plus the earlier
 * HASHED chunks of this stream -- the digests of clean chunks take part in the test only if
 * the caller put them into `known`.  chunk_size no power of two: PBS_ERR_NOT_POW2 (below
 * 4096: PBS_ERR_INVALID); len == 0: PBS_OK with *n_out = 0. */
int pbs_upload_fixed_host(uint64_t chunk_size, const uint8_t *host, size_t len, size_t piece,
                          const uint8_t *key, size_t key_len, int digest_cus, const uint8_t *known,
                          size_t n_known, int compress, const uint8_t *dirty, const uint8_t *prev_digests,
                          uint64_t *ends, uint8_t *digests, uint8_t *is_known, size_t cap, size_t *n_out,
                          uint8_t *blobs, size_t blobs_cap, uint64_t *blob_offsets, uint8_t *compressed,
                          uint8_t index_csum[32], pbs_upload_fixed_timing *timing);
/* ... of an encrypted backup, as pbs_upload_stream_host_crypt. */
int pbs_upload_fixed_host_crypt(uint64_t chunk_size, const uint8_t *host, size_t len, size_t piece,
                                const struct pbs_crypt_config *crypt, int digest_cus, const uint8_t *known,
                                size_t n_known, int compress, const uint8_t *dirty, const uint8_t *prev_digests,
                                uint64_t *ends, uint8_t *digests, uint8_t *is_known, size_t cap, size_t *n_out,
                                uint8_t *blobs, size_t blobs_cap, uint64_t *blob_offsets, uint8_t *compressed,
                                uint8_t index_csum[32], pbs_upload_fixed_timing *timing, double *encrypt_ms);

/* ---- 5. Restore ---- */

/* pbs_restore_range_device (pbs_restore.h) over the ends min((i + 1) * chunk_size, size) of a
 * fixed index (`digests`: n = pbs_fidx_count(size, chunk_size) entries, host; another n is
 * PBS_ERR_INVALID): image bytes [offset, offset + len) to out_dev, every byte verified.  The
 * covering entries come from pbs_fidx_chunk_from_offset; a chunk whose decoded length is not
 * its (clipped) length is PBS_BLOB_ST_BAD_SIZE.  Store, statuses, zeros for failed entries
 * and scratch as there. */
int pbs_restore_fixed_range_device(const uint8_t *digests, size_t n, uint64_t size, uint64_t chunk_size,
                                   const uint8_t *store_blobs_dev, const uint64_t *store_offsets,
                                   const uint8_t *store_digests, size_t m, const pbs_crypt_config *cfg,
                                   uint64_t offset, uint64_t len, uint8_t *out_dev, uint8_t *entry_status,
                                   pbs_restore_timing *timing, void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* PBS_FIXED_H */
