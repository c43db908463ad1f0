/*
 * pbs_verify.h -- C ABI of the datastore's verify job: the worker's memory of verified and
 * corrupt chunks as one state byte per store entry in device memory, the load plan of one index
 * (which chunk files to read, in which order), the verdict on the blobs the caller read, and
 * the per-index error count that decides the snapshot's VerifyState.
 *
 * Reference interfaces replaced:
 *  - `VerifyWorker` (src/backup/verify.rs:27-46): `verified_chunks` / `corrupt_chunks`, and
 *    `skip_chunk` (:163-188);
 *  - `DataStore::get_chunks_in_order` (pbs-datastore/src/datastore.rs:1249-1293) with its
 *    within-index deduplication and its inode sort;
 *  - `verify_index_chunks` (verify.rs:108-270): `load_chunk`, the crypt-mode check of chunk
 *    against index (:130-148), `verify_unencrypted` (data_blob.rs:310-333: an encrypted chunk is
 *    verified by its CRC alone, without a key), the error count;
 *  - `verify_fixed_index` / `verify_dynamic_index` (:272-314): index size and checksum against the
 *    manifest's FileInfo;
 *  - `verify_blob` (:48-70).
 *
 * Conventions are those of pbs_gc.h: a single-owner handle (distinct handles are independent and
 * may live at once), every call synchronous on the handle's `hip_stream`, timing pointers that
 * may be NULL, the codes of pbs_chunker.h, per-call work areas kept between calls until
 * pbs_verify_release().  No call touches a file: the caller lists the store, reads the chunk
 * files the plan names and renames the corrupt ones.  Every call on a handle that
 * pbs_verify_end has seen (or on NULL) is PBS_ERR_INVALID.
 *
 * One index is verified by pbs_verify_plan, pbs_verify_submit (as often as it takes to hand
 * over every planned blob) and pbs_verify_finish; pbs_verify_index_device does all three for a
 * store whose blobs are resident in device memory.
 *
 * THE ERROR COUNT.  errors = (index entries whose digest no store entry carries, or whose chunk
 * is CORRUPT when the index is finished, every occurrence) + (crypt-mode mismatches of this
 * index).  This is verify.rs's count with a decoder pool that answers at once and
 * ChunkOrder::None: every occurrence of a chunk an earlier index found corrupt logs "was marked
 * as corrupt" (:171-184); a chunk found corrupt here counts once at its load or verify and once
 * per later occurrence at the recheck (:209-212).  The reference's own number can be smaller:
 * its recheck races with its decoder pool, so a later occurrence of a chunk whose verdict has
 * not arrived yet is loaded again and deduplicated nowhere.  Only `errors > 0` is observable
 * there ("chunks could not be verified", :265), and that is the same here.
 */
#ifndef PBS_VERIFY_H
#define PBS_VERIFY_H

#include <stddef.h>
#include <stdint.h>

#include "pbs_blob.h"
#include "pbs_chunker.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pbs_verify pbs_verify;

/* states[j] of a store entry */
#define PBS_VERIFY_UNKNOWN 0
#define PBS_VERIFY_VERIFIED 1 /* in verified_chunks */
#define PBS_VERIFY_CORRUPT 2  /* in corrupt_chunks */

/* index_mode: FileInfo::chunk_crypt_mode() (pbs-datastore/src/manifest.rs:39-44; SignOnly maps to NONE) */
#define PBS_VERIFY_MODE_NONE 0
#define PBS_VERIFY_MODE_ENCRYPT 1

/* status[t] of a submitted blob: PBS_BLOB_ST_* (pbs_blob.h, pbs_restore.h: 0..10) or */
#define PBS_VERIFY_ST_LOAD_FAILED 32 /* the caller could not open or read the file (load_chunk's Err, :215) */

/* index_check of a result */
#define PBS_VERIFY_INDEX_OK 0
#define PBS_VERIFY_INDEX_WRONG_SIZE 1 /* index_bytes != FileInfo.size (:283-285, :305-307) */
#define PBS_VERIFY_INDEX_WRONG_CSUM 2 /* compute_csum != FileInfo.csum (:287-289, :309-311) */

typedef struct {
    uint64_t entries;          /* n of the plan */
    uint64_t skipped_verified; /* occurrences whose chunk was VERIFIED when the plan was made */
    uint64_t skipped_corrupt;  /* occurrences whose chunk was CORRUPT when the plan was made */
    uint64_t loaded;           /* submitted blobs that loaded (size, magic and CRC passed) */
    uint64_t newly_verified;   /* store entries that became VERIFIED in this index */
    uint64_t newly_corrupt;    /* ... CORRUPT */
    uint64_t mode_mismatch;    /* loaded blobs whose crypt mode is not index_mode */
    uint64_t missing;          /* occurrences whose digest no store entry carries */
    uint64_t read_bytes;       /* raw sizes of the loaded blobs (:235) */
    uint64_t decoded_bytes;    /* sizes[entry] of the loaded blobs (:237) */
    uint64_t errors;           /* see the head of this file */
    uint32_t ok;               /* errors == 0 and index_check == OK */
    uint32_t index_check;      /* PBS_VERIFY_INDEX_*; set by pbs_verify_index_* only */
} pbs_verify_result;

typedef struct {
    double total_ms;     /* call entry .. outputs on the host */
    double magic_ms;     /* the magic read (HIP events; the host mirror: 0) */
    double decode_ms;    /* pbs_blob_decode_inflate_device's total */
    double state_ms;     /* the state kernel */
    uint64_t blobs;      /* k */
    uint64_t decoded;    /* blobs handed to the decoder (k less the load failures) */
    uint64_t encrypted;  /* of those, blobs with an encrypted magic */
    uint64_t scratch_bytes; /* output scratch the decode was given: the sum of sizes[entry] over
                               the unencrypted blobs, 0 for an all-encrypted batch */
} pbs_verify_timing;

/* ---- 1. The worker ---- */

/* Uploads the listing of chunk files (entry j: the digest store_digests[32 j ..]; host; m < 2^32
 * - 16, m == 0 is legal) and builds the table of pbs_gc_begin: capacity 2^L, the smallest power
 * of two >= max(2 m, 64), home slot pbs_gc_home_slot, linear probing.  Duplicates are allowed:
 * the LOWEST position carrying a digest is the chunk (as in pbs_restore_range_device), and only
 * its state is ever read or written.  One state byte per entry, all PBS_VERIFY_UNKNOWN; they
 * live until pbs_verify_end: the worker's memory across indexes and snapshots.  *build_ms (may
 * be NULL): the table build by HIP events, without the upload. */
int pbs_verify_begin(const uint8_t *store_digests, size_t m, pbs_verify **h, double *build_ms,
                     void *hip_stream);
/* states_host[j] for all m entries (m must be the handle's). */
int pbs_verify_states(pbs_verify *h, uint8_t *states_host, size_t m);
/* Frees the handle and its device memory (NULL or a dead handle: nothing). */
void pbs_verify_end(pbs_verify *h);
/* Frees the idle per-call work areas of this header; legal with no handle alive. */
void pbs_verify_release(void);

/* ---- 2. One index: plan, submit, finish ---- */

/* skip_chunk + get_chunks_in_order.  `digests` (32 n) and `sizes` (n) are host arrays: entry i's
 * digest and chunk_info(i).size(), for .didx and .fidx alike; n < 2^32 - 16.  index_mode:
 * PBS_VERIFY_MODE_*.  The plan is every store position j that (a) is the lowest one carrying
 * the digest of some index entry and (b) has state UNKNOWN, in ASCENDING STORE POSITION -- the
 * caller's listing order is the read order, which is the role of the reference's inode sort.
 * todo_store[t] = j and todo_entry[t] = the lowest index position naming that chunk
 * (ChunkOrder::None); sizes[todo_entry[t]] is the size that will be checked.  The first `cap`
 * items go out (cap == 0 with both lists NULL is legal); *n_todo (required) is the plan's
 * length, and with *n_todo > cap the caller plans again (after pbs_verify_abort_index) with
 * larger lists.  A plan while another is unfinished is PBS_ERR_INVALID.  *plan_ms (may be NULL):
 * the kernels, by HIP events. */
int pbs_verify_plan(pbs_verify *h, const uint8_t *digests, const uint64_t *sizes, size_t n, int index_mode,
                    uint32_t *todo_store, uint32_t *todo_entry, size_t cap, size_t *n_todo, double *plan_ms);
/* Drops an unfinished plan without changing a state (no plan: nothing, PBS_OK). */
int pbs_verify_abort_index(pbs_verify *h);

/* The next k items of the plan, in plan order, as raw blob images: item t is
 * [blob_offsets[t], blob_offsets[t+1]) of blobs_dev (device memory, never written; k + 1
 * ascending host offsets).  load_failed (NULL or k host bytes): != 0 marks a file the caller
 * could not open or read; its bytes are ignored and its status is PBS_VERIFY_ST_LOAD_FAILED.
 * The rest goes through pbs_blob_decode_inflate_device with no config, the plan's digests and
 * sizes and sizes_exact = 1, into device scratch that is discarded; NO_CONFIG becomes OK (size,
 * magic and CRC passed and the blob is encrypted: load_chunk followed by verify_unencrypted
 * returning Ok).  The magic of every blob is read first and an encrypted blob gets a
 * zero-length output slot.  status OK makes the chunk VERIFIED, anything else CORRUPT.  The
 * crypt mode of every blob that loaded (status not LOAD_FAILED, TOO_SMALL, BAD_MAGIC, BAD_CRC)
 * is compared with index_mode; a mismatch is counted and does not make the chunk corrupt
 * (verify.rs:140-148).  A chunk LONGER than the index's size reports BAD_DIGEST (the slot rule of
 * pbs_blob_decode_inflate_device) where the reference says "wrong length": corrupt in both.
 * kinds / status (host, k each) may be NULL.  Submitting more than
 * remain, or with no plan: PBS_ERR_INVALID, nothing consumed. */
int pbs_verify_submit(pbs_verify *h, const uint8_t *blobs_dev, const uint64_t *blob_offsets,
                      const uint8_t *load_failed, size_t k, uint8_t *kinds, uint8_t *status,
                      pbs_verify_timing *timing);

/* Closes the index: the counts, corrupt_store (the store positions that became CORRUPT in this
 * index, ascending, the first ccap: the files to rename) and missing_pos (the index positions
 * whose digest is absent, ascending, the first mcap; they have no file to rename: `rename` gets
 * NotFound, ignored at :96).  res, n_corrupt, n_missing and the lists may be NULL (a list only
 * with a cap of 0).  Before every plan item was submitted, or with no plan: PBS_ERR_INVALID. */
int pbs_verify_finish(pbs_verify *h, pbs_verify_result *res, uint32_t *corrupt_store, size_t ccap,
                      size_t *n_corrupt, uint32_t *missing_pos, size_t mcap, size_t *n_missing);

/* A whole index image (host memory) against a store whose blobs are resident in device memory:
 * store entry j's chunk file is [store_offsets[j], store_offsets[j+1]) of store_blobs_dev (m + 1
 * ascending host offsets).  The image is recognised and checked as pbs_gc_mark_index_image does
 * it (same codes; nothing changes).  info_size / info_csum (each may be NULL: not checked) are
 * the manifest's FileInfo: index_bytes != *info_size gives index_check WRONG_SIZE; then the
 * index checksum (pbs_didx_parse's / pbs_fidx_parse's computed_csum) != info_csum gives
 * WRONG_CSUM; in both cases no chunk is touched, no state changes, ok = 0 and the call returns
 * PBS_OK (verify.rs:282-289).  Otherwise plan, then batches of the todo blobs packed with
 * pbs_copy_segments_device (a batch whose blobs already follow one another in the store is
 * taken where it lies) and submitted until the plan is drained, then finish.  A batch is
 * bounded so that its blobs plus its unencrypted output slots stay at or below budget_bytes (0:
 * no bound); a batch always takes at least one blob.  An unfinished plan on the handle:
 * PBS_ERR_INVALID.  A failure inside leaves no plan behind. */
int pbs_verify_index_device(pbs_verify *h, const uint8_t *image, size_t len, int index_mode,
                            const uint64_t *info_size, const uint8_t *info_csum,
                            const uint8_t *store_blobs_dev, const uint64_t *store_offsets,
                            size_t budget_bytes, pbs_verify_result *res, uint32_t *corrupt_store, size_t ccap,
                            size_t *n_corrupt, uint32_t *missing_pos, size_t mcap, size_t *n_missing);

/* ---- 3. verify_blob (:48-70), host only ---- */

#define PBS_VERIFY_BLOB_OK 0
#define PBS_VERIFY_BLOB_WRONG_SIZE 1 /* raw size != FileInfo.size */
#define PBS_VERIFY_BLOB_WRONG_CSUM 2 /* SHA-256 of the raw bytes != FileInfo.csum */
#define PBS_VERIFY_BLOB_LOAD 3       /* size, magic or CRC (load_blob) */
#define PBS_VERIFY_BLOB_DECODE 4     /* decode(None, None) of an unencrypted blob: the zstd frame */
/* The checks in this order: raw size, SHA-256 of the raw bytes, the load (size, magic, CRC), then
 * by magic: an encrypted blob is OK, an unencrypted one goes through decode(None, None), a
 * compressed one inflated by the host inflater.  *result: PBS_VERIFY_BLOB_*; the call returns
 * PBS_OK unless an argument is bad. */
int pbs_verify_blob_host(const uint8_t *raw, size_t len, uint64_t info_size, const uint8_t info_csum[32],
                         int *result);

/* ---- 4. Host mirror ---- */

/* The same calls on the host (every pointer host memory, no device): what the GPU is compared
 * against, and verify where there is no device.  Same arguments, same codes, same results. */
typedef struct pbs_verify_host pbs_verify_host;
int pbs_verify_begin_host(const uint8_t *store_digests, size_t m, pbs_verify_host **h, double *build_ms);
int pbs_verify_states_host(pbs_verify_host *h, uint8_t *states_host, size_t m);
void pbs_verify_end_host(pbs_verify_host *h);
int pbs_verify_plan_host(pbs_verify_host *h, const uint8_t *digests, const uint64_t *sizes, size_t n, int index_mode,
                         uint32_t *todo_store, uint32_t *todo_entry, size_t cap, size_t *n_todo, double *plan_ms);
int pbs_verify_abort_index_host(pbs_verify_host *h);
int pbs_verify_submit_host(pbs_verify_host *h, const uint8_t *blobs, const uint64_t *blob_offsets,
                           const uint8_t *load_failed, size_t k, uint8_t *kinds, uint8_t *status,
                           pbs_verify_timing *timing);
int pbs_verify_finish_host(pbs_verify_host *h, pbs_verify_result *res, uint32_t *corrupt_store, size_t ccap,
                           size_t *n_corrupt, uint32_t *missing_pos, size_t mcap, size_t *n_missing);
int pbs_verify_index_host(pbs_verify_host *h, const uint8_t *image, size_t len, int index_mode,
                          const uint64_t *info_size, const uint8_t *info_csum, const uint8_t *store_blobs,
                          const uint64_t *store_offsets, size_t budget_bytes, pbs_verify_result *res,
                          uint32_t *corrupt_store, size_t ccap, size_t *n_corrupt, uint32_t *missing_pos,
                          size_t mcap, size_t *n_missing);

#ifdef __cplusplus
}
#endif

#endif /* PBS_VERIFY_H */
