/*
 * pbs_backup.h -- C ABI of the datastore's backup session: the job that takes what a client
 * uploads (chunk blobs, then the index entries that name them) and puts it into the store.  The
 * store's listing and this session's `known_chunks` live in one table in device memory that
 * grows; the uploads of a batch are verified on the device and resolved against that table by
 * the insert rule of the chunk store; the appends of a batch are checked against the running sum
 * of the registered lengths; the index writers close into .didx / .fidx images.
 *
 * Reference interfaces replaced:
 *  - `BackupEnvironment` (src/api2/backup/environment.rs): register_chunk (:156-164),
 *    register_fixed_chunk / register_dynamic_chunk (:170-253), lookup_chunk (:255-259), the two
 *    writer registrations (:262-317), dynamic_writer_append_chunk / fixed_writer_append_chunk
 *    (:320-378), log_upload_stat (:380-428), the two closes (:431-564), add_blob (:566-591) and
 *    finish_backup's state checks (:594-606);
 *  - `UploadChunk` (src/api2/backup/upload_chunk.rs:62-85, schema :123-142);
 *  - `ChunkStore::insert_chunk` (pbs-datastore/src/chunk_store.rs:457-497);
 *  - the handlers of src/api2/backup/mod.rs: create_fixed_index with reuse-csum (:447-514),
 *    dynamic_append / fixed_append (:571-585 and its fixed twin), download_previous' chunk
 *    registration (:859-863).
 *
 * Conventions are those of pbs_sync.h: a single-owner handle (distinct handles are independent
 * and may live at once), every call synchronous on the handle's `hip_stream`, timing pointers
 * that may be NULL, the codes of pbs_chunker.h, per-call work areas kept between calls until
 * pbs_backup_release().  No call touches a file: the caller lists the store, writes the chunk
 * files of the items whose action is WRITE with `crc_out` in bytes 8..12, touches the others,
 * and writes the index images.  Every call on a handle that pbs_backup_end has seen (or on
 * NULL) is PBS_ERR_INVALID.  One handle is one session on one datastore.
 *
 * RETURN VALUES.  Negative: PBS_ERR_* (bad arguments, no device, no memory), nothing changed.
 * Positive: a PBS_BACKUP_E_* code, where the reference's request fails before it changes
 * anything.  Calls that handle a list report the list's failure through *err or *result and
 * return PBS_OK.
 *
 * THE ENTRIES.  The handle keeps a digest list: positions 0 .. m-1 are the listing handed to
 * pbs_backup_begin, later positions are appended in the order the sequential rules below meet
 * new digests.  Where the listing repeats a digest the LOWEST position is the chunk.  Each entry
 * carries `present` (1 for the listing), `enc_size` (u64, the file's length), `kind` (the file's
 * magic: PBS_BLOB_KIND_*; PBS_BLOB_KIND_NONE for a file too short to have one or one that was
 * not read; PBS_BACKUP_KIND_NOT_FILE for something at the path that is no file), `known` (a
 * byte) and `known_size` (u32): this session's known_chunks.  The table is sync's: capacity 2^L
 * by sync's rules, grown before a batch that might append (pbs_sync.h).
 */
#ifndef PBS_BACKUP_H
#define PBS_BACKUP_H

#include <stddef.h>
#include <stdint.h>

#include "pbs_blob.h"
#include "pbs_chunker.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pbs_backup pbs_backup;

#define PBS_BACKUP_KIND_NOT_FILE 254

/* status[t] of an uploaded chunk: PBS_BLOB_ST_* (pbs_blob.h, pbs_restore.h: 0..10) or */
#define PBS_BACKUP_ST_BAD_PARAM 33    /* size or encoded-size outside the API schema (upload_chunk.rs:123-142) */
#define PBS_BACKUP_ST_WRONG_LENGTH 34 /* the blob's length is not encoded-size (:62-74) */

/* ins[t]: what insert_chunk made of it (chunk_store.rs:457-497) */
#define PBS_BACKUP_INS_NONE 0             /* status not OK: never got there */
#define PBS_BACKUP_INS_NEW 1              /* no file: written */
#define PBS_BACKUP_INS_DUP_SAME 2         /* a file of the same length */
#define PBS_BACKUP_INS_OVERWRITE_EMPTY 3  /* an empty file: written over */
#define PBS_BACKUP_INS_DUP_KEEP_FIRST 4   /* encrypted, lengths differ: the first stays */
#define PBS_BACKUP_INS_DUP_KEEP_SMALLER 5 /* unencrypted, the file is smaller: it stays */
#define PBS_BACKUP_INS_REPLACE_BIGGER 6   /* unencrypted, the file is bigger: replaced */
#define PBS_BACKUP_INS_ERR_TYPE 16        /* the path holds something that is no file */
#define PBS_BACKUP_INS_ERR_READ 17        /* encrypted, and the file's magic cannot be read */
#define PBS_BACKUP_INS_ERR_UNENC_TO_ENC 18
#define PBS_BACKUP_INS_ERR_ENC_UNCOMPRESSED 19 /* two uncompressed encrypted chunks of unequal length */

/* action[t]: what the caller does with the chunk file */
#define PBS_BACKUP_ACT_NONE 0
#define PBS_BACKUP_ACT_WRITE 1
#define PBS_BACKUP_ACT_TOUCH 2

/* reg[t]: register_fixed_chunk / register_dynamic_chunk (environment.rs:170-253) */
#define PBS_BACKUP_REG_NONE 0 /* the insert failed or never ran */
#define PBS_BACKUP_REG_OK 1
#define PBS_BACKUP_REG_ERR_LARGE 2       /* fixed writer: size > chunk_size */
#define PBS_BACKUP_REG_ERR_MULTI_SMALL 3 /* fixed writer: a second chunk under chunk_size */

/* request failures (returned, or in *err / *result) */
#define PBS_BACKUP_E_NONE 0
#define PBS_BACKUP_E_FINISHED 64 /* ensure_unfinished */
#define PBS_BACKUP_E_NO_WRITER 65
#define PBS_BACKUP_E_NO_SUCH_CHUNK 66   /* lookup_chunk: None */
#define PBS_BACKUP_E_STRANGE_OFFSET 67  /* environment.rs:336-343 */
#define PBS_BACKUP_E_INDEX_RANGE 68     /* add_digest: idx >= index_length */
#define PBS_BACKUP_E_CHUNK_COUNT 69     /* close: chunk_count (:447, :509) */
#define PBS_BACKUP_E_SIZE 70            /* close: size (:456, :530) */
#define PBS_BACKUP_E_EXPECTED_COUNT 71  /* fixed close, not incremental: index_length (:521) */
#define PBS_BACKUP_E_CSUM 72            /* close: checksum (:469, :543) */
#define PBS_BACKUP_E_OPEN_WRITER 73     /* finish (:600) */
#define PBS_BACKUP_E_NO_FILES 74        /* finish (:604) */
#define PBS_BACKUP_E_REUSE_NO_IMAGE 75  /* reuse_csum without a readable previous index (mod.rs:473-488) */
#define PBS_BACKUP_E_REUSE_CSUM 76      /* the previous index's checksum is another (:490-498) */
#define PBS_BACKUP_E_REUSE_LENGTH 77    /* clone_data_from: index lengths differ */
#define PBS_BACKUP_E_TOO_MANY_WRITERS 78 /* wids are 1 .. 256 */

#define PBS_BACKUP_NONE UINT64_MAX /* first_failed of a batch with no failing item */
#define PBS_BACKUP_MAX_CHUNK (16u * 1024 * 1024)

/* UploadStatistic (environment.rs:24-29) and the numbers log_upload_stat prints (:380-428) */
typedef struct {
    uint64_t count, size, compressed_size, duplicates;
    uint64_t chunk_count, archive_size; /* the close's arguments */
    uint64_t upload_percent;            /* size * 100 / archive_size */
    uint64_t client_duplicates;         /* chunk_count - count, 0 if negative */
    uint64_t server_duplicates;         /* duplicates */
    uint64_t duplicate_percent;         /* (client + server) * 100 / chunk_count; 0 when there are none */
    uint64_t compression_percent;       /* compressed_size * 100 / size; 0 when size == 0 */
    uint32_t logged;                    /* 0: archive_size == 0 or chunk_count == 0, the five numbers above are 0 */
    uint32_t reserved;
} pbs_backup_writer_stat;

typedef struct {
    uint64_t file_counter, backup_size;
    uint64_t count, size, compressed_size, duplicates; /* backup_stat */
    uint32_t open_writers, finished;
} pbs_backup_stat;

typedef struct {
    double total_ms;   /* host clock */
    double decode_ms;  /* the decode-inflate calls */
    double insert_ms;  /* claim, sort, walk, register: HIP events */
    uint64_t blobs, decoded, encrypted, scratch_bytes;
} pbs_backup_timing;

/* ---- 1. The session ---- */

/* The store's listing (entry j: digest store_digests[32 j ..], file length store_sizes[j], magic
 * store_kinds[j]; host; duplicates allowed; m + reserve < 2^32 - 16; m == 0 is legal; sizes and
 * kinds may be NULL with m == 0 only) and the table of pbs_sync_begin.  count = m, present 1,
 * known 0. */
int pbs_backup_begin(const uint8_t *store_digests, const uint64_t *store_sizes, const uint8_t *store_kinds, size_t m,
                     size_t reserve, pbs_backup **h, double *build_ms, void *hip_stream);
size_t pbs_backup_count(pbs_backup *h);
uint32_t pbs_backup_table_log2(pbs_backup *h);
/* The entries as they stand: the first min(cap, count) of each list that is not NULL. */
int pbs_backup_listing(pbs_backup *h, uint8_t *digests_out, uint8_t *present_out, uint64_t *size_out,
                       uint8_t *kind_out, uint8_t *known_out, uint32_t *known_size_out, size_t cap, size_t *count);
/* lookup_chunk: PBS_OK and *size, or PBS_BACKUP_E_NO_SUCH_CHUNK. */
int pbs_backup_lookup(pbs_backup *h, const uint8_t digest[32], uint32_t *size);
/* The session's counters (legal on a finished session). */
int pbs_backup_stats(pbs_backup *h, pbs_backup_stat *stat);
/* E_OPEN_WRITER, then E_NO_FILES, then finished = 1; *stat (may be NULL) as pbs_backup_stats. */
int pbs_backup_finish(pbs_backup *h, pbs_backup_stat *stat);
void pbs_backup_end(pbs_backup *h);
void pbs_backup_release(void);

/* ---- 2. known_chunks of the previous backup ---- */

/* For i ascending: known[digests[i]] = sizes[i]; a digest not in the list is appended with
 * present = 0.  Within a call the highest i of a digest wins; a later call overwrites.  *ms (may
 * be NULL; the appends' too): the kernels by HIP events, a table growth included and the copies
 * left out; the mirror's host clock. */
int pbs_backup_register_previous(pbs_backup *h, const uint8_t *digests, const uint32_t *sizes, size_t n,
                                 double *ms);
/* The same from a .didx or .fidx image (host): recognised and checked as pbs_gc_mark_index_image
 * does it (same codes; nothing changes on a bad image), the sizes are the index's own chunk_info
 * ranges (one above 2^32 - 1: PBS_ERR_INVALID).  *n_entries (may be NULL): the image's entries. */
int pbs_backup_register_index_image(pbs_backup *h, const uint8_t *image, size_t len, size_t *n_entries, double *ms);

/* ---- 3. Uploads ---- */

/* k chunks for writer `wid`: blob t is [blob_offsets[t], blob_offsets[t+1]) of blobs_dev (device
 * memory, never written), announced as digests[32 t ..], sizes[t] and encoded_sizes[t]
 * (encoded_sizes NULL: taken as the blobs' lengths).  The result is that of handling t = 0 ..
 * k-1 one after the other:
 *  status[t], the first failing check of: BAD_PARAM (sizes[t] outside 1 .. 16 MiB, encoded size
 *    outside 13 .. 16 MiB + 44), WRONG_LENGTH, TOO_SMALL / BAD_MAGIC (from_raw), and for kinds 0
 *    and 1 only BAD_FRAME / UNSUPPORTED_FRAME, BAD_DIGEST, BAD_SIZE exactly as
 *    pbs_blob_decode_inflate_device reports them with no config, `digests`, `sizes` and
 *    sizes_exact = 1.  The stored CRC is NOT judged (upload_chunk.rs:77-85); an encrypted blob
 *    is accepted after from_raw.
 *  crc_out[t]: the CRC-32 of the bytes after the blob header, where from_raw passed (else 0).
 *  ins[t], for status OK, against the digest's entry (appended with present = 0 if new), the
 *    first that applies: !present NEW; kind NOT_FILE ERR_TYPE; len == enc_size DUP_SAME;
 *    enc_size == 0 OVERWRITE_EMPTY; incoming encrypted: entry kind NONE ERR_READ, 0 or 1
 *    ERR_UNENC_TO_ENC, 2 with incoming 2 ERR_ENC_UNCOMPRESSED, else DUP_KEEP_FIRST; enc_size <
 *    len DUP_KEEP_SMALLER; else REPLACE_BIGGER.  NEW, OVERWRITE_EMPTY and REPLACE_BIGGER set the
 *    entry to (1, len, kind): is_duplicate 0, compressed_size len, action WRITE.  DUP_*:
 *    is_duplicate 1, compressed_size the low 32 bits of enc_size, action TOUCH.
 *  reg[t], where the insert succeeded: fixed writer: sizes[t] > chunk_size ERR_LARGE; sizes[t] <
 *    chunk_size counts a small chunk (also when it then fails) and a count above 1 is
 *    ERR_MULTI_SMALL; REG_OK adds to the writer's UploadStatistic and sets known[digest] =
 *    sizes[t].  A chunk that fails here stays inserted.
 *  *first_failed: the lowest t that is not REG_OK, or PBS_BACKUP_NONE.
 * Every output array (k each, host) may be NULL. */
int pbs_backup_upload(pbs_backup *h, uint32_t wid, const uint8_t *digests, const uint32_t *sizes,
                      const uint32_t *encoded_sizes, const uint8_t *blobs_dev, const uint64_t *blob_offsets, size_t k,
                      uint8_t *status, uint32_t *crc_out, uint8_t *ins, uint8_t *action, uint8_t *is_duplicate,
                      uint32_t *compressed_size, uint8_t *reg, uint64_t *first_failed, pbs_backup_timing *timing);

/* ---- 4. Index writers ---- */

/* Wids count up from 1 across both kinds; the 257th is E_TOO_MANY_WRITERS. */
int pbs_backup_create_dynamic(pbs_backup *h, const uint8_t uuid[16], int64_t ctime, uint32_t *wid);
/* chunk_size == 0: PBS_ERR_INVALID.  reuse_csum != NULL: incremental (mod.rs:471-507): the
 * previous index image (host) must parse (E_REUSE_NO_IMAGE), its checksum equal reuse_csum
 * (E_REUSE_CSUM), its index length the new one's (E_REUSE_LENGTH); its digests are copied in. */
int pbs_backup_create_fixed(pbs_backup *h, uint64_t size, uint64_t chunk_size, const uint8_t uuid[16], int64_t ctime,
                            const uint8_t *reuse_image, size_t reuse_len, const uint8_t *reuse_csum, uint32_t *wid);

/* For i ascending: !known[digests[i]] E_NO_SUCH_CHUNK; offsets[i] != the writer's offset
 * E_STRANGE_OFFSET; else offset += known_size, chunk_count += 1, (offset, digest) joins the
 * index.  Stops at the first failure: *n_done = i (n when none), *err its code; the entries
 * before it stay appended. */
int pbs_backup_dynamic_append(pbs_backup *h, uint32_t wid, const uint8_t *digests, const uint64_t *offsets, size_t n,
                              size_t *n_done, int *err, double *ms);
/* The same with end = offsets[i] + known_size: pbs_fidx_check_chunk_alignment(size, chunk_size,
 * end, known_size)'s code (negative) is passed through, idx >= index_length is E_INDEX_RANGE,
 * else digest -> slot idx, chunk_count += 1.  Offsets come in any order; the higher i wins a
 * slot. */
int pbs_backup_fixed_append(pbs_backup *h, uint32_t wid, const uint8_t *digests, const uint64_t *offsets, size_t n,
                            size_t *n_done, int *err, double *ms);

/* environment.rs:431-564.  *result: E_NO_WRITER, or the first failing check: E_CHUNK_COUNT; for
 * the dynamic writer E_SIZE; for the fixed writer that is not incremental E_EXPECTED_COUNT, then
 * E_SIZE; E_CSUM.  The writer is removed whenever it existed.  On E_NONE the image
 * (pbs_didx_size(chunk_count) / pbs_fidx_size(index length) bytes) goes to image_out (NULL: not
 * wanted; else cap below that is PBS_ERR_CAPACITY with the writer left open), file_counter,
 * backup_size and backup_stat advance, and *stat (may be NULL) is filled. */
int pbs_backup_dynamic_close(pbs_backup *h, uint32_t wid, uint64_t chunk_count, uint64_t size, const uint8_t csum[32],
                             uint8_t *image_out, size_t cap, int *result, pbs_backup_writer_stat *stat);
int pbs_backup_fixed_close(pbs_backup *h, uint32_t wid, uint64_t chunk_count, uint64_t size, const uint8_t csum[32],
                           uint8_t *image_out, size_t cap, int *result, pbs_backup_writer_stat *stat);

/* add_blob (:566-591), a host call: from_raw + verify_crc into *status (PBS_BLOB_ST_OK,
 * TOO_SMALL, BAD_MAGIC, BAD_CRC); OK: file_counter += 1, backup_size += len, backup_stat.size +=
 * len. */
int pbs_backup_add_blob(pbs_backup *h, const uint8_t *raw, size_t len, uint8_t *status);

/* ---- 5. Host mirror ---- */

/* The same calls on the host (every pointer host memory, no device): what the GPU is compared
 * against, and a session where there is no device.  Same arguments, codes and results, the
 * table's L included. */
typedef struct pbs_backup_host pbs_backup_host;
int pbs_backup_begin_host(const uint8_t *store_digests, const uint64_t *store_sizes, const uint8_t *store_kinds,
                          size_t m, size_t reserve, pbs_backup_host **h, double *build_ms);
size_t pbs_backup_count_host(pbs_backup_host *h);
uint32_t pbs_backup_table_log2_host(pbs_backup_host *h);
int pbs_backup_listing_host(pbs_backup_host *h, uint8_t *digests_out, uint8_t *present_out, uint64_t *size_out,
                            uint8_t *kind_out, uint8_t *known_out, uint32_t *known_size_out, size_t cap,
                            size_t *count);
int pbs_backup_lookup_host(pbs_backup_host *h, const uint8_t digest[32], uint32_t *size);
int pbs_backup_stats_host(pbs_backup_host *h, pbs_backup_stat *stat);
int pbs_backup_finish_host(pbs_backup_host *h, pbs_backup_stat *stat);
void pbs_backup_end_host(pbs_backup_host *h);
int pbs_backup_register_previous_host(pbs_backup_host *h, const uint8_t *digests, const uint32_t *sizes, size_t n,
                                      double *ms);
int pbs_backup_register_index_image_host(pbs_backup_host *h, const uint8_t *image, size_t len, size_t *n_entries,
                                         double *ms);
int pbs_backup_upload_host(pbs_backup_host *h, uint32_t wid, const uint8_t *digests, const uint32_t *sizes,
                           const uint32_t *encoded_sizes, const uint8_t *blobs, const uint64_t *blob_offsets, size_t k,
                           uint8_t *status, uint32_t *crc_out, uint8_t *ins, uint8_t *action, uint8_t *is_duplicate,
                           uint32_t *compressed_size, uint8_t *reg, uint64_t *first_failed,
                           pbs_backup_timing *timing);
int pbs_backup_create_dynamic_host(pbs_backup_host *h, const uint8_t uuid[16], int64_t ctime, uint32_t *wid);
int pbs_backup_create_fixed_host(pbs_backup_host *h, uint64_t size, uint64_t chunk_size, const uint8_t uuid[16],
                                 int64_t ctime, const uint8_t *reuse_image, size_t reuse_len,
                                 const uint8_t *reuse_csum, uint32_t *wid);
int pbs_backup_dynamic_append_host(pbs_backup_host *h, uint32_t wid, const uint8_t *digests, const uint64_t *offsets,
                                   size_t n, size_t *n_done, int *err, double *ms);
int pbs_backup_fixed_append_host(pbs_backup_host *h, uint32_t wid, const uint8_t *digests, const uint64_t *offsets,
                                 size_t n, size_t *n_done, int *err, double *ms);
int pbs_backup_dynamic_close_host(pbs_backup_host *h, uint32_t wid, uint64_t chunk_count, uint64_t size,
                                  const uint8_t csum[32], uint8_t *image_out, size_t cap, int *result,
                                  pbs_backup_writer_stat *stat);
int pbs_backup_fixed_close_host(pbs_backup_host *h, uint32_t wid, uint64_t chunk_count, uint64_t size,
                                const uint8_t csum[32], uint8_t *image_out, size_t cap, int *result,
                                pbs_backup_writer_stat *stat);
int pbs_backup_add_blob_host(pbs_backup_host *h, const uint8_t *raw, size_t len, uint8_t *status);

#ifdef __cplusplus
}
#endif

#endif /* PBS_BACKUP_H */
