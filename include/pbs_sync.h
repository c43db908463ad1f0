/*
 * pbs_sync.h -- C ABI of the datastore's sync job (pull): the local chunk store's listing as a
 * table in device memory that GROWS, the fetch plan of one index (which entries are the first
 * occurrence of a chunk the store neither has nor has already asked for), the verdict on the
 * blobs the caller fetched, and the insert of the good ones.
 *
 * Reference interfaces replaced:
 *  - `pull_index_chunks` (src/server/pull.rs:605-705): the `downloaded_chunks` filter (:616-630),
 *    `cond_touch_chunk` (:657-663), `read_raw_chunk` with the byte and chunk counters (:665-674),
 *    `verify_unencrypted` + `insert_chunk` (:639-642);
 *  - `verify_archive` (:707-722): index size and checksum against the manifest's FileInfo;
 *  - the fresh `downloaded_chunks` of `pull_group` (:1134).
 *
 * Conventions are those of pbs_verify.h: a single-owner handle (distinct handles are independent
 * and may live at once), every call synchronous on the handle's `hip_stream`, timing pointers
 * that may be NULL, the codes of pbs_chunker.h, per-call work areas kept between calls until
 * pbs_sync_release().  No call touches a file: the caller lists the store, fetches the blobs the
 * plan names, writes the files of the inserted chunks and updates the atime of the touched ones.
 * Every call on a handle that pbs_sync_end has seen (or on NULL) is PBS_ERR_INVALID.
 *
 * THE ENTRIES.  The handle keeps a digest list: positions 0 .. m-1 are the listing handed to
 * pbs_sync_begin, later positions are appended by plans, in the order the reference would have
 * met them.  Each entry has a `present` byte (the chunk file exists: 1 for the listing, set by a
 * submit whose blob verified) and a `claimed` byte (the digest is in `downloaded_chunks` of the
 * current group).  Where a digest sits at several listing positions the LOWEST is the chunk, and
 * only its bytes are ever read or written.
 *
 * One index is pulled by pbs_sync_plan (or pbs_sync_index_image), pbs_sync_submit (as often as
 * it takes to hand over every fetch item) and pbs_sync_finish.
 */
#ifndef PBS_SYNC_H
#define PBS_SYNC_H

#include <stddef.h>
#include <stdint.h>

#include "pbs_blob.h"
#include "pbs_chunker.h"
#include "pbs_verify.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pbs_sync pbs_sync;

/* verdict[i] of an index entry */
#define PBS_SYNC_DUP 0    /* filtered by downloaded_chunks: claimed earlier in this index or this group */
#define PBS_SYNC_EXISTS 1 /* claimed here; the chunk is present: cond_touch_chunk returned true */
#define PBS_SYNC_FETCH 2  /* claimed here; the chunk is absent: read_raw_chunk */

/* status[t] of a submitted blob: PBS_BLOB_ST_* (pbs_blob.h, pbs_restore.h: 0..10) or */
#define PBS_SYNC_ST_LOAD_FAILED 32 /* the caller could not fetch the blob (read_raw_chunk's Err) */

/* first_failed of a result with no failing item */
#define PBS_SYNC_NONE UINT64_MAX

/* index_check of pbs_sync_index_image: PBS_VERIFY_INDEX_OK / WRONG_SIZE / WRONG_CSUM (pbs_verify.h) */

typedef struct {
    uint64_t entries;      /* n of the plan */
    uint64_t dup;          /* entries with verdict DUP */
    uint64_t exists;       /* ... EXISTS: the touch list's length */
    uint64_t fetch;        /* ... FETCH: the fetch list's length */
    uint64_t appended;     /* entries the plan appended to the digest list */
    uint64_t inserted;     /* fetch items whose status was OK: entries that became present */
    uint64_t failed;       /* fetch items with another status, load failures apart */
    uint64_t load_failed;  /* fetch items the caller could not fetch */
    uint64_t chunk_count;  /* PullStats::chunk_count: the items that were fetched (:674) */
    uint64_t bytes;        /* PullStats::bytes: their raw lengths (:673) */
    uint64_t first_failed; /* the lowest fetch item whose status is not OK -- where the reference
                              would have bailed -- or PBS_SYNC_NONE */
    uint32_t ok;           /* failed == 0 && load_failed == 0 */
    uint32_t reserved;
} pbs_sync_result;

/* one submit: the record of pbs_verify_submit (state_ms: the kernel that sets `present`) */
typedef pbs_verify_timing pbs_sync_timing;

/* ---- 1. The worker ---- */

/* Uploads the local store's listing (entry j: the digest store_digests[32 j ..]; host; duplicates
 * allowed, the lowest position is the chunk; m + reserve < 2^32 - 16, m == 0 is legal) and builds
 * the table of pbs_gc_begin for m + reserve entries: capacity 2^L, the smallest power of two >=
 * max(2 (m + reserve), 64), home slot pbs_gc_home_slot, linear probing.  `reserve` is the number
 * of chunks the caller expects to add: with enough of it no plan ever rebuilds the table.  count
 * = m, every present byte 1, every claimed byte 0.  *build_ms (may be NULL): the table build by
 * HIP events, without the upload. */
int pbs_sync_begin(const uint8_t *store_digests, size_t m, size_t reserve, pbs_sync **h, double *build_ms,
                   void *hip_stream);
/* The entry count and L as they stand (0 on a dead handle). */
size_t pbs_sync_count(pbs_sync *h);
uint32_t pbs_sync_table_log2(pbs_sync *h);
/* The entries as they stand, in host memory: the first min(cap, count) digests (32 each) and
 * present bytes; either list may be NULL; *count (may be NULL): the entry count. */
int pbs_sync_listing(pbs_sync *h, uint8_t *digests_out, uint8_t *present_out, size_t cap, size_t *count);
/* Clears every claimed byte: the fresh downloaded_chunks of the next group (pull.rs:1134).  With
 * an index open: PBS_ERR_INVALID. */
int pbs_sync_new_group(pbs_sync *h);
/* Frees the handle and its device memory (NULL or a dead handle: nothing). */
void pbs_sync_end(pbs_sync *h);
/* Frees the idle per-call work areas of this header; legal with no handle alive. */
void pbs_sync_release(void);

/* ---- 2. One index: plan, submit, finish ---- */

/* `digests` (32 n) and `sizes` (n) are host arrays, as pbs_verify_plan takes them; count + n <
 * 2^32 - 16, else PBS_ERR_INVALID.  The result is that of this sequential rule over i = 0 .. n-1
 * (pull.rs:616-663 with a chunk reader that answers at once):
 *   let c be the lowest entry position carrying digests[i], if any;
 *   c exists and claimed[c]:  verdict[i] = PBS_SYNC_DUP;
 *   otherwise claim it: with no c, append the digest at c = count++ with present = 0; claimed[c] = 1;
 *     present[c]:  verdict[i] = PBS_SYNC_EXISTS, c goes to the touch list;
 *     else:        verdict[i] = PBS_SYNC_FETCH, (c, i) goes to the fetch list.
 * So both lists are in ascending index position of the claiming entry, new entries get ascending
 * positions in that same order, and an entry that an earlier group left absent is fetched again
 * at its old position.  verdict (n bytes) may be NULL.  The first fcap / tcap items of the lists
 * go out (a list may be NULL with a cap of 0; caps of n are always enough); *n_fetch and *n_touch
 * (both required) are the lists' lengths, and pbs_sync_lists returns the lists again.  If 2
 * (count + n) exceeds the table's capacity the table is first rebuilt over all entries with L =
 * table_log2_for(count + n) + 1; positions, present and claimed are unchanged by that.  A plan
 * while an index is open is PBS_ERR_INVALID.  *plan_ms (may be NULL): the kernels, by HIP events
 * (a rebuild included). */
int pbs_sync_plan(pbs_sync *h, const uint8_t *digests, const uint64_t *sizes, size_t n, uint8_t *verdict,
                  uint32_t *fetch_store, uint32_t *fetch_entry, size_t fcap, size_t *n_fetch,
                  uint32_t *touch_store, size_t tcap, size_t *n_touch, double *plan_ms);
/* The lists of the open index again (no index open: PBS_ERR_INVALID). */
int pbs_sync_lists(pbs_sync *h, uint32_t *fetch_store, uint32_t *fetch_entry, size_t fcap, size_t *n_fetch,
                   uint32_t *touch_store, size_t tcap, size_t *n_touch);

/* The next k fetch items, in fetch order, as raw blob images: item t is [blob_offsets[t],
 * blob_offsets[t+1]) of blobs_dev (device memory, never written; k + 1 ascending host offsets).
 * load_failed (NULL or k host bytes): != 0 marks a blob the caller could not fetch; its bytes are
 * ignored and its status is PBS_SYNC_ST_LOAD_FAILED.  The rest is handled exactly as
 * pbs_verify_submit handles it: the magic of every blob is read first and an encrypted blob gets
 * a zero-length output slot; pbs_blob_decode_inflate_device with no config, the plan's digests
 * and sizes and sizes_exact = 1; NO_CONFIG becomes OK (an encrypted chunk is verified by its CRC
 * alone); a chunk LONGER than the index's size reports BAD_DIGEST.  There is no crypt-mode check:
 * the reference has none here.  Status OK sets present = 1 for the entry (insert_chunk: the
 * caller writes the file); any other status leaves the entry absent and still claimed.
 * chunk_count += 1 and bytes += the raw length for every item that is not load_failed (the
 * reference counts after read_raw_chunk, before the verdict).  kinds / status (host, k each) may
 * be NULL.  Submitting more than remain, or with no plan: PBS_ERR_INVALID, nothing consumed. */
int pbs_sync_submit(pbs_sync *h, const uint8_t *blobs_dev, const uint64_t *blob_offsets,
                    const uint8_t *load_failed, size_t k, uint8_t *kinds, uint8_t *status, pbs_sync_timing *timing);

/* Closes the index: *res (may be NULL).  Before every fetch item was submitted, or with no plan:
 * PBS_ERR_INVALID. */
int pbs_sync_finish(pbs_sync *h, pbs_sync_result *res);
/* Drops the rest of the plan (no plan: nothing, PBS_OK).  Claims, appended entries and the
 * inserts of the items already submitted stay: what the reference's `?` leaves behind in
 * downloaded_chunks and in the store. */
int pbs_sync_abort_index(pbs_sync *h);

/* A whole index image (host memory): recognised and checked as pbs_gc_mark_index_image does it
 * (same codes; nothing changes on a bad image), then verify_archive (pull.rs:707-722) against
 * the manifest's FileInfo (info_size / info_csum, each may be NULL: not checked).  *index_check
 * (required): PBS_VERIFY_INDEX_*; on WRONG_SIZE or WRONG_CSUM the call returns PBS_OK, nothing is
 * claimed, no plan is open and *n_fetch = *n_touch = 0.  Otherwise the image's digests and
 * chunk_info sizes are planned as pbs_sync_plan plans them; *n_entries (may be NULL): n. */
int pbs_sync_index_image(pbs_sync *h, const uint8_t *image, size_t len, const uint64_t *info_size,
                         const uint8_t *info_csum, uint32_t *index_check, size_t *n_entries, uint8_t *verdict,
                         size_t vcap, uint32_t *fetch_store, uint32_t *fetch_entry, size_t fcap, size_t *n_fetch,
                         uint32_t *touch_store, size_t tcap, size_t *n_touch, double *plan_ms);

/* ---- 3. Host mirror ---- */

/* The same calls on the host (every pointer host memory, no device): what the GPU is compared
 * against, and sync where there is no device.  Same arguments, same codes, same results, the
 * table's L included. */
typedef struct pbs_sync_host pbs_sync_host;
int pbs_sync_begin_host(const uint8_t *store_digests, size_t m, size_t reserve, pbs_sync_host **h, double *build_ms);
size_t pbs_sync_count_host(pbs_sync_host *h);
uint32_t pbs_sync_table_log2_host(pbs_sync_host *h);
int pbs_sync_listing_host(pbs_sync_host *h, uint8_t *digests_out, uint8_t *present_out, size_t cap, size_t *count);
int pbs_sync_new_group_host(pbs_sync_host *h);
void pbs_sync_end_host(pbs_sync_host *h);
int pbs_sync_plan_host(pbs_sync_host *h, const uint8_t *digests, const uint64_t *sizes, size_t n, uint8_t *verdict,
                       uint32_t *fetch_store, uint32_t *fetch_entry, size_t fcap, size_t *n_fetch,
                       uint32_t *touch_store, size_t tcap, size_t *n_touch, double *plan_ms);
int pbs_sync_lists_host(pbs_sync_host *h, uint32_t *fetch_store, uint32_t *fetch_entry, size_t fcap, size_t *n_fetch,
                        uint32_t *touch_store, size_t tcap, size_t *n_touch);
int pbs_sync_submit_host(pbs_sync_host *h, const uint8_t *blobs, const uint64_t *blob_offsets,
                         const uint8_t *load_failed, size_t k, uint8_t *kinds, uint8_t *status,
                         pbs_sync_timing *timing);
int pbs_sync_finish_host(pbs_sync_host *h, pbs_sync_result *res);
int pbs_sync_abort_index_host(pbs_sync_host *h);
int pbs_sync_index_image_host(pbs_sync_host *h, const uint8_t *image, size_t len, const uint64_t *info_size,
                              const uint8_t *info_csum, uint32_t *index_check, size_t *n_entries, uint8_t *verdict,
                              size_t vcap, uint32_t *fetch_store, uint32_t *fetch_entry, size_t fcap,
                              size_t *n_fetch, uint32_t *touch_store, size_t tcap, size_t *n_touch, double *plan_ms);

#ifdef __cplusplus
}
#endif

#endif /* PBS_SYNC_H */
