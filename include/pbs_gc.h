/*
 * pbs_gc.h -- C ABI of datastore garbage collection: the chunk store's listing as a hash set
 * resident in device memory, index files streamed through it (phase 1, "mark"), and the sweep
 * plan with the GC status (phase 2).
 *
 * Reference interfaces replaced:
 *  - `DataStore::garbage_collection` (pbs-datastore/src/datastore.rs:1065-1177);
 *  - `mark_used_chunks` / `index_mark_used_chunks` (:952-1055): one `cond_touch_chunk` per index
 *    entry, the ten `<digest>.N.bad` paths for an entry whose chunk is absent (:973-982);
 *  - `ChunkStore::get_chunk_iterator` (pbs-datastore/src/chunk_store.rs:247-343) and
 *    `sweep_unused_chunks` (:350-440);
 *  - `GarbageCollectionStatus` (pbs-api-types/src/datastore.rs:1308-1330).
 *
 * Nothing here touches a file: the caller lists the store, hands over sizes and atimes, and
 * applies the plan (set atimes, unlink).  Conventions are those of pbs_restore.h: the codes of
 * pbs_chunker.h, every call synchronous on the handle's `hip_stream`, timing pointers that may
 * be NULL, per-call work areas kept between calls until pbs_gc_release().  A handle is
 * single-owner; distinct handles are independent and may live at once.  Every call on a handle
 * that pbs_gc_end has seen (or on NULL) is PBS_ERR_INVALID.
 */
#ifndef PBS_GC_H
#define PBS_GC_H

#include <stddef.h>
#include <stdint.h>

#include "pbs_chunker.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pbs_gc pbs_gc;

/* flags[j] of a listing entry (any other bit: PBS_ERR_INVALID) */
#define PBS_GC_BAD 1     /* name ends in ".bad": counted as a bad file (chunk_store.rs:296) */
#define PBS_GC_FOREIGN 2 /* listed by get_chunk_iterator but at a path phase 1 never touches */

/* actions[j] */
#define PBS_GC_KEEP 0 /* "disk" class, or vanished */
#define PBS_GC_PENDING 1
#define PBS_GC_REMOVE 2
#define PBS_GC_VANISHED UINT64_MAX /* sizes[j]: stat failed, entry skipped (the `if let Ok(stat)` of :395) */

typedef struct { /* GarbageCollectionStatus without upid, same meaning field by field */
    uint64_t index_file_count, index_data_bytes, disk_bytes, disk_chunks, removed_bytes, removed_chunks,
        pending_bytes, pending_chunks, removed_bad, still_bad;
} pbs_gc_status;

/* ---- 1. The store ---- */

/* Uploads the listing (entry j: the digest store_digests[32 j ..] and flags[j]; host; m < 2^32 -
 * 16, m == 0 is legal) and builds an open-addressing table of u32 store positions in the memory
 * of `hip_stream`'s device.  Capacity 2^L, the smallest power of two >= max(2 m, 64); an entry's
 * home slot is pbs_gc_home_slot; probing is linear with wrap-around.  EVERY entry takes a slot
 * of its own: equal digests are not merged (a digest may have a chunk file and up to ten
 * ".N.bad" files).  Nothing depends on digests being uniform: equal 8-byte prefixes only make
 * clusters longer.  *build_ms (may be NULL): the table build (its memsets and the kernel) by HIP
 * events, without the upload of the listing.  The handle keeps the stream for all its later
 * calls. */
int pbs_gc_begin(const uint8_t *store_digests, const uint8_t *flags, size_t m, pbs_gc **h, double *build_ms,
                 void *hip_stream);
/* L of the handle's table; 0 for a handle that is not alive. */
uint32_t pbs_gc_table_log2(const pbs_gc *h);
/* (be64(digest[0..8]) * 0x9E3779B97F4A7C15) >> (64 - table_log2); table_log2 in [1, 63]. */
uint64_t pbs_gc_home_slot(const uint8_t digest[32], uint32_t table_log2);

/* ---- 2. Phase 1 ---- */

/* One index file: entry i's digest is the 32 bytes at base_dev + i * stride (device memory on the
 * handle's device, never written).  stride >= 32 and a multiple of 8, base_dev 8-byte aligned,
 * n < 2^32 - 16: anything else is PBS_ERR_INVALID.  So a raw .didx image is marked in place with
 * base = image + 4096 + 8, stride 40, and a .fidx image with base = image + 4096, stride 32.
 * Every store entry whose 32 bytes equal an index entry's becomes "referenced".  An index entry
 * is MISSING when no store entry with flags == 0 carries its digest (cond_touch_chunk returning
 * false, datastore.rs:966).  *n_missing (may be NULL) counts missing entries, every occurrence;
 * their positions go to missing_pos (host) in ascending order, the first `cap` of them; cap == 0
 * with missing_pos NULL is legal.  A call that returns PBS_OK adds 1 to index_file_count and
 * index_bytes to index_data_bytes (:959-960).  *mark_ms (may be NULL): the kernels, by HIP
 * events -- no sort and no table work. */
int pbs_gc_mark_device(pbs_gc *h, const uint8_t *base_dev, size_t stride, size_t n, uint64_t index_bytes,
                       uint32_t *missing_pos, size_t cap, size_t *n_missing, double *mark_ms);
/* The same for a piece of an index: counts no file and no bytes.  A caller that splits one index
 * over several calls uses pbs_gc_mark_device (with the index's bytes) once and this for the rest. */
int pbs_gc_mark_piece(pbs_gc *h, const uint8_t *base_dev, size_t stride, size_t n, uint32_t *missing_pos,
                      size_t cap, size_t *n_missing, double *mark_ms);
/* A whole index image in host memory: recognised by its magic and checked as pbs_didx_parse /
 * pbs_fidx_parse check it (their codes; the marks and counters stay unchanged), copied to the
 * device and marked in place.  index_bytes is index_bytes(): the last end for .didx, `size` for
 * .fidx. */
int pbs_gc_mark_index_image(pbs_gc *h, const uint8_t *image, size_t len, uint32_t *missing_pos, size_t cap,
                            size_t *n_missing, double *mark_ms);

/* What phase 1 would have touched: touched[j] (host, m bytes) = 1 iff entry j is referenced, not
 * FOREIGN, and either flags[j] == 0 or it is BAD and NO flags == 0 entry carries the same digest
 * (the reference touches "<digest>.{0..9}.bad" only when the chunk itself is absent).
 * *n_touched (may be NULL): the ones. */
int pbs_gc_touched(pbs_gc *h, uint8_t *touched, size_t *n_touched);

/* ---- 3. Phase 2 ---- */

/* sweep_unused_chunks clause by clause over sizes[j] / atimes[j] (host, m each; st_size and
 * st_atime of entry j, sizes[j] == PBS_GC_VANISHED for an entry that could not be stat'ed or is
 * no regular file).  min_atime = min(phase1_start - 86400, oldest_writer) - 300; oldest_writer
 * > phase1_start is PBS_ERR_INVALID (the reference derives it as unwrap_or(phase1_start)).
 *  - VANISHED: counted nowhere, KEEP;
 *  - touched (pbs_gc_touched): disk class whatever atimes[j] says (its atime would be "now");
 *  - atime < min_atime: REMOVE; removed_bad (BAD) or removed_chunks +1, removed_bytes += size;
 *  - atime < oldest_writer: PENDING; still_bad (BAD) or pending_chunks +1, pending_bytes += size;
 *  - else disk class, KEEP: disk_chunks +1 unless BAD, disk_bytes += size.
 * still_bad is not counted in the disk class, as in the reference.  *status: these nine fields
 * plus index_file_count / index_data_bytes as the marks so far left them.  May be called more
 * than once on a handle; marks persist until pbs_gc_end.  actions (host, m bytes) and status
 * may each be NULL. */
int pbs_gc_sweep(pbs_gc *h, const uint64_t *sizes, const int64_t *atimes, int64_t phase1_start,
                 int64_t oldest_writer, uint8_t *actions, pbs_gc_status *status, double *sweep_ms);

/* Frees the handle and its device memory (NULL or a dead handle: nothing). */
void pbs_gc_end(pbs_gc *h);
/* Frees the idle per-call work areas of this header; legal with no handle alive. */
void pbs_gc_release(void);

/* ---- 4. Host mirror ---- */

/* The same calls on the host (every pointer host memory, no device): what the GPU is compared
 * against, and the library's GC where there is no device.  Same arguments, same codes, the
 * alignment rules included. */
typedef struct pbs_gc_host pbs_gc_host;
int pbs_gc_begin_host(const uint8_t *store_digests, const uint8_t *flags, size_t m, pbs_gc_host **h,
                      double *build_ms);
int pbs_gc_mark_host(pbs_gc_host *h, const uint8_t *base, size_t stride, size_t n, uint64_t index_bytes,
                     uint32_t *missing_pos, size_t cap, size_t *n_missing, double *mark_ms);
int pbs_gc_mark_piece_host(pbs_gc_host *h, const uint8_t *base, size_t stride, size_t n, uint32_t *missing_pos,
                           size_t cap, size_t *n_missing, double *mark_ms);
int pbs_gc_mark_index_image_host(pbs_gc_host *h, const uint8_t *image, size_t len, uint32_t *missing_pos,
                                 size_t cap, size_t *n_missing, double *mark_ms);
int pbs_gc_touched_host(pbs_gc_host *h, uint8_t *touched, size_t *n_touched);
int pbs_gc_sweep_host(pbs_gc_host *h, const uint64_t *sizes, const int64_t *atimes, int64_t phase1_start,
                      int64_t oldest_writer, uint8_t *actions, pbs_gc_status *status, double *sweep_ms);
void pbs_gc_end_host(pbs_gc_host *h);

#ifdef __cplusplus
}
#endif

#endif /* PBS_GC_H */
