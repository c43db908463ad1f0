/*
 * pbs_restore.h -- C ABI of the restore side of a dynamic-index (.didx) stream: the index
 * reader, the lookup of index digests in a store's digest list, a segment copy at memory
 * speed, and the call that puts the original bytes of an archive range into device memory,
 * every byte verified.
 *
 * Reference interfaces replaced:
 *  - `DynamicIndexReader` (pbs-datastore/src/dynamic_index.rs:82-275): new (:103-153),
 *    chunk_end, binary_search (:172-195), index_count / index_digest / index_bytes /
 *    compute_csum / chunk_info (:199-248), chunk_from_offset (:258-274);
 *  - `BufferedDynamicReader` (:544-673): read of a byte range through the index, with
 *    `CachedChunk::new`'s length check (:532-541);
 *  - `ReadChunk::read_chunk` (pbs-datastore/src/local_chunk_reader.rs:57-63,
 *    pbs-client/src/remote_chunk_reader.rs:77-90): verify_crc, then decode(cfg, Some(digest)).
 *
 * Conventions are those of pbs_blob.h: offset arrays on the host, byte buffers on the
 * device, every call synchronous on `hip_stream`, a `timing` struct that may be NULL, the
 * codes of pbs_chunker.h.
 */
#ifndef PBS_RESTORE_H
#define PBS_RESTORE_H

#include <stddef.h>
#include <stdint.h>

#include "pbs_blob.h"
#include "pbs_chunker.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- 1. Index reader (host) ---- */

/* Entries of a .didx image of `image_len` bytes: (image_len - 4096) / 40, or (size_t)-1 when
 * the image is shorter than the 4096-byte header or its body is no multiple of 40 bytes. */
size_t pbs_didx_count(size_t image_len);

/* Reads the image pbs_didx_build writes.  PBS_ERR_INVALID for an image shorter than the
 * header, a wrong magic or a ragged body (the three `bail!`s of DynamicIndexReader::new,
 * :117-133) and for chunk ends that decrease anywhere (chunk_info, :236-247, would underflow;
 * equal neighbours are a legal zero-length chunk); PBS_ERR_CAPACITY when the image holds more
 * than `cap` entries (*n is still set).  `uuid`, `ctime`, `header_csum` (the header's
 * index_csum field) and `computed_csum` (compute_csum, :219-230: SHA-256 over end_le || digest
 * of every entry, by pbs_sha256) may each be NULL; `ends` (cap values) and `digests` (32 cap
 * bytes) may be NULL when cap == 0.  The two checksums are the caller's to compare: the
 * reference does not compare them at open either.  `ctime` is the header's field (the
 * reference's reader overwrites its own with the time of opening). */
int pbs_didx_parse(const uint8_t *image, size_t len, uint8_t uuid[16], int64_t *ctime,
                   uint8_t header_csum[32], uint8_t computed_csum[32], uint64_t *ends,
                   uint8_t *digests, size_t cap, size_t *n);

/* chunk_from_offset (:258-274) over the reference's binary_search (:172-195): the entry that
 * holds archive byte `offset` and the byte's position inside it.  n == 0 or offset >=
 * ends[n-1]: PBS_ERR_INVALID.  `ends` ascending (pbs_didx_parse checks it); a zero-length
 * chunk holds no byte and is never returned. */
int pbs_didx_chunk_from_offset(const uint64_t *ends, size_t n, uint64_t offset, size_t *idx,
                               uint64_t *within);

/* ---- 2. Digest lookup with grouping ---- */

#define PBS_LOOKUP_MISSING 0xFFFFFFFFu

/* For each of the n 32-byte digests at `digests_dev`: store_pos[i] = the lowest position in
 * `store_dev` (m digests in any order, duplicates allowed) that holds the same digest, or
 * PBS_LOOKUP_MISSING; first[i] = the lowest j <= i with digest j == digest i, the entry's
 * representative.  *n_missing: entries without a store position; *n_unique: representatives
 * (entries with first[i] == i).  Both lists are radix-sorted by their 8-byte big-endian
 * prefix with the position as value (a stable sort: every run of equal prefixes lists its
 * members in ascending position), runs are resolved with full 32-byte comparisons -- a
 * prefix shared by different digests gives the right answer -- and the sorted store is
 * binary-searched.  All four pointers are device memory, the digest lists 16-byte aligned;
 * store_pos_dev and first_dev hold n u32 each; n, m < 2^32 - 16.  The counts may be NULL. */
int pbs_digest_lookup_device(const uint8_t *digests_dev, size_t n, const uint8_t *store_dev, size_t m,
                             uint32_t *store_pos_dev, uint32_t *first_dev, size_t *n_missing,
                             size_t *n_unique, void *hip_stream);
/* The same outputs by a plain sort on the host (every pointer host memory): the mirror the
 * GPU is compared against. */
int pbs_digest_lookup_host(const uint8_t *digests, size_t n, const uint8_t *store, size_t m,
                           uint32_t *store_pos, uint32_t *first, size_t *n_missing, size_t *n_unique);

/* ---- 3. Segment copy ---- */

/* Segment k copies lens[k] bytes from src_dev + src_off[k] to dst_dev + dst_off[k] (host
 * arrays of nseg values; device buffers): any alignment on both sides, any length, 0
 * included; many segments may share a source.  The destinations must be disjoint from each
 * other and from every source: an overlap is PBS_ERR_INVALID before anything is written.
 * No byte outside a destination segment is written and no byte outside a source segment is
 * read.  The caller guarantees that every segment lies inside its buffer. */
int pbs_copy_segments_device(const uint8_t *src_dev, uint8_t *dst_dev, const uint64_t *src_off,
                             const uint64_t *dst_off, const uint64_t *lens, size_t nseg,
                             void *hip_stream);

/* ---- 4. Restore ---- */

#define PBS_BLOB_ST_MISSING 10         /* no blob in the store carries the entry's digest */
#define PBS_BLOB_ST_NONE_REQUESTED 255 /* the entry lies outside the requested range */

typedef struct {
    double total_ms;   /* call entry .. outputs on the host */
    double lookup_ms;  /* digests to the device, lookup, positions back (HIP events) */
    double pack_ms;    /* the representatives' blobs into scratch, back to back */
    double decode_ms;  /* pbs_blob_decode_inflate_device over the packed blobs */
    double scatter_ms; /* chunks into their places of the output, zeros for failed entries */
    uint64_t entries;  /* index entries that cover the range */
    uint64_t unique;   /* of those, distinct digests that the store holds: blobs decoded */
    uint64_t missing;  /* covering entries without a store blob */
    uint64_t failed;   /* covering entries whose status is not OK (the missing included) */
    uint64_t blob_bytes, decoded_bytes, out_bytes;
    pbs_blob_decode_inflate_timing decode;
} pbs_restore_timing;

/* Archive bytes [offset, offset + len) of the stream that the index (`ends`, `digests`: n
 * entries, host, as pbs_didx_parse returns them) describes, into out_dev[0 .. len).  The
 * store: blob j is [store_offsets[j], store_offsets[j+1]) of `store_blobs_dev` (device; m + 1
 * ascending host offsets) and is filed under the digest store_digests[32 j ..] (host; any
 * order, duplicates allowed: the lowest position is read).  offset + len above ends[n-1], or
 * `ends` / `store_offsets` that decrease: PBS_ERR_INVALID.  len == 0: PBS_OK.
 *
 * The covering entries are [i0, i1], i0 = chunk_from_offset(offset) and i1 =
 * chunk_from_offset(offset + len - 1); zero-length entries between them are read and checked
 * like any other.  Every distinct digest among them is looked up (pbs_digest_lookup_device),
 * its blob copied into scratch (pbs_copy_segments_device), loaded, opened, inflated and
 * verified ONCE (pbs_blob_decode_inflate_device with the index's chunk lengths and digests,
 * sizes_exact; a chunk of another length is BAD_SIZE for every kind, as CachedChunk::new
 * checks every chunk -- a longer one too: a blob that fails the digest in its entry's slot
 * and whose entry is shorter than the index's longest chunk is decoded once more into a slot
 * of that length, and is BAD_SIZE when its digest verifies there, as read_chunk verifies the
 * whole chunk before its length is looked at), and copied to the place of every entry that names it, clipped to the
 * range (pbs_copy_segments_device).
 *
 * entry_status[i] (host, n): PBS_BLOB_ST_NONE_REQUESTED outside [i0, i1], else the status of
 * the entry's blob: PBS_BLOB_ST_MISSING or a PBS_BLOB_ST_* of pbs_blob.h.  A bad chunk is
 * data: the call returns PBS_OK, and the output bytes of every entry that is not OK are zero
 * when the call returns, for every kind -- a restore hands out no unverified byte.
 * `store_blobs_dev` is never written.
 *
 * Device scratch: the packed blobs of the range plus its distinct chunks, from a work area
 * kept between calls until pbs_restore_release (beside what the decode call keeps, freed by
 * pbs_blob_encode_release). */
int pbs_restore_range_device(const uint64_t *ends, const uint8_t *digests, size_t n,
                             const uint8_t *store_blobs_dev, const uint64_t *store_offsets,
                             const uint8_t *store_digests, size_t m, const pbs_crypt_config *cfg,
                             uint64_t offset, uint64_t len, uint8_t *out_dev, uint8_t *entry_status,
                             pbs_restore_timing *timing, void *hip_stream);

/* Frees the idle work areas of the calls of this header. */
void pbs_restore_release(void);

#ifdef __cplusplus
}
#endif

#endif /* PBS_RESTORE_H */
