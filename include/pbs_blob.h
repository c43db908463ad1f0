/*
 * pbs_blob.h -- C ABI of the per-chunk blob CRC stage (SURVEY.md section 8(f) rank 4:
 * the client-side per-chunk work after the digest).
 *
 * Reference interfaces replaced:
 *  - `DataBlob::compute_crc` (pbs-datastore/src/data_blob.rs:70-75):
 *    crc32fast::Hasher over the blob payload -- the chunk bytes for an uncompressed blob,
 *    set by `DataBlob::encode` (data_blob.rs:87-179; set_crc :64-67) and checked by
 *    `DataBlob::verify_crc` (:78-84) on every load/verify.  crc32fast (Cargo.toml:111,
 *    "1") computes CRC-32/ISO-HDLC: reflected polynomial 0xEDB88320, init and final
 *    XOR 0xFFFFFFFF -- the same function as zlib's crc32.
 *  - the uncompressed blob layout (pbs-datastore/src/file_formats.rs:9 and :36-45):
 *    magic UNCOMPRESSED_BLOB_MAGIC_1_0 (8 bytes) || crc (u32 LE) || data.
 *
 * Chunk i of a stream is [bounds[i], bounds[i+1]) in absolute stream offsets, as in
 * pbs_digest.h.
 */
#ifndef PBS_BLOB_H
#define PBS_BLOB_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PBS_BLOB_HEADER_SIZE 12 /* DataBlobHeader: magic[8] + crc[4] */

/* CRC-32 of every chunk on the GPU.  `dev_data` (device) holds stream bytes
 * [base, base + data_len); `bounds` (host, n + 1 ascending absolute offsets); writes n
 * CRCs to host `crcs` (chunk order).  Synchronous.  Returns PBS_OK or PBS_ERR_*. */
int pbs_crc32_chunks_device(const uint8_t *dev_data, size_t data_len, uint64_t base,
                            const uint64_t *bounds, size_t n, uint32_t *crcs, void *hip_stream);

/* Device-only, asynchronous form: `bounds_dev` (n + 1 offsets), `order_dev` (NULL or a
 * permutation of 0..n-1; workgroup k takes chunk order_dev[k] -- longest first balances
 * the tail), `crcs_dev` (n u32) are device memory. */
int pbs_crc32_chunks_async(const uint8_t *dev_data, size_t data_len, uint64_t base,
                           const uint64_t *bounds_dev, const uint32_t *order_dev, size_t n,
                           uint32_t *crcs_dev, void *hip_stream);

/* Host CRC-32 (crc32fast::Hasher::update/finalize): continue `crc` (0 to start) over
 * `data`. */
uint32_t pbs_crc32(uint32_t crc, const uint8_t *data, size_t len);

/* Uncompressed DataBlob image of `data` with its precomputed CRC (from
 * pbs_crc32_chunks_*): magic || crc LE || data into `out` (cap >= len + 12).  Returns
 * the bytes written (len + 12) or 0 if `cap` is too small or len exceeds MAX_BLOB_SIZE
 * (128 MiB, data_blob.rs:13 / :92). */
size_t pbs_blob_encode_uncompressed(const uint8_t *data, size_t len, uint32_t crc, uint8_t *out,
                                    size_t cap);

/* DataBlob images of every chunk on the GPU (`DataBlob::encode(data, None, compress)`,
 * data_blob.rs:87-176, unencrypted path; the encrypted one is at the end of this file).  compress != 0: each chunk is compressed into a
 * zstd frame (64 KiB blocks: RLE, compressed -- Huffman, raw or RLE literals; sequences
 * with repeat offsets and predefined, RLE or own FSE tables -- or raw; the match window
 * reaches 16 KiB before each 8 KiB sub-block; decodable by any zstd decoder, the reference's
 * `zstd::stream::decode_all` :214 included -- but not byte-identical to libzstd level 1,
 * which is what the reference writes: "parity unpinned"); the blob
 * is {COMPRESSED_BLOB_MAGIC_1_0, CRC, frame} when the frame is shorter than the chunk
 * (:153), else {UNCOMPRESSED_BLOB_MAGIC_1_0, CRC, chunk}.  compress == 0: every blob
 * uncompressed.  CRC = crc32fast over the payload (compute_crc, :70-75).
 * `dev_data` (device) holds stream bytes [base, base + data_len); `bounds` (host, n + 1
 * ascending absolute offsets; every chunk <= 128 MiB, MAX_BLOB_SIZE :13/:92).  The blobs
 * are written back to back into `blobs_dev` (device, blobs_cap >= pbs_blob_stream_bound);
 * blob i is [blob_offsets[i], blob_offsets[i+1]) (host, n + 1); `crcs` (host, n) and
 * `compressed` (host, n: 1 = zstd) may be NULL.  Needs ~ (bytes of the chunks) of device
 * scratch, kept between calls until pbs_blob_encode_release.  Synchronous.  C ABI of include/pbs_chunker.h's codes. */
typedef struct {
    double total_ms;    /* call entry .. outputs on the host */
    double compress_ms; /* block compression + frame sizes + offset scans (HIP events) */
    double assemble_ms; /* blocks / chunk bytes into the blob images */
    double crc_ms;      /* payload CRCs + headers */
    uint64_t bytes_in, bytes_out, blocks, compressed_chunks;
} pbs_blob_encode_timing;
int pbs_blob_encode_chunks_device(const uint8_t *dev_data, size_t data_len, uint64_t base,
                                  const uint64_t *bounds, size_t n, int compress, uint8_t *blobs_dev,
                                  size_t blobs_cap, uint64_t *blob_offsets, uint32_t *crcs,
                                  uint8_t *compressed, pbs_blob_encode_timing *timing,
                                  void *hip_stream);
/* The same for chunks given as spans: chunk i = [spans[2i], spans[2i+1]) (host, absolute
 * offsets in any order, gaps allowed -- e.g. the new chunks of an upload stream). */
int pbs_blob_encode_spans_device(const uint8_t *dev_data, size_t data_len, uint64_t base,
                                 const uint64_t *spans, size_t n, int compress, uint8_t *blobs_dev,
                                 size_t blobs_cap, uint64_t *blob_offsets, uint32_t *crcs,
                                 uint8_t *compressed, pbs_blob_encode_timing *timing,
                                 void *hip_stream);
/* Frees the device scratch pbs_blob_encode_chunks_device keeps between calls. */
void pbs_blob_encode_release(void);
/* 12 n + (bounds[n] - bounds[0]): the largest blob stream of n chunks. */
size_t pbs_blob_stream_bound(const uint64_t *bounds, size_t n);
/* Largest zstd frame this encoder writes for `len` bytes (header + raw blocks). */
size_t pbs_zstd_frame_bound(size_t len);

/* ---- Encrypted blobs: the `Some(config)` half of DataBlob::encode (data_blob.rs:107-131) ----
 *
 * Blob i is magic[8] || crc LE[4] || iv[16] || tag[16] || ciphertext
 * (EncryptedDataBlobHeader, file_formats.rs:47-58): AES-256-GCM with a 16-byte IV and empty
 * AAD under the config's key; the plaintext is the zstd frame (ENCR_COMPR_BLOB_MAGIC_1_0)
 * when compress != 0 and the frame is shorter than the chunk (data_blob.rs:98-105), else the
 * chunk bytes (ENCRYPTED_BLOB_MAGIC_1_0); the CRC covers the ciphertext only. */
#define PBS_BLOB_ENC_HEADER_SIZE 44 /* EncryptedDataBlobHeader: magic[8] crc[4] iv[16] tag[16] */
#define PBS_GCM_SEGMENT_BYTES 65536 /* payload bytes one workgroup encrypts and hashes */
#define PBS_ERR_ARG PBS_ERR_INVALID /* bad argument (pbs_chunker.h's code, -6) */

/* `CryptConfig::new(enc_key)` (pbs-tools/src/crypt_config.rs:42-61): derives
 * id_key = PBKDF2-HMAC-SHA256(enc_key, "_id_key", 10 rounds, 32 bytes), the 15 AES-256 round
 * keys, H = AES_K(0^128) and the per-key GHASH tables.  The handle keeps no copy of enc_key;
 * pbs_crypt_config_free zeroes everything derived from it (host and device copies) before
 * the memory is released.  No key byte appears in any error text.  A handle may be used by
 * several threads and devices at once; free it when no call is using it. */
typedef struct pbs_crypt_config pbs_crypt_config;
int pbs_crypt_config_new(const uint8_t enc_key[32], pbs_crypt_config **out);
/* The 32-byte id_key (`CryptConfig::compute_digest` appends it to every chunk: pass it as
 * the digest `key` of pbs_digest.h).  Valid until the handle is freed. */
const uint8_t *pbs_crypt_config_id_key(const pbs_crypt_config *cfg);
void pbs_crypt_config_free(pbs_crypt_config *cfg);

/* AES-256-GCM of one buffer on the host with the same AES / GF(2^128) code the kernels use
 * (`Crypter::new(aes_256_gcm, Encrypt, key, Some(iv16))`, empty AAD): `out` (len bytes, may
 * alias `data`) and the 16-byte `tag`.  For tests and small blobs; not a fast path. */
int pbs_aes256gcm_encrypt_host(const pbs_crypt_config *cfg, const uint8_t iv[16], const uint8_t *data,
                               size_t len, uint8_t *out, uint8_t tag[16]);

/* pbs_blob_encode_{spans,chunks}_device with encryption.  `ivs`: NULL (the product mode: the
 * library draws 16 fresh bytes per blob from getrandom(2), as data_blob.rs:113 does) or 16 n
 * host bytes, IV i for blob i -- for reproducible tests only: REUSING AN IV UNDER ONE KEY
 * BREAKS GCM (it reveals the XOR of the plaintexts and lets tags be forged).
 * `cfg` NULL: PBS_ERR_ARG.  blobs_cap below pbs_blob_stream_bound_encrypted (44 n + the
 * chunks' bytes): PBS_ERR_CAPACITY before anything is written.  `timing->base` as in the
 * unencrypted call (crc_ms: the ciphertext CRCs + headers). */
typedef struct {
    pbs_blob_encode_timing base;
    double encrypt_ms;     /* IV/J0 setup, CTR + GHASH in place, tags (HIP events) */
    uint64_t gcm_segments; /* PBS_GCM_SEGMENT_BYTES pieces encrypted */
} pbs_blob_encode_timing_crypt;
int pbs_blob_encode_chunks_encrypted_device(const uint8_t *dev_data, size_t data_len, uint64_t base,
                                            const uint64_t *bounds, size_t n, int compress,
                                            const pbs_crypt_config *cfg, const uint8_t *ivs,
                                            uint8_t *blobs_dev, size_t blobs_cap, uint64_t *blob_offsets,
                                            uint32_t *crcs, uint8_t *compressed,
                                            pbs_blob_encode_timing_crypt *timing, void *hip_stream);
int pbs_blob_encode_spans_encrypted_device(const uint8_t *dev_data, size_t data_len, uint64_t base,
                                           const uint64_t *spans, size_t n, int compress,
                                           const pbs_crypt_config *cfg, const uint8_t *ivs,
                                           uint8_t *blobs_dev, size_t blobs_cap, uint64_t *blob_offsets,
                                           uint32_t *crcs, uint8_t *compressed,
                                           pbs_blob_encode_timing_crypt *timing, void *hip_stream);
/* 44 n + (bounds[n] - bounds[0]): the largest encrypted blob stream of n chunks. */
size_t pbs_blob_stream_bound_encrypted(const uint64_t *bounds, size_t n);

/* ---- Reading blobs: DataBlob::load_from_reader (from_raw + verify_crc, data_blob.rs:256-300,
 * :78-84), DataBlob::decode (:197-253), DataBlob::verify_unencrypted (:310-333) and
 * CryptConfig::decode_uncompressed_chunk / decode_compressed_chunk (:409-480) -- everything
 * but the zstd inflate.
 *
 * Blob i is [blob_offsets[i], blob_offsets[i+1]) of `blobs_dev` (device; offsets on the host,
 * n + 1 ascending values at any alignment, n < 2^32); the four kinds may be mixed freely and
 * the input is never written.  The payloads are written back to back into `out_dev`
 * (device): payload i is [out_offsets[i], out_offsets[i+1]) (host, n + 1) -- the chunk bytes
 * for kinds 0 and 2, the zstd frame (decrypted for kind 3) for kinds 1 and 3.  A blob that
 * fails before its payload length is known (TOO_SMALL, BAD_MAGIC) has a zero-length payload.
 * `kinds[i]`: PBS_BLOB_KIND_*, or PBS_BLOB_KIND_NONE where the magic is absent or unknown.
 *
 * `status[i]` is the first check that fails, in the reference's order (PBS_BLOB_ST_*); a bad
 * blob never fails the call -- it returns PBS_OK -- and never changes another blob's output.
 * `cfg` may be NULL: encrypted blobs then get NO_CONFIG (after their CRC check, as load
 * comes before decode).  `expect_digests` (NULL or 32 n host bytes) is checked for kinds 0
 * and 2 only -- SHA-256(payload), for kind 2 SHA-256(payload || id_key) -- and `expect_sizes`
 * (NULL or n host values) for kind 0 only (verify_unencrypted returns Ok for encrypted blobs).
 * FOR KINDS 1 AND 3 THE DIGEST AND THE SIZE BELONG TO THE INFLATED DATA: the call stops at
 * OK after CRC and tag and hands the frame back; pbs_blob_decode_inflate_device (below)
 * inflates it into the caller's slot and checks digest and size there.
 *
 * No unauthenticated plaintext is released: the output bytes of every encrypted blob whose
 * status is not OK are zero when the call returns.  (An unencrypted blob that fails keeps
 * its payload bytes in the output; its status says what is wrong with them.)  No key byte
 * appears in any error text.
 *
 * `out_cap` below pbs_blob_decode_bound: PBS_ERR_CAPACITY before anything is written.
 * Device scratch comes from a work area kept between calls until pbs_blob_encode_release.
 * All launches go on `hip_stream`; synchronous. */
#define PBS_BLOB_KIND_UNCOMPRESSED 0
#define PBS_BLOB_KIND_COMPRESSED 1
#define PBS_BLOB_KIND_ENCRYPTED 2
#define PBS_BLOB_KIND_ENCR_COMPR 3
#define PBS_BLOB_KIND_NONE 255

#define PBS_BLOB_ST_OK 0
#define PBS_BLOB_ST_TOO_SMALL 1  /* under 12 bytes, or an encrypted magic under 44 (from_raw :269-281) */
#define PBS_BLOB_ST_BAD_MAGIC 2  /* :287-289 */
#define PBS_BLOB_ST_BAD_CRC 3    /* stored CRC != CRC-32 of everything after the header (verify_crc) */
#define PBS_BLOB_ST_NO_CONFIG 4  /* encrypted kind and cfg == NULL (:247-249) */
#define PBS_BLOB_ST_BAD_TAG 5    /* GCM tag over the ciphertext != header tag (decrypt_aead) */
#define PBS_BLOB_ST_BAD_DIGEST 6 /* kinds 0 and 2 (verify_digest :335-349) */
#define PBS_BLOB_ST_BAD_SIZE 7   /* kind 0 (:324-331) */

#define PBS_ERR_TAG (-7) /* pbs_aes256gcm_decrypt_host: the tag does not match; `out` is zeroed */

typedef struct {
    double total_ms;    /* call entry .. outputs on the host */
    double classify_ms; /* size / magic checks, payload lengths, offset scan (HIP events) */
    double crc_ms;      /* payload CRCs */
    double decrypt_ms;  /* J0 setup, GHASH + CTR out of place, tag comparison; the copies of the
                           unencrypted payloads */
    double digest_ms;   /* SHA-256 lanes, verdicts, wipe of failed encrypted payloads */
    uint64_t bytes_in, bytes_out;
    uint64_t gcm_segments; /* PBS_GCM_SEGMENT_BYTES pieces opened */
    uint64_t failed;       /* blobs whose status is not OK */
} pbs_blob_decode_timing;

int pbs_blob_decode_device(const uint8_t *blobs_dev, const uint64_t *blob_offsets, size_t n,
                           const pbs_crypt_config *cfg, const uint8_t *expect_digests,
                           const uint64_t *expect_sizes, uint8_t *out_dev, size_t out_cap,
                           uint64_t *out_offsets, uint8_t *kinds, uint8_t *status,
                           pbs_blob_decode_timing *timing, void *hip_stream);
/* The most payload bytes n blobs at these offsets can hold: every blob's length less the
 * 12-byte header -- (blob_offsets[n] - blob_offsets[0]) - 12 n when no blob is shorter than
 * a header (a shorter one counts as empty). */
size_t pbs_blob_decode_bound(const uint64_t *blob_offsets, size_t n);

/* Opens what pbs_aes256gcm_encrypt_host seals: the tag over `data` (len ciphertext bytes) is
 * computed and compared first; PBS_OK and the plaintext in `out` (may alias `data`), or
 * PBS_ERR_TAG and `out` zeroed. */
int pbs_aes256gcm_decrypt_host(const pbs_crypt_config *cfg, const uint8_t iv[16], const uint8_t *data,
                               size_t len, const uint8_t tag[16], uint8_t *out);

/* pbs_blob_decode_device for one blob on the host, with the same kinds and status codes (for
 * small blobs and tests; not a fast path).  `expect_digest`: NULL or 32 bytes; `expect_size`:
 * NULL or one value.  The payload goes to `out` (cap >= len - header, else PBS_ERR_CAPACITY)
 * and its length to *out_len; a failed encrypted blob leaves zeros there. */
int pbs_blob_decode_host(const uint8_t *blob, size_t len, const pbs_crypt_config *cfg,
                         const uint8_t *expect_digest, const uint64_t *expect_size, uint8_t *out,
                         size_t cap, size_t *out_len, uint8_t *kind, uint8_t *status);

/* ---- Inflating zstd frames: `zstd::stream::decode_all` (data_blob.rs:214, :238) ----
 *
 * A decoder of the format (RFC 8878), not the inverse of this library's encoder: it reads
 * what libzstd writes at any level -- frames without a content size and with a window
 * descriptor (`copy_encode`, data_blob.rs:151), 128 KiB blocks, raw / RLE / compressed blocks,
 * raw, RLE, Huffman (1 and 4 streams, direct and FSE-described weights) and treeless
 * literals, predefined, RLE, FSE-described and repeated sequence tables.
 *
 * Per frame: PBS_ZST_OK; BAD_FRAME (corrupt or truncated, bytes left after the last block and
 * its optional checksum field, a block or literals size above 128 KiB or above the window,
 * an offset reaching before the frame's first byte); TOO_LARGE (the content does not fit the
 * slot -- also a content size in the header above the slot, found before anything is
 * written); UNSUPPORTED (dictionary id != 0, window above 128 MiB, a skippable frame, a
 * second frame after the first).  A bad frame is data: the call returns PBS_OK, and no
 * frame's outcome depends on another's.
 *
 * A Content_Checksum field is CONSUMED AND NOT VERIFIED: in this system the chunk digest is
 * the integrity check, and the reference's writers do not set the flag.
 *
 * A frame is decoded block by block; a block is checked completely before its first byte is
 * written, so `out_len` is the content of the good blocks before the first bad one. */
#define PBS_ZST_OK 0
#define PBS_ZST_BAD_FRAME 1
#define PBS_ZST_TOO_LARGE 2
#define PBS_ZST_UNSUPPORTED 3
#define PBS_ZSTD_SIZE_UNKNOWN (~(uint64_t)0)

/* The serial host decoder over the same format code as the kernel (csrc/zstd_dec.h): the
 * mirror the GPU is compared against; not a fast path.  `out` holds `cap` bytes. */
int pbs_zstd_inflate_host(const uint8_t *frame, size_t len, uint8_t *out, size_t cap, size_t *out_len,
                          uint8_t *status);
/* The frame header's content size, or PBS_ZSTD_SIZE_UNKNOWN when it carries none.
 * PBS_ERR_ARG when [frame, frame + len) holds no readable zstd frame header. */
int pbs_zstd_frame_content_size(const uint8_t *frame, size_t len, uint64_t *size);

typedef struct {
    double total_ms;   /* call entry .. outputs on the host */
    double inflate_ms; /* the inflate launch (HIP events) */
    uint64_t bytes_in, bytes_out, frames;
    uint64_t failed;     /* frames whose status is not OK */
    uint64_t workgroups; /* workgroups launched: min(frames, CUs x the resident workgroups per CU) */
} pbs_zstd_inflate_timing;

/* n frames on the GPU, one workgroup per frame.  Frame i is [frame_offsets[i],
 * frame_offsets[i+1]) of `frames_dev` (device; offsets on the host, n + 1 ascending values
 * at any alignment) and is never written.  Its content goes to the caller's slot
 * [out_offsets[i], out_offsets[i+1]) of `out_dev` (host offsets, n + 1 ascending: the caller
 * sizes the slots, as libzstd's streaming frames carry no size and the index knows every
 * chunk's length); out_lens[i] (host, n) is what was produced.  Slot bytes past it, and
 * everything outside the slots, stay untouched.  status[i] (host, n): PBS_ZST_*.
 * Device scratch comes from a work area kept between calls until pbs_blob_encode_release;
 * all launches go on `hip_stream`; synchronous. */
int pbs_zstd_inflate_device(const uint8_t *frames_dev, const uint64_t *frame_offsets, size_t n,
                            uint8_t *out_dev, const uint64_t *out_offsets, uint64_t *out_lens,
                            uint8_t *status, pbs_zstd_inflate_timing *timing, void *hip_stream);

/* ---- The read path, finished: load, open, inflate and verify in one call ----
 *
 * pbs_blob_decode_device's inputs (blobs of mixed kinds, `cfg` or NULL, `expect_digests` NULL or
 * 32 n host bytes) plus `chunk_sizes` (n host values, required: the index knows every chunk's
 * length): blob i's chunk goes to the slot [out_offsets[i], out_offsets[i+1]) of `out_dev`,
 * out_offsets being the running sum of chunk_sizes (written by the call, n + 1 host values;
 * out_cap below their sum: PBS_ERR_CAPACITY before anything is written); out_lens[i] (host,
 * n) is what the slot holds.  Stages: classify / CRC / GCM open as in pbs_blob_decode_device
 * (packed into device scratch); kinds 0 and 2 copied, kinds 1 and 3 inflated into the slots;
 * SHA-256 over [slot, slot + out_lens) for ALL FOUR kinds (keyed with id_key for 2 and 3)
 * against expect_digests; verdict; wipe.
 *
 * status[i]: the first failing check in the reference's order -- load (size, magic, CRC),
 * decrypt (config, tag), decode_all (BAD_FRAME, UNSUPPORTED_FRAME), verify_digest, then the
 * length: with `sizes_exact` != 0 a length != chunk_sizes[i] is BAD_SIZE for kinds 0 and 1
 * (verify_unencrypted, data_blob.rs:324, checks both unencrypted magics and returns Ok for
 * encrypted ones).  Content that overflows its slot is BAD_DIGEST when digests are given (a
 * message of another length cannot have that digest, and the reference would fail there
 * first), else BAD_SIZE -- for every kind; the slot then holds the content's first bytes
 * (kinds 0 and 2) or the blocks that fitted (kinds 1 and 3).
 *
 * The whole slot of an encrypted blob whose status is not OK is zero when the call returns
 * (out_lens 0) -- a kind 3 that fails in the inflater or at the digest included.  An
 * unencrypted blob that fails keeps what was written.  Slot bytes past out_lens are not
 * written otherwise.  Synchronous; scratch from the decode work areas
 * (pbs_blob_encode_release). */
#define PBS_BLOB_ST_BAD_FRAME 8         /* kinds 1 and 3: PBS_ZST_BAD_FRAME (decode_all fails) */
#define PBS_BLOB_ST_UNSUPPORTED_FRAME 9 /* kinds 1 and 3: PBS_ZST_UNSUPPORTED */

typedef struct {
    pbs_blob_decode_timing base; /* digest_ms: digests of all kinds, verdicts, wipe */
    double inflate_ms;           /* slot copies + the inflate launch (HIP events) */
    uint64_t frames;             /* frames handed to the inflater */
} pbs_blob_decode_inflate_timing;

int pbs_blob_decode_inflate_device(const uint8_t *blobs_dev, const uint64_t *blob_offsets, size_t n,
                                   const pbs_crypt_config *cfg, const uint8_t *expect_digests,
                                   const uint64_t *chunk_sizes, int sizes_exact, uint8_t *out_dev,
                                   size_t out_cap, uint64_t *out_offsets, uint64_t *out_lens,
                                   uint8_t *kinds, uint8_t *status, pbs_blob_decode_inflate_timing *timing,
                                   void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* PBS_BLOB_H */
