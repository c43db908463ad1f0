// What the device side (pbs_verify.hip) and the host mirror (pbs_verify_host.cpp) of
// include/pbs_verify.h share: the argument rules, the bookkeeping of one index (what is planned,
// what was submitted, the counters), the accounting of one submitted blob, the batches of the
// whole-index call and the manifest's check of an index image.  Plain C++, no device code.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cstring>
#include <vector>

#include "gc_common.h"
#include "pbs_blob.h"
#include "pbs_chunker.h"
#include "pbs_digest.h"
#include "pbs_verify.h"

namespace pbs {
namespace verify {

using gc::kGcMaxEntries;

// ENCRYPTED_BLOB_MAGIC_1_0 / ENCR_COMPR_BLOB_MAGIC_1_0 (pbs-datastore/src/file_formats.rs:15, :18),
// as little-endian 64-bit words
constexpr uint64_t kEncMagicLe = 0xF04C2D22BE85677Bull;      // 123 103 133 190 34 45 76 240
constexpr uint64_t kEncComprMagicLe = 0x0BD8BF0BBF1B59E6ull;  // 230 89 27 191 11 191 216 11

inline bool mode_valid(int index_mode) {
    return index_mode == PBS_VERIFY_MODE_NONE || index_mode == PBS_VERIFY_MODE_ENCRYPT;
}

// the rules of pbs_verify_plan's arguments
inline bool plan_args_valid(const uint8_t* digests, const uint64_t* sizes, size_t n, int index_mode,
                            const uint32_t* todo_store, const uint32_t* todo_entry, size_t cap, const size_t* n_todo) {
    if (n >= kGcMaxEntries || (n && (!digests || !sizes)) || !mode_valid(index_mode) || !n_todo) return false;
    if (cap && (!todo_store || !todo_entry)) return false;
    return true;
}

// The open index of a handle: the plan and what the submits have made of it so far.
struct IndexRun {
    bool open = false;
    int mode = PBS_VERIFY_MODE_NONE;
    size_t n = 0, done = 0;                     // entries; plan items submitted
    std::vector<uint32_t> todo_store, todo_entry;
    std::vector<uint8_t> todo_digests;          // 32 per plan item: the digest of todo_entry[t]
    std::vector<uint64_t> todo_sizes;           // sizes[todo_entry[t]]
    std::vector<uint32_t> missing, corrupt;     // index positions; store positions, both ascending
    pbs_verify_result res;

    void clear() {
        open = false;
        n = done = 0;
        todo_store.clear();
        todo_entry.clear();
        todo_digests.clear();
        todo_sizes.clear();
        missing.clear();
        corrupt.clear();
        std::memset(&res, 0, sizeof(res));
    }
    // after the lists are in: the per-item digests and sizes
    void gather(const uint8_t* digests, const uint64_t* sizes) {
        const size_t k = todo_entry.size();
        todo_digests.resize(32 * k);
        todo_sizes.resize(k);
        for (size_t t = 0; t < k; ++t) {
            std::memcpy(&todo_digests[32 * t], digests + 32 * (size_t)todo_entry[t], 32);
            todo_sizes[t] = sizes[todo_entry[t]];
        }
    }
    size_t remaining() const { return todo_store.size() - done; }
};

// the rules of pbs_verify_submit's arguments
inline bool submit_args_valid(const IndexRun& run, const void* blobs, const uint64_t* blob_offsets, size_t k) {
    if (!run.open || k > run.remaining()) return false;
    if (k == 0) return true;
    if (!blob_offsets) return false;
    for (size_t t = 0; t < k; ++t)
        if (blob_offsets[t] > blob_offsets[t + 1]) return false;
    return blobs || blob_offsets[k] == blob_offsets[0];
}

inline bool loaded(uint8_t status) {
    return status != PBS_VERIFY_ST_LOAD_FAILED && status != PBS_BLOB_ST_TOO_SMALL && status != PBS_BLOB_ST_BAD_MAGIC &&
           status != PBS_BLOB_ST_BAD_CRC;
}

// One submitted blob's verdict into the run: plan item run.done, which it consumes.  Returns the
// chunk's new state.
inline uint8_t account(IndexRun& run, uint8_t kind, uint8_t status, uint64_t raw_len) {
    const size_t t = run.done++;
    pbs_verify_result& r = run.res;
    if (loaded(status)) {
        r.loaded += 1;
        r.read_bytes += raw_len;
        r.decoded_bytes += run.todo_sizes[t];
        const bool enc = kind == PBS_BLOB_KIND_ENCRYPTED || kind == PBS_BLOB_KIND_ENCR_COMPR;
        if (enc != (run.mode == PBS_VERIFY_MODE_ENCRYPT)) r.mode_mismatch += 1;
    }
    if (status == PBS_BLOB_ST_OK) {
        r.newly_verified += 1;
        return PBS_VERIFY_VERIFIED;
    }
    r.newly_corrupt += 1;
    run.corrupt.push_back(run.todo_store[t]);
    return PBS_VERIFY_CORRUPT;
}

// pbs_verify_finish's outputs once the count of failing occurrences is known
inline void close_run(IndexRun& run, uint64_t failing_occurrences, pbs_verify_result* res, uint32_t* corrupt_store,
                      size_t ccap, size_t* n_corrupt, uint32_t* missing_pos, size_t mcap, size_t* n_missing) {
    run.res.errors = failing_occurrences + run.res.mode_mismatch;
    run.res.ok = run.res.errors == 0;
    run.res.index_check = PBS_VERIFY_INDEX_OK;
    if (res) *res = run.res;
    for (size_t c = 0; c < run.corrupt.size() && c < ccap; ++c) corrupt_store[c] = run.corrupt[c];
    for (size_t c = 0; c < run.missing.size() && c < mcap; ++c) missing_pos[c] = run.missing[c];
    if (n_corrupt) *n_corrupt = run.corrupt.size();
    if (n_missing) *n_missing = run.missing.size();
    run.clear();
}

inline bool finish_args_valid(const IndexRun& run, const uint32_t* corrupt_store, size_t ccap, const uint32_t* missing_pos,
                              size_t mcap) {
    return run.open && run.remaining() == 0 && (!ccap || corrupt_store) && (!mcap || missing_pos);
}

// The manifest's check of an index image (verify.rs:282-289, :304-311) after gc::index_layout
// has accepted it: PBS_VERIFY_INDEX_*.
inline uint32_t index_check(const uint8_t* image, const gc::IndexLayout& lo, const uint64_t* info_size,
                            const uint8_t* info_csum) {
    if (info_size && lo.index_bytes != *info_size) return PBS_VERIFY_INDEX_WRONG_SIZE;
    if (info_csum) {
        // compute_csum: SHA-256 over the entries as they stand in the file (end || digest, or digests)
        uint8_t c[32];
        const size_t entry = lo.stride == 40 ? 40 : 32;
        pbs_sha256(image + 4096, lo.n * entry, c);
        if (std::memcmp(c, info_csum, 32) != 0) return PBS_VERIFY_INDEX_WRONG_CSUM;
    }
    return PBS_VERIFY_INDEX_OK;
}

// entry i's digest and chunk_info(i).size() of an accepted image, as pbs_verify_plan takes them
inline void index_entries(const uint8_t* image, const gc::IndexLayout& lo, std::vector<uint8_t>& digests,
                          std::vector<uint64_t>& sizes) {
    digests.resize(32 * lo.n);
    sizes.resize(lo.n);
    if (lo.stride == 40) {
        uint64_t prev = 0;
        for (size_t i = 0; i < lo.n; ++i) {
            const uint8_t* e = image + 4096 + 40 * i;
            const uint64_t end = gc::get_le64(e);
            sizes[i] = end - prev;
            prev = end;
            std::memcpy(&digests[32 * i], e + 8, 32);
        }
    } else {
        const uint64_t cs = gc::get_le64(image + 72);
        if (lo.n) std::memcpy(digests.data(), image + 4096, 32 * lo.n);
        for (size_t i = 0; i < lo.n; ++i) {  // chunk_info: the last chunk is clipped to `size`
            const uint64_t start = (uint64_t)i * cs;
            sizes[i] = lo.index_bytes - start < cs ? lo.index_bytes - start : cs;
        }
    }
}

// pbs_verify_host.cpp: the host mirror's verdict on one blob image (p may be NULL with len == 0)
// with no config, the digest `want` and a slot of exactly `size` bytes -- what
// pbs_blob_decode_inflate_device reports for it (an encrypted blob that loads: NO_CONFIG).
// *kind: PBS_BLOB_KIND_*.  Throws std::bad_alloc when there is no memory for the slot.  Shared
// with the sync job's mirror (pbs_sync_host.cpp).
uint8_t host_blob_verdict(const uint8_t* p, size_t len, const uint8_t* want, uint64_t size, uint8_t* kind);
// The same verdict with the stored CRC not judged and the payload's CRC in *crc (0 where from_raw
// fails): the backup session's upload (pbs_backup_host.cpp).
uint8_t host_blob_verdict_upload(const uint8_t* p, size_t len, const uint8_t* want, uint64_t size, uint8_t* kind,
                                 uint32_t* crc);
// from_raw + verify_crc alone (an encrypted blob that loads: NO_CONFIG): add_blob of the backup session
uint8_t host_blob_load(const uint8_t* p, size_t len, uint8_t* kind);

// The next batch of the whole-index call: plan items [t0, t1), t1 > t0, such that the blobs plus
// the output slots of the unencrypted ones stay at or below `budget` (0: no bound) -- but one
// blob always goes.  blob_len(t) and enc[t] describe plan item t.
template <class LenOf>
inline size_t batch_end(const IndexRun& run, size_t t0, size_t budget, const uint8_t* enc, LenOf blob_len) {
    const size_t k = run.todo_store.size();
    uint64_t used = 0;
    size_t t = t0;
    while (t < k) {
        const uint64_t need = blob_len(t) + (enc[t] ? 0 : run.todo_sizes[t]);
        if (budget && t > t0 && (need > budget || used > budget - need)) break;
        used += need;
        ++t;
    }
    return t;
}

}  // namespace verify
}  // namespace pbs
