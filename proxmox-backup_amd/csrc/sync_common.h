// What the device side (pbs_sync.hip) and the host mirror (pbs_sync_host.cpp) of
// include/pbs_sync.h share: the table's size at the begin and its growth before a plan, the
// argument rules, the bookkeeping of one index (the two lists, what was submitted, the counters)
// and the accounting of one submitted blob.  Plain C++, no device code.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cstring>
#include <vector>

#include "gc_common.h"
#include "pbs_blob.h"
#include "pbs_chunker.h"
#include "pbs_sync.h"

namespace pbs {
namespace sync {

using gc::kGcMaxEntries;

// pbs_sync_begin: the table of gc::table_log2_for, sized for the listing and the reserve
inline uint32_t begin_log2(uint64_t m, uint64_t reserve) { return gc::table_log2_for(m + reserve); }

// Before a plan of n entries over `count` entries: every index entry may append one, and the
// load must stay <= 1/2 through the whole claim kernel (that is what ends every probe walk).  A
// table that is too small is rebuilt a factor of two above what the plan needs, so a run of
// plans of similar size rebuilds at every doubling of the store and not at every plan.
inline uint32_t plan_log2(uint64_t count, uint64_t n, uint32_t log2) {
    if (2 * (count + n) <= (1ull << log2)) return log2;
    return gc::table_log2_for(count + n) + 1;
}

// the rules of pbs_sync_begin's arguments
inline bool begin_args_valid(const uint8_t* store_digests, size_t m, size_t reserve, const void* out) {
    if (!out || (m && !store_digests)) return false;
    return m < kGcMaxEntries && reserve < kGcMaxEntries && (uint64_t)m + reserve < kGcMaxEntries;
}

// the rules of the list outputs of a plan
inline bool lists_args_valid(const uint32_t* fetch_store, const uint32_t* fetch_entry, size_t fcap, const size_t* n_fetch,
                             const uint32_t* touch_store, size_t tcap, const size_t* n_touch) {
    if (!n_fetch || !n_touch) return false;
    if (fcap && (!fetch_store || !fetch_entry)) return false;
    return !tcap || touch_store;
}

// does a plan of n entries fit a handle of `count` entries?  (count + i must stay a table value)
inline bool entries_fit(uint64_t count, uint64_t n) { return n < kGcMaxEntries && count + n < kGcMaxEntries; }

// the rules of pbs_sync_plan's arguments on a handle of `count` entries
inline bool plan_args_valid(uint64_t count, const uint8_t* digests, const uint64_t* sizes, size_t n,
                            const uint32_t* fetch_store, const uint32_t* fetch_entry, size_t fcap, const size_t* n_fetch,
                            const uint32_t* touch_store, size_t tcap, const size_t* n_touch) {
    if (!entries_fit(count, n) || (n && (!digests || !sizes))) return false;
    return lists_args_valid(fetch_store, fetch_entry, fcap, n_fetch, touch_store, tcap, n_touch);
}

// The open index of a handle: the two lists and what the submits have made of the fetch list.
struct IndexRun {
    bool open = false;
    size_t n = 0, done = 0;  // entries; fetch items submitted
    std::vector<uint32_t> fetch_store, fetch_entry, touch_store;
    std::vector<uint8_t> fetch_digests;  // 32 per fetch item: the digest of fetch_entry[t]
    std::vector<uint64_t> fetch_sizes;   // sizes[fetch_entry[t]]
    pbs_sync_result res;

    void clear() {
        open = false;
        n = done = 0;
        fetch_store.clear();
        fetch_entry.clear();
        touch_store.clear();
        fetch_digests.clear();
        fetch_sizes.clear();
        std::memset(&res, 0, sizeof(res));
        res.first_failed = PBS_SYNC_NONE;
    }
    // after the lists are in: the per-item digests and sizes, and the plan's counters
    void start(const uint8_t* digests, const uint64_t* sizes, size_t entries, uint64_t appended) {
        const size_t k = fetch_entry.size();
        fetch_digests.resize(32 * k);
        fetch_sizes.resize(k);
        for (size_t t = 0; t < k; ++t) {
            std::memcpy(&fetch_digests[32 * t], digests + 32 * (size_t)fetch_entry[t], 32);
            fetch_sizes[t] = sizes[fetch_entry[t]];
        }
        open = true;
        n = entries;
        done = 0;
        res.entries = entries;
        res.fetch = k;
        res.exists = touch_store.size();
        res.dup = entries - k - touch_store.size();
        res.appended = appended;
    }
    size_t remaining() const { return fetch_store.size() - done; }
};

// the lists of an open index into the caller's arrays
inline void copy_lists(const IndexRun& run, uint32_t* fetch_store, uint32_t* fetch_entry, size_t fcap, size_t* n_fetch,
                       uint32_t* touch_store, size_t tcap, size_t* n_touch) {
    for (size_t t = 0; t < run.fetch_store.size() && t < fcap; ++t) {
        fetch_store[t] = run.fetch_store[t];
        fetch_entry[t] = run.fetch_entry[t];
    }
    for (size_t t = 0; t < run.touch_store.size() && t < tcap; ++t) touch_store[t] = run.touch_store[t];
    *n_fetch = run.fetch_store.size();
    *n_touch = run.touch_store.size();
}

// the rules of pbs_sync_submit's arguments
inline bool submit_args_valid(const IndexRun& run, const void* blobs, const uint64_t* blob_offsets, size_t k) {
    if (!run.open || k > run.remaining()) return false;
    if (k == 0) return true;
    if (!blob_offsets) return false;
    for (size_t t = 0; t < k; ++t)
        if (blob_offsets[t] > blob_offsets[t + 1]) return false;
    return blobs || blob_offsets[k] == blob_offsets[0];
}

// One submitted blob's verdict into the run: fetch item run.done, which it consumes.  Returns
// whether the entry becomes present (insert_chunk).
inline bool account(IndexRun& run, uint8_t status, uint64_t raw_len) {
    const size_t t = run.done++;
    pbs_sync_result& r = run.res;
    if (status == PBS_SYNC_ST_LOAD_FAILED) {
        r.load_failed += 1;
    } else {  // counted after read_raw_chunk, before the verdict (pull.rs:665-674)
        r.chunk_count += 1;
        r.bytes += raw_len;
        if (status == PBS_BLOB_ST_OK)
            r.inserted += 1;
        else
            r.failed += 1;
    }
    if (status != PBS_BLOB_ST_OK && r.first_failed == PBS_SYNC_NONE) r.first_failed = t;
    return status == PBS_BLOB_ST_OK;
}

inline void close_run(IndexRun& run, pbs_sync_result* res) {
    run.res.ok = run.res.failed == 0 && run.res.load_failed == 0;
    if (res) *res = run.res;
    run.clear();
}

}  // namespace sync
}  // namespace pbs
