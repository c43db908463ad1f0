// Host mirror of the sync job (include/pbs_sync.h, pbs_sync_*_host): the sequential rule of the
// header, entry by entry over a hash map from digest to lowest entry position, and a blob at a
// time through the verify mirror's verdict (pbs_verify_host.cpp: from_raw's checks, the CRC, the
// host inflater, pbs_sha256).  The table itself is not kept, only its L by the rules of
// sync_common.h, so the mirror and the device agree on it.  Plain C++: no device code, so the
// sanitizer program of tests/cpp/sync_sanitize.cpp builds it with the host compiler.  It is what
// the GPU is compared against, and sync where there is no device.
#include <stdint.h>

#include <chrono>
#include <cstring>
#include <exception>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "gc_common.h"
#include "live_handles.h"
#include "pbs_blob.h"
#include "pbs_chunker.h"
#include "pbs_sync.h"
#include "sync_common.h"
#include "verify_common.h"

using namespace pbs::gc;
using namespace pbs::sync;

struct pbs_sync_host {
    std::vector<uint8_t> digests, present, claimed;     // 32, 1 and 1 per entry
    std::unordered_map<std::string, uint32_t> lowest;   // digest -> the lowest entry position carrying it
    uint32_t log2 = 0;
    IndexRun run;
    size_t count() const { return present.size(); }
};

namespace {

using Clock = std::chrono::steady_clock;
inline double ms_since(Clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
}

using Handles = pbs::Live<pbs_sync_host>;

inline std::string key(const uint8_t* d) { return std::string(reinterpret_cast<const char*>(d), 32); }

// pbs_sync_plan after the argument checks; the lists stay in the run
int plan(pbs_sync_host* h, const uint8_t* digests, const uint64_t* sizes, size_t n, uint8_t* verdict) {
    IndexRun& run = h->run;
    try {
        run.clear();
        h->log2 = plan_log2(h->count(), n, h->log2);
        uint64_t appended = 0;
        for (size_t i = 0; i < n; ++i) {
            const uint8_t* d = digests + 32 * i;
            auto it = h->lowest.find(key(d));
            uint32_t c;
            if (it != h->lowest.end()) {
                c = it->second;
                if (h->claimed[c]) {  // filtered by downloaded_chunks (:619-627)
                    if (verdict) verdict[i] = PBS_SYNC_DUP;
                    continue;
                }
            } else {
                c = (uint32_t)h->count();
                h->digests.insert(h->digests.end(), d, d + 32);
                h->present.push_back(0);
                h->claimed.push_back(0);
                h->lowest.emplace(key(d), c);
                ++appended;
            }
            h->claimed[c] = 1;
            if (h->present[c]) {  // cond_touch_chunk (:657-663)
                if (verdict) verdict[i] = PBS_SYNC_EXISTS;
                run.touch_store.push_back(c);
            } else {
                if (verdict) verdict[i] = PBS_SYNC_FETCH;
                run.fetch_store.push_back(c);
                run.fetch_entry.push_back((uint32_t)i);
            }
        }
        run.start(digests, sizes, n, appended);
    } catch (const std::bad_alloc&) {  // (claims and appended entries stay, as after an abort)
        run.clear();
        return PBS_ERR_NOMEM;
    }
    return PBS_OK;
}

}  // namespace

extern "C" int pbs_sync_begin_host(const uint8_t* store_digests, size_t m, size_t reserve, pbs_sync_host** out,
                                   double* build_ms) {
    const Clock::time_point t0 = Clock::now();
    if (out) *out = nullptr;
    if (build_ms) *build_ms = 0;
    if (!begin_args_valid(store_digests, m, reserve, out)) return PBS_ERR_INVALID;
    pbs_sync_host* h = new (std::nothrow) pbs_sync_host;
    if (!h) return PBS_ERR_NOMEM;
    try {
        if (m) h->digests.assign(store_digests, store_digests + 32 * m);
        h->present.assign(m, 1);
        h->claimed.assign(m, 0);
        h->lowest.reserve(m + reserve);
        for (size_t j = 0; j < m; ++j) h->lowest.emplace(key(store_digests + 32 * j), (uint32_t)j);  // (the first stays)
        h->log2 = begin_log2(m, reserve);
        h->run.clear();
    } catch (const std::bad_alloc&) {
        delete h;
        return PBS_ERR_NOMEM;
    }
    Handles::add(h);
    *out = h;
    if (build_ms) *build_ms = ms_since(t0);
    return PBS_OK;
}

extern "C" size_t pbs_sync_count_host(pbs_sync_host* h) { return Handles::alive(h) ? h->count() : 0; }

extern "C" uint32_t pbs_sync_table_log2_host(pbs_sync_host* h) { return Handles::alive(h) ? h->log2 : 0; }

extern "C" int pbs_sync_listing_host(pbs_sync_host* h, uint8_t* digests_out, uint8_t* present_out, size_t cap,
                                     size_t* count) {
    if (count) *count = 0;
    if (!Handles::alive(h)) return PBS_ERR_INVALID;
    const size_t k = cap < h->count() ? cap : h->count();
    if (k && digests_out) std::memcpy(digests_out, h->digests.data(), 32 * k);
    if (k && present_out) std::memcpy(present_out, h->present.data(), k);
    if (count) *count = h->count();
    return PBS_OK;
}

extern "C" int pbs_sync_new_group_host(pbs_sync_host* h) {
    if (!Handles::alive(h) || h->run.open) return PBS_ERR_INVALID;
    h->claimed.assign(h->count(), 0);
    return PBS_OK;
}

extern "C" void pbs_sync_end_host(pbs_sync_host* h) {
    if (h && Handles::remove(h)) delete h;
}

extern "C" int pbs_sync_plan_host(pbs_sync_host* h, const uint8_t* digests, const uint64_t* sizes, size_t n,
                                  uint8_t* verdict, uint32_t* fetch_store, uint32_t* fetch_entry, size_t fcap,
                                  size_t* n_fetch, uint32_t* touch_store, size_t tcap, size_t* n_touch, double* plan_ms) {
    const Clock::time_point t0 = Clock::now();
    if (n_fetch) *n_fetch = 0;
    if (n_touch) *n_touch = 0;
    if (plan_ms) *plan_ms = 0;
    if (!Handles::alive(h) || h->run.open ||
        !plan_args_valid(h->count(), digests, sizes, n, fetch_store, fetch_entry, fcap, n_fetch, touch_store, tcap, n_touch))
        return PBS_ERR_INVALID;
    const int rc = plan(h, digests, sizes, n, verdict);
    if (rc != PBS_OK) return rc;
    copy_lists(h->run, fetch_store, fetch_entry, fcap, n_fetch, touch_store, tcap, n_touch);
    if (plan_ms) *plan_ms = ms_since(t0);
    return PBS_OK;
}

extern "C" int pbs_sync_lists_host(pbs_sync_host* h, uint32_t* fetch_store, uint32_t* fetch_entry, size_t fcap,
                                   size_t* n_fetch, uint32_t* touch_store, size_t tcap, size_t* n_touch) {
    if (n_fetch) *n_fetch = 0;
    if (n_touch) *n_touch = 0;
    if (!Handles::alive(h) || !h->run.open || !n_fetch || !n_touch || (fcap && (!fetch_store || !fetch_entry)) ||
        (tcap && !touch_store))
        return PBS_ERR_INVALID;
    copy_lists(h->run, fetch_store, fetch_entry, fcap, n_fetch, touch_store, tcap, n_touch);
    return PBS_OK;
}

extern "C" int pbs_sync_submit_host(pbs_sync_host* h, const uint8_t* blobs, const uint64_t* blob_offsets,
                                    const uint8_t* load_failed, size_t k, uint8_t* kinds, uint8_t* status,
                                    pbs_sync_timing* timing) {
    const Clock::time_point t0 = Clock::now();
    if (timing) std::memset(timing, 0, sizeof(*timing));
    if (!Handles::alive(h) || !submit_args_valid(h->run, blobs, blob_offsets, k)) return PBS_ERR_INVALID;
    IndexRun& run = h->run;
    pbs_sync_timing tm;
    std::memset(&tm, 0, sizeof(tm));
    tm.blobs = k;
    for (size_t t = 0; t < k; ++t) {
        const size_t item = run.done;
        const uint64_t len = blob_offsets[t + 1] - blob_offsets[t];
        uint8_t kind = PBS_BLOB_KIND_NONE, st = PBS_SYNC_ST_LOAD_FAILED;
        if (!load_failed || !load_failed[t]) {
            try {
                st = pbs::verify::host_blob_verdict(len ? blobs + blob_offsets[t] : nullptr, (size_t)len,
                                                    &run.fetch_digests[32 * item], run.fetch_sizes[item], &kind);
            } catch (const std::exception&) {  // (no memory for a slot of the index's size: the items before stay consumed)
                return PBS_ERR_NOMEM;
            }
            if (st == PBS_BLOB_ST_NO_CONFIG) st = PBS_BLOB_ST_OK;  // verify_unencrypted: Ok for an encrypted chunk
            tm.decoded += 1;
            const bool enc = kind == PBS_BLOB_KIND_ENCRYPTED || kind == PBS_BLOB_KIND_ENCR_COMPR;
            tm.encrypted += enc;
            if (!enc) tm.scratch_bytes += run.fetch_sizes[item];
        }
        if (account(run, st, len)) h->present[run.fetch_store[item]] = 1;  // insert_chunk
        if (kinds) kinds[t] = kind;
        if (status) status[t] = st;
    }
    tm.decode_ms = tm.total_ms = ms_since(t0);
    if (timing) *timing = tm;
    return PBS_OK;
}

extern "C" int pbs_sync_finish_host(pbs_sync_host* h, pbs_sync_result* res) {
    if (!Handles::alive(h) || !h->run.open || h->run.remaining() != 0) return PBS_ERR_INVALID;
    close_run(h->run, res);
    return PBS_OK;
}

extern "C" int pbs_sync_abort_index_host(pbs_sync_host* h) {
    if (!Handles::alive(h)) return PBS_ERR_INVALID;
    h->run.clear();
    return PBS_OK;
}

extern "C" int pbs_sync_index_image_host(pbs_sync_host* h, const uint8_t* image, size_t len, const uint64_t* info_size,
                                         const uint8_t* info_csum, uint32_t* index_check, size_t* n_entries,
                                         uint8_t* verdict, size_t vcap, uint32_t* fetch_store, uint32_t* fetch_entry,
                                         size_t fcap, size_t* n_fetch, uint32_t* touch_store, size_t tcap,
                                         size_t* n_touch, double* plan_ms) {
    const Clock::time_point t0 = Clock::now();
    if (n_fetch) *n_fetch = 0;
    if (n_touch) *n_touch = 0;
    if (n_entries) *n_entries = 0;
    if (plan_ms) *plan_ms = 0;
    if (index_check) *index_check = PBS_VERIFY_INDEX_OK;
    if (!Handles::alive(h) || h->run.open || !index_check || (vcap && !verdict) ||
        !lists_args_valid(fetch_store, fetch_entry, fcap, n_fetch, touch_store, tcap, n_touch))
        return PBS_ERR_INVALID;
    IndexLayout lo;
    int rc = index_layout(image, len, &lo);
    if (rc != PBS_OK) return rc;
    if (!entries_fit(h->count(), lo.n)) return PBS_ERR_INVALID;
    if (n_entries) *n_entries = lo.n;
    *index_check = pbs::verify::index_check(image, lo, info_size, info_csum);
    if (*index_check != PBS_VERIFY_INDEX_OK) return PBS_OK;  // verify_archive bails: nothing is claimed
    try {
        std::vector<uint8_t> digests, v(lo.n);
        std::vector<uint64_t> sizes;
        pbs::verify::index_entries(image, lo, digests, sizes);
        rc = plan(h, digests.data(), sizes.data(), lo.n, v.data());
        if (rc != PBS_OK) return rc;
        if (lo.n && vcap) std::memcpy(verdict, v.data(), vcap < lo.n ? vcap : lo.n);
    } catch (const std::bad_alloc&) {
        return PBS_ERR_NOMEM;
    }
    copy_lists(h->run, fetch_store, fetch_entry, fcap, n_fetch, touch_store, tcap, n_touch);
    if (plan_ms) *plan_ms = ms_since(t0);
    return PBS_OK;
}
