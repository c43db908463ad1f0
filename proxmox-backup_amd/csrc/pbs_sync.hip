// Device side of the sync job (include/pbs_sync.h; DESIGN.md section 10, "Sync"): the local
// store's listing as the growing table of grow_table_dev.h, one present and one claimed byte per
// entry, the fetch plan of an index (its claim and ordered append, then this file's flags: first
// occurrence, ordered compaction over the index axis, commit) and the present bytes after a
// submit.  The blobs themselves go through the blob verdict of verify_dev.h, as the verify job's do.
//
// Like verify and garbage collection this path is bound by the latency of random reads (a table
// slot, the 32 bytes of the entry it names), so every kernel is one lane per entry in 256-thread
// blocks with few registers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "dev_arena.h"
#include "gc_common.h"
#include "gc_table_dev.h"
#include "grow_table_dev.h"
#include "live_handles.h"
#include "pbs_blob.h"
#include "pbs_chunker.h"
#include "pbs_chunker_internal.h"
#include "pbs_restore.h"
#include "pbs_sync.h"
#include "sync_common.h"
#include "verify_common.h"
#include "verify_dev.h"

struct pbs_sync {
    pbs::gc::GrowTable tab;         // the entries' digests and the table over them
    uint8_t* d_present = nullptr;  // cap
    uint8_t* d_claimed = nullptr;  // cap
    uint32_t* d_first = nullptr;   // cap: the lowest entry of the open plan naming entry j; kEmpty between plans
    pbs::sync::IndexRun run;
    pbs_sync() {
        tab.side(&d_present);
        tab.side(&d_claimed);
        tab.side(&d_first, 0xFF);
    }
};

namespace pbs {
namespace sync {
namespace {

using namespace pbs::gc;
using pbs::verify::blob_verdicts;
using pbs::verify::BlobSlots;
using pbs::verify::BlobTiming;

// what the flag kernel leaves per index entry
enum Flag : uint8_t {
    kClaim = 1,    // this lane claims its chunk: verdict EXISTS or FETCH
    kNew = 2,      // ... and appends it: it won a table slot
    kPresent = 4,  // ... and the chunk is there: the touch list
    kFirst = 8,    // the lowest lane naming a listed entry: it puts first[j] back
};

// (grow_claim_kernel, the probe with an insert where it ends: grow_table_dev.h)

// One lane per index entry, after the claim kernel has ended: who claims (the lowest lane of a
// digest, unless the chunk was claimed before this plan), who appends, who touches; and the
// block's counts of the three kinds for the ordered compaction.
__global__ __launch_bounds__(kGcThreads) void sync_flag_kernel(const uint64_t* __restrict__ ref, uint64_t n, uint32_t count,
                                                               const uint32_t* __restrict__ table,
                                                               const uint32_t* __restrict__ first,
                                                               const uint8_t* __restrict__ present,
                                                               const uint8_t* __restrict__ claimed, uint8_t* __restrict__ flag,
                                                               unsigned long long* __restrict__ block_new,
                                                               unsigned long long* __restrict__ block_fetch,
                                                               unsigned long long* __restrict__ block_touch) {
    __shared__ uint32_t wcnt[kGcWaves];
    const uint64_t i = (uint64_t)blockIdx.x * kGcThreads + threadIdx.x;
    uint8_t f = 0;
    if (i < n) {
        const uint64_t r = ref[i];
        if (r & kRefSlot) {
            if (table[r & ~kRefSlot] == count + (uint32_t)i) f = kClaim | kNew;
        } else if (first[r] == (uint32_t)i) {
            f = kFirst;
            if (!claimed[r]) f |= present[r] ? (kClaim | kPresent) : kClaim;
        }
        flag[i] = f;
    }
    const bool claim = f & kClaim, touch = f & kPresent;
    const uint32_t cn = block_count(f & kNew, wcnt), cf = block_count(claim && !touch, wcnt), ct = block_count(touch, wcnt);
    if (threadIdx.x == 0) {
        block_new[blockIdx.x] = cn;
        block_fetch[blockIdx.x] = cf;
        block_touch[blockIdx.x] = ct;
    }
}

// One lane per index entry: the plan takes effect.  An appending lane gets the entry position
// count + its rank among the appending lanes, writes it over its provisional table value, copies
// its digest to that position and sets present = 0; every claiming lane sets claimed and goes to
// the fetch or the touch list at its rank there (ascending index position); first[] goes back to
// kEmpty.  Every word written here has one writer, and nothing read here is written here.
__global__ __launch_bounds__(kGcThreads) void sync_commit_kernel(
    const uint8_t* __restrict__ dig, const uint64_t* __restrict__ ref, const uint8_t* __restrict__ flag, uint64_t n,
    uint32_t count, const unsigned long long* __restrict__ start_new, const unsigned long long* __restrict__ start_fetch,
    const unsigned long long* __restrict__ start_touch, uint32_t* __restrict__ table, uint8_t* __restrict__ store,
    uint8_t* __restrict__ present, uint8_t* __restrict__ claimed, uint32_t* __restrict__ first,
    uint8_t* __restrict__ verdict, uint32_t* __restrict__ fetch_store, uint32_t* __restrict__ fetch_entry,
    uint32_t* __restrict__ touch_store) {
    __shared__ uint32_t wcnt[kGcWaves];
    const uint64_t i = (uint64_t)blockIdx.x * kGcThreads + threadIdx.x;
    const uint8_t f = i < n ? flag[i] : 0;
    const bool claim = f & kClaim, touch = f & kPresent, fresh = f & kNew;
    const uint64_t rn = ordered_rank(fresh, start_new[blockIdx.x], wcnt);
    const uint64_t rf = ordered_rank(claim && !touch, start_fetch[blockIdx.x], wcnt);
    const uint64_t rt = ordered_rank(touch, start_touch[blockIdx.x], wcnt);
    if (i >= n) return;
    const uint64_t r = ref[i];
    uint32_t c = (uint32_t)r;
    if (fresh) {
        c = count + (uint32_t)rn;
        table[r & ~kRefSlot] = c;
        const uint64_t* src = reinterpret_cast<const uint64_t*>(dig + 32 * i);
        uint64_t* dst = reinterpret_cast<uint64_t*>(store + 32ull * c);
        dst[0] = src[0];
        dst[1] = src[1];
        dst[2] = src[2];
        dst[3] = src[3];
        present[c] = 0;
    }
    if (f & kFirst) first[c] = kEmpty;
    if (claim) {
        claimed[c] = 1;
        if (touch) {
            touch_store[rt] = c;
        } else {
            fetch_store[rf] = c;
            fetch_entry[rf] = (uint32_t)i;
        }
    }
    verdict[i] = !claim ? PBS_SYNC_DUP : touch ? PBS_SYNC_EXISTS : PBS_SYNC_FETCH;
}

// One lane per submitted blob: insert_chunk.  The fetch list names every entry once.
__global__ __launch_bounds__(kGcThreads) void sync_state_kernel(const uint32_t* __restrict__ store_pos,
                                                                const uint8_t* __restrict__ status, uint64_t k,
                                                                uint8_t* __restrict__ present) {
    const uint64_t t = (uint64_t)blockIdx.x * kGcThreads + threadIdx.x;
    if (t >= k) return;
    if (status[t] == PBS_BLOB_ST_OK) present[store_pos[t]] = 1;
}

ArenaPool& spool() {
    static ArenaPool* p = new ArenaPool;  // never destroyed (HIP may be torn down first at exit)
    return *p;
}

enum SSlot : unsigned { kSsDig, kSsRef, kSsFlag, kSsCountNew, kSsCountFetch, kSsCountTouch, kSsStartNew, kSsStartFetch,
                        kSsStartTouch, kSsScanTmp, kSsVerdict, kSsOutStore, kSsOutEntry, kSsOutTouch, kSsSpans, kSsEnc,
                        kSsOut, kSsPos, kSsStatus, kSsPack };

constexpr GrowSlots kGrowSlots = {kSsRef, kSsCountNew, kSsStartNew, kSsScanTmp};
constexpr BlobSlots kBlobSlots = {kSsSpans, kSsEnc, kSsOut, kSsPack};

using Handles = Live<pbs_sync>;

void free_handle(pbs_sync* h) {
    DeviceGuard dg(h->tab.dev);
    if (dg.ok) h->tab.free_all();
    delete h;
}

// pbs_sync_plan after the argument checks; the caller has set the device.  The lists stay in the
// run; verdict (host, n) may be NULL.
int plan_on(pbs_sync* h, const uint8_t* digests, const uint64_t* sizes, size_t n, uint8_t* verdict, double* plan_ms) {
    GrowTable& t = h->tab;
    hipStream_t st = t.st;
    IndexRun& run = h->run;
    run.clear();
    const unsigned nb = blocks_for(n);
    ArenaLease ar(spool(), t.dev);
    const int r = t.append_room(*ar, kGrowSlots, n, 3);  // (before the timed part)
    if (r != PBS_OK) return r;
    uint8_t* d_dig = ar->get<uint8_t>(kSsDig, 32 * n);
    uint8_t* flag = ar->get<uint8_t>(kSsFlag, n);
    uint8_t* d_verdict = ar->get<uint8_t>(kSsVerdict, n);
    uint32_t* out_store = ar->get<uint32_t>(kSsOutStore, n * 4);
    uint32_t* out_entry = ar->get<uint32_t>(kSsOutEntry, n * 4);
    uint32_t* out_touch = ar->get<uint32_t>(kSsOutTouch, n * 4);
    hipEvent_t e0 = ar->event(0), e1 = ar->event(1);
    if (!d_dig || !flag || !d_verdict || !out_store || !out_entry || !out_touch) return PBS_ERR_NOMEM;
    if (!e0 || !e1) return PBS_ERR_HIP;
    CallRc rc;
    unsigned long long totals[3] = {};
    (void)hipGetLastError();
    if (n) rc.ok(hipMemcpyAsync(d_dig, digests, 32 * n, hipMemcpyHostToDevice, st));
    if (rc.rc == PBS_OK && rc.ok(hipEventRecord(e0, st)))
        rc.fail(t.append(
            *ar, kGrowSlots, d_dig, nullptr, h->d_first, n, 3, totals,
            [&](const uint64_t* ref, uint32_t count, unsigned long long* const* counts) {
                hipLaunchKernelGGL(sync_flag_kernel, dim3(nb), dim3(kGcThreads), 0, st, ref, (uint64_t)n, count, t.d_table,
                                   h->d_first, h->d_present, h->d_claimed, flag, counts[0], counts[1], counts[2]);
                return hipGetLastError();
            },
            [&](const uint64_t* ref, uint32_t count, unsigned long long* const* starts) {
                hipLaunchKernelGGL(sync_commit_kernel, dim3(nb), dim3(kGcThreads), 0, st, d_dig, ref, flag, (uint64_t)n, count,
                                   starts[0], starts[1], starts[2], t.d_table, t.d_store, h->d_present, h->d_claimed,
                                   h->d_first, d_verdict, out_store, out_entry, out_touch);
                return hipGetLastError();
            },
            e1));
    const unsigned long long n_new = totals[0], n_fetch = totals[1], n_touch = totals[2];
    if (rc.rc == PBS_OK && (n_new > n_fetch || n_fetch + n_touch > n)) rc.fail(PBS_ERR_HIP);  // (never: one flag per lane)
    if (rc.rc == PBS_OK) {
        run.fetch_store.resize((size_t)n_fetch);
        run.fetch_entry.resize((size_t)n_fetch);
        run.touch_store.resize((size_t)n_touch);
        if (n_fetch && rc.ok(hipMemcpyAsync(run.fetch_store.data(), out_store, n_fetch * 4, hipMemcpyDeviceToHost, st)))
            rc.ok(hipMemcpyAsync(run.fetch_entry.data(), out_entry, n_fetch * 4, hipMemcpyDeviceToHost, st));
        if (n_touch && rc.rc == PBS_OK)
            rc.ok(hipMemcpyAsync(run.touch_store.data(), out_touch, n_touch * 4, hipMemcpyDeviceToHost, st));
        if (verdict && n && rc.rc == PBS_OK) rc.ok(hipMemcpyAsync(verdict, d_verdict, n, hipMemcpyDeviceToHost, st));
    }
    if (hipStreamSynchronize(st) != hipSuccess) rc.fail(PBS_ERR_HIP);  // (before the arena goes back)
    if (rc.rc == PBS_OK) {
        for (size_t i = 0; i < run.fetch_store.size(); ++i)
            if (run.fetch_store[i] >= t.count || run.fetch_entry[i] >= n) rc.fail(PBS_ERR_HIP);  // (never)
        for (size_t i = 0; i < run.touch_store.size(); ++i)
            if (run.touch_store[i] >= t.count) rc.fail(PBS_ERR_HIP);  // (never)
    }
    if (rc.rc != PBS_OK) {
        run.clear();
        return rc.rc;
    }
    run.start(digests, sizes, n, n_new);
    if (plan_ms) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, e0, e1);
        *plan_ms = ms;
    }
    return PBS_OK;
}

// pbs_sync_submit after the argument checks; the caller has set the device.  Nothing of the run
// changes unless every step went well.
int submit_on(pbs_sync* h, const uint8_t* blobs_dev, const uint64_t* blob_offsets, const uint8_t* load_failed, size_t k,
              uint8_t* kinds_out, uint8_t* status_out, pbs_sync_timing* timing) {
    const HClock::time_point t0 = HClock::now();
    IndexRun& run = h->run;
    hipStream_t st = h->tab.st;
    pbs_sync_timing tm;
    std::memset(&tm, 0, sizeof(tm));
    tm.blobs = k;
    if (k == 0) {
        if (timing) *timing = tm;
        return PBS_OK;
    }
    const size_t item0 = run.done;
    ArenaLease ar(spool(), h->tab.dev);
    std::vector<uint8_t> kinds(k, PBS_BLOB_KIND_NONE), status(k, PBS_SYNC_ST_LOAD_FAILED);
    BlobTiming bt;
    const int rc = blob_verdicts(*ar, kBlobSlots, st, blobs_dev, blob_offsets, load_failed, &run.fetch_digests[32 * item0],
                                 [&](size_t t) { return run.fetch_sizes[item0 + t]; }, k, kinds.data(), status.data(),
                                 nullptr, &bt);
    if (rc != PBS_OK) return rc;
    tm.magic_ms = bt.magic_ms;
    tm.decode_ms = bt.decode_ms;
    tm.decoded = bt.decoded;
    tm.encrypted = bt.encrypted;
    tm.scratch_bytes = bt.scratch_bytes;

    // insert_chunk
    uint32_t* d_sp = ar->get<uint32_t>(kSsPos, 4 * k);
    uint8_t* d_status = ar->get<uint8_t>(kSsStatus, k);
    hipEvent_t e0 = ar->event(0), e1 = ar->event(1);
    if (!d_sp || !d_status) return PBS_ERR_NOMEM;
    if (!e0 || !e1) return PBS_ERR_HIP;
    CallRc call;
    (void)hipGetLastError();
    if (call.ok(hipMemcpyAsync(d_sp, &run.fetch_store[item0], 4 * k, hipMemcpyHostToDevice, st)) &&
        call.ok(hipMemcpyAsync(d_status, status.data(), k, hipMemcpyHostToDevice, st)) && call.ok(hipEventRecord(e0, st))) {
        hipLaunchKernelGGL(sync_state_kernel, dim3(blocks_for(k)), dim3(kGcThreads), 0, st, d_sp, d_status, (uint64_t)k,
                           h->d_present);
        call.ok(hipGetLastError()) && call.ok(hipEventRecord(e1, st));
    }
    if (hipStreamSynchronize(st) != hipSuccess) call.fail(PBS_ERR_HIP);  // (before the arena goes back)
    if (call.rc != PBS_OK) return call.rc;
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    tm.state_ms = ms;
    for (size_t t = 0; t < k; ++t) {
        (void)account(run, status[t], blob_offsets[t + 1] - blob_offsets[t]);
        if (kinds_out) kinds_out[t] = kinds[t];
        if (status_out) status_out[t] = status[t];
    }
    tm.total_ms = hms(t0);
    if (timing) *timing = tm;
    return PBS_OK;
}

}  // namespace
}  // namespace sync
}  // namespace pbs

using namespace pbs;
using namespace pbs::gc;
using namespace pbs::sync;

extern "C" void pbs_sync_release(void) { spool().clear(); }

extern "C" int pbs_sync_begin(const uint8_t* store_digests, size_t m, size_t reserve, pbs_sync** out, double* build_ms,
                              void* hip_stream) {
    if (out) *out = nullptr;
    if (build_ms) *build_ms = 0;
    if (!begin_args_valid(store_digests, m, reserve, out)) return PBS_ERR_INVALID;
    hipStream_t st = (hipStream_t)hip_stream;
    const StreamDevice sd(st);
    if (!sd.ok) return PBS_ERR_NO_DEVICE;
    DeviceGuard dg(sd.dev);
    if (!dg.ok) return PBS_ERR_NO_DEVICE;
    pbs_sync* h = new (std::nothrow) pbs_sync;
    if (!h) return PBS_ERR_NOMEM;
    h->run.clear();
    const int rc = h->tab.begin(sd, st, store_digests, m, reserve, build_ms, [&](CallRc& up) {
        up.ok(hipMemsetAsync(h->d_present, 1, m, st)) && up.ok(hipMemsetAsync(h->d_claimed, 0, m, st));
    });
    if (rc != PBS_OK) {
        free_handle(h);
        return rc;
    }
    Handles::add(h);
    *out = h;
    return PBS_OK;
}

extern "C" size_t pbs_sync_count(pbs_sync* h) { return Handles::alive(h) ? h->tab.count : 0; }

extern "C" uint32_t pbs_sync_table_log2(pbs_sync* h) { return Handles::alive(h) ? h->tab.log2 : 0; }

extern "C" int pbs_sync_listing(pbs_sync* h, uint8_t* digests_out, uint8_t* present_out, size_t cap, size_t* count) {
    if (count) *count = 0;
    if (!Handles::alive(h)) return PBS_ERR_INVALID;
    const size_t k = std::min(cap, h->tab.count);
    if (count) *count = h->tab.count;
    if (k == 0 || (!digests_out && !present_out)) return PBS_OK;
    DeviceGuard dg(h->tab.dev);
    if (!dg.ok) return PBS_ERR_NO_DEVICE;
    CallRc rc;
    if (digests_out) rc.ok(hipMemcpyAsync(digests_out, h->tab.d_store, 32 * k, hipMemcpyDeviceToHost, h->tab.st));
    if (present_out && rc.rc == PBS_OK) rc.ok(hipMemcpyAsync(present_out, h->d_present, k, hipMemcpyDeviceToHost, h->tab.st));
    if (hipStreamSynchronize(h->tab.st) != hipSuccess) rc.fail(PBS_ERR_HIP);
    return rc.rc;
}

extern "C" int pbs_sync_new_group(pbs_sync* h) {
    if (!Handles::alive(h) || h->run.open) return PBS_ERR_INVALID;
    if (h->tab.count == 0) return PBS_OK;
    DeviceGuard dg(h->tab.dev);
    if (!dg.ok) return PBS_ERR_NO_DEVICE;
    CallRc rc;
    rc.ok(hipMemsetAsync(h->d_claimed, 0, h->tab.count, h->tab.st));
    if (hipStreamSynchronize(h->tab.st) != hipSuccess) rc.fail(PBS_ERR_HIP);
    return rc.rc;
}

extern "C" void pbs_sync_end(pbs_sync* h) {
    if (h && Handles::remove(h)) free_handle(h);
}

extern "C" int pbs_sync_plan(pbs_sync* h, const uint8_t* digests, const uint64_t* sizes, size_t n, uint8_t* verdict,
                             uint32_t* fetch_store, uint32_t* fetch_entry, size_t fcap, size_t* n_fetch,
                             uint32_t* touch_store, size_t tcap, size_t* n_touch, double* plan_ms) {
    if (n_fetch) *n_fetch = 0;
    if (n_touch) *n_touch = 0;
    if (plan_ms) *plan_ms = 0;
    if (!Handles::alive(h) || h->run.open ||
        !plan_args_valid(h->tab.count, digests, sizes, n, fetch_store, fetch_entry, fcap, n_fetch, touch_store, tcap, n_touch))
        return PBS_ERR_INVALID;
    DeviceGuard dg(h->tab.dev);
    if (!dg.ok) return PBS_ERR_NO_DEVICE;
    int rc;
    try {
        rc = plan_on(h, digests, sizes, n, verdict, plan_ms);
    } catch (const std::bad_alloc&) {
        h->run.clear();
        rc = PBS_ERR_NOMEM;
    }
    if (rc != PBS_OK) return rc;
    copy_lists(h->run, fetch_store, fetch_entry, fcap, n_fetch, touch_store, tcap, n_touch);
    return PBS_OK;
}

extern "C" int pbs_sync_lists(pbs_sync* h, uint32_t* fetch_store, uint32_t* fetch_entry, size_t fcap, size_t* n_fetch,
                              uint32_t* touch_store, size_t tcap, size_t* n_touch) {
    if (n_fetch) *n_fetch = 0;
    if (n_touch) *n_touch = 0;
    if (!Handles::alive(h) || !h->run.open || !lists_args_valid(fetch_store, fetch_entry, fcap, n_fetch, touch_store, tcap, n_touch))
        return PBS_ERR_INVALID;
    copy_lists(h->run, fetch_store, fetch_entry, fcap, n_fetch, touch_store, tcap, n_touch);
    return PBS_OK;
}

extern "C" int pbs_sync_submit(pbs_sync* h, const uint8_t* blobs_dev, const uint64_t* blob_offsets,
                               const uint8_t* load_failed, size_t k, uint8_t* kinds, uint8_t* status,
                               pbs_sync_timing* timing) {
    if (timing) std::memset(timing, 0, sizeof(*timing));
    if (!Handles::alive(h) || !submit_args_valid(h->run, blobs_dev, blob_offsets, k)) return PBS_ERR_INVALID;
    DeviceGuard dg(h->tab.dev);
    if (!dg.ok) return PBS_ERR_NO_DEVICE;
    try {
        return submit_on(h, blobs_dev, blob_offsets, load_failed, k, kinds, status, timing);
    } catch (const std::bad_alloc&) {
        return PBS_ERR_NOMEM;
    }
}

extern "C" int pbs_sync_finish(pbs_sync* h, pbs_sync_result* res) {
    if (!Handles::alive(h) || !h->run.open || h->run.remaining() != 0) return PBS_ERR_INVALID;
    close_run(h->run, res);
    return PBS_OK;
}

extern "C" int pbs_sync_abort_index(pbs_sync* h) {
    if (!Handles::alive(h)) return PBS_ERR_INVALID;
    h->run.clear();
    return PBS_OK;
}

extern "C" int pbs_sync_index_image(pbs_sync* h, const uint8_t* image, size_t len, const uint64_t* info_size,
                                    const uint8_t* info_csum, uint32_t* index_check, size_t* n_entries, uint8_t* verdict,
                                    size_t vcap, uint32_t* fetch_store, uint32_t* fetch_entry, size_t fcap,
                                    size_t* n_fetch, uint32_t* touch_store, size_t tcap, size_t* n_touch,
                                    double* plan_ms) {
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
    if (!entries_fit(h->tab.count, lo.n)) return PBS_ERR_INVALID;
    if (n_entries) *n_entries = lo.n;
    *index_check = pbs::verify::index_check(image, lo, info_size, info_csum);
    if (*index_check != PBS_VERIFY_INDEX_OK) return PBS_OK;  // verify_archive bails: nothing is claimed
    DeviceGuard dg(h->tab.dev);
    if (!dg.ok) return PBS_ERR_NO_DEVICE;
    try {
        std::vector<uint8_t> digests, v(vcap ? lo.n : 0);
        std::vector<uint64_t> sizes;
        pbs::verify::index_entries(image, lo, digests, sizes);
        rc = plan_on(h, digests.data(), sizes.data(), lo.n, vcap ? v.data() : nullptr, plan_ms);
        if (rc != PBS_OK) return rc;
        if (lo.n && vcap) std::memcpy(verdict, v.data(), std::min(vcap, lo.n));
    } catch (const std::bad_alloc&) {
        h->run.clear();
        return PBS_ERR_NOMEM;
    }
    copy_lists(h->run, fetch_store, fetch_entry, fcap, n_fetch, touch_store, tcap, n_touch);
    return PBS_OK;
}
