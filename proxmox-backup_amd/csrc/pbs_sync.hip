// Device side of the sync job (include/pbs_sync.h; DESIGN.md section 10, "Sync"): the local
// store's listing as the table of gc_table_dev.h over a digest list that grows, one present and
// one claimed byte per entry, the fetch plan of an index (probe or insert, first occurrence,
// ordered compaction over the index axis, commit) and the present bytes after a submit.  The
// blobs themselves go through pbs_blob_decode_inflate_device, exactly as the verify job's do.
//
// Like verify and garbage collection this path is bound by the latency of random reads (a table
// slot, the 32 bytes of the entry it names), so every kernel is one lane per entry in 256-thread
// blocks with few registers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <new>
#include <set>
#include <vector>

#include "dev_arena.h"
#include "gc_common.h"
#include "gc_table_dev.h"
#include "pbs_blob.h"
#include "pbs_chunker.h"
#include "pbs_chunker_internal.h"
#include "pbs_restore.h"
#include "pbs_sync.h"
#include "sync_common.h"
#include "verify_common.h"
#include "verify_dev.h"

struct pbs_sync {
    int dev = 0, ncu = 0;
    hipStream_t st = nullptr;
    size_t count = 0, cap = 0;     // entries; entries the four arrays below hold
    uint32_t log2 = 0;
    bool stale = false;            // a plan failed half-way: table and d_first are rebuilt before the next one
    uint8_t* d_store = nullptr;    // 32 cap: the entries' digests
    uint8_t* d_present = nullptr;  // cap
    uint8_t* d_claimed = nullptr;  // cap
    uint32_t* d_first = nullptr;   // cap: the lowest entry of the open plan naming entry j; kEmpty between plans
    uint32_t* d_table = nullptr;   // 2^log2 entry positions, kEmpty where free
    pbs::sync::IndexRun run;
};

namespace pbs {
namespace sync {
namespace {

using namespace pbs::gc;
using pbs::verify::block_count;
using pbs::verify::verify_magic_kernel;

// what the claim kernel leaves per index entry: the entry position found, or this bit and the
// slot the lane's digest sits in
constexpr uint64_t kRefSlot = 1ull << 63;

// what the flag kernel leaves per index entry
enum Flag : uint8_t {
    kClaim = 1,    // this lane claims its chunk: verdict EXISTS or FETCH
    kNew = 2,      // ... and appends it: it won a table slot
    kPresent = 4,  // ... and the chunk is there: the touch list
    kFirst = 8,    // the lowest lane naming a listed entry: it puts first[j] back
};

// One lane per index entry: the probe of verify_probe_kernel with an insert where it ends.
//
// The lane walks its cluster from the home slot and keeps the LOWEST entry position j carrying
// its digest (equal digests of the listing sit in slots of their own, so the walk goes to the
// cluster's end).  Found: first[j] = min(first[j], i).  Not found: the provisional value count + i
// goes into the first free slot by compare-and-swap; a value v >= count in a slot names
// dig[v - count], read-only input of this launch.  Where the swap is lost, or the walk meets a
// provisional value before a free slot, the lane compares with that occupant: an equal digest
// ends the walk with atomicMin(slot, count + i), another one sends it to the next slot.
//
// Why no order of the lanes changes the outcome:
//  - a slot only ever goes from free to occupied, and an occupant's digest never changes
//    (atomicMin swaps count + i values of equal digests only, and every entry position is below
//    every provisional value, so it never replaces an entry);
//  - so all lanes of one digest walk the same occupied prefix: entries that were there before the
//    launch (which hold every listed copy of the digest, all before the first slot that was
//    free at the launch) and occupants of other digests, which each of them passes.  The first
//    of them to reach a free slot takes it and all the others meet it there: one slot per new
//    digest, and its final value is the lowest index position, count + min i;
//  - a table read may be stale (it is a plain load; the L1 of a CU and the L2 of an XCD do not
//    see other XCDs' atomics): a slot read as free that is taken is put right by the swap, which
//    returns the occupant; an occupant read stale is another lane of the same digest;
//  - no lane waits for another lane's progress, and the table holds 2^L >= 2 (count + n) slots
//    (the growth runs before the launch), so a free slot always comes and every walk ends.
__global__ __launch_bounds__(kGcThreads) void sync_claim_kernel(const uint8_t* __restrict__ dig, uint64_t n,
                                                                const uint8_t* __restrict__ store, uint32_t count,
                                                                uint32_t* table, uint32_t shift, uint64_t mask,
                                                                uint32_t* __restrict__ first, uint64_t* __restrict__ ref) {
    const uint64_t i = (uint64_t)blockIdx.x * kGcThreads + threadIdx.x;
    if (i >= n) return;
    const Dig d = load_digest(dig + 32 * i);
    const uint32_t mine = count + (uint32_t)i;
    uint32_t j = kEmpty;
    uint64_t s = home_slot(d.w[0], shift);
    for (;;) {
        uint32_t k = table[s];
        if (k == kEmpty) {
            if (j != kEmpty) break;  // the cluster's end, and the chunk is listed
            k = atomicCAS(&table[s], kEmpty, mine);
            if (k == kEmpty) break;  // the slot is this lane's, until a lower lane of its digest comes
        }
        if (k < count) {
            if (k < j && same_digest(store, k, d)) j = k;
        } else if (j == kEmpty && same_digest(dig, k - count, d)) {
            atomicMin(&table[s], mine);
            break;
        }
        s = (s + 1) & mask;
    }
    if (j != kEmpty) {
        atomicMin(&first[j], (uint32_t)i);
        ref[i] = j;
    } else {
        ref[i] = kRefSlot | s;
    }
}

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

// a flagged lane's rank among the flagged lanes before it (the scheme of gc_compact_kernel:
// start is the exclusive sum of the blocks' counts, the rank inside the block comes from the
// ballots); all threads call it
__device__ __forceinline__ uint64_t ordered_rank(bool f, unsigned long long start, uint32_t* wcnt) {
    const unsigned long long b = __ballot(f);
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wcnt[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    uint64_t rank = start + __popcll(b & ((1ull << lane) - 1));
    for (uint32_t w = 0; w < wave; ++w) rank += wcnt[w];
    __syncthreads();  // (wcnt is written again by the next call)
    return rank;
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

struct Live {
    std::mutex mu;
    std::set<const pbs_sync*> handles;
};
Live& live() {
    static Live* l = new Live;
    return *l;
}
bool alive(const pbs_sync* h) {
    if (!h) return false;
    Live& l = live();
    std::lock_guard<std::mutex> g(l.mu);
    return l.handles.count(h) != 0;
}

void free_handle(pbs_sync* h) {
    DeviceGuard dg(h->dev);
    if (dg.ok) {
        (void)hipStreamSynchronize(h->st);
        if (h->d_store) (void)hipFree(h->d_store);
        if (h->d_present) (void)hipFree(h->d_present);
        if (h->d_claimed) (void)hipFree(h->d_claimed);
        if (h->d_first) (void)hipFree(h->d_first);
        if (h->d_table) (void)hipFree(h->d_table);
    }
    delete h;
}

// The entry arrays for at least `want` entries; what they hold moves along.  Synchronous.
int reserve_entries(pbs_sync* h, size_t want) {
    if (want <= h->cap) return PBS_OK;
    const size_t cap = std::max(want, h->cap + h->cap / 2);
    uint8_t *store = nullptr, *present = nullptr, *claimed = nullptr;
    uint32_t* first = nullptr;
    CallRc rc;
    if (hipMalloc(&store, 32 * cap) != hipSuccess || hipMalloc(&present, cap) != hipSuccess ||
        hipMalloc(&claimed, cap) != hipSuccess || hipMalloc(&first, 4 * cap) != hipSuccess) {
        (void)hipGetLastError();
        rc.fail(PBS_ERR_NOMEM);
    }
    hipStream_t st = h->st;
    if (rc.rc == PBS_OK && h->count) {
        rc.ok(hipMemcpyAsync(store, h->d_store, 32 * h->count, hipMemcpyDeviceToDevice, st)) &&
            rc.ok(hipMemcpyAsync(present, h->d_present, h->count, hipMemcpyDeviceToDevice, st)) &&
            rc.ok(hipMemcpyAsync(claimed, h->d_claimed, h->count, hipMemcpyDeviceToDevice, st));
    }
    if (rc.rc == PBS_OK) rc.ok(hipMemsetAsync(first, 0xFF, 4 * cap, st));
    if (hipStreamSynchronize(st) != hipSuccess) rc.fail(PBS_ERR_HIP);
    if (rc.rc != PBS_OK) {
        if (store) (void)hipFree(store);
        if (present) (void)hipFree(present);
        if (claimed) (void)hipFree(claimed);
        if (first) (void)hipFree(first);
        return rc.rc;
    }
    std::swap(h->d_store, store);
    std::swap(h->d_present, present);
    std::swap(h->d_claimed, claimed);
    std::swap(h->d_first, first);
    (void)hipFree(store);
    (void)hipFree(present);
    (void)hipFree(claimed);
    (void)hipFree(first);
    h->cap = cap;
    return PBS_OK;
}

// The table at 2^log2 slots over all entries (gc_build_kernel), queued on the stream.  A new
// allocation when the size changes.
int rebuild_table(pbs_sync* h, uint32_t log2) {
    const size_t slots = (size_t)1 << log2;
    if (log2 != h->log2 || !h->d_table) {
        uint32_t* t = nullptr;
        if (log2 >= 8 * sizeof(size_t) - 3 || hipMalloc(&t, slots * 4) != hipSuccess) {
            (void)hipGetLastError();
            return PBS_ERR_NOMEM;
        }
        if (h->d_table) {
            (void)hipStreamSynchronize(h->st);
            (void)hipFree(h->d_table);
        }
        h->d_table = t;
        h->log2 = log2;
    }
    CallRc rc;
    (void)hipGetLastError();
    if (rc.ok(hipMemsetAsync(h->d_table, 0xFF, slots * 4, h->st)) && h->count) {
        hipLaunchKernelGGL(gc_build_kernel, dim3(blocks_for(h->count)), dim3(kGcThreads), 0, h->st, h->d_store,
                           (uint64_t)h->count, h->d_table, 64 - log2, (uint64_t)slots - 1);
        rc.ok(hipGetLastError());
    }
    return rc.rc;
}

// pbs_sync_plan after the argument checks; the caller has set the device.  The lists stay in the
// run; verdict (host, n) may be NULL.
int plan_on(pbs_sync* h, const uint8_t* digests, const uint64_t* sizes, size_t n, uint8_t* verdict, double* plan_ms) {
    hipStream_t st = h->st;
    IndexRun& run = h->run;
    run.clear();
    int r = reserve_entries(h, h->count + n);
    if (r != PBS_OK) return r;
    const unsigned nb = blocks_for(n);
    ArenaLease ar(spool(), h->dev);
    uint8_t* d_dig = ar->get<uint8_t>(kSsDig, 32 * n);
    uint64_t* ref = ar->get<uint64_t>(kSsRef, 8 * n);
    uint8_t* flag = ar->get<uint8_t>(kSsFlag, n);
    unsigned long long* counts[3];
    unsigned long long* starts[3];
    for (int c = 0; c < 3; ++c) {
        counts[c] = ar->get<unsigned long long>(kSsCountNew + c, ((size_t)nb + 1) * 8);
        starts[c] = ar->get<unsigned long long>(kSsStartNew + c, ((size_t)nb + 1) * 8);
    }
    uint8_t* d_verdict = ar->get<uint8_t>(kSsVerdict, n);
    uint32_t* out_store = ar->get<uint32_t>(kSsOutStore, n * 4);
    uint32_t* out_entry = ar->get<uint32_t>(kSsOutEntry, n * 4);
    uint32_t* out_touch = ar->get<uint32_t>(kSsOutTouch, n * 4);
    size_t tb = 0;
    (void)exclusive_sum_u64(nullptr, &tb, nullptr, nullptr, nb + 1, st);
    void* tmp = ar->get<void>(kSsScanTmp, tb);
    hipEvent_t e0 = ar->event(0), e1 = ar->event(1);
    if (!d_dig || !ref || !flag || !counts[0] || !counts[1] || !counts[2] || !starts[0] || !starts[1] || !starts[2] ||
        !d_verdict || !out_store || !out_entry || !out_touch || !tmp)
        return PBS_ERR_NOMEM;
    if (!e0 || !e1) return PBS_ERR_HIP;
    const uint32_t count = (uint32_t)h->count;
    CallRc rc;
    unsigned long long totals[3] = {};
    (void)hipGetLastError();
    if (n) rc.ok(hipMemcpyAsync(d_dig, digests, 32 * n, hipMemcpyHostToDevice, st));
    if (rc.rc == PBS_OK) rc.ok(hipEventRecord(e0, st));
    // the growth comes first: the claim kernel needs a load <= 1/2 with every entry appended
    const uint32_t log2 = plan_log2(h->count, n, h->log2);
    if (rc.rc == PBS_OK && (log2 != h->log2 || h->stale)) {
        rc.fail(rebuild_table(h, log2));
        if (rc.rc == PBS_OK && h->stale) rc.ok(hipMemsetAsync(h->d_first, 0xFF, 4 * h->cap, st));
    }
    h->stale = true;  // (until the commit has been seen to end)
    const uint32_t shift = 64 - h->log2;
    const uint64_t mask = (1ull << h->log2) - 1;
    // (count[nb] = 0: the exclusive sum's last value is then the total)
    for (int c = 0; c < 3 && rc.rc == PBS_OK; ++c) rc.ok(hipMemsetAsync(counts[c] + nb, 0, 8, st));
    if (rc.rc == PBS_OK && n) {
        hipLaunchKernelGGL(sync_claim_kernel, dim3(nb), dim3(kGcThreads), 0, st, d_dig, (uint64_t)n, h->d_store, count,
                           h->d_table, shift, mask, h->d_first, ref);
        rc.ok(hipGetLastError());
        if (rc.rc == PBS_OK) {
            hipLaunchKernelGGL(sync_flag_kernel, dim3(nb), dim3(kGcThreads), 0, st, ref, (uint64_t)n, count, h->d_table,
                               h->d_first, h->d_present, h->d_claimed, flag, counts[0], counts[1], counts[2]);
            rc.ok(hipGetLastError());
        }
    }
    for (int c = 0; c < 3 && rc.rc == PBS_OK; ++c)
        rc.ok(exclusive_sum_u64(tmp, &tb, reinterpret_cast<const uint64_t*>(counts[c]),
                                reinterpret_cast<uint64_t*>(starts[c]), nb + 1, st));
    if (rc.rc == PBS_OK && n) {
        hipLaunchKernelGGL(sync_commit_kernel, dim3(nb), dim3(kGcThreads), 0, st, d_dig, ref, flag, (uint64_t)n, count,
                           starts[0], starts[1], starts[2], h->d_table, h->d_store, h->d_present, h->d_claimed, h->d_first,
                           d_verdict, out_store, out_entry, out_touch);
        rc.ok(hipGetLastError());
    }
    if (rc.rc == PBS_OK && rc.ok(hipEventRecord(e1, st))) {
        for (int c = 0; c < 3 && rc.rc == PBS_OK; ++c)
            rc.ok(hipMemcpyAsync(&totals[c], starts[c] + nb, 8, hipMemcpyDeviceToHost, st));
        if (rc.rc == PBS_OK) rc.ok(hipStreamSynchronize(st));
    }
    const unsigned long long n_new = totals[0], n_fetch = totals[1], n_touch = totals[2];
    if (rc.rc == PBS_OK && (n_new > n_fetch || n_fetch + n_touch > n)) rc.fail(PBS_ERR_HIP);  // (never: one flag per lane)
    if (rc.rc == PBS_OK) {
        h->stale = false;
        h->count += (size_t)n_new;  // (the entries are there, whatever becomes of the copies below)
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
        for (size_t t = 0; t < run.fetch_store.size(); ++t)
            if (run.fetch_store[t] >= h->count || run.fetch_entry[t] >= n) rc.fail(PBS_ERR_HIP);  // (never)
        for (size_t t = 0; t < run.touch_store.size(); ++t)
            if (run.touch_store[t] >= h->count) rc.fail(PBS_ERR_HIP);  // (never)
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
// changes unless every step went well.  The blob handling is pbs_verify_submit's.
int submit_on(pbs_sync* h, const uint8_t* blobs_dev, const uint64_t* blob_offsets, const uint8_t* load_failed, size_t k,
              uint8_t* kinds_out, uint8_t* status_out, pbs_sync_timing* timing) {
    const HClock::time_point t0 = HClock::now();
    IndexRun& run = h->run;
    hipStream_t st = h->st;
    pbs_sync_timing tm;
    std::memset(&tm, 0, sizeof(tm));
    tm.blobs = k;
    if (k == 0) {
        if (timing) *timing = tm;
        return PBS_OK;
    }
    const size_t item0 = run.done;
    ArenaLease ar(spool(), h->dev);
    if (!blobs_dev) {  // (k empty blobs: the decoder still wants an address)
        blobs_dev = ar->get<uint8_t>(kSsPack, 1);
        if (!blobs_dev) return PBS_ERR_NOMEM;
    }
    // the magic read: an encrypted blob is verified by its CRC alone and gets a zero-length slot
    std::vector<uint64_t> spans(2 * k);
    for (size_t t = 0; t < k; ++t) {
        spans[2 * t] = blob_offsets[t];
        spans[2 * t + 1] = load_failed && load_failed[t] ? 0 : blob_offsets[t + 1] - blob_offsets[t];
    }
    std::vector<uint8_t> enc(k, 0);
    uint64_t* d_spans = ar->get<uint64_t>(kSsSpans, 16 * k);
    uint8_t* d_enc = ar->get<uint8_t>(kSsEnc, k);
    uint32_t* d_sp = ar->get<uint32_t>(kSsPos, 4 * k);
    uint8_t* d_status = ar->get<uint8_t>(kSsStatus, k);
    hipEvent_t e0 = ar->event(0), e1 = ar->event(1), e2 = ar->event(2), e3 = ar->event(3);
    if (!d_spans || !d_enc || !d_sp || !d_status) return PBS_ERR_NOMEM;
    if (!e0 || !e1 || !e2 || !e3) return PBS_ERR_HIP;
    CallRc call;
    (void)hipGetLastError();
    if (call.ok(hipMemcpyAsync(d_spans, spans.data(), 16 * k, hipMemcpyHostToDevice, st)) && call.ok(hipEventRecord(e2, st))) {
        hipLaunchKernelGGL(verify_magic_kernel, dim3(blocks_for(k)), dim3(kGcThreads), 0, st, blobs_dev, d_spans,
                           (uint64_t)k, d_enc);
        call.ok(hipGetLastError()) && call.ok(hipEventRecord(e3, st)) &&
            call.ok(hipMemcpyAsync(enc.data(), d_enc, k, hipMemcpyDeviceToHost, st));
    }
    if (hipStreamSynchronize(st) != hipSuccess) call.fail(PBS_ERR_HIP);
    if (call.rc != PBS_OK) return call.rc;
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e2, e3);
    tm.magic_ms = ms;

    // the decoder takes blobs that follow one another: a run of items between two load failures per call
    std::vector<uint8_t> kinds(k, PBS_BLOB_KIND_NONE), status(k, PBS_SYNC_ST_LOAD_FAILED);
    std::vector<uint64_t> csz, ooff, olens;
    for (size_t a = 0; a < k;) {
        if (load_failed && load_failed[a]) {
            ++a;
            continue;
        }
        size_t b = a;
        while (b < k && !(load_failed && load_failed[b])) ++b;
        const size_t cnt = b - a;
        csz.assign(cnt, 0);
        uint64_t total = 0;
        bool plain = false;
        for (size_t t = a; t < b; ++t) {
            tm.encrypted += enc[t];
            if (enc[t]) continue;
            plain = true;
            csz[t - a] = run.fetch_sizes[item0 + t];
            if (csz[t - a] > UINT64_MAX - total) return PBS_ERR_NOMEM;
            total += csz[t - a];
        }
        if (total > SIZE_MAX) return PBS_ERR_NOMEM;
        // (an all-encrypted run takes no output scratch at all)
        uint8_t* d_out = plain ? ar->get<uint8_t>(kSsOut, (size_t)total, false) : nullptr;
        if (plain && !d_out) return PBS_ERR_NOMEM;
        ooff.assign(cnt + 1, 0);
        olens.assign(cnt, 0);
        pbs_blob_decode_inflate_timing dt;
        const int rc = pbs_blob_decode_inflate_device(blobs_dev, blob_offsets + a, cnt, nullptr,
                                                      &run.fetch_digests[32 * (item0 + a)], csz.data(), 1, d_out,
                                                      (size_t)total, ooff.data(), olens.data(), kinds.data() + a,
                                                      status.data() + a, &dt, st);
        if (rc != PBS_OK) return rc;
        tm.decode_ms += dt.base.total_ms;
        tm.decoded += cnt;
        tm.scratch_bytes += total;
        a = b;
    }
    for (size_t t = 0; t < k; ++t)
        if (status[t] == PBS_BLOB_ST_NO_CONFIG) status[t] = PBS_BLOB_ST_OK;  // verify_unencrypted: Ok for an encrypted chunk

    // insert_chunk
    if (call.ok(hipMemcpyAsync(d_sp, &run.fetch_store[item0], 4 * k, hipMemcpyHostToDevice, st)) &&
        call.ok(hipMemcpyAsync(d_status, status.data(), k, hipMemcpyHostToDevice, st)) && call.ok(hipEventRecord(e0, st))) {
        hipLaunchKernelGGL(sync_state_kernel, dim3(blocks_for(k)), dim3(kGcThreads), 0, st, d_sp, d_status, (uint64_t)k,
                           h->d_present);
        call.ok(hipGetLastError()) && call.ok(hipEventRecord(e1, st));
    }
    if (hipStreamSynchronize(st) != hipSuccess) call.fail(PBS_ERR_HIP);  // (before the arena goes back)
    if (call.rc != PBS_OK) return call.rc;
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
    h->dev = sd.dev;
    h->ncu = sd.ncu;
    h->st = st;
    h->run.clear();
    hipEvent_t e0 = nullptr, e1 = nullptr;
    CallRc rc;
    rc.fail(reserve_entries(h, std::max<size_t>(m + reserve, 1)));
    if (rc.rc == PBS_OK && m) {
        rc.ok(hipMemcpyAsync(h->d_store, store_digests, 32 * m, hipMemcpyHostToDevice, st)) &&
            rc.ok(hipMemsetAsync(h->d_present, 1, m, st)) && rc.ok(hipMemsetAsync(h->d_claimed, 0, m, st));
    }
    h->count = m;
    if (rc.rc == PBS_OK && rc.ok(hipEventCreate(&e0)) && rc.ok(hipEventCreate(&e1)) && rc.ok(hipEventRecord(e0, st)))
        rc.fail(rebuild_table(h, begin_log2(m, reserve)));
    if (rc.rc == PBS_OK && rc.ok(hipEventRecord(e1, st))) rc.ok(hipStreamSynchronize(st));
    if (rc.rc == PBS_OK && build_ms) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, e0, e1);
        *build_ms = ms;
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (rc.rc != PBS_OK) {
        free_handle(h);
        return rc.rc;
    }
    {
        Live& l = live();
        std::lock_guard<std::mutex> g(l.mu);
        l.handles.insert(h);
    }
    *out = h;
    return PBS_OK;
}

extern "C" size_t pbs_sync_count(pbs_sync* h) { return alive(h) ? h->count : 0; }

extern "C" uint32_t pbs_sync_table_log2(pbs_sync* h) { return alive(h) ? h->log2 : 0; }

extern "C" int pbs_sync_listing(pbs_sync* h, uint8_t* digests_out, uint8_t* present_out, size_t cap, size_t* count) {
    if (count) *count = 0;
    if (!alive(h)) return PBS_ERR_INVALID;
    const size_t k = std::min(cap, h->count);
    if (count) *count = h->count;
    if (k == 0 || (!digests_out && !present_out)) return PBS_OK;
    DeviceGuard dg(h->dev);
    if (!dg.ok) return PBS_ERR_NO_DEVICE;
    CallRc rc;
    if (digests_out) rc.ok(hipMemcpyAsync(digests_out, h->d_store, 32 * k, hipMemcpyDeviceToHost, h->st));
    if (present_out && rc.rc == PBS_OK) rc.ok(hipMemcpyAsync(present_out, h->d_present, k, hipMemcpyDeviceToHost, h->st));
    if (hipStreamSynchronize(h->st) != hipSuccess) rc.fail(PBS_ERR_HIP);
    return rc.rc;
}

extern "C" int pbs_sync_new_group(pbs_sync* h) {
    if (!alive(h) || h->run.open) return PBS_ERR_INVALID;
    if (h->count == 0) return PBS_OK;
    DeviceGuard dg(h->dev);
    if (!dg.ok) return PBS_ERR_NO_DEVICE;
    CallRc rc;
    rc.ok(hipMemsetAsync(h->d_claimed, 0, h->count, h->st));
    if (hipStreamSynchronize(h->st) != hipSuccess) rc.fail(PBS_ERR_HIP);
    return rc.rc;
}

extern "C" void pbs_sync_end(pbs_sync* h) {
    if (!h) return;
    {
        Live& l = live();
        std::lock_guard<std::mutex> g(l.mu);
        if (!l.handles.erase(h)) return;
    }
    free_handle(h);
}

extern "C" int pbs_sync_plan(pbs_sync* h, const uint8_t* digests, const uint64_t* sizes, size_t n, uint8_t* verdict,
                             uint32_t* fetch_store, uint32_t* fetch_entry, size_t fcap, size_t* n_fetch,
                             uint32_t* touch_store, size_t tcap, size_t* n_touch, double* plan_ms) {
    if (n_fetch) *n_fetch = 0;
    if (n_touch) *n_touch = 0;
    if (plan_ms) *plan_ms = 0;
    if (!alive(h) || h->run.open ||
        !plan_args_valid(h->count, digests, sizes, n, fetch_store, fetch_entry, fcap, n_fetch, touch_store, tcap, n_touch))
        return PBS_ERR_INVALID;
    DeviceGuard dg(h->dev);
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
    if (!alive(h) || !h->run.open || !lists_args_valid(fetch_store, fetch_entry, fcap, n_fetch, touch_store, tcap, n_touch))
        return PBS_ERR_INVALID;
    copy_lists(h->run, fetch_store, fetch_entry, fcap, n_fetch, touch_store, tcap, n_touch);
    return PBS_OK;
}

extern "C" int pbs_sync_submit(pbs_sync* h, const uint8_t* blobs_dev, const uint64_t* blob_offsets,
                               const uint8_t* load_failed, size_t k, uint8_t* kinds, uint8_t* status,
                               pbs_sync_timing* timing) {
    if (timing) std::memset(timing, 0, sizeof(*timing));
    if (!alive(h) || !submit_args_valid(h->run, blobs_dev, blob_offsets, k)) return PBS_ERR_INVALID;
    DeviceGuard dg(h->dev);
    if (!dg.ok) return PBS_ERR_NO_DEVICE;
    try {
        return submit_on(h, blobs_dev, blob_offsets, load_failed, k, kinds, status, timing);
    } catch (const std::bad_alloc&) {
        return PBS_ERR_NOMEM;
    }
}

extern "C" int pbs_sync_finish(pbs_sync* h, pbs_sync_result* res) {
    if (!alive(h) || !h->run.open || h->run.remaining() != 0) return PBS_ERR_INVALID;
    close_run(h->run, res);
    return PBS_OK;
}

extern "C" int pbs_sync_abort_index(pbs_sync* h) {
    if (!alive(h)) return PBS_ERR_INVALID;
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
    if (!alive(h) || h->run.open || !index_check || (vcap && !verdict) ||
        !lists_args_valid(fetch_store, fetch_entry, fcap, n_fetch, touch_store, tcap, n_touch))
        return PBS_ERR_INVALID;
    IndexLayout lo;
    int rc = index_layout(image, len, &lo);
    if (rc != PBS_OK) return rc;
    if (!entries_fit(h->count, lo.n)) return PBS_ERR_INVALID;
    if (n_entries) *n_entries = lo.n;
    *index_check = pbs::verify::index_check(image, lo, info_size, info_csum);
    if (*index_check != PBS_VERIFY_INDEX_OK) return PBS_OK;  // verify_archive bails: nothing is claimed
    DeviceGuard dg(h->dev);
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
