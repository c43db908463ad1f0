// The table of gc_table_dev.h over a digest list that grows, for the jobs that insert (sync,
// the backup session): the claim-or-insert kernel, the handle state with its entry arrays and
// their growth, and the sequence that appends a batch's new digests in the batch's order.  What
// a job makes of the claims (its flag and commit kernels) stays with the job.  Device code:
// include it from a .hip file only; everything is in an unnamed namespace.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "dev_arena.h"
#include "gc_table_dev.h"
#include "pbs_blob.h"
#include "pbs_chunker_internal.h"
#include "sync_common.h"

namespace pbs {
namespace gc {
namespace {

// what the claim kernel leaves per item: the entry position found, or kRefSlot and the slot the
// lane's digest sits in, or kRefNone for an item that takes no part
constexpr uint64_t kRefSlot = 1ull << 63;
constexpr uint64_t kRefNone = ~0ull;

// One lane per item of a batch: the probe of lowest_entry with an insert where it ends.
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
//    digest, and its final value is the lowest batch position, count + min i;
//  - a table read may be stale (it is a plain load; the L1 of a CU and the L2 of an XCD do not
//    see other XCDs' atomics): a slot read as free that is taken is put right by the swap, which
//    returns the occupant; an occupant read stale is another lane of the same digest;
//  - no lane waits for another lane's progress, and the table holds 2^L >= 2 (count + n) slots
//    (the growth runs before the launch), so a free slot always comes and every walk ends.
//
// first (may be NULL: no first occurrence is kept) and active (may be NULL; otherwise an item
// with active[i] != PBS_BLOB_ST_OK takes no part and gets kRefNone) are uniform over the launch.
__global__ __launch_bounds__(kGcThreads) void grow_claim_kernel(const uint8_t* __restrict__ dig, uint64_t n,
                                                                const uint8_t* __restrict__ active,
                                                                const uint8_t* __restrict__ store, uint32_t count,
                                                                uint32_t* table, uint32_t shift, uint64_t mask,
                                                                uint32_t* __restrict__ first, uint64_t* __restrict__ ref) {
    const uint64_t i = (uint64_t)blockIdx.x * kGcThreads + threadIdx.x;
    if (i >= n) return;
    if (active && active[i] != PBS_BLOB_ST_OK) {
        ref[i] = kRefNone;
        return;
    }
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
        if (first) atomicMin(&first[j], (uint32_t)i);
        ref[i] = j;
    } else {
        ref[i] = kRefSlot | s;
    }
}

// the arena slots an append works in; list c of a job counts in count0 + c and starts in start0 + c
struct GrowSlots {
    unsigned ref, count0, start0, scan_tmp;
};

// The state of a handle whose digest list grows: the digests, the table over them, and the job's
// arrays of one element per entry, which move along when the list outgrows them.
struct GrowTable {
    static constexpr int kMaxSides = 6, kMaxLists = 3;
    // one per-entry array of the job.  fill < 0: a growth copies the entries over; otherwise the
    // array holds that byte between batches, so a growth, and the rebuild after a batch that
    // failed half-way, fill all of it.
    struct Side {
        void** p;
        size_t elem;
        int fill;
    };
    int dev = 0, ncu = 0;
    hipStream_t st = nullptr;
    size_t count = 0, cap = 0;   // entries; entries the arrays hold
    uint32_t log2 = 0;
    bool stale = false;          // a batch failed half-way: table and filled arrays are rebuilt before the next one
    uint8_t* d_store = nullptr;  // 32 cap: the entries' digests
    uint32_t* d_table = nullptr; // 2^log2 entry positions, kEmpty where free
    Side sides[kMaxSides];
    int n_sides = 0;

    GrowTable() = default;
    GrowTable(const GrowTable&) = delete;  // (sides point into the owner)
    GrowTable& operator=(const GrowTable&) = delete;

    template <class T>
    void side(T** p, int fill = -1) {
        sides[n_sides++] = {reinterpret_cast<void**>(p), sizeof(T), fill};
    }

    void free_all() {
        (void)hipStreamSynchronize(st);
        if (d_store) (void)hipFree(d_store);
        for (int i = 0; i < n_sides; ++i)
            if (*sides[i].p) (void)hipFree(*sides[i].p);
        if (d_table) (void)hipFree(d_table);
    }

    // the entry arrays for at least `want` entries; what they hold moves along.  Synchronous.
    int reserve_entries(size_t want) {
        if (want <= cap) return PBS_OK;
        const size_t ncap = std::max(want, cap + cap / 2);
        void* fresh[kMaxSides + 1] = {};
        CallRc rc;
        for (int i = 0; i <= n_sides && rc.rc == PBS_OK; ++i)
            if (hipMalloc(&fresh[i], (i ? sides[i - 1].elem : 32) * ncap) != hipSuccess) {
                (void)hipGetLastError();
                rc.fail(PBS_ERR_NOMEM);
            }
        if (rc.rc == PBS_OK && count) rc.ok(hipMemcpyAsync(fresh[0], d_store, 32 * count, hipMemcpyDeviceToDevice, st));
        for (int i = 0; i < n_sides && rc.rc == PBS_OK; ++i) {
            const Side& s = sides[i];
            if (s.fill >= 0) rc.ok(hipMemsetAsync(fresh[i + 1], s.fill, s.elem * ncap, st));
            else if (count) rc.ok(hipMemcpyAsync(fresh[i + 1], *s.p, s.elem * count, hipMemcpyDeviceToDevice, st));
        }
        if (hipStreamSynchronize(st) != hipSuccess) rc.fail(PBS_ERR_HIP);
        for (int i = 0; i <= n_sides; ++i) {
            void** p = i ? sides[i - 1].p : reinterpret_cast<void**>(&d_store);
            if (rc.rc == PBS_OK) std::swap(*p, fresh[i]);
            if (fresh[i]) (void)hipFree(fresh[i]);
        }
        if (rc.rc == PBS_OK) cap = ncap;
        return rc.rc;
    }

    // The table at 2^log2v slots over all entries (gc_build_kernel), queued on the stream.  A new
    // allocation when the size changes.
    int rebuild_table(uint32_t log2v) {
        const size_t slots = (size_t)1 << log2v;
        if (log2v != log2 || !d_table) {
            uint32_t* t = nullptr;
            if (log2v >= 8 * sizeof(size_t) - 3 || hipMalloc(&t, slots * 4) != hipSuccess) {
                (void)hipGetLastError();
                return PBS_ERR_NOMEM;
            }
            if (d_table) {
                (void)hipStreamSynchronize(st);
                (void)hipFree(d_table);
            }
            d_table = t;
            log2 = log2v;
        }
        CallRc rc;
        (void)hipGetLastError();
        if (rc.ok(hipMemsetAsync(d_table, 0xFF, slots * 4, st)) && count) {
            hipLaunchKernelGGL(gc_build_kernel, dim3(blocks_for(count)), dim3(kGcThreads), 0, st, d_store, (uint64_t)count,
                               d_table, 64 - log2v, (uint64_t)slots - 1);
            rc.ok(hipGetLastError());
        }
        return rc.rc;
    }

    // after a batch that failed half-way: the table holds provisional values and the filled
    // arrays what the batch left in them.  Queued on the stream.
    int rebuild_stale(uint32_t log2v) {
        CallRc rc;
        rc.fail(rebuild_table(log2v));
        for (int i = 0; i < n_sides && rc.rc == PBS_OK; ++i)
            if (sides[i].fill >= 0) rc.ok(hipMemsetAsync(*sides[i].p, sides[i].fill, sides[i].elem * cap, st));
        return rc.rc;
    }

    // begin: room for m + reserve entries, the listing's digests, the job's own first values of
    // its arrays for the m entries (upload_sides(rc), queued on the stream), then the table's
    // build, timed by HIP events into *build_ms (may be NULL).  Synchronous.
    template <class Upload>
    int begin(const StreamDevice& sd, hipStream_t stream, const uint8_t* store_digests, size_t m, size_t reserve,
              double* build_ms, Upload upload_sides) {
        dev = sd.dev;
        ncu = sd.ncu;
        st = stream;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        CallRc rc;
        rc.fail(reserve_entries(std::max<size_t>(m + reserve, 1)));
        if (rc.rc == PBS_OK && m && rc.ok(hipMemcpyAsync(d_store, store_digests, 32 * m, hipMemcpyHostToDevice, st)))
            upload_sides(rc);
        count = m;
        if (rc.rc == PBS_OK && rc.ok(hipEventCreate(&e0)) && rc.ok(hipEventCreate(&e1)) && rc.ok(hipEventRecord(e0, st)))
            rc.fail(rebuild_table(sync::begin_log2(m, reserve)));
        if (rc.rc == PBS_OK && rc.ok(hipEventRecord(e1, st))) rc.ok(hipStreamSynchronize(st));
        if (rc.rc == PBS_OK && build_ms) {
            float ms = 0;
            (void)hipEventElapsedTime(&ms, e0, e1);
            *build_ms = ms;
        }
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        return rc.rc;
    }

    // What an append of n items with `lists` lists allocates: n more entries and the arena slots.
    // append calls it first; a caller that times its batch calls it before the timed part (it
    // waits for the stream when the arrays grow), and append's own call then finds all in place.
    int append_room(DevArena& ar, const GrowSlots& sl, size_t n, int lists) {
        const int r = reserve_entries(count + n);
        if (r != PBS_OK) return r;
        const size_t words = (size_t)blocks_for(n) + 1;
        size_t tb = 0;
        (void)exclusive_sum_u64(nullptr, &tb, nullptr, nullptr, (uint32_t)words, st);
        bool have = ar.get<uint64_t>(sl.ref, 8 * n) && ar.get<void>(sl.scan_tmp, tb);
        for (int c = 0; c < lists; ++c)
            have = have && ar.get<void>(sl.count0 + c, words * 8) && ar.get<void>(sl.start0 + c, words * 8);
        return have ? PBS_OK : PBS_ERR_NOMEM;
    }

    // A batch of n items (d_dig: their digests, device) against the list: every digest that is
    // not listed is appended, in the order of its lowest item.
    //   room for n more entries (append_room);
    //   the growth per sync::plan_log2, or the rebuild after a batch that failed half-way -- before
    //   the claim launch, which needs a load <= 1/2 with every item appended;
    //   stale, until the commit has been seen to end;
    //   the claim kernel with `count` as it is at the launch (first, active: see there);
    //   flag(ref, count, counts): the job's kernel that leaves per block, for each of its `lists`
    //   lists, the count of the lanes that go there (list 0: the lanes that append);
    //   the exclusive sums of the counts;
    //   commit(ref, count, starts): the job's kernel that gives an appending lane the entry
    //   position count + its rank in list 0, writes it over the provisional table value and
    //   fills the entry, and whatever the job queues right behind it; `committed` (may be NULL)
    //   is recorded there;
    //   the lists' totals read back into totals[]; count advances by totals[0].
    // flag and commit launch on the stream and return a hipError_t.  Synchronous.
    template <class Flag, class Commit>
    int append(DevArena& ar, const GrowSlots& sl, const uint8_t* d_dig, const uint8_t* active, uint32_t* first, size_t n,
               int lists, unsigned long long* totals, Flag flag, Commit commit,
               hipEvent_t committed = nullptr) {
        const int r = append_room(ar, sl, n, lists);
        if (r != PBS_OK) return r;
        const unsigned nb = blocks_for(n);
        uint64_t* ref = ar.get<uint64_t>(sl.ref, 8 * n);
        unsigned long long* counts[kMaxLists] = {};
        unsigned long long* starts[kMaxLists] = {};
        for (int c = 0; c < lists; ++c) {
            counts[c] = ar.get<unsigned long long>(sl.count0 + c, ((size_t)nb + 1) * 8);
            starts[c] = ar.get<unsigned long long>(sl.start0 + c, ((size_t)nb + 1) * 8);
            totals[c] = 0;
        }
        size_t tb = 0;
        (void)exclusive_sum_u64(nullptr, &tb, nullptr, nullptr, nb + 1, st);
        void* tmp = ar.get<void>(sl.scan_tmp, tb);
        CallRc rc;
        (void)hipGetLastError();
        const uint32_t want = sync::plan_log2(count, n, log2);
        if (want != log2 || stale) rc.fail(stale ? rebuild_stale(want) : rebuild_table(want));
        stale = true;  // (until the commit has been seen to end)
        const uint32_t at = (uint32_t)count, shift = 64 - log2;
        const uint64_t mask = (1ull << log2) - 1;
        // (count[nb] = 0: the exclusive sum's last value is then the total)
        for (int c = 0; c < lists && rc.rc == PBS_OK; ++c) rc.ok(hipMemsetAsync(counts[c] + nb, 0, 8, st));
        if (rc.rc == PBS_OK && n) {
            hipLaunchKernelGGL(grow_claim_kernel, dim3(nb), dim3(kGcThreads), 0, st, d_dig, (uint64_t)n, active, d_store, at,
                               d_table, shift, mask, first, ref);
            rc.ok(hipGetLastError()) && rc.ok(flag(ref, at, counts));
        }
        for (int c = 0; c < lists && rc.rc == PBS_OK; ++c)
            rc.ok(exclusive_sum_u64(tmp, &tb, reinterpret_cast<const uint64_t*>(counts[c]),
                                    reinterpret_cast<uint64_t*>(starts[c]), nb + 1, st));
        if (rc.rc == PBS_OK && n) rc.ok(commit(ref, at, starts));
        if (rc.rc == PBS_OK && committed) rc.ok(hipEventRecord(committed, st));
        for (int c = 0; c < lists && rc.rc == PBS_OK; ++c)
            rc.ok(hipMemcpyAsync(&totals[c], starts[c] + nb, 8, hipMemcpyDeviceToHost, st));
        if (hipStreamSynchronize(st) != hipSuccess) rc.fail(PBS_ERR_HIP);
        for (int c = 0; c < lists && rc.rc == PBS_OK; ++c)
            if (totals[c] > n) rc.fail(PBS_ERR_HIP);  // (never: one flag per lane and list)
        if (rc.rc != PBS_OK) return rc.rc;
        stale = false;
        count += (size_t)totals[0];  // (the entries are there, whatever becomes of the caller's copies)
        return PBS_OK;
    }
};

}  // namespace
}  // namespace gc
}  // namespace pbs
