// Device side of the backup session (include/pbs_backup.h; DESIGN.md section 10, "Backup
// session"): the store's listing as the growing table of grow_table_dev.h,
// with the file's state (present, length, magic) and this session's known_chunks (known, length)
// per entry.  Three kinds of batch run on it:
//   register   probe or insert (the claim and ordered append of grow_table_dev.h), then the highest index
//              position of each digest writes known / known_size;
//   upload     the blobs go through the blob verdict of verify_dev.h with the CRC computed and not
//              judged; the good ones probe or insert; (entry, t) keys are sorted by entry with the
//              stable radix sort of pbs_sort.hip and the first lane of each group walks its items
//              in ascending t through insert_chunk's rule; a scan counts the fixed writer's
//              small chunks; the highest registered t of each entry writes known / known_size;
//   append     probe, gather of known_size, a 64-bit exclusive scan, the comparison with the
//              offsets (or the alignment rule of the fixed index), a minimum over the failing i.
// The writers, the counters and the closes are backup_common.h's, on the host.
//
// Like sync this path is bound by the latency of random reads, so every kernel is one lane per
// item in 256-thread blocks with few registers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "backup_common.h"
#include "dev_arena.h"
#include "gc_common.h"
#include "gc_table_dev.h"
#include "grow_table_dev.h"
#include "pbs_backup.h"
#include "pbs_blob.h"
#include "pbs_chunker.h"
#include "pbs_chunker_internal.h"
#include "sync_common.h"
#include "verify_common.h"
#include "verify_dev.h"

namespace pbs {
namespace backup {
namespace {

using namespace pbs::gc;
using pbs::verify::blob_verdicts;
using pbs::verify::BlobSlots;
using pbs::verify::BlobTiming;

constexpr uint64_t kKeyNone = ~0ull;

// (grow_claim_kernel, the probe with an insert where it ends: grow_table_dev.h)

// after the claim kernel has ended: who appends (the lowest lane of a new digest), and the
// block's count of them
__global__ __launch_bounds__(kGcThreads) void bk_flag_kernel(const uint64_t* __restrict__ ref, uint64_t n, uint32_t count,
                                                             const uint32_t* __restrict__ table,
                                                             uint8_t* __restrict__ fresh,
                                                             unsigned long long* __restrict__ block_new) {
    __shared__ uint32_t wcnt[kGcWaves];
    const uint64_t i = (uint64_t)blockIdx.x * kGcThreads + threadIdx.x;
    bool f = false;
    if (i < n) {
        const uint64_t r = ref[i];
        f = r != kRefNone && (r & kRefSlot) && table[r & ~kRefSlot] == count + (uint32_t)i;
        fresh[i] = f;
    }
    const uint32_t c = block_count(f, wcnt);
    if (threadIdx.x == 0) block_new[blockIdx.x] = c;
}

// An appending lane gets the entry position count + its rank among the appending lanes (the
// order the sequential rule meets new digests), writes it over its provisional table value,
// copies its digest there and clears the entry's state.  One writer per word.
__global__ __launch_bounds__(kGcThreads) void bk_commit_kernel(
    const uint8_t* __restrict__ dig, const uint64_t* __restrict__ ref, const uint8_t* __restrict__ fresh, uint64_t n,
    uint32_t count, const unsigned long long* __restrict__ start_new, uint32_t* __restrict__ table,
    uint8_t* __restrict__ store, uint8_t* __restrict__ present, uint64_t* __restrict__ size, uint8_t* __restrict__ kind,
    uint8_t* __restrict__ known, uint32_t* __restrict__ ksize) {
    __shared__ uint32_t wcnt[kGcWaves];
    const uint64_t i = (uint64_t)blockIdx.x * kGcThreads + threadIdx.x;
    const bool f = i < n && fresh[i];
    const uint64_t rank = ordered_rank(f, start_new[blockIdx.x], wcnt);
    if (!f) return;
    const uint32_t c = count + (uint32_t)rank;
    table[ref[i] & ~kRefSlot] = c;
    const uint64_t* src = reinterpret_cast<const uint64_t*>(dig + 32 * i);
    uint64_t* dst = reinterpret_cast<uint64_t*>(store + 32ull * c);
    dst[0] = src[0];
    dst[1] = src[1];
    dst[2] = src[2];
    dst[3] = src[3];
    present[c] = 0;
    size[c] = 0;
    kind[c] = PBS_BLOB_KIND_NONE;
    known[c] = 0;
    ksize[c] = 0;
}

// after the commit has ended: every item's entry position (kEmpty: no part in the batch)
__global__ __launch_bounds__(kGcThreads) void bk_pos_kernel(const uint64_t* __restrict__ ref, uint64_t n,
                                                            const uint32_t* __restrict__ table,
                                                            uint32_t* __restrict__ pos) {
    const uint64_t i = (uint64_t)blockIdx.x * kGcThreads + threadIdx.x;
    if (i >= n) return;
    const uint64_t r = ref[i];
    pos[i] = r == kRefNone ? kEmpty : (r & kRefSlot) ? table[r & ~kRefSlot] : (uint32_t)r;
}

// known_chunks.insert in ascending i: the highest i of an entry is what stays.  mark[] is zero
// between batches; ok (may be NULL): only items with ok[i] == PBS_BACKUP_REG_OK take part.
__global__ __launch_bounds__(kGcThreads) void bk_mark_kernel(const uint32_t* __restrict__ pos,
                                                             const uint8_t* __restrict__ ok, uint64_t n, uint32_t* mark) {
    const uint64_t i = (uint64_t)blockIdx.x * kGcThreads + threadIdx.x;
    if (i >= n || pos[i] == kEmpty || (ok && ok[i] != PBS_BACKUP_REG_OK)) return;
    atomicMax(&mark[pos[i]], (uint32_t)i + 1);
}
// (a lane that is not the highest reads the highest's i + 1 or the 0 it leaves: neither is its own)
__global__ __launch_bounds__(kGcThreads) void bk_known_kernel(const uint32_t* __restrict__ pos,
                                                              const uint8_t* __restrict__ ok,
                                                              const uint32_t* __restrict__ sizes, uint64_t n,
                                                              uint32_t* mark, uint8_t* __restrict__ known,
                                                              uint32_t* __restrict__ ksize) {
    const uint64_t i = (uint64_t)blockIdx.x * kGcThreads + threadIdx.x;
    if (i >= n || pos[i] == kEmpty || (ok && ok[i] != PBS_BACKUP_REG_OK)) return;
    const uint32_t c = pos[i];
    if (mark[c] != (uint32_t)i + 1) return;
    known[c] = 1;
    ksize[c] = sizes[i];
    mark[c] = 0;
}

// (entry, t) as one key, the entry in the bits from tb up: the stable sort over those bits
// leaves each entry's items together in ascending t
__global__ __launch_bounds__(kGcThreads) void bk_key_kernel(const uint32_t* __restrict__ pos, uint64_t k, uint32_t tb,
                                                            uint64_t* __restrict__ keys) {
    const uint64_t t = (uint64_t)blockIdx.x * kGcThreads + threadIdx.x;
    if (t >= k) return;
    keys[t] = pos[t] == kEmpty ? kKeyNone : ((uint64_t)pos[t] << tb) | t;
}

// One lane per sorted key; the first lane of each entry's group walks the group: insert_chunk
// item after item, as if the uploads had arrived one after the other.  Only that lane touches the
// entry's state, and every item is written by one lane.
__global__ __launch_bounds__(kGcThreads) void bk_walk_kernel(
    const uint64_t* __restrict__ sorted, uint64_t k, uint32_t tb, const uint8_t* __restrict__ kinds,
    const uint32_t* __restrict__ lens, uint8_t* __restrict__ present, uint64_t* __restrict__ size,
    uint8_t* __restrict__ kind, uint8_t* __restrict__ ins, uint8_t* __restrict__ action, uint8_t* __restrict__ dup,
    uint32_t* __restrict__ comp) {
    const uint64_t r = (uint64_t)blockIdx.x * kGcThreads + threadIdx.x;
    if (r >= k) return;
    const uint64_t key = sorted[r];
    if (key == kKeyNone) return;
    const uint64_t c = key >> tb;
    if (r > 0 && sorted[r - 1] != kKeyNone && (sorted[r - 1] >> tb) == c) return;
    EntryState e{size[c], present[c], kind[c]};
    const uint64_t tmask = (1ull << tb) - 1;
    for (uint64_t q = r; q < k; ++q) {
        const uint64_t kq = sorted[q];
        if (kq == kKeyNone || (kq >> tb) != c) break;
        const uint64_t t = kq & tmask;
        if (t >= k) break;  // (never: t is a lane number of the key kernel)
        uint8_t a, d;
        uint32_t cs;
        ins[t] = insert_step(e, lens[t], kinds[t], &a, &d, &cs);
        action[t] = a;
        dup[t] = d;
        comp[t] = cs;
    }
    present[c] = e.present;
    size[c] = e.size;
    kind[c] = e.kind;
}

// the fixed writer's small chunks, one flag per item (lane k: the scan's closing zero)
__global__ __launch_bounds__(kGcThreads) void bk_small_kernel(const uint8_t* __restrict__ ins,
                                                              const uint32_t* __restrict__ sizes, uint64_t k, int fixed,
                                                              uint64_t chunk_size, uint64_t* __restrict__ small) {
    const uint64_t t = (uint64_t)blockIdx.x * kGcThreads + threadIdx.x;
    if (t > k) return;
    small[t] = t < k && fixed && ins_ok(ins[t]) && sizes[t] < chunk_size;
}

// register_fixed_chunk / register_dynamic_chunk: ex[t] small chunks came before item t
__global__ __launch_bounds__(kGcThreads) void bk_register_kernel(const uint8_t* __restrict__ ins,
                                                                 const uint32_t* __restrict__ sizes,
                                                                 const uint64_t* __restrict__ small,
                                                                 const uint64_t* __restrict__ ex, uint64_t k, int fixed,
                                                                 uint64_t chunk_size, uint64_t small_before,
                                                                 uint8_t* __restrict__ reg) {
    const uint64_t t = (uint64_t)blockIdx.x * kGcThreads + threadIdx.x;
    if (t >= k) return;
    reg[t] = ins_ok(ins[t]) ? register_rule(fixed != 0, chunk_size, sizes[t], small_before + ex[t] + small[t])
                            : (uint8_t)PBS_BACKUP_REG_NONE;
}

// One lane per appended digest: the probe (lowest_entry: the lowest entry carrying it), then
// known_chunks: len[i] = known_size or 0, kn[i] = known.  Lane n writes the scan's closing zero.
// No kernel changes the table while this one runs, so plain loads do.
__global__ __launch_bounds__(kGcThreads) void bk_probe_kernel(const uint8_t* __restrict__ dig, uint64_t n,
                                                              const uint8_t* __restrict__ store,
                                                              const uint32_t* __restrict__ table, uint32_t shift,
                                                              uint64_t mask, const uint8_t* __restrict__ known,
                                                              const uint32_t* __restrict__ ksize,
                                                              uint64_t* __restrict__ len, uint8_t* __restrict__ kn) {
    const uint64_t i = (uint64_t)blockIdx.x * kGcThreads + threadIdx.x;
    if (i > n) return;
    if (i == n) {
        len[n] = 0;
        return;
    }
    const uint32_t j = lowest_entry(table, store, load_digest(dig + 32 * i), shift, mask);
    const bool is_known = j != kEmpty && known[j];
    kn[i] = is_known;
    len[i] = is_known ? ksize[j] : 0;
}

// dynamic_writer_append_chunk for every i at once: ex[i] is the sum of the lengths before i, which
// is the writer's offset at i if nothing failed before i -- and the lowest failing i is all that
// is read of the failures.
__global__ __launch_bounds__(kGcThreads) void bk_dynamic_check_kernel(const uint8_t* __restrict__ kn,
                                                                      const uint64_t* __restrict__ len,
                                                                      const uint64_t* __restrict__ ex,
                                                                      const uint64_t* __restrict__ offsets, uint64_t n,
                                                                      uint64_t start, uint64_t* __restrict__ ends,
                                                                      int* __restrict__ code,
                                                                      unsigned long long* first) {
    const uint64_t i = (uint64_t)blockIdx.x * kGcThreads + threadIdx.x;
    if (i >= n) return;
    const uint64_t at = start + ex[i];
    const int c = dynamic_append_code(kn[i] != 0, offsets[i], at);
    code[i] = c;
    ends[i] = at + len[i];
    if (c != PBS_BACKUP_E_NONE) atomicMin(first, (unsigned long long)i);
}

// fixed_writer_append_chunk for every i at once: nothing carries over from one entry to the next
__global__ __launch_bounds__(kGcThreads) void bk_fixed_check_kernel(const uint8_t* __restrict__ kn,
                                                                    const uint64_t* __restrict__ len,
                                                                    const uint64_t* __restrict__ offsets, uint64_t n,
                                                                    uint64_t size, uint64_t chunk_size,
                                                                    uint64_t index_length, uint64_t* __restrict__ idx,
                                                                    int* __restrict__ code, unsigned long long* first) {
    const uint64_t i = (uint64_t)blockIdx.x * kGcThreads + threadIdx.x;
    if (i >= n) return;
    uint64_t at = 0;
    const int c = fixed_append_code(kn[i] != 0, (uint32_t)len[i], offsets[i], size, chunk_size, index_length, &at);
    code[i] = c;
    idx[i] = at;
    if (c != PBS_BACKUP_E_NONE) atomicMin(first, (unsigned long long)i);
}

ArenaPool& bpool() {
    static ArenaPool* p = new ArenaPool;  // never destroyed (HIP may be torn down first at exit)
    return *p;
}

enum BSlot : unsigned { kBsDig, kBsRef, kBsFresh, kBsCount, kBsStart, kBsScanTmp, kBsPos, kBsSizes, kBsStatus, kBsKinds,
                        kBsLens, kBsKeys, kBsSorted, kBsSortTmp, kBsIns, kBsAction, kBsDup, kBsComp, kBsReg, kBsSmall,
                        kBsEx, kBsKn, kBsOffsets, kBsOut64, kBsCode, kBsFirst, kBsSpans, kBsEnc, kBsOut, kBsPack };

inline uint32_t bits_for(uint64_t v) {  // the smallest b with 2^b > v
    uint32_t b = 0;
    while (b < 64 && (1ull << b) <= v) ++b;
    return b;
}

constexpr GrowSlots kGrowSlots = {kBsRef, kBsCount, kBsStart, kBsScanTmp};
constexpr BlobSlots kBlobSlots = {kBsSpans, kBsEnc, kBsOut, kBsPack};

struct DevEntries {
    GrowTable tab;                 // the entries' digests and the table over them
    double last_ms = 0;            // the kernels of the last register or append, by HIP events (the copies outside)
    uint8_t* d_present = nullptr;  // cap
    uint8_t* d_kind = nullptr;     // cap
    uint8_t* d_known = nullptr;    // cap
    uint64_t* d_size = nullptr;    // cap
    uint32_t* d_ksize = nullptr;   // cap
    uint32_t* d_mark = nullptr;    // cap: zero between batches

    DevEntries() {
        tab.side(&d_present);
        tab.side(&d_kind);
        tab.side(&d_known);
        tab.side(&d_size);
        tab.side(&d_ksize);
        tab.side(&d_mark, 0);
    }
    size_t count() const { return tab.count; }
    uint32_t log2() const { return tab.log2; }

    // A batch of n items against the list (GrowTable::append with one list: the digests that
    // are appended), then the items' entry positions into pos (device, n).  d_dig: the batch's
    // digests (device); active: NULL or the items' status (device).
    int resolve(DevArena& ar, const uint8_t* d_dig, const uint8_t* active, size_t n, uint32_t* pos) {
        const unsigned nb = blocks_for(n);
        uint8_t* fresh = ar.get<uint8_t>(kBsFresh, n);
        if (!fresh) return PBS_ERR_NOMEM;
        hipStream_t st = tab.st;
        unsigned long long total = 0;
        return tab.append(
            ar, kGrowSlots, d_dig, active, nullptr, n, 1, &total,
            [&](const uint64_t* ref, uint32_t count, unsigned long long* const* counts) {
                hipLaunchKernelGGL(bk_flag_kernel, dim3(nb), dim3(kGcThreads), 0, st, ref, (uint64_t)n, count, tab.d_table,
                                   fresh, counts[0]);
                return hipGetLastError();
            },
            [&](const uint64_t* ref, uint32_t count, unsigned long long* const* starts) {
                hipLaunchKernelGGL(bk_commit_kernel, dim3(nb), dim3(kGcThreads), 0, st, d_dig, ref, fresh, (uint64_t)n, count,
                                   starts[0], tab.d_table, tab.d_store, d_present, d_size, d_kind, d_known, d_ksize);
                hipLaunchKernelGGL(bk_pos_kernel, dim3(nb), dim3(kGcThreads), 0, st, ref, (uint64_t)n, tab.d_table, pos);
                return hipGetLastError();
            });
    }

    int listing(uint8_t* d, uint8_t* p, uint64_t* s, uint8_t* k, uint8_t* kn, uint32_t* ks, size_t n) {
        hipStream_t st = tab.st;
        CallRc rc;
        if (d) rc.ok(hipMemcpyAsync(d, tab.d_store, 32 * n, hipMemcpyDeviceToHost, st));
        if (p && rc.rc == PBS_OK) rc.ok(hipMemcpyAsync(p, d_present, n, hipMemcpyDeviceToHost, st));
        if (s && rc.rc == PBS_OK) rc.ok(hipMemcpyAsync(s, d_size, 8 * n, hipMemcpyDeviceToHost, st));
        if (k && rc.rc == PBS_OK) rc.ok(hipMemcpyAsync(k, d_kind, n, hipMemcpyDeviceToHost, st));
        if (kn && rc.rc == PBS_OK) rc.ok(hipMemcpyAsync(kn, d_known, n, hipMemcpyDeviceToHost, st));
        if (ks && rc.rc == PBS_OK) rc.ok(hipMemcpyAsync(ks, d_ksize, 4 * n, hipMemcpyDeviceToHost, st));
        if (hipStreamSynchronize(st) != hipSuccess) rc.fail(PBS_ERR_HIP);
        return rc.rc;
    }

    static double elapsed(hipEvent_t e0, hipEvent_t e1) {
        float f = 0;
        (void)hipEventElapsedTime(&f, e0, e1);
        return f;
    }

    // the probe of n digests (host): len (n + 1) and kn (n) stay in the arena; `after_copy` (may
    // be NULL) is recorded between the upload and the kernel
    int probe(DevArena& ar, const uint8_t* digests, size_t n, uint64_t** len, uint8_t** kn, hipEvent_t after_copy = nullptr) {
        hipStream_t st = tab.st;
        uint8_t* d_dig = ar.get<uint8_t>(kBsDig, 32 * n);
        *len = ar.get<uint64_t>(kBsLens, 8 * (n + 1));
        *kn = ar.get<uint8_t>(kBsKn, n);
        if (!d_dig || !*len || !*kn) return PBS_ERR_NOMEM;
        CallRc rc;
        (void)hipGetLastError();
        if (tab.stale) {  // (a batch failed half-way: the table holds provisional values)
            if (!rc.fail(tab.rebuild_stale(tab.log2))) return rc.rc;
            tab.stale = false;
        }
        if (rc.ok(hipMemcpyAsync(d_dig, digests, 32 * n, hipMemcpyHostToDevice, st)) &&
            (!after_copy || rc.ok(hipEventRecord(after_copy, st)))) {
            hipLaunchKernelGGL(bk_probe_kernel, dim3(blocks_for(n + 1)), dim3(kGcThreads), 0, st, d_dig, (uint64_t)n, tab.d_store,
                               tab.d_table, 64 - tab.log2, (1ull << tab.log2) - 1, d_known, d_ksize, *len, *kn);
            rc.ok(hipGetLastError());
        }
        return rc.rc;
    }

    int lookup(const uint8_t* digest, bool* is_known, uint32_t* sz) {
        hipStream_t st = tab.st;
        ArenaLease ar(bpool(), tab.dev);
        uint64_t* len = nullptr;
        uint8_t* kn = nullptr;
        CallRc rc;
        uint64_t hl = 0;
        uint8_t hk = 0;
        rc.fail(probe(*ar, digest, 1, &len, &kn)) && rc.ok(hipMemcpyAsync(&hl, len, 8, hipMemcpyDeviceToHost, st)) &&
            rc.ok(hipMemcpyAsync(&hk, kn, 1, hipMemcpyDeviceToHost, st));
        if (hipStreamSynchronize(st) != hipSuccess) rc.fail(PBS_ERR_HIP);  // (before the arena goes back)
        *is_known = hk != 0;
        *sz = (uint32_t)hl;
        return rc.rc;
    }

    int register_previous(const uint8_t* digests, const uint32_t* sizes, size_t n) {
        hipStream_t st = tab.st;
        ArenaLease ar(bpool(), tab.dev);
        uint8_t* d_dig = ar->get<uint8_t>(kBsDig, 32 * n);
        uint32_t* d_sizes = ar->get<uint32_t>(kBsSizes, 4 * n);
        uint32_t* pos = ar->get<uint32_t>(kBsPos, 4 * n);
        hipEvent_t e0 = ar->event(0), e1 = ar->event(1);
        if (!d_dig || !d_sizes || !pos) return PBS_ERR_NOMEM;
        if (!e0 || !e1) return PBS_ERR_HIP;
        CallRc rc;
        (void)hipGetLastError();
        rc.ok(hipMemcpyAsync(d_dig, digests, 32 * n, hipMemcpyHostToDevice, st)) &&
            rc.ok(hipMemcpyAsync(d_sizes, sizes, 4 * n, hipMemcpyHostToDevice, st)) && rc.ok(hipEventRecord(e0, st)) &&
            rc.fail(resolve(*ar, d_dig, nullptr, n, pos));
        if (rc.rc == PBS_OK) {
            const unsigned nb = blocks_for(n);
            hipLaunchKernelGGL(bk_mark_kernel, dim3(nb), dim3(kGcThreads), 0, st, pos, (const uint8_t*)nullptr, (uint64_t)n,
                               d_mark);
            hipLaunchKernelGGL(bk_known_kernel, dim3(nb), dim3(kGcThreads), 0, st, pos, (const uint8_t*)nullptr, d_sizes,
                               (uint64_t)n, d_mark, d_known, d_ksize);
            rc.ok(hipGetLastError()) && rc.ok(hipEventRecord(e1, st));
        }
        if (hipStreamSynchronize(st) != hipSuccess) rc.fail(PBS_ERR_HIP);  // (before the arena goes back)
        if (rc.rc == PBS_OK) last_ms = elapsed(e0, e1);
        return rc.rc;
    }

    // the blob verdict of verify_dev.h with the CRC handed out instead of judged
    int verdicts(const uint8_t* blobs_dev, const uint64_t* off, const uint8_t* digests, const uint32_t* sizes, size_t k,
                 const uint8_t* pre, uint8_t* kinds, uint8_t* status, uint32_t* crc, pbs_backup_timing* tm) {
        ArenaLease ar(bpool(), tab.dev);
        BlobTiming bt;
        // (sizes: <= 16 MiB each, the schema check came first)
        const int rc = blob_verdicts(*ar, kBlobSlots, tab.st, blobs_dev, off, pre, digests,
                                     [&](size_t t) -> uint64_t { return sizes[t]; }, k, kinds, status, crc, &bt);
        tm->decode_ms += bt.decode_ms;
        tm->decoded += bt.decoded;
        tm->encrypted += bt.encrypted;
        tm->scratch_bytes += bt.scratch_bytes;
        return rc;
    }

    int insert_batch(const uint8_t* digests, const uint8_t* status, const uint8_t* kinds, const uint32_t* lens,
                     const uint32_t* sizes, size_t k, bool fixed, uint64_t chunk_size, uint64_t small_before, uint8_t* ins,
                     uint8_t* action, uint8_t* dup, uint32_t* comp, uint8_t* reg, double* ms) {
        hipStream_t st = tab.st;
        ArenaLease ar(bpool(), tab.dev);
        const unsigned nb = blocks_for(k), nb1 = blocks_for(k + 1);
        // the key's layout: t in the low tb bits, the entry above; the refused items' key is all ones
        const uint32_t tb = std::max<uint32_t>(1, bits_for(k - 1)), pb = bits_for((uint64_t)tab.count + k);
        size_t sort_b = 0, scan_b = 0;
        (void)radix_sort(nullptr, &sort_b, nullptr, nullptr, nullptr, nullptr, k, (int)tb, (int)(tb + pb), st);
        (void)exclusive_sum_u64(nullptr, &scan_b, nullptr, nullptr, (uint32_t)(k + 1), st);
        uint8_t* d_dig = ar->get<uint8_t>(kBsDig, 32 * k);
        uint8_t* d_status = ar->get<uint8_t>(kBsStatus, k);
        uint8_t* d_kinds = ar->get<uint8_t>(kBsKinds, k);
        uint32_t* d_lens = ar->get<uint32_t>(kBsOffsets, 4 * k);
        uint32_t* d_sizes = ar->get<uint32_t>(kBsSizes, 4 * k);
        uint32_t* pos = ar->get<uint32_t>(kBsPos, 4 * k);
        uint64_t* keys = ar->get<uint64_t>(kBsKeys, 8 * k);
        uint64_t* sorted = ar->get<uint64_t>(kBsSorted, 8 * k);
        void* sort_tmp = ar->get<void>(kBsSortTmp, sort_b);
        uint8_t* d_ins = ar->get<uint8_t>(kBsIns, k);
        uint8_t* d_action = ar->get<uint8_t>(kBsAction, k);
        uint8_t* d_dup = ar->get<uint8_t>(kBsDup, k);
        uint32_t* d_comp = ar->get<uint32_t>(kBsComp, 4 * k);
        uint8_t* d_reg = ar->get<uint8_t>(kBsReg, k);
        uint64_t* small = ar->get<uint64_t>(kBsSmall, 8 * (k + 1));
        uint64_t* ex = ar->get<uint64_t>(kBsEx, 8 * (k + 1));
        void* scan_tmp = ar->get<void>(kBsOut64, scan_b);
        hipEvent_t e0 = ar->event(0), e1 = ar->event(1);
        if (!d_dig || !d_status || !d_kinds || !d_lens || !d_sizes || !pos || !keys || !sorted || !sort_tmp || !d_ins ||
            !d_action || !d_dup || !d_comp || !d_reg || !small || !ex || !scan_tmp)
            return PBS_ERR_NOMEM;
        if (!e0 || !e1) return PBS_ERR_HIP;
        CallRc rc;
        (void)hipGetLastError();
        rc.ok(hipMemcpyAsync(d_dig, digests, 32 * k, hipMemcpyHostToDevice, st)) &&
            rc.ok(hipMemcpyAsync(d_status, status, k, hipMemcpyHostToDevice, st)) &&
            rc.ok(hipMemcpyAsync(d_kinds, kinds, k, hipMemcpyHostToDevice, st)) &&
            rc.ok(hipMemcpyAsync(d_lens, lens, 4 * k, hipMemcpyHostToDevice, st)) &&
            rc.ok(hipMemcpyAsync(d_sizes, sizes, 4 * k, hipMemcpyHostToDevice, st)) &&
            rc.ok(hipMemsetAsync(d_ins, 0, k, st)) && rc.ok(hipMemsetAsync(d_action, 0, k, st)) &&
            rc.ok(hipMemsetAsync(d_dup, 0, k, st)) && rc.ok(hipMemsetAsync(d_comp, 0, 4 * k, st)) &&
            rc.ok(hipEventRecord(e0, st)) && rc.fail(resolve(*ar, d_dig, d_status, k, pos));
        if (rc.rc == PBS_OK) {
            hipLaunchKernelGGL(bk_key_kernel, dim3(nb), dim3(kGcThreads), 0, st, pos, (uint64_t)k, tb, keys);
            rc.ok(hipGetLastError()) &&
                rc.ok(radix_sort(sort_tmp, &sort_b, keys, sorted, nullptr, nullptr, k, (int)tb, (int)(tb + pb), st));
        }
        if (rc.rc == PBS_OK) {
            hipLaunchKernelGGL(bk_walk_kernel, dim3(nb), dim3(kGcThreads), 0, st, sorted, (uint64_t)k, tb, d_kinds, d_lens,
                               d_present, d_size, d_kind, d_ins, d_action, d_dup, d_comp);
            hipLaunchKernelGGL(bk_small_kernel, dim3(nb1), dim3(kGcThreads), 0, st, d_ins, d_sizes, (uint64_t)k,
                               fixed ? 1 : 0, chunk_size, small);
            rc.ok(hipGetLastError()) && rc.ok(exclusive_sum_u64(scan_tmp, &scan_b, small, ex, (uint32_t)(k + 1), st));
        }
        if (rc.rc == PBS_OK) {
            hipLaunchKernelGGL(bk_register_kernel, dim3(nb), dim3(kGcThreads), 0, st, d_ins, d_sizes, small, ex, (uint64_t)k,
                               fixed ? 1 : 0, chunk_size, small_before, d_reg);
            hipLaunchKernelGGL(bk_mark_kernel, dim3(nb), dim3(kGcThreads), 0, st, pos, d_reg, (uint64_t)k, d_mark);
            hipLaunchKernelGGL(bk_known_kernel, dim3(nb), dim3(kGcThreads), 0, st, pos, d_reg, d_sizes, (uint64_t)k, d_mark,
                               d_known, d_ksize);
            rc.ok(hipGetLastError()) && rc.ok(hipEventRecord(e1, st)) &&
                rc.ok(hipMemcpyAsync(ins, d_ins, k, hipMemcpyDeviceToHost, st)) &&
                rc.ok(hipMemcpyAsync(action, d_action, k, hipMemcpyDeviceToHost, st)) &&
                rc.ok(hipMemcpyAsync(dup, d_dup, k, hipMemcpyDeviceToHost, st)) &&
                rc.ok(hipMemcpyAsync(comp, d_comp, 4 * k, hipMemcpyDeviceToHost, st)) &&
                rc.ok(hipMemcpyAsync(reg, d_reg, k, hipMemcpyDeviceToHost, st));
        }
        if (hipStreamSynchronize(st) != hipSuccess) rc.fail(PBS_ERR_HIP);  // (before the arena goes back)
        if (rc.rc == PBS_OK) {
            float f = 0;
            (void)hipEventElapsedTime(&f, e0, e1);
            *ms = f;
        }
        return rc.rc;
    }

    // after a check kernel: the lowest failing i, its code, and the first n_done values of out64
    int collect(const unsigned long long* first, const int* code, const uint64_t* d_out64, size_t n, size_t* n_done, int* err,
                uint64_t* out64) {
        hipStream_t st = tab.st;
        unsigned long long f = 0;
        CallRc rc;
        rc.ok(hipMemcpyAsync(&f, first, 8, hipMemcpyDeviceToHost, st)) && rc.ok(hipStreamSynchronize(st));
        if (rc.rc != PBS_OK) return rc.rc;
        const size_t done = f < n ? (size_t)f : n;
        *err = PBS_BACKUP_E_NONE;
        if (done < n) rc.ok(hipMemcpyAsync(err, code + done, sizeof(int), hipMemcpyDeviceToHost, st));
        if (done && rc.rc == PBS_OK) rc.ok(hipMemcpyAsync(out64, d_out64, 8 * done, hipMemcpyDeviceToHost, st));
        if (hipStreamSynchronize(st) != hipSuccess) rc.fail(PBS_ERR_HIP);
        *n_done = done;
        return rc.rc;
    }

    int append_common(bool fixed, const uint8_t* digests, const uint64_t* offsets, size_t n, uint64_t start, uint64_t size,
                      uint64_t chunk_size, uint64_t index_length, size_t* n_done, int* err, uint64_t* out64) {
        hipStream_t st = tab.st;
        ArenaLease ar(bpool(), tab.dev);
        uint64_t* len = nullptr;
        uint8_t* kn = nullptr;
        uint64_t* d_off = ar->get<uint64_t>(kBsOffsets, 8 * n);
        uint64_t* ex = ar->get<uint64_t>(kBsEx, 8 * (n + 1));
        uint64_t* d_out64 = ar->get<uint64_t>(kBsOut64, 8 * n);
        int* code = ar->get<int>(kBsCode, sizeof(int) * n);
        unsigned long long* first = ar->get<unsigned long long>(kBsFirst, 8);
        size_t scan_b = 0;
        (void)exclusive_sum_u64(nullptr, &scan_b, nullptr, nullptr, (uint32_t)(n + 1), st);
        void* scan_tmp = ar->get<void>(kBsScanTmp, scan_b);
        hipEvent_t e0 = ar->event(0), e1 = ar->event(1);
        if (!d_off || !ex || !d_out64 || !code || !first || !scan_tmp) return PBS_ERR_NOMEM;
        if (!e0 || !e1) return PBS_ERR_HIP;
        CallRc rc;
        rc.ok(hipMemcpyAsync(d_off, offsets, 8 * n, hipMemcpyHostToDevice, st)) && rc.fail(probe(*ar, digests, n, &len, &kn, e0)) &&
            rc.ok(hipMemsetAsync(first, 0xFF, 8, st));
        if (rc.rc == PBS_OK && !fixed) rc.ok(exclusive_sum_u64(scan_tmp, &scan_b, len, ex, (uint32_t)(n + 1), st));
        if (rc.rc == PBS_OK) {
            if (fixed)
                hipLaunchKernelGGL(bk_fixed_check_kernel, dim3(blocks_for(n)), dim3(kGcThreads), 0, st, kn, len, d_off,
                                   (uint64_t)n, size, chunk_size, index_length, d_out64, code, first);
            else
                hipLaunchKernelGGL(bk_dynamic_check_kernel, dim3(blocks_for(n)), dim3(kGcThreads), 0, st, kn, len, ex, d_off,
                                   (uint64_t)n, start, d_out64, code, first);
            rc.ok(hipGetLastError()) && rc.ok(hipEventRecord(e1, st)) &&
                rc.fail(collect(first, code, d_out64, n, n_done, err, out64));
        }
        if (hipStreamSynchronize(st) != hipSuccess) rc.fail(PBS_ERR_HIP);  // (before the arena goes back)
        if (rc.rc == PBS_OK) last_ms = elapsed(e0, e1);
        return rc.rc;
    }

    int append_dynamic(const uint8_t* digests, const uint64_t* offsets, size_t n, uint64_t start, size_t* n_done, int* err,
                       uint64_t* ends) {
        return append_common(false, digests, offsets, n, start, 0, 0, 0, n_done, err, ends);
    }
    int append_fixed(const uint8_t* digests, const uint64_t* offsets, size_t n, uint64_t size, uint64_t chunk_size,
                     uint64_t index_length, size_t* n_done, int* err, uint64_t* idx) {
        return append_common(true, digests, offsets, n, 0, size, chunk_size, index_length, n_done, err, idx);
    }
};

}  // namespace
}  // namespace backup
}  // namespace pbs

struct pbs_backup {
    pbs::backup::Session<pbs::backup::DevEntries> s;
};

namespace {
// the handle's device for the call's scope
struct HandleGuard {
    pbs::DeviceGuard dg;
    bool ok;
    explicit HandleGuard(const pbs_backup* h) : dg(h->s.e.tab.dev), ok(dg.ok) {}
};
void free_handle(pbs_backup* h) {
    pbs::DeviceGuard dg(h->s.e.tab.dev);
    if (dg.ok) h->s.e.tab.free_all();
    delete h;
}
}  // namespace

using namespace pbs;
using namespace pbs::backup;

extern "C" void pbs_backup_release(void) { bpool().clear(); }

extern "C" int pbs_backup_begin(const uint8_t* store_digests, const uint64_t* store_sizes, const uint8_t* store_kinds,
                                size_t m, size_t reserve, pbs_backup** out, double* build_ms, void* hip_stream) {
    if (out) *out = nullptr;
    if (build_ms) *build_ms = 0;
    if (!begin_args_valid(store_digests, store_sizes, store_kinds, m, reserve, out)) return PBS_ERR_INVALID;
    hipStream_t st = (hipStream_t)hip_stream;
    const StreamDevice sd(st);
    if (!sd.ok) return PBS_ERR_NO_DEVICE;
    DeviceGuard dg(sd.dev);
    if (!dg.ok) return PBS_ERR_NO_DEVICE;
    pbs_backup* h = new (std::nothrow) pbs_backup;
    if (!h) return PBS_ERR_NOMEM;
    DevEntries& e = h->s.e;
    const int rc = e.tab.begin(sd, st, store_digests, m, reserve, build_ms, [&](CallRc& up) {
        up.ok(hipMemcpyAsync(e.d_size, store_sizes, 8 * m, hipMemcpyHostToDevice, st)) &&
            up.ok(hipMemcpyAsync(e.d_kind, store_kinds, m, hipMemcpyHostToDevice, st)) &&
            up.ok(hipMemsetAsync(e.d_present, 1, m, st)) && up.ok(hipMemsetAsync(e.d_known, 0, m, st)) &&
            up.ok(hipMemsetAsync(e.d_ksize, 0, 4 * m, st));
    });
    if (rc != PBS_OK) {
        free_handle(h);
        return rc;
    }
    Live<pbs_backup>::add(h);
    *out = h;
    return PBS_OK;
}

extern "C" void pbs_backup_end(pbs_backup* h) {
    if (h && Live<pbs_backup>::remove(h)) free_handle(h);
}

PBS_BACKUP_DEFINE_ABI(, pbs_backup, HandleGuard)
