// Device side of the restore path (include/pbs_restore.h): the segment copy kernel that every
// read-path call uses (dev_copy.h), the digest lookup with grouping and
// pbs_restore_range_device, which strings them together with pbs_blob_decode_inflate_device
// ("Restoring a stream").
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "dev_arena.h"
#include "dev_copy.h"
#include "pbs_chunker.h"
#include "pbs_chunker_internal.h"
#include "pbs_restore.h"

namespace pbs {

// ---- segment copy (dev_copy.h) -----------------------------------------------------------------

// One workgroup per item, the items of a launch in any order.  The contract, for every caller:
//  - an item's length is at most kPiece + 15 (add_items cuts segments so);
//  - src == 0 means zeros;
//  - the destinations of the items of one launch are pairwise disjoint (two workgroups would
//    otherwise write the same bytes in no order);
//  - nothing outside [dst, dst + len) is written and nothing outside [src, src + len) is read:
//    the destination is written 16 bytes per lane on 16-byte boundaries, and the up to 15 head
//    bytes before the first boundary and up to 15 tail bytes after the last go as bytes;
//  - the host item vector and the arena slot outlive the stream's next synchronisation.
__global__ __launch_bounds__(kCopyThreads) void segment_copy_kernel(const CopyItem* __restrict__ items,
                                                                    uint64_t nitems) {
    for (uint64_t k = blockIdx.x; k < nitems; k += gridDim.x) {
        const CopyItem it = items[k];
        const gbytes d = (gbytes)it.dst;
        const gcbytes s = (gcbytes)it.src;
        const uint64_t len = it.len;
        uint64_t head = (0 - it.dst) & 15;
        if (head > len) head = len;
        const uint64_t nvec = (len - head) >> 4;
        const uint64_t tail = head + (nvec << 4);  // first tail byte
        const uint32_t t = threadIdx.x;
        PBS_GLOBAL u32x4* const dv = reinterpret_cast<PBS_GLOBAL u32x4*>(d + head);
        if (it.src == 0) {  // (uniform)
            if (t < head) d[t] = 0;
            if (t < len - tail) d[tail + t] = 0;
            const u32x4 z = {0, 0, 0, 0};
            for (uint64_t v = t; v < nvec; v += kCopyThreads) dv[v] = z;
            continue;
        }
        if (t < head) d[t] = s[t];
        if (t < len - tail) d[tail + t] = s[tail + t];
        const gcbytes sv = s + head;
        uint64_t v = t;
        // four loads in flight per lane, then their four stores
        for (; v + 3 * kCopyThreads < nvec; v += 4 * kCopyThreads) {
            const u32x4 a = load16(sv + 16 * v);
            const u32x4 b = load16(sv + 16 * (v + kCopyThreads));
            const u32x4 c = load16(sv + 16 * (v + 2 * kCopyThreads));
            const u32x4 e = load16(sv + 16 * (v + 3 * kCopyThreads));
            dv[v] = a;
            dv[v + kCopyThreads] = b;
            dv[v + 2 * kCopyThreads] = c;
            dv[v + 3 * kCopyThreads] = e;
        }
        for (; v < nvec; v += kCopyThreads) dv[v] = load16(sv + 16 * v);
    }
}

void add_items(std::vector<CopyItem>& items, uint64_t src, uint64_t dst, uint64_t len) {
    if (len == 0) return;
    uint64_t at = 0, m = std::min<uint64_t>(len, ((0 - dst) & 15) + kPiece);
    for (;;) {
        items.push_back({src ? src + at : 0, dst + at, m});
        at += m;
        if (at >= len) break;
        m = std::min<uint64_t>(len - at, kPiece);
    }
}

int copy_items_async(const std::vector<CopyItem>& items, DevArena& ar, unsigned slot, int ncu, hipStream_t st) {
    if (items.empty()) return PBS_OK;
    CopyItem* d_items = ar.get<CopyItem>(slot, items.size() * sizeof(CopyItem));
    if (!d_items) return PBS_ERR_NOMEM;
    if (hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(CopyItem), hipMemcpyHostToDevice, st) != hipSuccess)
        return PBS_ERR_HIP;
    (void)hipGetLastError();
    const unsigned grid = (unsigned)std::min<uint64_t>(items.size(), (uint64_t)std::max(ncu, 1) * 8);
    hipLaunchKernelGGL(segment_copy_kernel, dim3(grid), dim3(kCopyThreads), 0, st, d_items, (uint64_t)items.size());
    return hipGetLastError() == hipSuccess ? PBS_OK : PBS_ERR_HIP;
}

namespace restore {
namespace {

// ---- digest lookup: the known-chunk test's method (pbs_digest.hip) with positions as output ----

// byte-string order of two 32-byte digests (16-byte aligned)
__device__ __forceinline__ int cmp32(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b) {
    const uint4* x = reinterpret_cast<const uint4*>(a);
    const uint4* y = reinterpret_cast<const uint4*>(b);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const uint4 u = x[q], v = y[q];
        const uint32_t uu[4] = {u.x, u.y, u.z, u.w}, vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int w = 0; w < 4; ++w)
            if (uu[w] != vv[w]) {
                const uint32_t bu = __builtin_bswap32(uu[w]), bv = __builtin_bswap32(vv[w]);
                return bu < bv ? -1 : 1;
            }
    }
    return 0;
}

__global__ void prefix_kernel(const uint8_t* __restrict__ dig, uint64_t n, uint64_t* __restrict__ key,
                              uint32_t* __restrict__ idx) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* d = reinterpret_cast<const uint32_t*>(dig + 32 * i);
    key[i] = ((uint64_t)__builtin_bswap32(d[0]) << 32) | __builtin_bswap32(d[1]);
    idx[i] = (uint32_t)i;
}

__global__ void run_head_kernel(const uint64_t* __restrict__ key, uint64_t n, uint32_t* __restrict__ head) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    head[p] = (p == 0 || key[p] != key[p - 1]) ? (uint32_t)p : 0u;
}

// One lane per sorted index entry p (entry i = sidx[p], its prefix run starts at rstart[p]).
// The sort is stable, so the run lists its entries in ascending i and the first earlier
// member with the same digest is the lowest: the representative.  The store: lower bound of
// the prefix among the sorted store prefixes, then its run in ascending store position.
// counts[0]: entries without a store position; counts[1]: representatives.
__global__ void lookup_kernel(const uint8_t* __restrict__ dig, uint64_t n, const uint64_t* __restrict__ skey,
                              const uint32_t* __restrict__ sidx, const uint32_t* __restrict__ rstart,
                              const uint8_t* __restrict__ store, uint64_t m,
                              const uint64_t* __restrict__ tkey, const uint32_t* __restrict__ tidx,
                              uint32_t* __restrict__ store_pos, uint32_t* __restrict__ first,
                              unsigned int* __restrict__ counts) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint32_t i = sidx[p];
    const uint8_t* di = dig + 32ull * i;
    uint32_t rep = i;
    for (uint32_t q = rstart[p]; q < p; ++q)
        if (cmp32(dig + 32ull * sidx[q], di) == 0) {
            rep = sidx[q];
            break;
        }
    const uint64_t key = skey[p];
    uint64_t lo = 0, hi = m;  // first store prefix >= key
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (tkey[mid] < key)
            lo = mid + 1;
        else
            hi = mid;
    }
    uint32_t pos = PBS_LOOKUP_MISSING;
    for (; lo < m && tkey[lo] == key; ++lo)
        if (cmp32(store + 32ull * tidx[lo], di) == 0) {
            pos = tidx[lo];
            break;
        }
    store_pos[i] = pos;
    first[i] = rep;
    if (pos == PBS_LOOKUP_MISSING) atomicAdd(&counts[0], 1u);
    if (rep == i) atomicAdd(&counts[1], 1u);
}

ArenaPool& rpool() {
    static ArenaPool* p = new ArenaPool;  // never destroyed (HIP may be torn down first at exit)
    return *p;
}
ArenaPool& lpool() {
    static ArenaPool* p = new ArenaPool;
    return *p;
}
ArenaPool& cpool() {
    static ArenaPool* p = new ArenaPool;
    return *p;
}

struct Range {
    uint64_t lo, hi;
};

// no destination overlaps another destination or any source (absolute addresses; empty
// segments take part in nothing); false also when a segment wraps the address space
bool segments_disjoint(uint64_t src, uint64_t dst, const uint64_t* so, const uint64_t* dof, const uint64_t* lens,
                       size_t nseg) {
    std::vector<Range> d;
    d.reserve(nseg);
    for (size_t k = 0; k < nseg; ++k) {
        if (!lens[k]) continue;
        const uint64_t a = dst + dof[k], b = src + so[k];
        if (a + lens[k] < a || b + lens[k] < b) return false;
        d.push_back({a, a + lens[k]});
    }
    std::sort(d.begin(), d.end(), [](const Range& x, const Range& y) { return x.lo < y.lo; });
    for (size_t k = 1; k < d.size(); ++k)
        if (d[k].lo < d[k - 1].hi) return false;
    for (size_t k = 0; k < nseg; ++k) {
        if (!lens[k]) continue;
        const uint64_t lo = src + so[k], hi = lo + lens[k];
        // the first destination that ends after lo
        const auto it = std::upper_bound(d.begin(), d.end(), lo, [](uint64_t v, const Range& r) { return v < r.hi; });
        if (it != d.end() && it->lo < hi) return false;
    }
    return true;
}

enum RSlot : unsigned { kRsDigests, kRsStore, kRsPos, kRsFirst, kRsPacked, kRsChunks, kRsItems, kRsRetry };

}  // namespace
}  // namespace restore
}  // namespace pbs

using namespace pbs;
using namespace pbs::restore;

extern "C" void pbs_restore_release(void) {
    rpool().clear();
    lpool().clear();
    cpool().clear();
}

extern "C" int pbs_digest_lookup_device(const uint8_t* digests_dev, size_t n, const uint8_t* store_dev, size_t m,
                                        uint32_t* store_pos_dev, uint32_t* first_dev, size_t* n_missing,
                                        size_t* n_unique, void* hip_stream) {
    if (n_missing) *n_missing = 0;
    if (n_unique) *n_unique = 0;
    if (n == 0) return PBS_OK;
    if (!digests_dev || !store_pos_dev || !first_dev || (m && !store_dev) || n > 0xFFFFFFF0u || m > 0xFFFFFFF0u ||
        ((uintptr_t)digests_dev & 15) || ((uintptr_t)store_dev & 15))
        return PBS_ERR_INVALID;
    hipStream_t st = (hipStream_t)hip_stream;
    const StreamDevice sd(st);
    if (!sd.ok) return PBS_ERR_NO_DEVICE;
    DeviceGuard dg(sd.dev);
    if (!dg.ok) return PBS_ERR_NO_DEVICE;
    ArenaLease ar(lpool(), sd.dev);
    const size_t big = std::max(n, m);
    uint64_t* key = ar->get<uint64_t>(0, big * 8);   // unsorted prefixes (of either list in turn)
    uint32_t* idx = ar->get<uint32_t>(1, big * 4);
    uint64_t* skey = ar->get<uint64_t>(2, n * 8);    // the index, sorted
    uint32_t* sidx = ar->get<uint32_t>(3, n * 4);
    uint64_t* tkey = ar->get<uint64_t>(4, m * 8);    // the store, sorted
    uint32_t* tidx = ar->get<uint32_t>(5, m * 4);
    uint32_t* head = ar->get<uint32_t>(6, n * 4);
    uint32_t* rstart = ar->get<uint32_t>(7, n * 4);
    unsigned int* cnt = ar->get<unsigned int>(8, 8);
    void* tmp = nullptr;
    int rc = PBS_OK;
    size_t tb_n = 0, tb_m = 0, tb_scan = 0, tb = 0;
    const unsigned grid = (unsigned)((n + 255) / 256);
    if (!key || !idx || !skey || !sidx || !tkey || !tidx || !head || !rstart || !cnt) {
        rc = PBS_ERR_NOMEM;
        goto done;
    }
    if (radix_sort(nullptr, &tb_n, key, skey, idx, sidx, n, 0, 64, st) != hipSuccess ||
        radix_sort(nullptr, &tb_m, key, tkey, idx, tidx, m, 0, 64, st) != hipSuccess ||
        inclusive_max_u32(nullptr, &tb_scan, head, rstart, n, st) != hipSuccess ||
        !(tmp = ar->get<void>(9, tb = std::max(std::max(tb_n, tb_m), tb_scan)))) {
        rc = PBS_ERR_NOMEM;
        goto done;
    }
    (void)hipGetLastError();
    if (m) {
        hipLaunchKernelGGL(prefix_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, store_dev, (uint64_t)m,
                           key, idx);
        tb_m = tb;
        if (radix_sort(tmp, &tb_m, key, tkey, idx, tidx, m, 0, 64, st) != hipSuccess) {
            rc = PBS_ERR_HIP;
            goto done;
        }
    }
    hipLaunchKernelGGL(prefix_kernel, dim3(grid), dim3(256), 0, st, digests_dev, (uint64_t)n, key, idx);
    tb_n = tb;
    if (radix_sort(tmp, &tb_n, key, skey, idx, sidx, n, 0, 64, st) != hipSuccess) {
        rc = PBS_ERR_HIP;
        goto done;
    }
    hipLaunchKernelGGL(run_head_kernel, dim3(grid), dim3(256), 0, st, skey, (uint64_t)n, head);
    tb_scan = tb;
    if (inclusive_max_u32(tmp, &tb_scan, head, rstart, n, st) != hipSuccess ||
        hipMemsetAsync(cnt, 0, 8, st) != hipSuccess) {
        rc = PBS_ERR_HIP;
        goto done;
    }
    hipLaunchKernelGGL(lookup_kernel, dim3(grid), dim3(256), 0, st, digests_dev, (uint64_t)n, skey, sidx, rstart,
                       store_dev, (uint64_t)m, tkey, tidx, store_pos_dev, first_dev, cnt);
    if (hipGetLastError() != hipSuccess) {
        rc = PBS_ERR_HIP;
        goto done;
    }
    {
        unsigned int h[2] = {0, 0};
        if (hipMemcpyAsync(h, cnt, 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess) {
            rc = PBS_ERR_HIP;
            goto done;
        }
        if (n_missing) *n_missing = h[0];
        if (n_unique) *n_unique = h[1];
    }
done:
    if (rc != PBS_OK) (void)hipStreamSynchronize(st);  // (before the arena goes back)
    return rc;
}

extern "C" int pbs_copy_segments_device(const uint8_t* src_dev, uint8_t* dst_dev, const uint64_t* src_off,
                                        const uint64_t* dst_off, const uint64_t* lens, size_t nseg,
                                        void* hip_stream) {
    if (nseg == 0) return PBS_OK;
    if (!src_off || !dst_off || !lens) return PBS_ERR_INVALID;
    uint64_t total = 0;
    for (size_t k = 0; k < nseg; ++k) total |= lens[k];
    if (total == 0) return PBS_OK;
    if (!src_dev || !dst_dev) return PBS_ERR_INVALID;
    if (!segments_disjoint((uint64_t)(uintptr_t)src_dev, (uint64_t)(uintptr_t)dst_dev, src_off, dst_off, lens, nseg))
        return PBS_ERR_INVALID;
    hipStream_t st = (hipStream_t)hip_stream;
    const StreamDevice sd(st);
    if (!sd.ok) return PBS_ERR_NO_DEVICE;
    DeviceGuard dg(sd.dev);
    if (!dg.ok) return PBS_ERR_NO_DEVICE;
    std::vector<CopyItem> items;
    for (size_t k = 0; k < nseg; ++k)
        add_items(items, (uint64_t)(uintptr_t)src_dev + src_off[k], (uint64_t)(uintptr_t)dst_dev + dst_off[k], lens[k]);
    ArenaLease ar(cpool(), sd.dev);
    int rc = copy_items_async(items, *ar, 0, sd.ncu, st);
    if (hipStreamSynchronize(st) != hipSuccess && rc == PBS_OK) rc = PBS_ERR_HIP;  // (before the arena goes back)
    return rc;
}

extern "C" int pbs_restore_range_device(const uint64_t* ends, const uint8_t* digests, size_t n,
                                        const uint8_t* store_blobs_dev, const uint64_t* store_offsets,
                                        const uint8_t* store_digests, size_t m, const pbs_crypt_config* cfg,
                                        uint64_t offset, uint64_t len, uint8_t* out_dev, uint8_t* entry_status,
                                        pbs_restore_timing* timing, void* hip_stream) {
    const HClock::time_point t0 = HClock::now();
    if (timing) std::memset(timing, 0, sizeof(*timing));
    if ((n && (!ends || !digests || !entry_status)) || (m && (!store_offsets || !store_digests)) ||
        n > 0xFFFFFFF0u || m > 0xFFFFFFF0u)
        return PBS_ERR_INVALID;
    for (size_t i = 1; i < n; ++i)
        if (ends[i] < ends[i - 1]) return PBS_ERR_INVALID;
    for (size_t j = 0; j < m; ++j)
        if (store_offsets[j + 1] < store_offsets[j]) return PBS_ERR_INVALID;
    const uint64_t total = n ? ends[n - 1] : 0;
    if (offset > total || len > total - offset) return PBS_ERR_INVALID;
    if (n) std::memset(entry_status, PBS_BLOB_ST_NONE_REQUESTED, n);
    if (len == 0) return PBS_OK;
    if (!out_dev || (m && !store_blobs_dev)) return PBS_ERR_INVALID;

    // 1. the covering entries [i0, i1]
    size_t i0 = 0, i1 = 0;
    if (pbs_didx_chunk_from_offset(ends, n, offset, &i0, nullptr) != PBS_OK ||
        pbs_didx_chunk_from_offset(ends, n, offset + len - 1, &i1, nullptr) != PBS_OK || i1 < i0)
        return PBS_ERR_INVALID;
    const size_t nc = i1 - i0 + 1;
    auto start_of = [&](size_t i) { return i ? ends[i - 1] : 0; };

    hipStream_t st = (hipStream_t)hip_stream;
    const StreamDevice sd(st);
    if (!sd.ok) return PBS_ERR_NO_DEVICE;
    DeviceGuard dg(sd.dev);
    if (!dg.ok) return PBS_ERR_NO_DEVICE;
    ArenaLease ar(rpool(), sd.dev);
    hipEvent_t ev[5];
    for (int k = 0; k < 5; ++k)
        if (!(ev[k] = ar->event(k))) return PBS_ERR_HIP;

    // host arrays that device copies read: alive until the last synchronisation
    std::vector<uint32_t> pos(nc), first(nc);
    std::vector<CopyItem> items;
    int rc = PBS_OK;
    size_t n_missing = 0, n_unique = 0;
    std::vector<uint32_t> reps;          // covering entries (relative to i0) that are decoded
    std::vector<uint32_t> slot_of(nc);   // entry -> its representative's place in `reps`
    std::vector<uint64_t> poff, sizes, src_off, dst_off, lens, out_offsets, out_lens;
    std::vector<uint8_t> rep_digests, kinds, status;
    uint8_t *d_packed = nullptr, *d_chunks = nullptr;
    uint64_t blob_bytes = 0, chunk_bytes = 0, failed = 0;

    // 2. lookup
    {
        uint8_t* d_dig = ar->get<uint8_t>(kRsDigests, nc * 32);
        uint8_t* d_store = ar->get<uint8_t>(kRsStore, m * 32);
        uint32_t* d_pos = ar->get<uint32_t>(kRsPos, nc * 4);
        uint32_t* d_first = ar->get<uint32_t>(kRsFirst, nc * 4);
        if (!d_dig || !d_store || !d_pos || !d_first) return PBS_ERR_NOMEM;
        if (hipEventRecord(ev[0], st) != hipSuccess ||
            hipMemcpyAsync(d_dig, digests + 32 * i0, nc * 32, hipMemcpyHostToDevice, st) != hipSuccess ||
            (m && hipMemcpyAsync(d_store, store_digests, m * 32, hipMemcpyHostToDevice, st) != hipSuccess)) {
            rc = PBS_ERR_HIP;
            goto done;
        }
        rc = pbs_digest_lookup_device(d_dig, nc, d_store, m, d_pos, d_first, &n_missing, &n_unique, st);
        if (rc != PBS_OK) goto done;
        if (hipMemcpyAsync(pos.data(), d_pos, nc * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipMemcpyAsync(first.data(), d_first, nc * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipEventRecord(ev[1], st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
            rc = PBS_ERR_HIP;
            goto done;
        }
    }

    // 3. pack: the blobs of the representatives that the store holds, back to back
    poff.push_back(0);
    for (size_t k = 0; k < nc; ++k) {
        if (first[k] > k || (pos[k] != PBS_LOOKUP_MISSING && pos[k] >= m)) {  // (never: the lookup's contract)
            rc = PBS_ERR_HIP;
            goto done;
        }
        if (pos[k] == PBS_LOOKUP_MISSING || first[k] != k) continue;
        slot_of[k] = (uint32_t)reps.size();
        reps.push_back((uint32_t)k);
        const uint64_t blen = store_offsets[pos[k] + 1] - store_offsets[pos[k]];
        src_off.push_back(store_offsets[pos[k]]);
        dst_off.push_back(blob_bytes);
        lens.push_back(blen);
        blob_bytes += blen;
        poff.push_back(blob_bytes);
        const uint64_t csize = ends[i0 + k] - start_of(i0 + k);
        sizes.push_back(csize);
        chunk_bytes += csize;
        rep_digests.insert(rep_digests.end(), digests + 32 * (i0 + k), digests + 32 * (i0 + k) + 32);
    }
    for (size_t k = 0; k < nc; ++k)
        if (pos[k] != PBS_LOOKUP_MISSING && first[k] != k) slot_of[k] = slot_of[first[k]];
    d_packed = ar->get<uint8_t>(kRsPacked, blob_bytes, false);
    d_chunks = ar->get<uint8_t>(kRsChunks, chunk_bytes, false);
    if (!d_packed || !d_chunks) {
        rc = PBS_ERR_NOMEM;
        goto done;
    }
    if (!reps.empty()) {
        rc = pbs_copy_segments_device(store_blobs_dev, d_packed, src_off.data(), dst_off.data(), lens.data(),
                                      reps.size(), st);
        if (rc != PBS_OK) goto done;
    }
    if (hipEventRecord(ev[2], st) != hipSuccess) {
        rc = PBS_ERR_HIP;
        goto done;
    }

    // 4. decode every representative once
    out_offsets.assign(reps.size() + 1, 0);
    out_lens.assign(reps.size(), 0);
    kinds.assign(reps.size(), 0);
    status.assign(reps.size(), 0);
    if (!reps.empty()) {
        rc = pbs_blob_decode_inflate_device(d_packed, poff.data(), reps.size(), cfg, rep_digests.data(), sizes.data(), 1,
                                            d_chunks, chunk_bytes, out_offsets.data(), out_lens.data(), kinds.data(),
                                            status.data(), timing ? &timing->decode : nullptr, st);
        if (rc != PBS_OK) goto done;
        for (size_t u = 0; u < reps.size(); ++u)  // CachedChunk::new: every chunk's length, whatever its kind
            if (status[u] == PBS_BLOB_ST_OK && out_lens[u] != sizes[u]) status[u] = PBS_BLOB_ST_BAD_SIZE;
        // ... a LONGER chunk included.  The call above hashes what fits the entry's slot, so a
        // chunk that overflows it comes back as BAD_DIGEST whether it is the chunk the index
        // names or not.  read_chunk verifies the digest over the whole chunk before
        // CachedChunk::new looks at its length: a BAD_DIGEST blob of an entry shorter than the
        // index's longest chunk (a fixed index's clipped last entry, above all) is decoded once
        // more, alone, into a slot of that length; if its digest verifies there, the length is
        // what is wrong.  Only failed entries pay for this.
        uint64_t longest = 0;
        for (size_t i = 0; i < n; ++i) longest = std::max(longest, ends[i] - start_of(i));
        for (size_t u = 0; u < reps.size() && rc == PBS_OK; ++u) {
            if (status[u] != PBS_BLOB_ST_BAD_DIGEST || sizes[u] >= longest) continue;
            uint8_t* d_retry = ar->get<uint8_t>(kRsRetry, longest, false);
            if (!d_retry) break;  // (no memory for the second look: the first verdict stands)
            uint64_t oo[2] = {0, 0}, olen = 0;
            uint8_t kind = 0, st2 = 0;
            rc = pbs_blob_decode_inflate_device(d_packed, poff.data() + u, 1, cfg, rep_digests.data() + 32 * u, &longest, 0,
                                                d_retry, longest, oo, &olen, &kind, &st2, nullptr, st);
            if (rc == PBS_OK && st2 == PBS_BLOB_ST_OK && olen != sizes[u]) status[u] = PBS_BLOB_ST_BAD_SIZE;
        }
        if (rc != PBS_OK) goto done;
    }
    if (hipEventRecord(ev[3], st) != hipSuccess) {
        rc = PBS_ERR_HIP;
        goto done;
    }

    // 5. + 6. scatter: every covering entry takes its representative's status; an OK chunk is
    // copied to the entry's place, clipped to the range; any other entry's place is zeroed
    for (size_t k = 0; k < nc; ++k) {
        const uint8_t s = pos[k] == PBS_LOOKUP_MISSING ? (uint8_t)PBS_BLOB_ST_MISSING : status[slot_of[k]];
        entry_status[i0 + k] = s;
        if (s != PBS_BLOB_ST_OK) ++failed;
        const uint64_t cs = start_of(i0 + k), ce = ends[i0 + k];
        const uint64_t lo = std::max(cs, offset), hi = std::min(ce, offset + len);
        if (hi <= lo) continue;  // (a zero-length entry)
        const uint64_t src = s == PBS_BLOB_ST_OK ? (uint64_t)(uintptr_t)d_chunks + out_offsets[slot_of[k]] + (lo - cs) : 0;
        add_items(items, src, (uint64_t)(uintptr_t)out_dev + (lo - offset), hi - lo);
    }
    rc = copy_items_async(items, *ar, kRsItems, sd.ncu, st);
    if (rc == PBS_OK && hipEventRecord(ev[4], st) != hipSuccess) rc = PBS_ERR_HIP;
done:
    if (hipStreamSynchronize(st) != hipSuccess && rc == PBS_OK) rc = PBS_ERR_HIP;  // (before the arena goes back)
    if (rc == PBS_OK && timing) {
        float ms[4] = {0, 0, 0, 0};
        for (int k = 0; k < 4; ++k) (void)hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]);
        timing->lookup_ms = ms[0];
        timing->pack_ms = ms[1];
        timing->decode_ms = ms[2];
        timing->scatter_ms = ms[3];
        timing->entries = nc;
        timing->unique = reps.size();
        timing->missing = n_missing;
        timing->failed = failed;
        timing->blob_bytes = blob_bytes;
        timing->decoded_bytes = chunk_bytes;
        timing->out_bytes = len;
        timing->total_ms = hms(t0);
    }
    return rc;
}
