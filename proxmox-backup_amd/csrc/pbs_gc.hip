// Device side of garbage collection (include/pbs_gc.h; DESIGN.md section 10, "Garbage
// collection"): the chunk store's listing as an open-addressing table of store positions in
// device memory, built once per GC run; index files streamed through it, one lane per entry;
// the "touched" rule for .bad files; the sweep's classification with its counters.
//
// This path is bound by the latency of random reads (a table slot, then the 32 bytes of the
// store entry it names), so every kernel is one lane per entry in 256-thread blocks with few
// registers: many waves resident per CU is what hides the latency.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "dev_arena.h"
#include "gc_common.h"
#include "gc_table_dev.h"
#include "live_handles.h"
#include "pbs_chunker.h"
#include "pbs_chunker_internal.h"
#include "pbs_gc.h"

struct pbs_gc {
    int dev = 0, ncu = 0;
    hipStream_t st = nullptr;
    size_t m = 0;
    uint32_t log2 = 0;
    uint8_t* d_store = nullptr;  // 32 m: the listing's digests
    uint8_t* d_flags = nullptr;  // m
    uint8_t* d_ref = nullptr;    // m: 1 = an index entry named this entry's digest
    uint32_t* d_table = nullptr; // 2^log2 store positions, kEmpty where free
    uint64_t index_file_count = 0, index_data_bytes = 0;
};

namespace pbs {
namespace gc {
namespace {

// One lane per index entry: walks the cluster from the home slot to the first free slot, marks
// every store entry with the entry's digest (the byte is read first: consecutive snapshots
// repeat most digests, and a store of 1 over a 1 would only make write traffic), and is missing
// when none of them has flags == 0.  miss[i] and the block's count of missing entries go out
// for the ordered compaction.
__global__ __launch_bounds__(kGcThreads) void gc_mark_kernel(const uint8_t* __restrict__ base, uint64_t stride,
                                                             uint64_t n, const uint8_t* __restrict__ store,
                                                             const uint8_t* __restrict__ flags,
                                                             const uint32_t* __restrict__ table, uint32_t shift,
                                                             uint64_t mask, uint8_t* __restrict__ ref,
                                                             uint8_t* __restrict__ miss,
                                                             unsigned long long* __restrict__ block_missing) {
    __shared__ uint32_t wcnt[kGcWaves];
    const uint64_t i = (uint64_t)blockIdx.x * kGcThreads + threadIdx.x;
    bool missing = false;
    if (i < n) {
        const Dig d = load_digest(base + i * stride);
        bool chunk = false;
        uint64_t s = home_slot(d.w[0], shift);
        for (;;) {
            const uint32_t j = table[s];
            if (j == kEmpty) break;
            if (same_digest(store, j, d)) {
                if (ref[j] == 0) ref[j] = 1;
                if (flags[j] == 0) chunk = true;
            }
            s = (s + 1) & mask;
        }
        missing = !chunk;
        miss[i] = missing ? 1 : 0;
    }
    const uint32_t c = block_count(missing, wcnt);
    if (threadIdx.x == 0) block_missing[blockIdx.x] = c;
}

// (gc_compact_kernel, the positions of the missing entries in ascending order: gc_table_dev.h)

// One lane per store entry: what phase 1 would have touched.  A referenced .bad entry probes the
// table for a flags == 0 entry with its digest; they are rare.
__global__ __launch_bounds__(kGcThreads) void gc_touched_kernel(const uint8_t* __restrict__ store,
                                                                const uint8_t* __restrict__ flags,
                                                                const uint8_t* __restrict__ ref, uint64_t m,
                                                                const uint32_t* __restrict__ table, uint32_t shift,
                                                                uint64_t mask, uint8_t* __restrict__ touched) {
    const uint64_t j = (uint64_t)blockIdx.x * kGcThreads + threadIdx.x;
    if (j >= m) return;
    const uint8_t f = flags[j];
    uint8_t t = 0;
    if (ref[j] && !(f & PBS_GC_FOREIGN)) {
        t = 1;
        if (f != 0) {
            const Dig d = load_digest(store + 32 * j);
            uint64_t s = home_slot(d.w[0], shift);
            for (;;) {
                const uint32_t k = table[s];
                if (k == kEmpty) break;
                if (flags[k] == 0 && same_digest(store, k, d)) {
                    t = 0;  // the chunk itself is there: its .bad files are left alone
                    break;
                }
                s = (s + 1) & mask;
            }
        }
    }
    touched[j] = t;
}

enum Ctr : int { kDiskBytes, kDiskChunks, kRemovedBytes, kRemovedChunks, kPendingBytes, kPendingChunks, kRemovedBad, kStillBad, kCtrs };

// sweep_unused_chunks (chunk_store.rs:395-435) for every entry, grid-strided: the action, and the
// six counters and three byte sums reduced per wave, per block, then one atomic each per block.
__global__ __launch_bounds__(kGcThreads) void gc_sweep_kernel(const uint64_t* __restrict__ sizes,
                                                              const int64_t* __restrict__ atimes,
                                                              const uint8_t* __restrict__ flags,
                                                              const uint8_t* __restrict__ touched, uint64_t m,
                                                              int64_t min_atime, int64_t oldest_writer,
                                                              uint8_t* __restrict__ actions,
                                                              unsigned long long* __restrict__ ctr) {
    __shared__ unsigned long long part[kGcWaves][kCtrs];
    unsigned long long c[kCtrs];
#pragma unroll
    for (int k = 0; k < kCtrs; ++k) c[k] = 0;
    for (uint64_t j = (uint64_t)blockIdx.x * kGcThreads + threadIdx.x; j < m; j += (uint64_t)gridDim.x * kGcThreads) {
        const uint64_t size = sizes[j];
        uint8_t act = PBS_GC_KEEP;
        if (size != PBS_GC_VANISHED) {
            // (constant indices only: c[] stays in registers)
            const unsigned long long bad = flags[j] & PBS_GC_BAD, good = bad ^ 1;
            const int64_t atime = atimes[j];
            const bool kept = touched[j] != 0;
            if (!kept && atime < min_atime) {
                act = PBS_GC_REMOVE;
                c[kRemovedBad] += bad;
                c[kRemovedChunks] += good;
                c[kRemovedBytes] += size;
            } else if (!kept && atime < oldest_writer) {
                act = PBS_GC_PENDING;
                c[kStillBad] += bad;
                c[kPendingChunks] += good;
                c[kPendingBytes] += size;
            } else {
                c[kDiskChunks] += good;
                c[kDiskBytes] += size;
            }
        }
        actions[j] = act;
    }
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < kCtrs; ++k) {
        unsigned long long x = c[k];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) x += __shfl_down(x, d, 64);
        if (lane == 0) part[wave][k] = x;
    }
    __syncthreads();
    if (threadIdx.x < kCtrs) {
        unsigned long long x = 0;
        for (int w = 0; w < kGcWaves; ++w) x += part[w][threadIdx.x];
        if (x) atomicAdd(&ctr[threadIdx.x], x);
    }
}

ArenaPool& gpool() {
    static ArenaPool* p = new ArenaPool;  // never destroyed (HIP may be torn down first at exit)
    return *p;
}

enum GSlot : unsigned { kGsMiss, kGsCount, kGsStart, kGsScanTmp, kGsOut, kGsImage, kGsSizes, kGsAtimes, kGsTouched, kGsActions, kGsCtr };

using Handles = Live<pbs_gc>;

void free_handle(pbs_gc* h) {
    DeviceGuard dg(h->dev);
    if (dg.ok) {
        (void)hipStreamSynchronize(h->st);
        if (h->d_store) (void)hipFree(h->d_store);
        if (h->d_flags) (void)hipFree(h->d_flags);
        if (h->d_ref) (void)hipFree(h->d_ref);
        if (h->d_table) (void)hipFree(h->d_table);
    }
    delete h;
}

// the touched map into `out` (device, m bytes), asynchronous on the handle's stream
void touched_async(const pbs_gc* h, uint8_t* out) {
    if (h->m == 0) return;
    hipLaunchKernelGGL(gc_touched_kernel, dim3(blocks_for(h->m)), dim3(kGcThreads), 0, h->st, h->d_store, h->d_flags,
                       h->d_ref, (uint64_t)h->m, h->d_table, 64 - h->log2, (1ull << h->log2) - 1, out);
}

// pbs_gc_mark_device / pbs_gc_mark_piece on a leased arena (pbs_gc_mark_index_image holds the
// image in it); the caller has checked the handle and set the device
int mark_on(pbs_gc* h, DevArena& ar, const uint8_t* base_dev, size_t stride, size_t n, uint32_t* missing_pos,
            size_t cap, size_t* n_missing, double* mark_ms) {
    if (n == 0) return PBS_OK;
    hipStream_t st = h->st;
    const unsigned nb = blocks_for(n);
    const size_t ncap = std::min(cap, n);
    uint8_t* miss = ar.get<uint8_t>(kGsMiss, n);
    unsigned long long* count = ar.get<unsigned long long>(kGsCount, ((size_t)nb + 1) * 8);
    unsigned long long* start = ar.get<unsigned long long>(kGsStart, ((size_t)nb + 1) * 8);
    uint32_t* out = ar.get<uint32_t>(kGsOut, ncap * 4);
    size_t tb = 0;
    (void)exclusive_sum_u64(nullptr, &tb, nullptr, nullptr, nb + 1, st);
    void* tmp = ar.get<void>(kGsScanTmp, tb);
    hipEvent_t e0 = ar.event(0), e1 = ar.event(1);
    if (!miss || !count || !start || !out || !tmp) return PBS_ERR_NOMEM;
    if (!e0 || !e1) return PBS_ERR_HIP;
    CallRc rc;
    unsigned long long total = 0;
    (void)hipGetLastError();
    // (count[nb] = 0: the exclusive sum's last value is then the total)
    if (rc.ok(hipEventRecord(e0, st)) && rc.ok(hipMemsetAsync(count + nb, 0, 8, st))) {
        hipLaunchKernelGGL(gc_mark_kernel, dim3(nb), dim3(kGcThreads), 0, st, base_dev, (uint64_t)stride, (uint64_t)n,
                           h->d_store, h->d_flags, h->d_table, 64 - h->log2, (1ull << h->log2) - 1, h->d_ref, miss,
                           count);
        rc.ok(hipGetLastError());
    }
    if (rc.rc == PBS_OK && rc.ok(exclusive_sum_u64(tmp, &tb, reinterpret_cast<const uint64_t*>(count),
                                                   reinterpret_cast<uint64_t*>(start), nb + 1, st)) &&
        ncap) {
        hipLaunchKernelGGL(gc_compact_kernel<false>, dim3(nb), dim3(kGcThreads), 0, st, miss, (uint64_t)n, start, out,
                           (uint64_t)ncap, (const uint32_t*)nullptr, (uint32_t*)nullptr);
        rc.ok(hipGetLastError());
    }
    if (rc.rc == PBS_OK && rc.ok(hipEventRecord(e1, st)) &&
        rc.ok(hipMemcpyAsync(&total, start + nb, 8, hipMemcpyDeviceToHost, st)))
        rc.ok(hipStreamSynchronize(st));
    if (rc.rc == PBS_OK && total > n) rc.fail(PBS_ERR_HIP);  // (never: n lanes set at most n flags)
    if (rc.rc == PBS_OK && ncap && total) {
        if (rc.ok(hipMemcpyAsync(missing_pos, out, std::min<size_t>(ncap, total) * 4, hipMemcpyDeviceToHost, st)))
            rc.ok(hipStreamSynchronize(st));
    }
    if (rc.rc != PBS_OK) {
        (void)hipStreamSynchronize(st);  // (before the arena goes back)
        return rc.rc;
    }
    if (n_missing) *n_missing = (size_t)total;
    if (mark_ms) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, e0, e1);
        *mark_ms = ms;
    }
    return PBS_OK;
}

int mark_call(pbs_gc* h, const uint8_t* base_dev, size_t stride, size_t n, bool whole, uint64_t index_bytes,
              uint32_t* missing_pos, size_t cap, size_t* n_missing, double* mark_ms) {
    if (n_missing) *n_missing = 0;
    if (mark_ms) *mark_ms = 0;
    if (!Handles::alive(h) || !mark_args_valid(base_dev, stride, n, missing_pos, cap)) return PBS_ERR_INVALID;
    DeviceGuard dg(h->dev);
    if (!dg.ok) return PBS_ERR_NO_DEVICE;
    ArenaLease ar(gpool(), h->dev);
    const int rc = mark_on(h, *ar, base_dev, stride, n, missing_pos, cap, n_missing, mark_ms);
    if (rc == PBS_OK && whole) {
        h->index_file_count += 1;
        h->index_data_bytes += index_bytes;
    }
    return rc;
}

}  // namespace
}  // namespace gc
}  // namespace pbs

using namespace pbs;
using namespace pbs::gc;

extern "C" void pbs_gc_release(void) { gpool().clear(); }

extern "C" int pbs_gc_begin(const uint8_t* store_digests, const uint8_t* flags, size_t m, pbs_gc** out,
                            double* build_ms, void* hip_stream) {
    if (out) *out = nullptr;
    if (build_ms) *build_ms = 0;
    if (!out || (m && (!store_digests || !flags)) || m >= kGcMaxEntries || !flags_valid(flags, m))
        return PBS_ERR_INVALID;
    hipStream_t st = (hipStream_t)hip_stream;
    const StreamDevice sd(st);
    if (!sd.ok) return PBS_ERR_NO_DEVICE;
    DeviceGuard dg(sd.dev);
    if (!dg.ok) return PBS_ERR_NO_DEVICE;
    pbs_gc* h = new (std::nothrow) pbs_gc;
    if (!h) return PBS_ERR_NOMEM;
    h->dev = sd.dev;
    h->ncu = sd.ncu;
    h->st = st;
    h->m = m;
    h->log2 = table_log2_for(m);
    const size_t slots = (size_t)1 << h->log2;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    CallRc rc;
    if (hipMalloc(&h->d_store, std::max<size_t>(32 * m, 1)) != hipSuccess ||
        hipMalloc(&h->d_flags, std::max<size_t>(m, 1)) != hipSuccess ||
        hipMalloc(&h->d_ref, std::max<size_t>(m, 1)) != hipSuccess ||
        hipMalloc(&h->d_table, slots * 4) != hipSuccess) {
        (void)hipGetLastError();
        rc.fail(PBS_ERR_NOMEM);
    }
    if (rc.rc == PBS_OK && m && rc.ok(hipMemcpyAsync(h->d_store, store_digests, 32 * m, hipMemcpyHostToDevice, st)))
        rc.ok(hipMemcpyAsync(h->d_flags, flags, m, hipMemcpyHostToDevice, st));
    if (rc.rc == PBS_OK && rc.ok(hipEventCreate(&e0)) && rc.ok(hipEventCreate(&e1)) && rc.ok(hipEventRecord(e0, st)) &&
        rc.ok(hipMemsetAsync(h->d_table, 0xFF, slots * 4, st)) &&
        rc.ok(hipMemsetAsync(h->d_ref, 0, std::max<size_t>(m, 1), st)) && m) {
        (void)hipGetLastError();
        hipLaunchKernelGGL(gc_build_kernel, dim3(blocks_for(m)), dim3(kGcThreads), 0, st, h->d_store, (uint64_t)m,
                           h->d_table, 64 - h->log2, (uint64_t)slots - 1);
        rc.ok(hipGetLastError());
    }
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
    Handles::add(h);
    *out = h;
    return PBS_OK;
}

extern "C" uint32_t pbs_gc_table_log2(const pbs_gc* h) { return Handles::alive(h) ? h->log2 : 0; }

extern "C" int pbs_gc_mark_device(pbs_gc* h, const uint8_t* base_dev, size_t stride, size_t n, uint64_t index_bytes,
                                  uint32_t* missing_pos, size_t cap, size_t* n_missing, double* mark_ms) {
    return mark_call(h, base_dev, stride, n, true, index_bytes, missing_pos, cap, n_missing, mark_ms);
}

extern "C" int pbs_gc_mark_piece(pbs_gc* h, const uint8_t* base_dev, size_t stride, size_t n, uint32_t* missing_pos,
                                 size_t cap, size_t* n_missing, double* mark_ms) {
    return mark_call(h, base_dev, stride, n, false, 0, missing_pos, cap, n_missing, mark_ms);
}

extern "C" int pbs_gc_mark_index_image(pbs_gc* h, const uint8_t* image, size_t len, uint32_t* missing_pos, size_t cap,
                                       size_t* n_missing, double* mark_ms) {
    if (n_missing) *n_missing = 0;
    if (mark_ms) *mark_ms = 0;
    if (!Handles::alive(h)) return PBS_ERR_INVALID;
    IndexLayout lo;
    int rc = index_layout(image, len, &lo);
    if (rc != PBS_OK) return rc;
    if (cap && !missing_pos) return PBS_ERR_INVALID;
    DeviceGuard dg(h->dev);
    if (!dg.ok) return PBS_ERR_NO_DEVICE;
    ArenaLease ar(gpool(), h->dev);
    if (lo.n) {
        // the body as it stands, marked in place: a .didx entry's digest follows its 8-byte end,
        // so those digests are 8- but not 16-byte aligned
        constexpr size_t kHeader = 4096;
        uint8_t* d_body = ar->get<uint8_t>(kGsImage, len - kHeader);
        if (!d_body) return PBS_ERR_NOMEM;
        rc = hipMemcpyAsync(d_body, image + kHeader, len - kHeader, hipMemcpyHostToDevice, h->st) == hipSuccess
                 ? mark_on(h, *ar, d_body + (lo.off - kHeader), lo.stride, lo.n, missing_pos, cap, n_missing, mark_ms)
                 : PBS_ERR_HIP;
        if (rc != PBS_OK) {
            (void)hipStreamSynchronize(h->st);  // (before the arena goes back)
            return rc;
        }
    }
    h->index_file_count += 1;
    h->index_data_bytes += lo.index_bytes;
    return PBS_OK;
}

extern "C" int pbs_gc_touched(pbs_gc* h, uint8_t* touched, size_t* n_touched) {
    if (n_touched) *n_touched = 0;
    if (!Handles::alive(h) || (h->m && !touched)) return PBS_ERR_INVALID;
    if (h->m == 0) return PBS_OK;
    DeviceGuard dg(h->dev);
    if (!dg.ok) return PBS_ERR_NO_DEVICE;
    ArenaLease ar(gpool(), h->dev);
    uint8_t* d_t = ar->get<uint8_t>(kGsTouched, h->m);
    if (!d_t) return PBS_ERR_NOMEM;
    CallRc rc;
    (void)hipGetLastError();
    touched_async(h, d_t);
    if (rc.ok(hipGetLastError())) rc.ok(hipMemcpyAsync(touched, d_t, h->m, hipMemcpyDeviceToHost, h->st));
    if (hipStreamSynchronize(h->st) != hipSuccess) rc.fail(PBS_ERR_HIP);  // (before the arena goes back)
    if (rc.rc != PBS_OK) return rc.rc;
    size_t cnt = 0;
    for (size_t j = 0; j < h->m; ++j) cnt += touched[j];
    if (n_touched) *n_touched = cnt;
    return PBS_OK;
}

extern "C" int pbs_gc_sweep(pbs_gc* h, const uint64_t* sizes, const int64_t* atimes, int64_t phase1_start,
                            int64_t oldest_writer, uint8_t* actions, pbs_gc_status* status, double* sweep_ms) {
    if (sweep_ms) *sweep_ms = 0;
    if (!Handles::alive(h)) return PBS_ERR_INVALID;
    const size_t m = h->m;
    int64_t min_atime = 0;
    if ((m && (!sizes || !atimes)) || !sweep_min_atime(phase1_start, oldest_writer, &min_atime)) return PBS_ERR_INVALID;
    pbs_gc_status s;
    std::memset(&s, 0, sizeof(s));
    s.index_file_count = h->index_file_count;
    s.index_data_bytes = h->index_data_bytes;
    if (m) {
        DeviceGuard dg(h->dev);
        if (!dg.ok) return PBS_ERR_NO_DEVICE;
        ArenaLease ar(gpool(), h->dev);
        hipStream_t st = h->st;
        uint64_t* d_sizes = ar->get<uint64_t>(kGsSizes, m * 8);
        int64_t* d_atimes = ar->get<int64_t>(kGsAtimes, m * 8);
        uint8_t* d_t = ar->get<uint8_t>(kGsTouched, m);
        uint8_t* d_act = ar->get<uint8_t>(kGsActions, m);
        unsigned long long* d_ctr = ar->get<unsigned long long>(kGsCtr, kCtrs * 8);
        hipEvent_t e0 = ar->event(0), e1 = ar->event(1);
        if (!d_sizes || !d_atimes || !d_t || !d_act || !d_ctr) return PBS_ERR_NOMEM;
        if (!e0 || !e1) return PBS_ERR_HIP;
        unsigned long long c[kCtrs] = {};
        CallRc rc;
        (void)hipGetLastError();
        if (rc.ok(hipMemcpyAsync(d_sizes, sizes, m * 8, hipMemcpyHostToDevice, st)) &&
            rc.ok(hipMemcpyAsync(d_atimes, atimes, m * 8, hipMemcpyHostToDevice, st)) &&
            rc.ok(hipMemsetAsync(d_ctr, 0, kCtrs * 8, st)) && rc.ok(hipEventRecord(e0, st))) {
            touched_async(h, d_t);
            const unsigned grid = std::min<unsigned>(blocks_for(m), (unsigned)std::max(h->ncu, 1) * 8);
            hipLaunchKernelGGL(gc_sweep_kernel, dim3(grid), dim3(kGcThreads), 0, st, d_sizes, d_atimes, h->d_flags, d_t,
                               (uint64_t)m, min_atime, oldest_writer, d_act, d_ctr);
            if (rc.ok(hipGetLastError()) && rc.ok(hipEventRecord(e1, st)) &&
                rc.ok(hipMemcpyAsync(c, d_ctr, kCtrs * 8, hipMemcpyDeviceToHost, st)) && actions)
                rc.ok(hipMemcpyAsync(actions, d_act, m, hipMemcpyDeviceToHost, st));
        }
        if (hipStreamSynchronize(st) != hipSuccess) rc.fail(PBS_ERR_HIP);  // (before the arena goes back)
        if (rc.rc != PBS_OK) return rc.rc;
        s.disk_bytes = c[kDiskBytes];
        s.disk_chunks = c[kDiskChunks];
        s.removed_bytes = c[kRemovedBytes];
        s.removed_chunks = c[kRemovedChunks];
        s.pending_bytes = c[kPendingBytes];
        s.pending_chunks = c[kPendingChunks];
        s.removed_bad = c[kRemovedBad];
        s.still_bad = c[kStillBad];
        if (sweep_ms) {
            float ms = 0;
            (void)hipEventElapsedTime(&ms, e0, e1);
            *sweep_ms = ms;
        }
    }
    if (status) *status = s;
    return PBS_OK;
}

extern "C" void pbs_gc_end(pbs_gc* h) {
    if (h && Handles::remove(h)) free_handle(h);
}
