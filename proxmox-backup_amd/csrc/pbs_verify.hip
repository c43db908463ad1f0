// Device side of the verify job (include/pbs_verify.h; DESIGN.md section 10, "Verify"): the
// store's listing as the table of gc_table_dev.h, one state byte per store entry, the load plan
// of an index (probe, first occurrence, compaction over the store axis), the states after a
// submit and the count of failing occurrences.  The blobs themselves go through
// pbs_blob_decode_inflate_device.
//
// Like garbage collection this path is bound by the latency of random reads (a table slot, the
// 32 bytes of the store entry it names, that entry's state), so every kernel is one lane per
// entry in 256-thread blocks with few registers.
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
#include "pbs_blob.h"
#include "pbs_chunker.h"
#include "pbs_chunker_internal.h"
#include "pbs_restore.h"
#include "pbs_verify.h"
#include "verify_common.h"
#include "verify_dev.h"

struct pbs_verify {
    int dev = 0, ncu = 0;
    hipStream_t st = nullptr;
    size_t m = 0;
    uint32_t log2 = 0;
    uint8_t* d_store = nullptr;   // 32 m: the listing's digests
    uint8_t* d_state = nullptr;   // m: PBS_VERIFY_*
    uint32_t* d_table = nullptr;  // 2^log2 store positions, kEmpty where free
    uint32_t* d_first = nullptr;  // m: the lowest entry of the open index naming store entry j, kEmpty
    uint32_t* d_pos = nullptr;    // of the open index: entry -> lowest store position, kEmpty
    size_t pos_cap = 0;           // entries d_pos holds
    pbs::verify::IndexRun run;
};

namespace pbs {
namespace verify {
namespace {

using namespace pbs::gc;

enum VCtr : int { kSkipVerified, kSkipCorrupt, kFailing, kVCtrs };

// One lane per index entry: the LOWEST store position with the entry's digest (lowest_entry).
// Present: first[j] = min(first[j], i), and the occurrence is counted by the chunk's state.
// Absent: miss[i], and the block's count of them for the ordered compaction.
__global__ __launch_bounds__(kGcThreads) void verify_probe_kernel(
    const uint8_t* __restrict__ dig, uint64_t n, const uint8_t* __restrict__ store, const uint8_t* __restrict__ state,
    const uint32_t* __restrict__ table, uint32_t shift, uint64_t mask, uint32_t* __restrict__ pos,
    uint32_t* __restrict__ first, uint8_t* __restrict__ miss, unsigned long long* __restrict__ block_missing,
    unsigned long long* __restrict__ ctr) {
    __shared__ uint32_t wcnt[kGcWaves];
    const uint64_t i = (uint64_t)blockIdx.x * kGcThreads + threadIdx.x;
    bool missing = false, sv = false, sc = false;
    if (i < n) {
        const Dig d = load_digest(dig + 32 * i);
        const uint32_t j = lowest_entry(table, store, d, shift, mask);
        pos[i] = j;
        if (j == kEmpty) {
            missing = true;
        } else {
            atomicMin(&first[j], (uint32_t)i);
            const uint8_t stj = state[j];
            sv = stj == PBS_VERIFY_VERIFIED;
            sc = stj == PBS_VERIFY_CORRUPT;
        }
        miss[i] = missing ? 1 : 0;
    }
    const uint32_t cm = block_count(missing, wcnt), cv = block_count(sv, wcnt), cc = block_count(sc, wcnt);
    if (threadIdx.x == 0) {
        block_missing[blockIdx.x] = cm;
        if (cv) atomicAdd(&ctr[kSkipVerified], (unsigned long long)cv);
        if (cc) atomicAdd(&ctr[kSkipCorrupt], (unsigned long long)cc);
    }
}

// One lane per store entry: in the plan when an entry of the index named it and nothing is known
// about it yet.
__global__ __launch_bounds__(kGcThreads) void verify_select_kernel(const uint32_t* __restrict__ first,
                                                                   const uint8_t* __restrict__ state, uint64_t m,
                                                                   uint8_t* __restrict__ sel,
                                                                   unsigned long long* __restrict__ block_sel) {
    __shared__ uint32_t wcnt[kGcWaves];
    const uint64_t j = (uint64_t)blockIdx.x * kGcThreads + threadIdx.x;
    bool s = false;
    if (j < m) {
        s = first[j] != kEmpty && state[j] == PBS_VERIFY_UNKNOWN;
        sel[j] = s ? 1 : 0;
    }
    const uint32_t c = block_count(s, wcnt);
    if (threadIdx.x == 0) block_sel[blockIdx.x] = c;
}

// (gc_compact_kernel, the ordered compaction with its optional gather: gc_table_dev.h;
// verify_magic_kernel, the magic read of a submit: verify_dev.h)

// One lane per submitted blob, scattered by store position (the plan names every position once).
__global__ __launch_bounds__(kGcThreads) void verify_state_kernel(const uint32_t* __restrict__ store_pos,
                                                                  const uint8_t* __restrict__ status, uint64_t k,
                                                                  uint8_t* __restrict__ state) {
    const uint64_t t = (uint64_t)blockIdx.x * kGcThreads + threadIdx.x;
    if (t >= k) return;
    state[store_pos[t]] = status[t] == PBS_BLOB_ST_OK ? PBS_VERIFY_VERIFIED : PBS_VERIFY_CORRUPT;
}

// One lane per index entry: does this occurrence count as an error now?
__global__ __launch_bounds__(kGcThreads) void verify_count_kernel(const uint32_t* __restrict__ pos, uint64_t n,
                                                                  const uint8_t* __restrict__ state,
                                                                  unsigned long long* __restrict__ ctr) {
    __shared__ uint32_t wcnt[kGcWaves];
    const uint64_t i = (uint64_t)blockIdx.x * kGcThreads + threadIdx.x;
    bool bad = false;
    if (i < n) {
        const uint32_t j = pos[i];
        bad = j == kEmpty || state[j] == PBS_VERIFY_CORRUPT;
    }
    const uint32_t c = block_count(bad, wcnt);
    if (threadIdx.x == 0 && c) atomicAdd(&ctr[kFailing], (unsigned long long)c);
}

ArenaPool& vpool() {
    static ArenaPool* p = new ArenaPool;  // never destroyed (HIP may be torn down first at exit)
    return *p;
}

enum VSlot : unsigned { kVsDig, kVsMiss, kVsSel, kVsCountN, kVsStartN, kVsCountM, kVsStartM, kVsScanTmp, kVsOutMiss,
                        kVsOutStore, kVsOutEntry, kVsCtr, kVsSpans, kVsEnc, kVsOut, kVsPos, kVsStatus, kVsPack };

constexpr BlobSlots kBlobSlots = {kVsSpans, kVsEnc, kVsOut, kVsPack};

using Handles = Live<pbs_verify>;

void free_handle(pbs_verify* h) {
    DeviceGuard dg(h->dev);
    if (dg.ok) {
        (void)hipStreamSynchronize(h->st);
        if (h->d_store) (void)hipFree(h->d_store);
        if (h->d_state) (void)hipFree(h->d_state);
        if (h->d_table) (void)hipFree(h->d_table);
        if (h->d_first) (void)hipFree(h->d_first);
        if (h->d_pos) (void)hipFree(h->d_pos);
    }
    delete h;
}

// pbs_verify_plan after the argument checks; the caller has set the device
int plan_on(pbs_verify* h, const uint8_t* digests, const uint64_t* sizes, size_t n, int index_mode, double* plan_ms) {
    hipStream_t st = h->st;
    const size_t m = h->m;
    IndexRun& run = h->run;
    run.clear();
    if (n > h->pos_cap) {
        if (h->d_pos) (void)hipFree(h->d_pos);
        h->d_pos = nullptr;
        h->pos_cap = 0;
        if (hipMalloc(&h->d_pos, n * 4) != hipSuccess) {
            (void)hipGetLastError();
            return PBS_ERR_NOMEM;
        }
        h->pos_cap = n;
    }
    const unsigned nbn = blocks_for(n), nbm = n ? blocks_for(m) : 0;  // (no entry: nothing is named)
    const size_t kcap = std::min(n, m);
    ArenaLease ar(vpool(), h->dev);
    uint8_t* d_dig = ar->get<uint8_t>(kVsDig, 32 * n);
    uint8_t* miss = ar->get<uint8_t>(kVsMiss, n);
    uint8_t* sel = ar->get<uint8_t>(kVsSel, m);
    unsigned long long* count_n = ar->get<unsigned long long>(kVsCountN, ((size_t)nbn + 1) * 8);
    unsigned long long* start_n = ar->get<unsigned long long>(kVsStartN, ((size_t)nbn + 1) * 8);
    unsigned long long* count_m = ar->get<unsigned long long>(kVsCountM, ((size_t)nbm + 1) * 8);
    unsigned long long* start_m = ar->get<unsigned long long>(kVsStartM, ((size_t)nbm + 1) * 8);
    uint32_t* out_miss = ar->get<uint32_t>(kVsOutMiss, n * 4);
    uint32_t* out_store = ar->get<uint32_t>(kVsOutStore, kcap * 4);
    uint32_t* out_entry = ar->get<uint32_t>(kVsOutEntry, kcap * 4);
    unsigned long long* d_ctr = ar->get<unsigned long long>(kVsCtr, kVCtrs * 8);
    size_t tb = 0;
    (void)exclusive_sum_u64(nullptr, &tb, nullptr, nullptr, std::max(nbn, nbm) + 1, st);
    void* tmp = ar->get<void>(kVsScanTmp, tb);
    hipEvent_t e0 = ar->event(0), e1 = ar->event(1);
    if (!d_dig || !miss || !sel || !count_n || !start_n || !count_m || !start_m || !out_miss || !out_store ||
        !out_entry || !d_ctr || !tmp)
        return PBS_ERR_NOMEM;
    if (!e0 || !e1) return PBS_ERR_HIP;
    const uint32_t shift = 64 - h->log2;
    const uint64_t mask = (1ull << h->log2) - 1;
    CallRc rc;
    unsigned long long n_missing = 0, n_todo = 0, ctr[kVCtrs] = {};
    (void)hipGetLastError();
    if (n) rc.ok(hipMemcpyAsync(d_dig, digests, 32 * n, hipMemcpyHostToDevice, st));
    // (count[nb] = 0: the exclusive sum's last value is then the total)
    if (rc.rc == PBS_OK && rc.ok(hipEventRecord(e0, st)) && rc.ok(hipMemsetAsync(count_n + nbn, 0, 8, st)) &&
        rc.ok(hipMemsetAsync(count_m + nbm, 0, 8, st)) && rc.ok(hipMemsetAsync(d_ctr, 0, kVCtrs * 8, st)) &&
        rc.ok(hipMemsetAsync(h->d_first, 0xFF, std::max<size_t>(m, 1) * 4, st)) && n) {
        hipLaunchKernelGGL(verify_probe_kernel, dim3(nbn), dim3(kGcThreads), 0, st, d_dig, (uint64_t)n, h->d_store,
                           h->d_state, h->d_table, shift, mask, h->d_pos, h->d_first, miss, count_n, d_ctr);
        rc.ok(hipGetLastError());
        if (rc.rc == PBS_OK && nbm) {
            hipLaunchKernelGGL(verify_select_kernel, dim3(nbm), dim3(kGcThreads), 0, st, h->d_first, h->d_state,
                               (uint64_t)m, sel, count_m);
            rc.ok(hipGetLastError());
        }
    }
    if (rc.rc == PBS_OK &&
        rc.ok(exclusive_sum_u64(tmp, &tb, reinterpret_cast<const uint64_t*>(count_n), reinterpret_cast<uint64_t*>(start_n),
                                nbn + 1, st)) &&
        rc.ok(exclusive_sum_u64(tmp, &tb, reinterpret_cast<const uint64_t*>(count_m), reinterpret_cast<uint64_t*>(start_m),
                                nbm + 1, st))) {
        if (nbn) {
            hipLaunchKernelGGL(gc_compact_kernel<false>, dim3(nbn), dim3(kGcThreads), 0, st, miss, (uint64_t)n, start_n,
                               out_miss, (uint64_t)n, (const uint32_t*)nullptr, (uint32_t*)nullptr);
            rc.ok(hipGetLastError());
        }
        if (rc.rc == PBS_OK && nbm) {
            hipLaunchKernelGGL(gc_compact_kernel<true>, dim3(nbm), dim3(kGcThreads), 0, st, sel, (uint64_t)m, start_m,
                               out_store, (uint64_t)kcap, (const uint32_t*)h->d_first, out_entry);
            rc.ok(hipGetLastError());
        }
    }
    if (rc.rc == PBS_OK && rc.ok(hipEventRecord(e1, st)) &&
        rc.ok(hipMemcpyAsync(&n_missing, start_n + nbn, 8, hipMemcpyDeviceToHost, st)) &&
        rc.ok(hipMemcpyAsync(&n_todo, start_m + nbm, 8, hipMemcpyDeviceToHost, st)) &&
        rc.ok(hipMemcpyAsync(ctr, d_ctr, kVCtrs * 8, hipMemcpyDeviceToHost, st)))
        rc.ok(hipStreamSynchronize(st));
    if (rc.rc == PBS_OK && (n_missing > n || n_todo > kcap)) rc.fail(PBS_ERR_HIP);  // (never: one flag per lane)
    if (rc.rc == PBS_OK) {
        run.missing.resize((size_t)n_missing);
        run.todo_store.resize((size_t)n_todo);
        run.todo_entry.resize((size_t)n_todo);
        if (n_missing) rc.ok(hipMemcpyAsync(run.missing.data(), out_miss, n_missing * 4, hipMemcpyDeviceToHost, st));
        if (n_todo && rc.rc == PBS_OK &&
            rc.ok(hipMemcpyAsync(run.todo_store.data(), out_store, n_todo * 4, hipMemcpyDeviceToHost, st)))
            rc.ok(hipMemcpyAsync(run.todo_entry.data(), out_entry, n_todo * 4, hipMemcpyDeviceToHost, st));
    }
    if (hipStreamSynchronize(st) != hipSuccess) rc.fail(PBS_ERR_HIP);  // (before the arena goes back)
    if (rc.rc == PBS_OK)
        for (size_t t = 0; t < run.todo_store.size(); ++t)
            if (run.todo_store[t] >= m || run.todo_entry[t] >= n) rc.fail(PBS_ERR_HIP);  // (never)
    if (rc.rc != PBS_OK) {
        run.clear();
        return rc.rc;
    }
    run.gather(digests, sizes);
    run.open = true;
    run.mode = index_mode;
    run.n = n;
    run.res.entries = n;
    run.res.missing = n_missing;
    run.res.skipped_verified = ctr[kSkipVerified];
    run.res.skipped_corrupt = ctr[kSkipCorrupt];
    if (plan_ms) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, e0, e1);
        *plan_ms = ms;
    }
    return PBS_OK;
}

// pbs_verify_submit after the argument checks; the caller has set the device.  Nothing of the
// run changes unless every step went well.
int submit_on(pbs_verify* h, const uint8_t* blobs_dev, const uint64_t* blob_offsets, const uint8_t* load_failed,
              size_t k, uint8_t* kinds_out, uint8_t* status_out, pbs_verify_timing* timing) {
    const HClock::time_point t0 = HClock::now();
    IndexRun& run = h->run;
    hipStream_t st = h->st;
    pbs_verify_timing tm;
    std::memset(&tm, 0, sizeof(tm));
    tm.blobs = k;
    if (k == 0) {
        if (timing) *timing = tm;
        return PBS_OK;
    }
    const size_t item0 = run.done;
    ArenaLease ar(vpool(), h->dev);
    std::vector<uint8_t> kinds(k, PBS_BLOB_KIND_NONE), status(k, PBS_VERIFY_ST_LOAD_FAILED);
    BlobTiming bt;
    const int rc = blob_verdicts(*ar, kBlobSlots, st, blobs_dev, blob_offsets, load_failed, &run.todo_digests[32 * item0],
                                 [&](size_t t) { return run.todo_sizes[item0 + t]; }, k, kinds.data(), status.data(),
                                 nullptr, &bt);
    if (rc != PBS_OK) return rc;
    tm.magic_ms = bt.magic_ms;
    tm.decode_ms = bt.decode_ms;
    tm.decoded = bt.decoded;
    tm.encrypted = bt.encrypted;
    tm.scratch_bytes = bt.scratch_bytes;

    // the states
    uint32_t* d_sp = ar->get<uint32_t>(kVsPos, 4 * k);
    uint8_t* d_status = ar->get<uint8_t>(kVsStatus, k);
    hipEvent_t e0 = ar->event(0), e1 = ar->event(1);
    if (!d_sp || !d_status) return PBS_ERR_NOMEM;
    if (!e0 || !e1) return PBS_ERR_HIP;
    CallRc call;
    (void)hipGetLastError();
    if (call.ok(hipMemcpyAsync(d_sp, &run.todo_store[item0], 4 * k, hipMemcpyHostToDevice, st)) &&
        call.ok(hipMemcpyAsync(d_status, status.data(), k, hipMemcpyHostToDevice, st)) && call.ok(hipEventRecord(e0, st))) {
        hipLaunchKernelGGL(verify_state_kernel, dim3(blocks_for(k)), dim3(kGcThreads), 0, st, d_sp, d_status, (uint64_t)k,
                           h->d_state);
        call.ok(hipGetLastError()) && call.ok(hipEventRecord(e1, st));
    }
    if (hipStreamSynchronize(st) != hipSuccess) call.fail(PBS_ERR_HIP);  // (before the arena goes back)
    if (call.rc != PBS_OK) return call.rc;
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    tm.state_ms = ms;
    for (size_t t = 0; t < k; ++t) {
        (void)account(run, kinds[t], status[t], blob_offsets[t + 1] - blob_offsets[t]);
        if (kinds_out) kinds_out[t] = kinds[t];
        if (status_out) status_out[t] = status[t];
    }
    tm.total_ms = hms(t0);
    if (timing) *timing = tm;
    return PBS_OK;
}

int finish_on(pbs_verify* h, pbs_verify_result* res, uint32_t* corrupt_store, size_t ccap, size_t* n_corrupt,
              uint32_t* missing_pos, size_t mcap, size_t* n_missing) {
    IndexRun& run = h->run;
    unsigned long long failing = 0;
    if (run.n) {
        hipStream_t st = h->st;
        ArenaLease ar(vpool(), h->dev);
        unsigned long long* d_ctr = ar->get<unsigned long long>(kVsCtr, kVCtrs * 8);
        if (!d_ctr) return PBS_ERR_NOMEM;
        CallRc rc;
        (void)hipGetLastError();
        if (rc.ok(hipMemsetAsync(d_ctr, 0, kVCtrs * 8, st))) {
            hipLaunchKernelGGL(verify_count_kernel, dim3(blocks_for(run.n)), dim3(kGcThreads), 0, st, h->d_pos,
                               (uint64_t)run.n, h->d_state, d_ctr);
            rc.ok(hipGetLastError()) && rc.ok(hipMemcpyAsync(&failing, d_ctr + kFailing, 8, hipMemcpyDeviceToHost, st));
        }
        if (hipStreamSynchronize(st) != hipSuccess) rc.fail(PBS_ERR_HIP);  // (before the arena goes back)
        if (rc.rc != PBS_OK) return rc.rc;
    }
    close_run(run, failing, res, corrupt_store, ccap, n_corrupt, missing_pos, mcap, n_missing);
    return PBS_OK;
}

}  // namespace
}  // namespace verify
}  // namespace pbs

using namespace pbs;
using namespace pbs::gc;
using namespace pbs::verify;

extern "C" void pbs_verify_release(void) { vpool().clear(); }

extern "C" int pbs_verify_begin(const uint8_t* store_digests, size_t m, pbs_verify** out, double* build_ms,
                                void* hip_stream) {
    if (out) *out = nullptr;
    if (build_ms) *build_ms = 0;
    if (!out || (m && !store_digests) || m >= kGcMaxEntries) return PBS_ERR_INVALID;
    hipStream_t st = (hipStream_t)hip_stream;
    const StreamDevice sd(st);
    if (!sd.ok) return PBS_ERR_NO_DEVICE;
    DeviceGuard dg(sd.dev);
    if (!dg.ok) return PBS_ERR_NO_DEVICE;
    pbs_verify* h = new (std::nothrow) pbs_verify;
    if (!h) return PBS_ERR_NOMEM;
    h->dev = sd.dev;
    h->ncu = sd.ncu;
    h->st = st;
    h->m = m;
    h->log2 = table_log2_for(m);
    h->run.clear();
    const size_t slots = (size_t)1 << h->log2;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    CallRc rc;
    if (hipMalloc(&h->d_store, std::max<size_t>(32 * m, 1)) != hipSuccess ||
        hipMalloc(&h->d_state, std::max<size_t>(m, 1)) != hipSuccess ||
        hipMalloc(&h->d_first, std::max<size_t>(m, 1) * 4) != hipSuccess ||
        hipMalloc(&h->d_table, slots * 4) != hipSuccess) {
        (void)hipGetLastError();
        rc.fail(PBS_ERR_NOMEM);
    }
    if (rc.rc == PBS_OK && m) rc.ok(hipMemcpyAsync(h->d_store, store_digests, 32 * m, hipMemcpyHostToDevice, st));
    if (rc.rc == PBS_OK && rc.ok(hipEventCreate(&e0)) && rc.ok(hipEventCreate(&e1)) && rc.ok(hipEventRecord(e0, st)) &&
        rc.ok(hipMemsetAsync(h->d_table, 0xFF, slots * 4, st)) &&
        rc.ok(hipMemsetAsync(h->d_state, PBS_VERIFY_UNKNOWN, std::max<size_t>(m, 1), st)) && m) {
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

extern "C" int pbs_verify_states(pbs_verify* h, uint8_t* states_host, size_t m) {
    if (!Handles::alive(h) || m != h->m || (m && !states_host)) return PBS_ERR_INVALID;
    if (m == 0) return PBS_OK;
    DeviceGuard dg(h->dev);
    if (!dg.ok) return PBS_ERR_NO_DEVICE;
    CallRc rc;
    rc.ok(hipMemcpyAsync(states_host, h->d_state, m, hipMemcpyDeviceToHost, h->st));
    if (hipStreamSynchronize(h->st) != hipSuccess) rc.fail(PBS_ERR_HIP);
    return rc.rc;
}

extern "C" void pbs_verify_end(pbs_verify* h) {
    if (h && Handles::remove(h)) free_handle(h);
}

extern "C" int pbs_verify_plan(pbs_verify* h, const uint8_t* digests, const uint64_t* sizes, size_t n, int index_mode,
                               uint32_t* todo_store, uint32_t* todo_entry, size_t cap, size_t* n_todo,
                               double* plan_ms) {
    if (n_todo) *n_todo = 0;
    if (plan_ms) *plan_ms = 0;
    if (!Handles::alive(h) || h->run.open ||
        !plan_args_valid(digests, sizes, n, index_mode, todo_store, todo_entry, cap, n_todo))
        return PBS_ERR_INVALID;
    DeviceGuard dg(h->dev);
    if (!dg.ok) return PBS_ERR_NO_DEVICE;
    int rc;
    try {
        rc = plan_on(h, digests, sizes, n, index_mode, plan_ms);
    } catch (const std::bad_alloc&) {
        h->run.clear();
        rc = PBS_ERR_NOMEM;
    }
    if (rc != PBS_OK) return rc;
    const size_t k = h->run.todo_store.size();
    for (size_t t = 0; t < k && t < cap; ++t) {
        todo_store[t] = h->run.todo_store[t];
        todo_entry[t] = h->run.todo_entry[t];
    }
    *n_todo = k;
    return PBS_OK;
}

extern "C" int pbs_verify_abort_index(pbs_verify* h) {
    if (!Handles::alive(h)) return PBS_ERR_INVALID;
    h->run.clear();
    return PBS_OK;
}

extern "C" int pbs_verify_submit(pbs_verify* h, const uint8_t* blobs_dev, const uint64_t* blob_offsets,
                                 const uint8_t* load_failed, size_t k, uint8_t* kinds, uint8_t* status,
                                 pbs_verify_timing* timing) {
    if (timing) std::memset(timing, 0, sizeof(*timing));
    if (!Handles::alive(h) || !submit_args_valid(h->run, blobs_dev, blob_offsets, k)) return PBS_ERR_INVALID;
    DeviceGuard dg(h->dev);
    if (!dg.ok) return PBS_ERR_NO_DEVICE;
    try {
        return submit_on(h, blobs_dev, blob_offsets, load_failed, k, kinds, status, timing);
    } catch (const std::bad_alloc&) {
        return PBS_ERR_NOMEM;
    }
}

extern "C" int pbs_verify_finish(pbs_verify* h, pbs_verify_result* res, uint32_t* corrupt_store, size_t ccap,
                                 size_t* n_corrupt, uint32_t* missing_pos, size_t mcap, size_t* n_missing) {
    if (n_corrupt) *n_corrupt = 0;
    if (n_missing) *n_missing = 0;
    if (!Handles::alive(h) || !finish_args_valid(h->run, corrupt_store, ccap, missing_pos, mcap)) return PBS_ERR_INVALID;
    DeviceGuard dg(h->dev);
    if (!dg.ok) return PBS_ERR_NO_DEVICE;
    return finish_on(h, res, corrupt_store, ccap, n_corrupt, missing_pos, mcap, n_missing);
}

extern "C" int pbs_verify_index_device(pbs_verify* h, const uint8_t* image, size_t len, int index_mode,
                                       const uint64_t* info_size, const uint8_t* info_csum,
                                       const uint8_t* store_blobs_dev, const uint64_t* store_offsets,
                                       size_t budget_bytes, pbs_verify_result* res, uint32_t* corrupt_store, size_t ccap,
                                       size_t* n_corrupt, uint32_t* missing_pos, size_t mcap, size_t* n_missing) {
    if (res) std::memset(res, 0, sizeof(*res));
    if (n_corrupt) *n_corrupt = 0;
    if (n_missing) *n_missing = 0;
    if (!Handles::alive(h) || h->run.open || !mode_valid(index_mode) || (ccap && !corrupt_store) || (mcap && !missing_pos))
        return PBS_ERR_INVALID;
    const size_t m = h->m;
    if (m && !store_offsets) return PBS_ERR_INVALID;
    for (size_t j = 0; j < m; ++j)
        if (store_offsets[j] > store_offsets[j + 1]) return PBS_ERR_INVALID;
    if (m && store_offsets[m] > store_offsets[0] && !store_blobs_dev) return PBS_ERR_INVALID;
    IndexLayout lo;
    int rc = index_layout(image, len, &lo);
    if (rc != PBS_OK) return rc;
    const uint32_t chk = index_check(image, lo, info_size, info_csum);
    if (chk != PBS_VERIFY_INDEX_OK) {  // no chunk is touched, no state changes (verify.rs:282-289)
        if (res) {
            res->entries = lo.n;
            res->index_check = chk;
        }
        return PBS_OK;
    }
    DeviceGuard dg(h->dev);
    if (!dg.ok) return PBS_ERR_NO_DEVICE;
    try {
        std::vector<uint8_t> digests, enc;
        std::vector<uint64_t> sizes;
        index_entries(image, lo, digests, sizes);
        rc = plan_on(h, digests.data(), sizes.data(), lo.n, index_mode, nullptr);
        if (rc != PBS_OK) return rc;
        const IndexRun& run = h->run;
        const size_t k = run.todo_store.size();
        auto blob_len = [&](size_t t) { return store_offsets[run.todo_store[t] + 1] - store_offsets[run.todo_store[t]]; };
        ArenaLease ar(vpool(), h->dev);
        std::vector<uint64_t> spans(2 * k);
        for (size_t t = 0; t < k; ++t) {
            spans[2 * t] = store_offsets[run.todo_store[t]];
            spans[2 * t + 1] = blob_len(t);
        }
        rc = magic_flags(*ar, kBlobSlots, h->st, store_blobs_dev, spans, k, enc, nullptr);
        std::vector<uint64_t> src, dst, lens, offs;
        for (size_t t0 = 0; rc == PBS_OK && t0 < k;) {
            const size_t t1 = batch_end(run, t0, budget_bytes, enc.data(), blob_len);
            src.clear();
            dst.clear();
            lens.clear();
            offs.assign(1, 0);
            for (size_t t = t0; t < t1; ++t) {
                src.push_back(spans[2 * t]);
                dst.push_back(offs.back());
                lens.push_back(spans[2 * t + 1]);
                offs.push_back(offs.back() + spans[2 * t + 1]);
            }
            // blobs that already follow one another in the store are submitted where they lie
            bool in_place = offs.back() != 0;
            for (size_t t = t0 + 1; t < t1 && in_place; ++t) in_place = spans[2 * t] == spans[2 * t - 2] + spans[2 * t - 1];
            if (in_place) {
                for (size_t t = t0; t <= t1; ++t) offs[t - t0] += spans[2 * t0];
                rc = submit_on(h, store_blobs_dev, offs.data(), nullptr, t1 - t0, nullptr, nullptr, nullptr);
            } else {
                uint8_t* d_pack = ar->get<uint8_t>(kVsPack, (size_t)offs.back(), false);
                if (!d_pack) {
                    rc = PBS_ERR_NOMEM;
                    break;
                }
                if (offs.back())
                    rc = pbs_copy_segments_device(store_blobs_dev, d_pack, src.data(), dst.data(), lens.data(), t1 - t0,
                                                  h->st);
                if (rc == PBS_OK) rc = submit_on(h, d_pack, offs.data(), nullptr, t1 - t0, nullptr, nullptr, nullptr);
            }
            t0 = t1;
        }
    } catch (const std::bad_alloc&) {
        rc = PBS_ERR_NOMEM;
    }
    if (rc != PBS_OK) {
        h->run.clear();  // (the states of the blobs already submitted stay: they were verified)
        return rc;
    }
    return finish_on(h, res, corrupt_store, ccap, n_corrupt, missing_pos, mcap, n_missing);
}
