// The device side of the store table that every datastore job shares (garbage collection, verify,
// sync, backup): the chunk store's listing as an open-addressing table of u32 store positions
// (capacity 2^L >= max(2 m, 64), home slot pbs_gc_home_slot, linear probing with wrap-around;
// gc_common.h has the size rule and the hash constant), its build kernel, the read-only probe,
// and the block-wide count, ordered rank and compaction that the jobs' plans are made of.  The
// insert into a table that grows is grow_table_dev.h.  Device code: include it from a .hip file
// only.  Everything is in an unnamed namespace, so each translation unit gets kernels of its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gc_common.h"

namespace pbs {
namespace gc {
namespace {

constexpr uint32_t kEmpty = 0xFFFFFFFFu;
constexpr int kGcThreads = 256;
constexpr int kGcWaves = kGcThreads / 64;

struct Dig {
    uint64_t w[4];
};
// four 8-byte loads: the digests of a .didx image are 8- but not 16-byte aligned
__device__ __forceinline__ Dig load_digest(const uint8_t* __restrict__ p) {
    const uint64_t* q = reinterpret_cast<const uint64_t*>(p);
    Dig d;
    d.w[0] = q[0];
    d.w[1] = q[1];
    d.w[2] = q[2];
    d.w[3] = q[3];
    return d;
}
__device__ __forceinline__ uint64_t home_slot(uint64_t w0, uint32_t shift) {
    return (__builtin_bswap64(w0) * kGcHashMul) >> shift;  // w0: the first 8 bytes, loaded little-endian
}
// does store entry j carry the digest d?  (first word first: most slots of a cluster differ there)
__device__ __forceinline__ bool same_digest(const uint8_t* __restrict__ store, uint32_t j, const Dig& d) {
    const uint64_t* q = reinterpret_cast<const uint64_t*>(store + 32ull * j);
    if (q[0] != d.w[0]) return false;
    return q[1] == d.w[1] && q[2] == d.w[2] && q[3] == d.w[3];
}

// One lane per store entry: claims the first free slot from its home slot on.  The table holds
// 2^L >= 2 m slots, so a free slot always comes.
__global__ __launch_bounds__(kGcThreads) void gc_build_kernel(const uint8_t* __restrict__ store, uint64_t m,
                                                              uint32_t* __restrict__ table, uint32_t shift,
                                                              uint64_t mask) {
    const uint64_t j = (uint64_t)blockIdx.x * kGcThreads + threadIdx.x;
    if (j >= m) return;
    uint64_t s = home_slot(*reinterpret_cast<const uint64_t*>(store + 32 * j), shift);
    while (atomicCAS(&table[s], kEmpty, (uint32_t)j) != kEmpty) s = (s + 1) & mask;
}

// The read-only probe: the LOWEST store position carrying the digest d, or kEmpty.  The lane walks
// its cluster from the home slot to the first free slot (equal digests of the listing sit in slots
// of their own, so the walk goes to the cluster's end).  No kernel changes the table meanwhile.
__device__ __forceinline__ uint32_t lowest_entry(const uint32_t* __restrict__ table, const uint8_t* __restrict__ store,
                                                 const Dig& d, uint32_t shift, uint64_t mask) {
    uint32_t j = kEmpty;
    for (uint64_t s = home_slot(d.w[0], shift);; s = (s + 1) & mask) {
        const uint32_t k = table[s];
        if (k == kEmpty) break;
        if (k < j && same_digest(store, k, d)) j = k;
    }
    return j;
}

// the block's sum of one flag per lane, by ballots; all threads call it (wcnt: kGcWaves words of LDS)
__device__ __forceinline__ uint32_t block_count(bool flag, uint32_t* wcnt) {
    const unsigned long long b = __ballot(flag);
    if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = (uint32_t)__popcll(b);
    __syncthreads();
    uint32_t c = 0;
    for (int w = 0; w < kGcWaves; ++w) c += wcnt[w];
    __syncthreads();  // (wcnt is written again by the next call)
    return c;
}

// A flagged lane's rank among the flagged lanes before it, over the whole grid: block_start is
// the exclusive sum of the blocks' counts (block_count), the rank inside the block comes from the
// ballots.  All threads call it.
__device__ __forceinline__ uint64_t ordered_rank(bool flag, unsigned long long block_start, uint32_t* wcnt) {
    const unsigned long long b = __ballot(flag);
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wcnt[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    uint64_t rank = block_start + __popcll(b & ((1ull << lane) - 1));
    for (uint32_t w = 0; w < wave; ++w) rank += wcnt[w];
    __syncthreads();  // (wcnt is written again by the next call)
    return rank;
}

// The positions with flag != 0, ascending, as far as `cap` goes; with kGather, out2[rank] =
// gather[position] beside it (without, both pointers are NULL).
template <bool kGather>
__global__ __launch_bounds__(kGcThreads) void gc_compact_kernel(
    const uint8_t* __restrict__ flag, uint64_t n, const unsigned long long* __restrict__ block_start,
    uint32_t* __restrict__ out, uint64_t cap, const uint32_t* __restrict__ gather, uint32_t* __restrict__ out2) {
    __shared__ uint32_t wcnt[kGcWaves];
    const uint64_t i = (uint64_t)blockIdx.x * kGcThreads + threadIdx.x;
    const bool f = i < n && flag[i] != 0;
    const uint64_t rank = ordered_rank(f, block_start[blockIdx.x], wcnt);
    if (!f || rank >= cap) return;
    out[rank] = (uint32_t)i;
    if (kGather) out2[rank] = gather[i];
}

inline unsigned blocks_for(uint64_t n) { return (unsigned)((n + kGcThreads - 1) / kGcThreads); }

}  // namespace
}  // namespace gc
}  // namespace pbs
