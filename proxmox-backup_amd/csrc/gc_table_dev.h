// The device side of the store table that garbage collection (pbs_gc.hip), the verify job
// (pbs_verify.hip) and the sync job (pbs_sync.hip, which also inserts into it) share: the chunk store's listing as an open-addressing table of u32 store
// positions (capacity 2^L >= max(2 m, 64), home slot pbs_gc_home_slot, linear probing with
// wrap-around; gc_common.h has the size rule and the hash constant).  Device code: include it
// from a .hip file only.  Everything is in an unnamed namespace, so each translation unit gets
// kernels of its own.
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

inline unsigned blocks_for(uint64_t n) { return (unsigned)((n + kGcThreads - 1) / kGcThreads); }

}  // namespace
}  // namespace gc
}  // namespace pbs
