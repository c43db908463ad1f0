// Device code that the verify job (pbs_verify.hip) and the sync job (pbs_sync.hip) share: the
// block's count of one flag per lane, and the magic read that tells the encrypted blobs of a
// submit apart.  Include it from a .hip file only; everything is in an unnamed namespace, so each
// translation unit gets kernels of its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gc_table_dev.h"
#include "pbs_blob.h"
#include "verify_common.h"

namespace pbs {
namespace verify {
namespace {

using namespace pbs::gc;

// the block's sum of one flag per lane into out (thread 0), by ballots; all threads call it
__device__ __forceinline__ uint32_t block_count(bool flag, uint32_t* wcnt) {
    const unsigned long long b = __ballot(flag);
    if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = (uint32_t)__popcll(b);
    __syncthreads();
    uint32_t c = 0;
    for (int w = 0; w < kGcWaves; ++w) c += wcnt[w];
    __syncthreads();  // (wcnt is written again by the next call)
    return c;
}

// One lane per submitted blob: is its magic one of the two encrypted ones?  spans[2 t] is the
// blob's start in `blobs`, spans[2 t + 1] its length; a blob under a header has no magic.
__global__ __launch_bounds__(kGcThreads) void verify_magic_kernel(const uint8_t* __restrict__ blobs,
                                                                  const uint64_t* __restrict__ spans, uint64_t k,
                                                                  uint8_t* __restrict__ enc) {
    const uint64_t t = (uint64_t)blockIdx.x * kGcThreads + threadIdx.x;
    if (t >= k) return;
    uint8_t e = 0;
    if (spans[2 * t + 1] >= PBS_BLOB_HEADER_SIZE) {
        const uint8_t* p = blobs + spans[2 * t];
        uint64_t v = 0;
#pragma unroll
        for (int b = 0; b < 8; ++b) v |= (uint64_t)p[b] << (8 * b);  // (a blob starts at any alignment)
        e = v == kEncMagicLe || v == kEncComprMagicLe;
    }
    enc[t] = e;
}

}  // namespace
}  // namespace verify
}  // namespace pbs
