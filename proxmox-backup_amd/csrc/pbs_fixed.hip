// Device side of the fixed-size chunk path (include/pbs_fixed.h): the dirty map of two
// resident images, the digests of an image's (dirty) chunks over the kernels of pbs_digest.hip,
// and the restore of a range through pbs_restore_range_device ("The fixed
// path").
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "dev_arena.h"
#include "dev_copy.h"
#include "pbs_chunker.h"
#include "pbs_chunker_internal.h"
#include "pbs_fixed.h"

namespace pbs {
namespace fixed {
namespace {

constexpr uint64_t kMinChunk = 4096;     // the smallest chunk_size of the device calls
constexpr uint32_t kItemBytes = 262144;  // bytes of both images one workgroup compares per item
constexpr int kDirtyThreads = 256;
constexpr uint64_t kPackBytes = 1ull << 30;  // scattered long chunks packed per hybrid digest call

// Item k is bytes [k * item, min((k + 1) * item, size)) of both images, item = min(chunk_size,
// kItemBytes): both are powers of two, so an item never straddles a chunk and its chunk is
// k >> item_shift (item_shift = log2(chunk_size / item)).  Lane t compares the 16-byte vectors
// t, t + 256, ... of the item, four from each image in flight; the < 16 tail bytes are compared
// bytewise by the first lanes.  Nothing outside the item is read.  A wave that saw a
// difference stores 1 to the chunk's flag: a plain byte store from one lane; every writer of
// a flag writes the same value, and the flags were cleared on the stream before the launch.
__global__ __launch_bounds__(kDirtyThreads) void fixed_dirty_kernel(uint64_t prev, uint64_t cur, uint64_t size,
                                                                    uint32_t item, uint32_t item_shift,
                                                                    uint64_t nitems, uint8_t* __restrict__ dirty) {
    const uint32_t t = threadIdx.x;
    for (uint64_t k = blockIdx.x; k < nitems; k += gridDim.x) {
        const uint64_t off = k * item;
        const uint32_t len = (uint32_t)(size - off < item ? size - off : item);
        const gcbytes a = (gcbytes)(prev + off);
        const gcbytes b = (gcbytes)(cur + off);
        const uint32_t nvec = len >> 4;
        u32x4 acc = {0, 0, 0, 0};
        uint32_t v = t;
        for (; v + 3 * kDirtyThreads < nvec; v += 4 * kDirtyThreads) {
            const u32x4 a0 = load16(a + 16 * v);
            const u32x4 a1 = load16(a + 16 * (v + kDirtyThreads));
            const u32x4 a2 = load16(a + 16 * (v + 2 * kDirtyThreads));
            const u32x4 a3 = load16(a + 16 * (v + 3 * kDirtyThreads));
            const u32x4 b0 = load16(b + 16 * v);
            const u32x4 b1 = load16(b + 16 * (v + kDirtyThreads));
            const u32x4 b2 = load16(b + 16 * (v + 2 * kDirtyThreads));
            const u32x4 b3 = load16(b + 16 * (v + 3 * kDirtyThreads));
            acc |= (a0 ^ b0) | (a1 ^ b1) | (a2 ^ b2) | (a3 ^ b3);
        }
        for (; v < nvec; v += kDirtyThreads) acc |= load16(a + 16 * v) ^ load16(b + 16 * v);
        uint32_t diff = acc.x | acc.y | acc.z | acc.w;
        const uint32_t tail = nvec << 4;  // first tail byte
        if (t < len - tail) diff |= (uint32_t)(a[tail + t] ^ b[tail + t]);
        if (__builtin_amdgcn_ballot_w64(diff != 0) != 0 && (t & 63) == 0) dirty[k >> item_shift] = 1;
    }
}

// the ones among n flags (0/1 bytes), added to *count (zeroed on the stream before)
__global__ __launch_bounds__(256) void count_flags_kernel(const uint8_t* __restrict__ flags, uint64_t n,
                                                          unsigned long long* __restrict__ count) {
    unsigned int c = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        c += flags[i] != 0;
    for (int s = 32; s > 0; s >>= 1) c += __shfl_down(c, s, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, (unsigned long long)c);
}

ArenaPool& fpool() {
    static ArenaPool* p = new ArenaPool;  // never destroyed (HIP may be torn down first at exit);
    return *p;                            // its idle arenas go with every pool's when memory runs out
}

// PBS_OK for a power of two >= 4096
int check_chunk_size(uint64_t chunk_size) {
    if (__builtin_popcountll(chunk_size) != 1) return PBS_ERR_NOT_POW2;
    return chunk_size < kMinChunk ? PBS_ERR_INVALID : PBS_OK;
}

}  // namespace
}  // namespace fixed
}  // namespace pbs

using namespace pbs;
using namespace pbs::fixed;

extern "C" int pbs_fixed_dirty_device(const uint8_t* prev_dev, const uint8_t* cur_dev, uint64_t size,
                                      uint64_t chunk_size, uint8_t* dirty_dev, size_t* n_dirty, void* hip_stream) {
    if (n_dirty) *n_dirty = 0;
    const int cs = check_chunk_size(chunk_size);
    if (cs != PBS_OK) return cs;
    if (size == 0) return PBS_OK;
    if (!prev_dev || !cur_dev || !dirty_dev) return PBS_ERR_INVALID;
    hipStream_t st = (hipStream_t)hip_stream;
    const StreamDevice sd(st);
    if (!sd.ok) return PBS_ERR_NO_DEVICE;
    DeviceGuard dg(sd.dev);
    if (!dg.ok) return PBS_ERR_NO_DEVICE;
    const uint64_t n = pbs_fidx_count(size, chunk_size);
    const uint32_t item = (uint32_t)std::min<uint64_t>(chunk_size, kItemBytes);
    const uint32_t item_shift = (uint32_t)__builtin_ctzll(chunk_size / item);
    const uint64_t nitems = size / item + (size % item ? 1 : 0);
    ArenaLease ar(fpool(), sd.dev);
    unsigned long long* d_count = n_dirty ? ar->get<unsigned long long>(0, 8) : nullptr;
    if (n_dirty && !d_count) return PBS_ERR_NOMEM;
    int rc = PBS_OK;
    (void)hipGetLastError();
    if (hipMemsetAsync(dirty_dev, 0, n, st) != hipSuccess) {
        rc = PBS_ERR_HIP;
    } else {
        const unsigned grid = (unsigned)std::min<uint64_t>(nitems, (uint64_t)std::max(sd.ncu, 1) * 8);
        hipLaunchKernelGGL(fixed_dirty_kernel, dim3(grid), dim3(kDirtyThreads), 0, st, (uint64_t)(uintptr_t)prev_dev,
                           (uint64_t)(uintptr_t)cur_dev, size, item, item_shift, nitems, dirty_dev);
        if (hipGetLastError() != hipSuccess) rc = PBS_ERR_HIP;
    }
    unsigned long long cnt = 0;
    if (rc == PBS_OK && n_dirty) {
        const unsigned cgrid = (unsigned)std::min<uint64_t>((n + 255) / 256, (uint64_t)std::max(sd.ncu, 1) * 4);
        if (hipMemsetAsync(d_count, 0, 8, st) != hipSuccess) {
            rc = PBS_ERR_HIP;
        } else {
            hipLaunchKernelGGL(count_flags_kernel, dim3(cgrid), dim3(256), 0, st, dirty_dev, n, d_count);
            if (hipGetLastError() != hipSuccess ||
                hipMemcpyAsync(&cnt, d_count, 8, hipMemcpyDeviceToHost, st) != hipSuccess)
                rc = PBS_ERR_HIP;
        }
    }
    if (hipStreamSynchronize(st) != hipSuccess && rc == PBS_OK) rc = PBS_ERR_HIP;  // (before the arena goes back)
    if (rc == PBS_OK && n_dirty) *n_dirty = (size_t)cnt;
    return rc;
}

extern "C" int pbs_fixed_digests_device(const uint8_t* dev_data, uint64_t size, uint64_t chunk_size,
                                        const uint8_t* key, size_t key_len, const uint8_t* dirty,
                                        const uint8_t* prev_digests, uint8_t* digests, uint8_t index_csum[32],
                                        pbs_fixed_digest_timing* timing, void* hip_stream) {
    const HClock::time_point t0 = HClock::now();
    if (timing) std::memset(timing, 0, sizeof(*timing));
    const int cs = check_chunk_size(chunk_size);
    if (cs != PBS_OK) return cs;
    if ((dirty && !prev_digests) || key_len > PBS_DIGEST_MAX_KEY || (key_len && !key)) return PBS_ERR_INVALID;
    const uint64_t n = pbs_fidx_count(size, chunk_size);
    if (n > 0xFFFFFFFFull || (n && (!digests || !dev_data))) return PBS_ERR_INVALID;
    // the grid's bounds and the chunks to hash, in index order
    std::vector<uint64_t> bounds(n + 1);
    for (uint64_t i = 0; i <= n; ++i) bounds[i] = std::min<uint64_t>(i * chunk_size, size);
    std::vector<uint32_t> list;
    list.reserve(n);
    uint64_t hashed_bytes = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (dirty && !dirty[i]) {
            std::memcpy(digests + 32 * i, prev_digests + 32 * i, 32);
        } else {
            list.push_back((uint32_t)i);
            hashed_bytes += bounds[i + 1] - bounds[i];
        }
    }
    const size_t g = list.size();
    hipStream_t st = (hipStream_t)hip_stream;
    int rc = PBS_OK;
    double gpu_ms = 0;
    if (g && chunk_size >= (1u << 20) && list[g - 1] - list[0] + 1 == g) {
        // long chains, one run of consecutive indices: the hybrid split, unchanged, where they lie
        pbs_digest_hybrid_timing ht{};
        rc = pbs_digest_chunks_hybrid(dev_data, nullptr, size, 0, bounds.data() + list[0], g, key, key_len,
                                      digests + 32 * (size_t)list[0], nullptr, &ht, hip_stream);
        gpu_ms = ht.gpu_ms;
    } else if (g && chunk_size >= (1u << 20)) {
        // long chains, scattered: the hybrid call wants chunks back to back, so the dirty chunks
        // are packed into scratch by the segment copy kernel, up to kPackBytes per call (one
        // hybrid call per run of indices cost a synchronisation and a one-chunk host share
        // each: 1.7 ms per run, profiles/fixed/)
        const StreamDevice sd(st);
        if (!sd.ok) return PBS_ERR_NO_DEVICE;
        DeviceGuard dg(sd.dev);
        if (!dg.ok) return PBS_ERR_NO_DEVICE;
        ArenaLease ar(fpool(), sd.dev);
        const uint64_t pack_cap = std::max<uint64_t>(kPackBytes, chunk_size);
        uint8_t* d_pack = ar->get<uint8_t>(4, std::min<uint64_t>(pack_cap, hashed_bytes), false);
        if (!d_pack) return PBS_ERR_NOMEM;
        std::vector<uint64_t> src, dst, lens, pb;
        std::vector<uint8_t> pd;
        for (size_t p = 0; p < g && rc == PBS_OK;) {
            src.clear(), dst.clear(), lens.clear();
            pb.assign(1, 0);
            size_t q = p;
            for (; q < g; ++q) {
                const uint64_t l = bounds[list[q] + 1] - bounds[list[q]];
                if (q > p && pb.back() + l > pack_cap) break;
                src.push_back(bounds[list[q]]);
                dst.push_back(pb.back());
                lens.push_back(l);
                pb.push_back(pb.back() + l);
            }
            pd.resize(32 * (q - p));
            pbs_digest_hybrid_timing ht{};
            rc = pbs_copy_segments_device(dev_data, d_pack, src.data(), dst.data(), lens.data(), q - p, hip_stream);
            if (rc == PBS_OK)
                rc = pbs_digest_chunks_hybrid(d_pack, nullptr, pb.back(), 0, pb.data(), q - p, key, key_len, pd.data(),
                                              nullptr, &ht, hip_stream);
            gpu_ms += ht.gpu_ms;
            for (size_t k = p; k < q && rc == PBS_OK; ++k)
                std::memcpy(digests + 32 * (size_t)list[k], pd.data() + 32 * (k - p), 32);
            p = q;
        }
        if (hipStreamSynchronize(st) != hipSuccess && rc == PBS_OK) rc = PBS_ERR_HIP;  // (before the arena goes back)
    } else if (g) {
        const StreamDevice sd(st);
        if (!sd.ok) return PBS_ERR_NO_DEVICE;
        DeviceGuard dg(sd.dev);
        if (!dg.ok) return PBS_ERR_NO_DEVICE;
        // the short last chunk, if it is to be hashed, at the end of the order: the lanes of a
        // wave then hold equal lengths (the order is "longest first" already)
        ArenaLease ar(fpool(), sd.dev);
        uint64_t* d_bounds = ar->get<uint64_t>(1, (n + 1) * 8);
        uint32_t* d_order = ar->get<uint32_t>(2, g * 4);
        uint8_t* d_dig = ar->get<uint8_t>(3, n * 32);
        hipEvent_t e0 = ar->event(0), e1 = ar->event(1);
        std::vector<uint8_t> gd(n * 32);
        float ms = 0;
        if (!d_bounds || !d_order || !d_dig) {
            rc = PBS_ERR_NOMEM;
        } else if (!e0 || !e1 ||
                   hipMemcpyAsync(d_bounds, bounds.data(), (n + 1) * 8, hipMemcpyHostToDevice, st) != hipSuccess ||
                   hipMemcpyAsync(d_order, list.data(), g * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
                   hipEventRecord(e0, st) != hipSuccess) {
            rc = PBS_ERR_HIP;
        } else {
            // lane k hashes chunk order[k] and writes at 32 * order[k]: exactly the subset
            rc = pbs_digest_chunks_async(dev_data, size, 0, d_bounds, d_order, g, key, key_len, d_dig, hip_stream);
            if (rc == PBS_OK && (hipEventRecord(e1, st) != hipSuccess ||
                                 hipMemcpyAsync(gd.data(), d_dig, n * 32, hipMemcpyDeviceToHost, st) != hipSuccess))
                rc = PBS_ERR_HIP;
        }
        if (hipStreamSynchronize(st) != hipSuccess && rc == PBS_OK) rc = PBS_ERR_HIP;  // (before the arena goes back)
        if (rc == PBS_OK && hipEventElapsedTime(&ms, e0, e1) != hipSuccess) rc = PBS_ERR_HIP;
        gpu_ms = ms;
        if (rc == PBS_OK)
            for (uint32_t i : list) std::memcpy(digests + 32 * (size_t)i, gd.data() + 32 * (size_t)i, 32);
    }
    if (rc == PBS_OK && index_csum) pbs_sha256(digests, 32 * n, index_csum);
    if (timing) {
        timing->total_ms = hms(t0);
        timing->gpu_ms = gpu_ms;
        timing->hashed_chunks = g;
        timing->hashed_bytes = hashed_bytes;
    }
    return rc;
}

extern "C" int pbs_restore_fixed_range_device(const uint8_t* digests, size_t n, uint64_t size, uint64_t chunk_size,
                                              const uint8_t* store_blobs_dev, const uint64_t* store_offsets,
                                              const uint8_t* store_digests, size_t m, const pbs_crypt_config* cfg,
                                              uint64_t offset, uint64_t len, uint8_t* out_dev, uint8_t* entry_status,
                                              pbs_restore_timing* timing, void* hip_stream) {
    if (timing) std::memset(timing, 0, sizeof(*timing));
    const int cs = check_chunk_size(chunk_size);
    if (cs != PBS_OK) return cs;
    if (n != pbs_fidx_count(size, chunk_size) || offset + len < offset || offset + len > size)
        return PBS_ERR_INVALID;
    if (len) {
        // the covering entries [i0, i1] by chunk_from_offset (fixed_index.rs:205-214); the
        // dynamic call's binary search over the ends below finds the same two
        size_t i0 = 0, i1 = 0;
        if (pbs_fidx_chunk_from_offset(size, chunk_size, offset, &i0, nullptr) != PBS_OK ||
            pbs_fidx_chunk_from_offset(size, chunk_size, offset + len - 1, &i1, nullptr) != PBS_OK || i0 > i1 ||
            i1 >= n)
            return PBS_ERR_INVALID;
    }
    // chunk_info's ends (:165-182): the last one clipped, so a last chunk that decodes to
    // chunk_size bytes instead is BAD_SIZE there
    std::vector<uint64_t> ends(n);
    for (size_t i = 0; i < n; ++i) ends[i] = std::min<uint64_t>((uint64_t)(i + 1) * chunk_size, size);
    return pbs_restore_range_device(ends.data(), digests, n, store_blobs_dev, store_offsets, store_digests, m, cfg,
                                    offset, len, out_dev, entry_status, timing, hip_stream);
}
