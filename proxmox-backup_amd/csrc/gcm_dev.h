// What the sealing kernels (pbs_crypt.hip) and the opening kernels (pbs_decode.hip) of the
// AES-256-GCM blob stage share: the per-key device record, the per-blob context, the crypt
// config, the LDS forms of Te0 and of the H^256 table.  The geometry and the table layouts
// are described at the top of pbs_crypt.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <map>
#include <mutex>

#include "aes_gcm.h"
#include "dev_copy.h"
#include "pbs_blob.h"

namespace pbs {
namespace gcm {

// the geometry both directions share (pbs_crypt.hip states it for the sealing kernel and
// checks it against these)
constexpr int kGcmThreads = 256;
constexpr int kGcmRows = PBS_GCM_SEGMENT_BYTES / 16 / kGcmThreads;  // 16 blocks per lane and segment
constexpr uint32_t kGcmSegBlocks = PBS_GCM_SEGMENT_BYTES / 16;
constexpr int kGcmGroupsPerCu = 3;  // 40 KiB of LDS and 160-164 VGPRs each: three fit a CU

// what the kernels read of a key, one copy per device
struct KeyDev {
    uint32_t rk[60];
    uint32_t pad[4];
    uint32_t te0[256];
    uint8_t tab_g[32 * 16 * 16];  // [nibble position][value]: (value at position) * H^256, as bytes
    B128 lane_pow[kGcmThreads];   // H^(256 - t)
    B128 h, h_seg;                // H, H^4096
};

struct BlobCtx {
    uint4 j0;  // big-endian columns
    B128 ek;   // AES_K(J0)
};

}  // namespace gcm
}  // namespace pbs

struct pbs_crypt_config {
    uint8_t id_key[32];
    pbs::gcm::KeyDev key;
    std::mutex mu;
    std::map<int, pbs::gcm::KeyDev*> dev;
};

namespace pbs {
namespace gcm {

// the config's key record on device `dev`, copied there on first use (pbs_crypt.hip)
KeyDev* device_key(const pbs_crypt_config* cc, int dev);

// (u32x4: dev_copy.h) a 16-byte block of a payload, at any address, as the GCM kernels load and store it
typedef u32x4 u32x4_u __attribute__((aligned(1)));

__host__ __device__ __forceinline__ B128 words_to_b128(uint4 w) {
    return B128{(uint64_t)__builtin_bswap32(w.x) << 32 | __builtin_bswap32(w.y),
                (uint64_t)__builtin_bswap32(w.z) << 32 | __builtin_bswap32(w.w)};
}

// x * H^256 with x and the result as the block's four little-endian memory words
__host__ __device__ __forceinline__ uint4 mul_tab(const uint4* tg, uint4 x) {
    const uint32_t w[4] = {x.x, x.y, x.z, x.w};
    uint4 r = make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const uint32_t b = (w[i >> 2] >> (8 * (i & 3))) & 255u;
        const uint4 a = tg[(2 * i) * 16 + (b >> 4)];
        const uint4 c = tg[(2 * i + 1) * 16 + (b & 15u)];
        r.x ^= a.x ^ c.x;
        r.y ^= a.y ^ c.y;
        r.z ^= a.z ^ c.z;
        r.w ^= a.w ^ c.w;
    }
    return r;
}

struct Te0Lds {
    const uint32_t* t;  // te + (lane & 31)
    __device__ __forceinline__ uint32_t operator()(uint32_t x) const { return t[x << 5]; }
};

}  // namespace gcm
}  // namespace pbs
