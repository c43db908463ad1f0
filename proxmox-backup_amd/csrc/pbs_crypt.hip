// AES-256-GCM of blob payloads on the GPU: the `Some(config)` half of `DataBlob::encode`
// (pbs-datastore/src/data_blob.rs:107-131) -- `CryptConfig::encrypt_to` with a random
// 16-byte IV, empty AAD (pbs-tools/src/crypt_config.rs:127-150).  C ABI: include/pbs_blob.h.
//
// The blob encoder has placed every plaintext payload at blob + 44; three launches turn
// the images into encrypted blobs in place:
//  1. gcm_prepare_kernel, one lane per blob: IV into the header, J0 = ((IV H) ^ 128) H
//     (a 16-byte IV goes through GHASH; the 96-bit shortcut does not apply) and AES_K(J0).
//  2. gcm_ctr_ghash_kernel, one 256-lane workgroup per 64 KiB segment (4096 GCM blocks):
//     lane t takes blocks t, t + 256, ... of the segment (each row of the workgroup is 4 KiB
//     of consecutive bytes), encrypts block k with AES_K(inc32^(k+1)(J0)) -- the counter is
//     J0's low word plus k + 1 in 32-bit arithmetic, so it wraps as inc32 does -- writes
//     the ciphertext and folds it into its Horner sum acc = acc H^256 ^ C.  The lane sums
//     times H^(256 - t) XOR-reduce to the segment's partial P = sum C_q H^(4096 - q).
//     Segments are counted from the chunk's END, so only the first one is ragged; its
//     missing leading blocks are zeros, which a Horner sum ignores.
//  3. gcm_tag_kernel, one lane per blob: Y = Horner of the partials by H^4096, then
//     tag = ((Y ^ [0]_64 [8 len]_64) H) ^ AES_K(J0).
// AES: the single table Te0, 32 copies in LDS laid out [x][lane & 31] (ds_read_b32 banks
// are (a / 4) % 32 per 32-lane half, so lane l always reads bank l % 32: conflict-free
// whatever the data, and the access pattern does not depend on key or plaintext); the
// other three columns by rotation, the last round's S-box from Te0's second byte; the
// round keys are read through a uniform pointer (scalar registers).  GHASH: the multiply
// by the fixed H^256 is 32 lookups in a per-key 4-bit table (32 nibble positions x 16
// entries x 16 bytes = 8 KiB of LDS); the 16 entries of one position fill exactly one
// 256-byte bank row, so two lanes of a ds_read_b128 group either read the same address
// (broadcast) or different banks.  The rare multiplies by other elements (lane powers,
// H^4096, the IV) are the plain shift-and-xor of aes_gcm.h.
// GCM blocks count from the payload start (blob + 44, any alignment): full blocks move as
// unaligned 16-byte global accesses, the last partial block byte by byte; nothing outside
// [blob + 12, blob end) is read or written.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <sys/random.h>

#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <vector>

#include "aes_gcm.h"
#include "dev_arena.h"
#include "gcm_dev.h"
#include "pbs_blob.h"
#include "pbs_chunker.h"
#include "pbs_chunker_internal.h"
#include "pbs_digest.h"

using pbs::gcm::B128;

namespace pbs {
namespace gcm {

constexpr int kThreads = 256;
constexpr int kRows = PBS_GCM_SEGMENT_BYTES / 16 / kThreads;  // 16 blocks per lane and segment
constexpr uint32_t kSegBlocks = PBS_GCM_SEGMENT_BYTES / 16;
constexpr int kGroupsPerCu = 3;  // 40 KiB of LDS and 160 VGPRs each: three fit a CU
static_assert(kThreads == kGcmThreads && kRows == kGcmRows && kSegBlocks == kGcmSegBlocks &&
                  kGroupsPerCu == kGcmGroupsPerCu,
              "the sealing kernel's geometry is the one gcm_dev.h shares with pbs_decode.hip");

namespace {

void wipe(void* p, size_t n) {
    volatile uint8_t* v = static_cast<volatile uint8_t*>(p);
    for (size_t i = 0; i < n; ++i) v[i] = 0;
}

void hmac_sha256(const uint8_t key[32], const uint8_t* msg, size_t len, uint8_t out[32]) {
    uint8_t in[64 + 64], outer[64 + 32];
    for (int i = 0; i < 64; ++i) {
        const uint8_t k = i < 32 ? key[i] : 0;
        in[i] = k ^ 0x36;
        outer[i] = k ^ 0x5C;
    }
    std::memcpy(in + 64, msg, len);  // len <= 64
    pbs_sha256(in, 64 + len, outer + 64);
    pbs_sha256(outer, 64 + 32, out);
    wipe(in, sizeof in);
    wipe(outer, sizeof outer);
}

// PBKDF2-HMAC-SHA256, one 32-byte block
void pbkdf2_sha256_32(const uint8_t pass[32], const char* salt, size_t salt_len, int rounds, uint8_t out[32]) {
    uint8_t u[64] = {};
    std::memcpy(u, salt, salt_len);
    u[salt_len + 3] = 1;  // INT(1)
    uint8_t t[32];
    hmac_sha256(pass, u, salt_len + 4, t);
    std::memcpy(out, t, 32);
    for (int r = 1; r < rounds; ++r) {
        hmac_sha256(pass, t, 32, u);
        std::memcpy(t, u, 32);
        for (int i = 0; i < 32; ++i) out[i] ^= t[i];
    }
    wipe(u, sizeof u);
    wipe(t, sizeof t);
}

B128 nibble_elem(int pos, uint32_t v) {
    return pos < 16 ? B128{(uint64_t)v << (60 - 4 * pos), 0} : B128{0, (uint64_t)v << (60 - 4 * (pos - 16))};
}

void make_key(const uint8_t enc_key[32], KeyDev& k) {
    std::memset(&k, 0, sizeof k);
    make_te0(k.te0);
    aes256_expand_key(enc_key, k.te0, k.rk);
    uint32_t z[4] = {0, 0, 0, 0};
    aes256_encrypt(k.rk, Te0Array{k.te0}, z);
    k.h = B128{(uint64_t)z[0] << 32 | z[1], (uint64_t)z[2] << 32 | z[3]};
    B128 p = k.h;  // H^1
    k.lane_pow[kThreads - 1] = p;
    for (int t = kThreads - 2; t >= 0; --t) k.lane_pow[t] = p = gf_mul(p, k.h);
    const B128 g = k.lane_pow[0];  // H^256
    B128 s = g;
    for (uint32_t e = kThreads; e < kSegBlocks; e *= 2) s = gf_mul(s, s);
    k.h_seg = s;
    for (int pos = 0; pos < 32; ++pos)
        for (uint32_t v = 0; v < 16; ++v) store_block(k.tab_g + (pos * 16 + v) * 16, gf_mul(nibble_elem(pos, v), g));
}

__global__ void gcm_prepare_kernel(const KeyDev* __restrict__ key, const uint8_t* __restrict__ ivs,
                                   const uint64_t* __restrict__ boff, uint64_t n, uint8_t* __restrict__ blobs,
                                   BlobCtx* __restrict__ ctx) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t* const iv = ivs + 16 * i;
    uint8_t* const hdr = blobs + boff[i];
    for (int b = 0; b < 16; ++b) hdr[12 + b] = iv[b];
    const B128 j0 = j0_of_iv16(load_block(iv), key->h);
    uint32_t s[4] = {(uint32_t)(j0.hi >> 32), (uint32_t)j0.hi, (uint32_t)(j0.lo >> 32), (uint32_t)j0.lo};
    ctx[i].j0 = make_uint4(s[0], s[1], s[2], s[3]);
    aes256_encrypt(key->rk, Te0Array{key->te0}, s);
    ctx[i].ek = B128{(uint64_t)s[0] << 32 | s[1], (uint64_t)s[2] << 32 | s[3]};
}

__global__ __launch_bounds__(kThreads) void gcm_ctr_ghash_kernel(
    const KeyDev* __restrict__ key, const uint64_t* __restrict__ items, uint64_t nitems,
    const uint64_t* __restrict__ boff, const BlobCtx* __restrict__ ctx, uint8_t* __restrict__ blobs,
    B128* __restrict__ part) {
    __shared__ uint32_t te[256 * 32];
    __shared__ __attribute__((aligned(256))) uint4 tg[32 * 16];
    __shared__ B128 red[kThreads / 64];
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < 256 * 32; i += kThreads) te[i] = key->te0[i >> 5];
    for (uint32_t i = tid; i < 32 * 16; i += kThreads) tg[i] = reinterpret_cast<const uint4*>(key->tab_g)[i];
    __syncthreads();
    const Te0Lds T{te + (tid & 31u)};
    const uint32_t* const rk = key->rk;
    const B128 lp = key->lane_pow[tid];

    for (uint64_t k = blockIdx.x; k < nitems; k += gridDim.x) {
        const uint64_t it = items[k];
        const uint64_t ci = it >> 32;
        const int64_t seg = (int64_t)(uint32_t)it;
        const uint64_t b0 = boff[ci];
        const uint64_t len = boff[ci + 1] - b0 - PBS_BLOB_ENC_HEADER_SIZE;
        uint8_t* const pay = blobs + b0 + PBS_BLOB_ENC_HEADER_SIZE;
        const uint64_t m = (len + 15) >> 4;
        const uint64_t nseg = (m + kSegBlocks - 1) / kSegBlocks;
        const int64_t first = (int64_t)(m - (nseg - 1) * kSegBlocks);  // blocks of segment 0
        const int64_t kbase = first + (seg - 1) * (int64_t)kSegBlocks + (int64_t)tid;
        const uint4 j0 = ctx[ci].j0;
        uint4 acc = make_uint4(0, 0, 0, 0);
        // (not unrolled: one row at a time keeps 160 VGPRs, three waves per SIMD; two rows in
        // flight took 174 and ran 7 % slower, profiles/crypt/ab_unroll.txt)
#pragma unroll 1
        for (int r = 0; r < kRows; ++r) {
            const int64_t kb = kbase + r * kThreads;
            if (kb < 0) continue;  // the ragged first segment's leading zeros (acc is still 0)
            uint32_t s[4] = {j0.x, j0.y, j0.z, j0.w + (uint32_t)(kb + 1)};  // inc32: low word only
            aes256_encrypt(rk, T, s);
            const uint32_t ks[4] = {__builtin_bswap32(s[0]), __builtin_bswap32(s[1]), __builtin_bswap32(s[2]),
                                    __builtin_bswap32(s[3])};
            const uint64_t off = (uint64_t)kb * 16;
            uint8_t* const p = pay + off;
            uint32_t c[4];
            if (off + 16 <= len) {
                const u32x4 v = *reinterpret_cast<const u32x4_u*>(p);
                c[0] = v.x ^ ks[0];
                c[1] = v.y ^ ks[1];
                c[2] = v.z ^ ks[2];
                c[3] = v.w ^ ks[3];
                u32x4 o;
                o.x = c[0];
                o.y = c[1];
                o.z = c[2];
                o.w = c[3];
                *reinterpret_cast<u32x4_u*>(p) = o;
            } else {  // the chunk's last, partial block: zero padded for GHASH
                const uint32_t rem = (uint32_t)(len - off);
                c[0] = c[1] = c[2] = c[3] = 0;
#pragma unroll
                for (int b = 0; b < 16; ++b)
                    if ((uint32_t)b < rem) {
                        const uint32_t x = (p[b] ^ (ks[b >> 2] >> (8 * (b & 3)))) & 255u;
                        p[b] = (uint8_t)x;
                        c[b >> 2] |= x << (8 * (b & 3));
                    }
            }
            acc = mul_tab(tg, acc);
            acc.x ^= c[0];
            acc.y ^= c[1];
            acc.z ^= c[2];
            acc.w ^= c[3];
        }
        // the lane's sum to the segment end, then the XOR of the 256 lanes
        B128 v = gf_mul(words_to_b128(acc), lp);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            v.hi ^= __shfl_xor(v.hi, o, 64);
            v.lo ^= __shfl_xor(v.lo, o, 64);
        }
        if ((tid & 63u) == 0) red[tid >> 6] = v;
        __syncthreads();
        if (tid == 0) {
            B128 x{0, 0};
#pragma unroll
            for (int i = 0; i < kThreads / 64; ++i) x = gf_xor(x, red[i]);
            part[k] = x;
        }
        __syncthreads();  // red is reused by the next item
    }
}

__global__ void gcm_tag_kernel(const KeyDev* __restrict__ key, const uint64_t* __restrict__ boff,
                               const uint64_t* __restrict__ ifirst, const BlobCtx* __restrict__ ctx,
                               const B128* __restrict__ part, uint64_t n, uint8_t* __restrict__ blobs) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t len = boff[i + 1] - boff[i] - PBS_BLOB_ENC_HEADER_SIZE;
    const B128 hs = key->h_seg;
    B128 y{0, 0};
    for (uint64_t k = ifirst[i]; k < ifirst[i + 1]; ++k) {
        if (k != ifirst[i]) y = gf_mul(y, hs);
        y = gf_xor(y, part[k]);
    }
    y.lo ^= 8 * len;  // [len(A) = 0]_64 || [len(C)]_64
    y = gf_xor(gf_mul(y, key->h), ctx[i].ek);
    store_block(blobs + boff[i] + 28, y);
}

}  // namespace

KeyDev* device_key(const pbs_crypt_config* cc, int dev) {
    pbs_crypt_config* c = const_cast<pbs_crypt_config*>(cc);
    std::lock_guard<std::mutex> g(c->mu);
    auto it = c->dev.find(dev);
    if (it != c->dev.end()) return it->second;
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess) return nullptr;
    if (cur != dev && hipSetDevice(dev) != hipSuccess) return nullptr;
    KeyDev* d = nullptr;
    bool ok = hipMalloc(&d, sizeof(KeyDev)) == hipSuccess;
    // on a private non-blocking stream, as the CRC tables (pbs_blob.hip)
    hipStream_t cs = nullptr;
    if (ok && (hipStreamCreateWithFlags(&cs, hipStreamNonBlocking) != hipSuccess ||
               hipMemcpyAsync(d, &c->key, sizeof(KeyDev), hipMemcpyHostToDevice, cs) != hipSuccess ||
               hipStreamSynchronize(cs) != hipSuccess)) {
        (void)hipFree(d);
        ok = false;
    }
    if (cs) (void)hipStreamDestroy(cs);
    if (cur != dev) (void)hipSetDevice(cur);
    if (!ok) return nullptr;
    c->dev[dev] = d;
    return d;
}

}  // namespace gcm

// Encrypts the payloads of n blob images in place (blob i = [boff[i], boff[i+1]) of
// `blobs`, plaintext at + 44) and writes IV and tag into the headers; asynchronous on
// `st`.  `hs` keeps the host arrays of the copies alive until the caller has synchronised.
int gcm_encrypt_blobs(const pbs_crypt_config* cfg, uint8_t* blobs, const uint64_t* boff_host,
                      const uint64_t* boff_dev, size_t n, const uint8_t* ivs_host, DevArena& ar, unsigned slot0,
                      GcmHostScratch& hs, hipStream_t st) {
    using namespace gcm;
    if (n == 0) return PBS_OK;
    int dev = 0, ncu = 0;
    if (hipStreamGetDevice(st, &dev) != hipSuccess ||
        hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        return PBS_ERR_NO_DEVICE;
    const KeyDev* key = device_key(cfg, dev);
    if (!key) return PBS_ERR_NOMEM;
    hs.ivs.resize(16 * n);
    if (ivs_host) {
        std::memcpy(hs.ivs.data(), ivs_host, 16 * n);
    } else {  // 16 fresh bytes per blob (proxmox_sys::linux::random_data, data_blob.rs:113)
        for (size_t got = 0; got < 16 * n;) {
            const ssize_t r = getrandom(hs.ivs.data() + got, 16 * n - got, 0);
            if (r < 0) return PBS_ERR_INVALID;
            got += (size_t)r;
        }
    }
    hs.items.clear();
    hs.first.resize(n + 1);
    for (size_t i = 0; i < n; ++i) {
        hs.first[i] = hs.items.size();
        const uint64_t len = boff_host[i + 1] - boff_host[i] - PBS_BLOB_ENC_HEADER_SIZE;
        const uint64_t nseg = (len + PBS_GCM_SEGMENT_BYTES - 1) / PBS_GCM_SEGMENT_BYTES;
        for (uint64_t j = 0; j < nseg; ++j) hs.items.push_back((uint64_t)i << 32 | j);
    }
    hs.first[n] = hs.items.size();
    const uint64_t ni = hs.items.size();
    hs.segments = ni;
    uint8_t* d_ivs = ar.get<uint8_t>(slot0, 16 * n);
    BlobCtx* d_ctx = ar.get<BlobCtx>(slot0 + 1, n * sizeof(BlobCtx));
    uint64_t* d_items = ar.get<uint64_t>(slot0 + 2, std::max<uint64_t>(ni, 1) * 8);
    uint64_t* d_first = ar.get<uint64_t>(slot0 + 3, (n + 1) * 8);
    B128* d_part = ar.get<B128>(slot0 + 4, std::max<uint64_t>(ni, 1) * sizeof(B128));
    if (!d_ivs || !d_ctx || !d_items || !d_first || !d_part) return PBS_ERR_NOMEM;
    if (hipMemcpyAsync(d_ivs, hs.ivs.data(), 16 * n, hipMemcpyHostToDevice, st) != hipSuccess ||
        (ni && hipMemcpyAsync(d_items, hs.items.data(), ni * 8, hipMemcpyHostToDevice, st) != hipSuccess) ||
        hipMemcpyAsync(d_first, hs.first.data(), (n + 1) * 8, hipMemcpyHostToDevice, st) != hipSuccess)
        return PBS_ERR_HIP;
    (void)hipGetLastError();
    hipLaunchKernelGGL(gcm_prepare_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, key, d_ivs, boff_dev,
                       (uint64_t)n, blobs, d_ctx);
    if (ni)
        hipLaunchKernelGGL(gcm_ctr_ghash_kernel, dim3((unsigned)std::min<uint64_t>(ni, (uint64_t)ncu * kGroupsPerCu)),
                           dim3(kThreads), 0, st, key, d_items, ni, boff_dev, d_ctx, blobs, d_part);
    hipLaunchKernelGGL(gcm_tag_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, key, boff_dev, d_first,
                       d_ctx, d_part, (uint64_t)n, blobs);
    return hipGetLastError() == hipSuccess ? PBS_OK : PBS_ERR_HIP;
}

}  // namespace pbs

using namespace pbs;
using namespace pbs::gcm;

extern "C" int pbs_crypt_config_new(const uint8_t enc_key[32], pbs_crypt_config** out) {
    if (!out) return PBS_ERR_ARG;
    *out = nullptr;
    if (!enc_key) return PBS_ERR_ARG;
    pbs_crypt_config* c = new (std::nothrow) pbs_crypt_config;
    if (!c) return PBS_ERR_NOMEM;
    // CryptConfig::new (crypt_config.rs:42-61): id_key = PBKDF2-HMAC-SHA256(enc_key, "_id_key", 10)
    pbkdf2_sha256_32(enc_key, "_id_key", 7, 10, c->id_key);
    make_key(enc_key, c->key);
    *out = c;
    return PBS_OK;
}

extern "C" const uint8_t* pbs_crypt_config_id_key(const pbs_crypt_config* cfg) { return cfg ? cfg->id_key : nullptr; }

extern "C" void pbs_crypt_config_free(pbs_crypt_config* cfg) {
    if (!cfg) return;
    int cur = -1;
    const bool have = hipGetDevice(&cur) == hipSuccess;
    for (auto& kv : cfg->dev) {  // zero the device copies before their memory goes back
        if (hipSetDevice(kv.first) != hipSuccess) continue;
        (void)hipMemset(kv.second, 0, sizeof(KeyDev));
        (void)hipDeviceSynchronize();
        (void)hipFree(kv.second);
    }
    if (have && !cfg->dev.empty()) (void)hipSetDevice(cur);
    (void)hipGetLastError();
    cfg->dev.clear();
    wipe(cfg->id_key, sizeof cfg->id_key);
    wipe(&cfg->key, sizeof cfg->key);
    delete cfg;
}

extern "C" int pbs_aes256gcm_encrypt_host(const pbs_crypt_config* cfg, const uint8_t iv[16], const uint8_t* data,
                                          size_t len, uint8_t* out, uint8_t tag[16]) {
    if (!cfg || !iv || !tag || (len && (!data || !out))) return PBS_ERR_ARG;
    const KeyDev& k = cfg->key;
    const Te0Array T{k.te0};
    const B128 j0 = j0_of_iv16(load_block(iv), k.h);
    uint32_t ctr[4] = {(uint32_t)(j0.hi >> 32), (uint32_t)j0.hi, (uint32_t)(j0.lo >> 32), (uint32_t)j0.lo};
    B128 y{0, 0};
    for (size_t off = 0; off < len; off += 16) {
        uint32_t s[4] = {ctr[0], ctr[1], ctr[2], ctr[3] + (uint32_t)(off / 16 + 1)};
        aes256_encrypt(k.rk, T, s);
        uint8_t c[16] = {};
        const size_t nb = len - off < 16 ? len - off : 16;
        for (size_t b = 0; b < nb; ++b) out[off + b] = c[b] = data[off + b] ^ (uint8_t)(s[b >> 2] >> (24 - 8 * (b & 3)));
        y = gf_mul(gf_xor(y, load_block(c)), k.h);
    }
    y.lo ^= 8 * (uint64_t)len;
    y = gf_mul(y, k.h);
    uint32_t e[4] = {ctr[0], ctr[1], ctr[2], ctr[3]};
    aes256_encrypt(k.rk, T, e);
    store_block(tag, gf_xor(y, B128{(uint64_t)e[0] << 32 | e[1], (uint64_t)e[2] << 32 | e[3]}));
    return PBS_OK;
}

// Test hook (not in include/): the tag of ciphertext `ct` under `iv` computed on the host the
// way the kernels do -- segments from the end, lane-strided Horner sums through the 4-bit
// table of H^256, lane powers, H^4096 -- so the per-key tables and the decomposition are
// pinned without a GPU.
extern "C" int pbs_test_gcm_tag_segments_host(const pbs_crypt_config* cfg, const uint8_t iv[16], const uint8_t* ct,
                                              size_t len, uint8_t tag[16]) {
    if (!cfg || !iv || !tag || (len && !ct)) return PBS_ERR_ARG;
    const KeyDev& k = cfg->key;
    std::vector<uint4> tg(32 * 16);
    std::memcpy(tg.data(), k.tab_g, sizeof k.tab_g);
    const uint64_t m = (len + 15) >> 4, nseg = (m + kSegBlocks - 1) / kSegBlocks;
    const int64_t first = (int64_t)(m - (nseg ? nseg - 1 : 0) * kSegBlocks);
    B128 y{0, 0};
    for (uint64_t seg = 0; seg < nseg; ++seg) {
        B128 p{0, 0};
        for (int t = 0; t < kThreads; ++t) {
            uint4 acc = make_uint4(0, 0, 0, 0);
            for (int r = 0; r < kRows; ++r) {
                const int64_t kb = first + ((int64_t)seg - 1) * (int64_t)kSegBlocks + t + r * kThreads;
                if (kb < 0) continue;
                uint8_t b[16] = {};
                const size_t off = (size_t)kb * 16;
                std::memcpy(b, ct + off, len - off < 16 ? len - off : 16);
                uint4 c;
                std::memcpy(&c, b, 16);
                acc = mul_tab(tg.data(), acc);
                acc.x ^= c.x;
                acc.y ^= c.y;
                acc.z ^= c.z;
                acc.w ^= c.w;
            }
            p = gf_xor(p, gf_mul(words_to_b128(acc), k.lane_pow[t]));
        }
        if (seg) y = gf_mul(y, k.h_seg);
        y = gf_xor(y, p);
    }
    y.lo ^= 8 * (uint64_t)len;
    y = gf_mul(y, k.h);
    const B128 j0 = j0_of_iv16(load_block(iv), k.h);
    uint32_t e[4] = {(uint32_t)(j0.hi >> 32), (uint32_t)j0.hi, (uint32_t)(j0.lo >> 32), (uint32_t)j0.lo};
    aes256_encrypt(k.rk, Te0Array{k.te0}, e);
    store_block(tag, gf_xor(y, B128{(uint64_t)e[0] << 32 | e[1], (uint64_t)e[2] << 32 | e[3]}));
    return PBS_OK;
}

extern "C" size_t pbs_blob_stream_bound_encrypted(const uint64_t* bounds, size_t n) {
    if (!bounds || n == 0) return 0;
    return PBS_BLOB_ENC_HEADER_SIZE * n + (size_t)(bounds[n] - bounds[0]);
}
