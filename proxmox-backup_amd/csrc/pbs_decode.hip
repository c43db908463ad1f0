// Reading blobs on the GPU: `DataBlob::load_from_reader` (from_raw + verify_crc,
// pbs-datastore/src/data_blob.rs:256-300, :78-84), `DataBlob::decode` (:197-253),
// `DataBlob::verify_unencrypted` (:310-333) and `CryptConfig::decode_{un,}compressed_chunk`
// (:409-480) for a stream of blob images of mixed kinds -- everything but the zstd inflate
// (the frame of a compressed blob is the payload handed back).  C ABI: include/pbs_blob.h,
// "Reading blobs".
//
// One call:
//  1. classify_kernel, one lane per blob: size and magic checks (from_raw), kind, header
//     length (12 or 44), stored CRC, payload length, the payload's span for the CRC; the
//     lengths go through the in-house scan to the output offsets, which the host reads
//     (it needs them for the item lists, as the encoder needs its blob offsets).
//  2. the CRC kernel of pbs_blob.hip over the spans (launch_crc32_spans).
//  3. segment_copy_kernel (dev_copy.h), one workgroup per 64 KiB piece of an unencrypted
//     payload, into the packed output; the host builds its items from the offsets it read.
//  4. gcm_open_prepare_kernel, one lane per encrypted blob: J0 from the header's IV through
//     GHASH and AES_K(J0); gcm_open_kernel, the sibling of gcm_ctr_ghash_kernel
//     (pbs_crypt.hip: the same 256 lanes, 64 KiB segments counted from the payload's end,
//     Te0 and the H^256 table in LDS, lane powers): it folds each CIPHERTEXT block into the
//     lane's Horner sum as loaded, XORs the keystream afterwards and stores the plaintext
//     OUT OF PLACE at out + out_offsets[i] + 16 k, whose residue mod 16 differs from the
//     source's -- full blocks are unaligned 16-byte accesses on both sides, the last partial
//     block moves byte by byte; nothing outside [blob + 44, blob end) is read and nothing
//     outside the payload's output range written.  gcm_open_tag_kernel, one lane per blob:
//     Horner of the partials by H^4096, the tag, and its comparison with the header's (every
//     byte is compared: no early exit).
//  5. the SHA-256 lanes (pbs_digest_chunks_async over the packed output, whose offsets are
//     contiguous bounds): kind 0 plain, kind 2 with the config's id_key.
//  6. verdict_kernel, one lane per blob: the first failing check in the reference's order;
//     wipe_kernel, one workgroup per failed encrypted blob: zeros over its output range, so
//     no unauthenticated plaintext is left when the call returns.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "aes_gcm.h"
#include "dev_arena.h"
#include "dev_copy.h"
#include "gcm_dev.h"
#include "pbs_blob.h"
#include "pbs_chunker.h"
#include "pbs_chunker_internal.h"
#include "pbs_digest.h"

namespace pbs {
namespace dec {
namespace {

using namespace gcm;

constexpr int kThreads = kGcmThreads;
constexpr int kRows = kGcmRows;
constexpr uint32_t kSegBlocks = kGcmSegBlocks;
constexpr int kGroupsPerCu = kGcmGroupsPerCu;

// file_formats.rs:9-18
__device__ __constant__ uint8_t kMagicsDev[4][8] = {{66, 171, 56, 7, 190, 131, 112, 161},
                                                    {49, 185, 88, 66, 111, 182, 163, 127},
                                                    {123, 103, 133, 190, 34, 45, 76, 240},
                                                    {230, 89, 27, 191, 11, 191, 216, 11}};
const uint8_t kMagicsHost[4][8] = {{66, 171, 56, 7, 190, 131, 112, 161},
                                   {49, 185, 88, 66, 111, 182, 163, 127},
                                   {123, 103, 133, 190, 34, 45, 76, 240},
                                   {230, 89, 27, 191, 11, 191, 216, 11}};

// from_raw (data_blob.rs:268-290) of one blob of `len` bytes at `p`: kind (or NONE), the
// failing check (0: none), header length
__host__ __device__ inline void classify(const uint8_t* p, uint64_t len, const uint8_t (*magics)[8], uint8_t* kind,
                                         uint8_t* pre, uint32_t* hdr) {
    *kind = PBS_BLOB_KIND_NONE;
    *hdr = 0;
    if (len < PBS_BLOB_HEADER_SIZE) {
        *pre = PBS_BLOB_ST_TOO_SMALL;
        return;
    }
    for (int k = 0; k < 4; ++k) {
        bool eq = true;
        for (int b = 0; b < 8; ++b) eq &= p[b] == magics[k][b];
        if (eq) *kind = (uint8_t)k;
    }
    if (*kind == PBS_BLOB_KIND_NONE) {
        *pre = PBS_BLOB_ST_BAD_MAGIC;
        return;
    }
    const uint32_t h = *kind >= 2 ? PBS_BLOB_ENC_HEADER_SIZE : PBS_BLOB_HEADER_SIZE;
    if (len < h) {
        *pre = PBS_BLOB_ST_TOO_SMALL;
        return;
    }
    *pre = 0;
    *hdr = h;
}

// the first failing check, in the reference's order: load (size, magic, CRC), then decode
// (config, tag, digest), then verify_unencrypted's length
__host__ __device__ inline uint8_t verdict(uint8_t kind, uint8_t pre, bool crc_ok, bool have_cfg, bool tag_ok,
                                           bool check_digest, bool digest_ok, bool check_size, bool size_ok) {
    if (pre) return pre;
    if (!crc_ok) return PBS_BLOB_ST_BAD_CRC;
    if (kind >= 2) {
        if (!have_cfg) return PBS_BLOB_ST_NO_CONFIG;
        if (!tag_ok) return PBS_BLOB_ST_BAD_TAG;
    }
    if (check_digest && (kind == 0 || kind == 2) && !digest_ok) return PBS_BLOB_ST_BAD_DIGEST;
    if (check_size && kind == 0 && !size_ok) return PBS_BLOB_ST_BAD_SIZE;
    return PBS_BLOB_ST_OK;
}

// one lane per blob; lane n writes the scan's closing zero
__global__ void classify_kernel(const uint8_t* __restrict__ blobs, const uint64_t* __restrict__ boff, uint64_t n,
                                uint8_t* __restrict__ kind, uint8_t* __restrict__ pre,
                                uint32_t* __restrict__ stored, uint64_t* __restrict__ dlen,
                                uint64_t* __restrict__ spans, uint32_t* __restrict__ order) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    if (i == n) {
        dlen[n] = 0;
        return;
    }
    const uint64_t b0 = boff[i], b1 = boff[i + 1];
    const uint8_t* const p = blobs + b0;
    uint8_t k, f;
    uint32_t h;
    classify(p, b1 - b0, kMagicsDev, &k, &f, &h);
    kind[i] = k;
    pre[i] = f;
    stored[i] = f ? 0u : (uint32_t)p[8] | (uint32_t)p[9] << 8 | (uint32_t)p[10] << 16 | (uint32_t)p[11] << 24;
    dlen[i] = f ? 0 : b1 - b0 - h;
    spans[2 * i] = f ? b1 : b0 + h;
    spans[2 * i + 1] = b1;
    order[i] = (uint32_t)(2 * i);
}

__global__ void gcm_open_prepare_kernel(const KeyDev* __restrict__ key, const uint8_t* __restrict__ blobs,
                                        const uint64_t* __restrict__ boff, const uint8_t* __restrict__ kind,
                                        const uint8_t* __restrict__ pre, uint64_t n, BlobCtx* __restrict__ ctx) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || pre[i] || kind[i] < 2) return;
    const B128 j0 = j0_of_iv16(load_block(blobs + boff[i] + 12), key->h);
    uint32_t s[4] = {(uint32_t)(j0.hi >> 32), (uint32_t)j0.hi, (uint32_t)(j0.lo >> 32), (uint32_t)j0.lo};
    ctx[i].j0 = make_uint4(s[0], s[1], s[2], s[3]);
    aes256_encrypt(key->rk, Te0Array{key->te0}, s);
    ctx[i].ek = B128{(uint64_t)s[0] << 32 | s[1], (uint64_t)s[2] << 32 | s[3]};
}

// The opening direction of gcm_ctr_ghash_kernel (pbs_crypt.hip; the geometry, the tables and
// the reduction are the same): item = blob << 32 | segment, segments counted from the
// payload's end.  The ciphertext block is folded as loaded, then XOR-ed with the keystream
// and stored to the packed output.
__global__ __launch_bounds__(kThreads) void gcm_open_kernel(
    const KeyDev* __restrict__ key, const uint64_t* __restrict__ items, uint64_t nitems,
    const uint64_t* __restrict__ boff, const uint64_t* __restrict__ ooff, const BlobCtx* __restrict__ ctx,
    const uint8_t* __restrict__ blobs, uint8_t* __restrict__ out, B128* __restrict__ part) {
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
        const uint64_t o0 = ooff[ci];
        const uint64_t len = ooff[ci + 1] - o0;
        const uint8_t* const src = blobs + boff[ci] + PBS_BLOB_ENC_HEADER_SIZE;
        uint8_t* const dst = out + o0;
        const uint64_t m = (len + 15) >> 4;
        const uint64_t nseg = (m + kSegBlocks - 1) / kSegBlocks;
        const int64_t first = (int64_t)(m - (nseg - 1) * kSegBlocks);  // blocks of segment 0
        const int64_t kbase = first + (seg - 1) * (int64_t)kSegBlocks + (int64_t)tid;
        const uint4 j0 = ctx[ci].j0;
        uint4 acc = make_uint4(0, 0, 0, 0);
        // (one row at a time, as the sealing kernel: its register balance, profiles/crypt/ab_unroll.txt)
#pragma unroll 1
        for (int r = 0; r < kRows; ++r) {
            const int64_t kb = kbase + r * kThreads;
            if (kb < 0) continue;  // the ragged first segment's leading zeros (acc is still 0)
            uint32_t s[4] = {j0.x, j0.y, j0.z, j0.w + (uint32_t)(kb + 1)};  // inc32: low word only
            aes256_encrypt(rk, T, s);
            const uint32_t ks[4] = {__builtin_bswap32(s[0]), __builtin_bswap32(s[1]), __builtin_bswap32(s[2]),
                                    __builtin_bswap32(s[3])};
            const uint64_t off = (uint64_t)kb * 16;
            uint32_t c[4];
            if (off + 16 <= len) {
                const u32x4 v = *reinterpret_cast<const u32x4_u*>(src + off);
                c[0] = v.x;
                c[1] = v.y;
                c[2] = v.z;
                c[3] = v.w;
                u32x4 o;
                o.x = c[0] ^ ks[0];
                o.y = c[1] ^ ks[1];
                o.z = c[2] ^ ks[2];
                o.w = c[3] ^ ks[3];
                *reinterpret_cast<u32x4_u*>(dst + off) = o;
            } else {  // the payload's last, partial block: zero padded for GHASH
                const uint32_t rem = (uint32_t)(len - off);
                c[0] = c[1] = c[2] = c[3] = 0;
#pragma unroll
                for (int b = 0; b < 16; ++b)
                    if ((uint32_t)b < rem) {
                        const uint32_t x = src[off + b];
                        c[b >> 2] |= x << (8 * (b & 3));
                        dst[off + b] = (uint8_t)(x ^ (ks[b >> 2] >> (8 * (b & 3))));
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

__global__ void gcm_open_tag_kernel(const KeyDev* __restrict__ key, const uint8_t* __restrict__ blobs,
                                    const uint64_t* __restrict__ boff, const uint64_t* __restrict__ ooff,
                                    const uint8_t* __restrict__ kind, const uint8_t* __restrict__ pre,
                                    const uint64_t* __restrict__ ifirst, const BlobCtx* __restrict__ ctx,
                                    const B128* __restrict__ part, uint64_t n, uint8_t* __restrict__ tag_ok) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (pre[i] || kind[i] < 2) {
        tag_ok[i] = 0;
        return;
    }
    const uint64_t len = ooff[i + 1] - ooff[i];
    const B128 hs = key->h_seg;
    B128 y{0, 0};
    for (uint64_t k = ifirst[i]; k < ifirst[i + 1]; ++k) {
        if (k != ifirst[i]) y = gf_mul(y, hs);
        y = gf_xor(y, part[k]);
    }
    y.lo ^= 8 * len;  // [len(A) = 0]_64 || [len(C)]_64
    y = gf_xor(gf_mul(y, key->h), ctx[i].ek);
    const B128 t = load_block(blobs + boff[i] + 28);
    tag_ok[i] = ((y.hi ^ t.hi) | (y.lo ^ t.lo)) == 0 ? 1 : 0;
}

__global__ void verdict_kernel(const uint8_t* __restrict__ kind, const uint8_t* __restrict__ pre,
                               const uint32_t* __restrict__ stored, const uint32_t* __restrict__ crc2, int judge_crc,
                               const uint8_t* __restrict__ tag_ok, int have_cfg, const uint8_t* __restrict__ dig,
                               const uint8_t* __restrict__ expect, const uint64_t* __restrict__ ooff,
                               const uint64_t* __restrict__ expect_sizes, uint64_t n, uint8_t* __restrict__ status) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t k = kind[i], f = pre[i];
    bool dig_ok = true;
    if (expect && !f && (k == 0 || (k == 2 && have_cfg))) {
        uint32_t d = 0;
        for (int b = 0; b < 32; ++b) d |= (uint32_t)(dig[32 * i + b] ^ expect[32 * i + b]);
        dig_ok = d == 0;
    }
    const bool size_ok = !expect_sizes || ooff[i + 1] - ooff[i] == expect_sizes[i];
    status[i] = verdict(k, f, f || !judge_crc || stored[i] == crc2[2 * i], have_cfg != 0, have_cfg && tag_ok[i], expect != nullptr,
                        dig_ok, expect_sizes != nullptr, size_ok);
}

// one workgroup per blob: zeros over the output range of an encrypted blob that failed.  Not
// items of segment_copy_kernel with src == 0: which blobs failed is in d_status alone at this
// point of the stream, and a host-built item list would cost a synchronisation to read it.
__global__ __launch_bounds__(kThreads) void wipe_kernel(const uint8_t* __restrict__ kind,
                                                        const uint8_t* __restrict__ status,
                                                        const uint64_t* __restrict__ ooff, uint64_t n,
                                                        uint8_t* __restrict__ out) {
    for (uint64_t i = blockIdx.x; i < n; i += gridDim.x) {
        const uint8_t k = kind[i];
        if (status[i] == PBS_BLOB_ST_OK || (k != PBS_BLOB_KIND_ENCRYPTED && k != PBS_BLOB_KIND_ENCR_COMPR)) continue;
        const uint64_t e = ooff[i + 1];
        for (uint64_t o = ooff[i] + threadIdx.x; o < e; o += kThreads) out[o] = 0;
    }
}

ArenaPool& dpool() {
    static ArenaPool* p = new ArenaPool;  // never destroyed (HIP may be torn down first at exit)
    return *p;
}
enum DSlot : unsigned { kDsBoff, kDsKind, kDsPre, kDsStored, kDsLen, kDsOoff, kDsSpans, kDsOrder, kDsCrc, kDsTmp,
                        kDsItems, kDsFirst, kDsPart, kDsCtx, kDsPItems, kDsTagOk, kDsDig, kDsExpect, kDsExpSize,
                        kDsDigOrd, kDsStatus };

// tag of `ct` under the config (the sequential form, as pbs_aes256gcm_encrypt_host)
void host_tag(const KeyDev& k, const uint32_t j0w[4], const uint8_t* ct, size_t len, uint8_t tag[16]) {
    B128 y{0, 0};
    for (size_t off = 0; off < len; off += 16) {
        uint8_t c[16] = {};
        std::memcpy(c, ct + off, len - off < 16 ? len - off : 16);
        y = gf_mul(gf_xor(y, load_block(c)), k.h);
    }
    y.lo ^= 8 * (uint64_t)len;
    y = gf_mul(y, k.h);
    uint32_t e[4] = {j0w[0], j0w[1], j0w[2], j0w[3]};
    aes256_encrypt(k.rk, Te0Array{k.te0}, e);
    store_block(tag, gf_xor(y, B128{(uint64_t)e[0] << 32 | e[1], (uint64_t)e[2] << 32 | e[3]}));
}

}  // namespace
}  // namespace dec

void decode_release() {
    dec::dpool().clear();
    inflate::inflate_release();
}

size_t digest_order(const uint8_t* cls, const uint64_t* bounds, uint32_t stride, size_t n, std::vector<uint32_t>& ord) {
    ord.clear();
    size_t nplain = 0;
    for (uint8_t c = 1; c <= 2; ++c) {
        for (size_t i = 0; i < n; ++i)
            if (cls[i] == c) ord.push_back((uint32_t)(stride * i));
        if (c == 1) nplain = ord.size();
    }
    auto longer = [&](uint32_t a, uint32_t b) { return bounds[a + 1] - bounds[a] > bounds[b + 1] - bounds[b]; };
    std::stable_sort(ord.begin(), ord.begin() + nplain, longer);
    std::stable_sort(ord.begin() + nplain, ord.end(), longer);
    return nplain;
}

int digest_in_order(const uint8_t* data_dev, uint64_t data_len, const uint64_t* bounds_dev, const uint32_t* ord_dev,
                    size_t nplain, size_t nord, const pbs_crypt_config* cfg, uint8_t* dig_dev, hipStream_t st) {
    int r = pbs_digest_chunks_async(data_dev, data_len, 0, bounds_dev, ord_dev, nplain, nullptr, 0, dig_dev, st);
    if (r == PBS_OK && nord > nplain)
        r = pbs_digest_chunks_async(data_dev, data_len, 0, bounds_dev, ord_dev + nplain, nord - nplain, cfg->id_key, 32,
                                    dig_dev, st);
    return r;
}

}  // namespace pbs

using namespace pbs;
using namespace pbs::gcm;
using namespace pbs::dec;

extern "C" size_t pbs_blob_decode_bound(const uint64_t* blob_offsets, size_t n) {
    if (!blob_offsets) return 0;
    size_t s = 0;
    for (size_t i = 0; i < n; ++i) {
        if (blob_offsets[i + 1] < blob_offsets[i]) return 0;
        const uint64_t len = blob_offsets[i + 1] - blob_offsets[i];
        if (len > PBS_BLOB_HEADER_SIZE) s += (size_t)(len - PBS_BLOB_HEADER_SIZE);
    }
    return s;
}

extern "C" int pbs_aes256gcm_decrypt_host(const pbs_crypt_config* cfg, const uint8_t iv[16], const uint8_t* data,
                                          size_t len, const uint8_t tag[16], uint8_t* out) {
    if (!cfg || !iv || !tag || (len && (!data || !out))) return PBS_ERR_ARG;
    const KeyDev& k = cfg->key;
    const Te0Array T{k.te0};
    const B128 j0 = j0_of_iv16(load_block(iv), k.h);
    const uint32_t ctr[4] = {(uint32_t)(j0.hi >> 32), (uint32_t)j0.hi, (uint32_t)(j0.lo >> 32), (uint32_t)j0.lo};
    uint8_t t[16];
    host_tag(k, ctr, data, len, t);
    uint8_t d = 0;
    for (int b = 0; b < 16; ++b) d |= (uint8_t)(t[b] ^ tag[b]);
    if (d) {
        if (len) std::memset(out, 0, len);
        return PBS_ERR_TAG;
    }
    for (size_t off = 0; off < len; off += 16) {
        uint32_t s[4] = {ctr[0], ctr[1], ctr[2], ctr[3] + (uint32_t)(off / 16 + 1)};
        aes256_encrypt(k.rk, T, s);
        const size_t nb = len - off < 16 ? len - off : 16;
        for (size_t b = 0; b < nb; ++b) out[off + b] = data[off + b] ^ (uint8_t)(s[b >> 2] >> (24 - 8 * (b & 3)));
    }
    return PBS_OK;
}

extern "C" int pbs_blob_decode_host(const uint8_t* blob, size_t len, const pbs_crypt_config* cfg,
                                    const uint8_t* expect_digest, const uint64_t* expect_size, uint8_t* out,
                                    size_t cap, size_t* out_len, uint8_t* kind, uint8_t* status) {
    if (!out_len || !kind || !status || (len && !blob)) return PBS_ERR_ARG;
    *out_len = 0;
    uint8_t k, f;
    uint32_t h;
    classify(blob, len, kMagicsHost, &k, &f, &h);
    *kind = k;
    *status = f;
    if (f) return PBS_OK;
    const size_t plen = len - h;
    if (plen > cap || (plen && !out)) return PBS_ERR_CAPACITY;
    *out_len = plen;
    const uint8_t* const pay = blob + h;
    const uint32_t stored = (uint32_t)blob[8] | (uint32_t)blob[9] << 8 | (uint32_t)blob[10] << 16 |
                            (uint32_t)blob[11] << 24;
    const bool crc_ok = stored == pbs_crc32(0, pay, plen);
    bool tag_ok = false, dig_ok = true;
    if (k >= 2) {
        if (crc_ok && cfg) tag_ok = pbs_aes256gcm_decrypt_host(cfg, blob + 12, pay, plen, blob + 28, out) == PBS_OK;
    } else if (plen) {
        std::memcpy(out, pay, plen);
    }
    if (expect_digest && crc_ok && (k == 0 || (k == 2 && tag_ok))) {
        std::vector<uint8_t> msg(out, out + plen);
        if (k == 2) msg.insert(msg.end(), cfg->id_key, cfg->id_key + 32);
        uint8_t d[32];
        pbs_sha256(msg.data(), msg.size(), d);
        dig_ok = std::memcmp(d, expect_digest, 32) == 0;
        if (k == 2) std::fill(msg.begin(), msg.end(), 0);
    }
    *status = verdict(k, 0, crc_ok, cfg != nullptr, tag_ok, expect_digest != nullptr, dig_ok, expect_size != nullptr,
                      !expect_size || *expect_size == plen);
    if (k >= 2 && *status != PBS_BLOB_ST_OK && plen) std::memset(out, 0, plen);
    return PBS_OK;
}

extern "C" int pbs_blob_decode_device(const uint8_t* blobs_dev, const uint64_t* blob_offsets, size_t n,
                                      const pbs_crypt_config* cfg, const uint8_t* expect_digests,
                                      const uint64_t* expect_sizes, uint8_t* out_dev, size_t out_cap,
                                      uint64_t* out_offsets, uint8_t* kinds, uint8_t* status,
                                      pbs_blob_decode_timing* timing, void* hip_stream) {
    return pbs::decode_device_impl(blobs_dev, blob_offsets, n, cfg, expect_digests, expect_sizes, out_dev, out_cap,
                                   out_offsets, kinds, status, timing, hip_stream, nullptr);
}

// pbs_blob_decode_device, and the internal mode of the backup session's upload (crc_out != NULL,
// n host words): the payloads' CRCs are computed and handed out, the stored ones are not judged
// (upload_chunk.rs:77-85), so BAD_CRC never occurs.  A blob that fails from_raw has CRC 0.
int pbs::decode_device_impl(const uint8_t* blobs_dev, const uint64_t* blob_offsets, size_t n, const pbs_crypt_config* cfg,
                            const uint8_t* expect_digests, const uint64_t* expect_sizes, uint8_t* out_dev, size_t out_cap,
                            uint64_t* out_offsets, uint8_t* kinds, uint8_t* status, pbs_blob_decode_timing* timing,
                            void* hip_stream, uint32_t* crc_out) {
    const HClock::time_point t0 = HClock::now();
    if (timing) std::memset(timing, 0, sizeof(*timing));
    if (!out_offsets) return PBS_ERR_ARG;
    out_offsets[0] = 0;
    if (n == 0) return PBS_OK;
    if (!blob_offsets || !blobs_dev || !kinds || !status || n >= 0x7FFFFFFFull) return PBS_ERR_ARG;
    for (size_t i = 0; i < n; ++i)
        if (blob_offsets[i] > blob_offsets[i + 1]) return PBS_ERR_ARG;
    const size_t bound = pbs_blob_decode_bound(blob_offsets, n);
    if (out_cap < bound) return PBS_ERR_CAPACITY;
    if (bound && !out_dev) return PBS_ERR_ARG;
    hipStream_t st = (hipStream_t)hip_stream;
    const StreamDevice sd(st);
    if (!sd.ok) return PBS_ERR_NO_DEVICE;
    DeviceGuard dg(sd.dev);
    if (!dg.ok) return PBS_ERR_NO_DEVICE;
    const KeyDev* key = nullptr;
    if (cfg && !(key = device_key(cfg, sd.dev))) return PBS_ERR_NOMEM;

    CallRc call;
    size_t tmpb = 0;
    (void)exclusive_sum_u64(nullptr, &tmpb, nullptr, nullptr, (uint32_t)(n + 1), st);
    ArenaLease ar(dpool(), sd.dev);
    uint64_t* d_boff = ar->get<uint64_t>(kDsBoff, (n + 1) * 8);
    uint8_t* d_kind = ar->get<uint8_t>(kDsKind, n);
    uint8_t* d_pre = ar->get<uint8_t>(kDsPre, n);
    uint32_t* d_stored = ar->get<uint32_t>(kDsStored, n * 4);
    uint64_t* d_len = ar->get<uint64_t>(kDsLen, (n + 1) * 8);
    uint64_t* d_ooff = ar->get<uint64_t>(kDsOoff, (n + 1) * 8);
    uint64_t* d_spans = ar->get<uint64_t>(kDsSpans, 2 * n * 8);
    uint32_t* d_order = ar->get<uint32_t>(kDsOrder, n * 4);
    uint32_t* d_crc = ar->get<uint32_t>(kDsCrc, 2 * n * 4);
    void* d_tmp = ar->get<void>(kDsTmp, std::max<size_t>(tmpb, 256));
    uint8_t* d_tagok = ar->get<uint8_t>(kDsTagOk, n);
    uint8_t* d_status = ar->get<uint8_t>(kDsStatus, n);
    uint8_t* d_dig = expect_digests ? ar->get<uint8_t>(kDsDig, 32 * n) : nullptr;
    uint8_t* d_expect = expect_digests ? ar->get<uint8_t>(kDsExpect, 32 * n) : nullptr;
    uint32_t* d_digord = expect_digests ? ar->get<uint32_t>(kDsDigOrd, n * 4) : nullptr;
    uint64_t* d_expsize = expect_sizes ? ar->get<uint64_t>(kDsExpSize, n * 8) : nullptr;
    if (!d_boff || !d_kind || !d_pre || !d_stored || !d_len || !d_ooff || !d_spans || !d_order || !d_crc || !d_tmp ||
        !d_tagok || !d_status || (expect_digests && (!d_dig || !d_expect || !d_digord)) ||
        (expect_sizes && !d_expsize))
        call.fail(PBS_ERR_NOMEM);
    hipEvent_t ev[6] = {};
    for (unsigned i = 0; i < 6 && call.rc == PBS_OK; ++i)
        if (!(ev[i] = ar->event(i))) call.fail(PBS_ERR_HIP);

    // 1. classify, output offsets
    std::vector<uint8_t> h_pre(n);
    std::vector<uint32_t> h_crc(crc_out ? 2 * n : 0);
    if (call.rc == PBS_OK) {
        (void)hipGetLastError();
        call.ok(hipMemcpyAsync(d_boff, blob_offsets, (n + 1) * 8, hipMemcpyHostToDevice, st)) &&
            (!expect_digests ||
             call.ok(hipMemcpyAsync(d_expect, expect_digests, 32 * n, hipMemcpyHostToDevice, st))) &&
            (!expect_sizes || call.ok(hipMemcpyAsync(d_expsize, expect_sizes, n * 8, hipMemcpyHostToDevice, st))) &&
            call.ok(hipEventRecord(ev[0], st));
    }
    if (call.rc == PBS_OK) {
        hipLaunchKernelGGL(classify_kernel, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, st, blobs_dev, d_boff,
                           (uint64_t)n, d_kind, d_pre, d_stored, d_len, d_spans, d_order);
        call.ok(hipGetLastError()) && call.ok(exclusive_sum_u64(d_tmp, &tmpb, d_len, d_ooff, (uint32_t)(n + 1), st)) &&
            call.ok(hipEventRecord(ev[1], st)) &&
            call.ok(hipMemcpyAsync(out_offsets, d_ooff, (n + 1) * 8, hipMemcpyDeviceToHost, st)) &&
            call.ok(hipMemcpyAsync(kinds, d_kind, n, hipMemcpyDeviceToHost, st)) &&
            call.ok(hipMemcpyAsync(h_pre.data(), d_pre, n, hipMemcpyDeviceToHost, st)) && call.ok(hipStreamSynchronize(st));
    }
    // (the bound covers every outcome of the classification; checked all the same, before
    // the first write to the output)
    if (call.rc == PBS_OK && out_offsets[n] > out_cap) call.fail(PBS_ERR_CAPACITY);

    // the item lists: copy items of the unencrypted payloads (disjoint ranges of the packed
    // output), GCM segments of the encrypted; the host vectors live until the last synchronisation
    std::vector<CopyItem> pitems;
    std::vector<uint64_t> gitems, first(n + 1);
    std::vector<uint32_t> digord;
    size_t ndig0 = 0;
    if (call.rc == PBS_OK) {
        std::vector<uint8_t> cls(expect_digests ? n : 0, 0);  // digest_order: kind 0 plain, kind 2 with the id_key
        for (size_t i = 0; i < n; ++i) {
            first[i] = gitems.size();
            const uint64_t len = out_offsets[i + 1] - out_offsets[i];
            if (h_pre[i] || kinds[i] == PBS_BLOB_KIND_NONE) continue;
            if (kinds[i] < 2) {
                add_items(pitems, (uint64_t)(uintptr_t)blobs_dev + blob_offsets[i] + PBS_BLOB_HEADER_SIZE,
                          (uint64_t)(uintptr_t)out_dev + out_offsets[i], len);
            } else if (cfg) {
                const uint64_t ns = (len + PBS_GCM_SEGMENT_BYTES - 1) / PBS_GCM_SEGMENT_BYTES;
                for (uint64_t j = 0; j < ns; ++j) gitems.push_back((uint64_t)i << 32 | j);
            }
            if (expect_digests)
                cls[i] = kinds[i] == PBS_BLOB_KIND_UNCOMPRESSED ? 1 : (kinds[i] == PBS_BLOB_KIND_ENCRYPTED && cfg) ? 2 : 0;
        }
        first[n] = gitems.size();
        if (expect_digests) ndig0 = digest_order(cls.data(), out_offsets, 1, n, digord);
    }
    const uint64_t ngi = gitems.size();
    uint64_t* d_gitems = nullptr;
    uint64_t* d_first = nullptr;
    B128* d_part = nullptr;
    BlobCtx* d_ctx = nullptr;
    if (call.rc == PBS_OK) {
        d_gitems = ar->get<uint64_t>(kDsItems, std::max<uint64_t>(ngi, 1) * 8);
        d_first = ar->get<uint64_t>(kDsFirst, (n + 1) * 8);
        d_part = ar->get<B128>(kDsPart, std::max<uint64_t>(ngi, 1) * sizeof(B128));
        d_ctx = ar->get<BlobCtx>(kDsCtx, n * sizeof(BlobCtx));
        if (!d_gitems || !d_first || !d_part || !d_ctx) call.fail(PBS_ERR_NOMEM);
    }
    if (call.rc == PBS_OK)
        (!ngi || call.ok(hipMemcpyAsync(d_gitems, gitems.data(), ngi * 8, hipMemcpyHostToDevice, st))) &&
            call.ok(hipMemcpyAsync(d_first, first.data(), (n + 1) * 8, hipMemcpyHostToDevice, st)) &&
            (digord.empty() ||
             call.ok(hipMemcpyAsync(d_digord, digord.data(), digord.size() * 4, hipMemcpyHostToDevice, st)));
    // 2. CRCs (timed from ev[5]: the host built the lists while the stream was idle)
    if (call.rc == PBS_OK) call.ok(hipEventRecord(ev[5], st));
    if (call.rc == PBS_OK) {
        const hipError_t e = launch_crc32_spans(blobs_dev, d_spans, d_order, n, d_crc, st);
        if (e != hipSuccess) call.fail(e == hipErrorOutOfMemory ? PBS_ERR_NOMEM : PBS_ERR_HIP);
        else call.ok(hipEventRecord(ev[2], st));
    }
    // 3. + 4. payloads into the packed output
    if (call.rc == PBS_OK) {
        const unsigned g64 = (unsigned)((n + 63) / 64);
        call.fail(copy_items_async(pitems, *ar, kDsPItems, sd.ncu, st));
        if (call.rc == PBS_OK && cfg) {
            hipLaunchKernelGGL(gcm_open_prepare_kernel, dim3(g64), dim3(64), 0, st, key, blobs_dev, d_boff, d_kind,
                               d_pre, (uint64_t)n, d_ctx);
            if (ngi)
                hipLaunchKernelGGL(gcm_open_kernel,
                                   dim3((unsigned)std::min<uint64_t>(ngi, (uint64_t)sd.ncu * kGroupsPerCu)),
                                   dim3(kThreads), 0, st, key, d_gitems, ngi, d_boff, d_ooff, d_ctx, blobs_dev, out_dev,
                                   d_part);
            hipLaunchKernelGGL(gcm_open_tag_kernel, dim3(g64), dim3(64), 0, st, key, blobs_dev, d_boff, d_ooff, d_kind,
                               d_pre, d_first, d_ctx, d_part, (uint64_t)n, d_tagok);
        }
        call.ok(hipGetLastError()) && call.ok(hipEventRecord(ev[3], st));
    }
    // 5. + 6. digests, verdicts, wipe
    if (call.rc == PBS_OK && expect_digests)
        call.fail(digest_in_order(out_dev, out_offsets[n], d_ooff, d_digord, ndig0, digord.size(), cfg, d_dig, st));
    if (call.rc == PBS_OK) {
        hipLaunchKernelGGL(verdict_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_kind, d_pre, d_stored,
                           d_crc, crc_out ? 0 : 1, d_tagok, cfg ? 1 : 0, d_dig, d_expect, d_ooff, d_expsize, (uint64_t)n, d_status);
        hipLaunchKernelGGL(wipe_kernel, dim3((unsigned)std::min<uint64_t>(n, (uint64_t)sd.ncu * 8)), dim3(kThreads), 0, st,
                           d_kind, d_status, d_ooff, (uint64_t)n, out_dev);
        call.ok(hipGetLastError()) && call.ok(hipEventRecord(ev[4], st)) &&
            call.ok(hipMemcpyAsync(status, d_status, n, hipMemcpyDeviceToHost, st)) &&
            (!crc_out || call.ok(hipMemcpyAsync(h_crc.data(), d_crc, 2 * n * 4, hipMemcpyDeviceToHost, st))) &&
            call.ok(hipStreamSynchronize(st));
        if (call.rc == PBS_OK && crc_out)
            for (size_t i = 0; i < n; ++i) crc_out[i] = h_pre[i] ? 0 : h_crc[2 * i];
    }
    if (call.rc == PBS_OK && timing) {
        float a = 0, b = 0, c = 0, d = 0;
        (void)hipEventElapsedTime(&a, ev[0], ev[1]);
        (void)hipEventElapsedTime(&b, ev[5], ev[2]);
        (void)hipEventElapsedTime(&c, ev[2], ev[3]);
        (void)hipEventElapsedTime(&d, ev[3], ev[4]);
        timing->classify_ms = a;
        timing->crc_ms = b;
        timing->decrypt_ms = c;
        timing->digest_ms = d;
        timing->bytes_in = blob_offsets[n] - blob_offsets[0];
        timing->bytes_out = out_offsets[n];
        timing->gcm_segments = ngi;
        for (size_t i = 0; i < n; ++i) timing->failed += status[i] != PBS_BLOB_ST_OK;
    }
    if (call.rc != PBS_OK) (void)hipStreamSynchronize(st);  // the arena goes back idle
    if (timing) timing->total_ms = hms(t0);
    return call.rc;
}
