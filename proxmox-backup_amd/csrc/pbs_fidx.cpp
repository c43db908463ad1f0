// Host side of the fixed-size chunk path (include/pbs_fixed.h): the fixed index (.fidx) image,
// FixedIndexWriter / FixedIndexReader of pbs-datastore/src/fixed_index.rs, and the host mirror
// of the dirty map.  Plain C++: no device code, so the sanitizer program of
// tests/cpp/fidx_sanitize.cpp builds it with the host compiler.
// Format (fixed_index.rs:20-32): header (4096 bytes) magic [u8; 8] = FIXED_SIZED_CHUNK_INDEX_1_0
// (file_formats.rs:20-21), uuid [u8; 16], ctime i64 LE, index_csum [u8; 32], size u64 LE,
// chunk_size u64 LE, reserved zeros; then ceil(size / chunk_size) digests of 32 bytes;
// index_csum = SHA-256(digest1 || digest2 || ...) (close, :341-362).
#include <stdint.h>

#include <cstring>

#include "pbs_chunker.h"
#include "pbs_digest.h"
#include "pbs_fixed.h"

namespace {

// FIXED_SIZED_CHUNK_INDEX_1_0 (pbs-datastore/src/file_formats.rs:20-21)
constexpr uint8_t kFidxMagic[8] = {47, 127, 65, 237, 145, 253, 15, 205};
constexpr size_t kHeader = 4096;
constexpr size_t kDigest = 32;

inline uint64_t get_le64(const uint8_t* p) {
    uint64_t v = 0;
    for (int i = 0; i < 8; ++i) v |= (uint64_t)p[i] << (8 * i);
    return v;
}
inline void put_le64(uint8_t* p, uint64_t v) {
    for (int i = 0; i < 8; ++i) p[i] = (uint8_t)(v >> (8 * i));
}
inline bool pow2(uint64_t v) { return v && !(v & (v - 1)); }

// ceil(size / chunk_size) without the overflow of size + chunk_size - 1
inline uint64_t count64(uint64_t size, uint64_t chunk_size) {
    return chunk_size ? size / chunk_size + (size % chunk_size ? 1 : 0) : 0;
}

}  // namespace

extern "C" size_t pbs_fidx_count(uint64_t size, uint64_t chunk_size) { return (size_t)count64(size, chunk_size); }

extern "C" size_t pbs_fidx_size(size_t n) { return kHeader + kDigest * n; }

extern "C" int pbs_fidx_build(const uint8_t* digests, uint64_t size, uint64_t chunk_size, const uint8_t uuid[16],
                              int64_t ctime, uint8_t* out, size_t cap, uint8_t csum_out[32]) {
    if (!out || chunk_size == 0) return PBS_ERR_INVALID;
    const uint64_t n = count64(size, chunk_size);
    if (n && !digests) return PBS_ERR_INVALID;
    if (n > (SIZE_MAX - kHeader) / kDigest || cap < pbs_fidx_size((size_t)n)) return PBS_ERR_CAPACITY;
    std::memset(out, 0, kHeader);
    std::memcpy(out, kFidxMagic, 8);
    if (uuid) std::memcpy(out + 8, uuid, 16);
    put_le64(out + 24, (uint64_t)ctime);
    put_le64(out + 64, size);
    put_le64(out + 72, chunk_size);
    if (n) std::memcpy(out + kHeader, digests, (size_t)n * kDigest);
    uint8_t c[32];
    pbs_sha256(out + kHeader, (size_t)n * kDigest, c);  // close: sha256 over the mapped digests
    std::memcpy(out + 32, c, 32);
    if (csum_out) std::memcpy(csum_out, c, 32);
    return PBS_OK;
}

extern "C" int pbs_fidx_parse(const uint8_t* image, size_t len, uint8_t uuid[16], int64_t* ctime,
                              uint8_t header_csum[32], uint8_t computed_csum[32], uint64_t* size,
                              uint64_t* chunk_size, uint8_t* digests, size_t cap, size_t* n) {
    if (n) *n = 0;
    if (!image || len < kHeader) return PBS_ERR_INVALID;                 // "index too small"
    if (std::memcmp(image, kFidxMagic, 8) != 0) return PBS_ERR_INVALID;  // "got unknown magic number"
    const uint64_t sz = get_le64(image + 64), cs = get_le64(image + 72);
    if (cs == 0) return PBS_ERR_INVALID;  // (size + chunk_size - 1) / chunk_size divides by it
    const uint64_t cnt = count64(sz, cs);
    // "got unexpected file size": index_length * 32 != st_size - header_size
    if (cnt > (SIZE_MAX - kHeader) / kDigest || cnt * kDigest != len - kHeader) return PBS_ERR_INVALID;
    if (sz == 0) return PBS_ERR_INVALID;  // "invalid index size": no zero-length mmap
    if (!pow2(cs)) return PBS_ERR_NOT_POW2;  // (deviation, see the header)
    if (n) *n = (size_t)cnt;
    if (cap < cnt) return PBS_ERR_CAPACITY;
    if (digests) std::memcpy(digests, image + kHeader, (size_t)cnt * kDigest);
    if (uuid) std::memcpy(uuid, image + 8, 16);
    if (ctime) *ctime = (int64_t)get_le64(image + 24);
    if (header_csum) std::memcpy(header_csum, image + 32, 32);
    if (computed_csum) pbs_sha256(image + kHeader, (size_t)cnt * kDigest, computed_csum);
    if (size) *size = sz;
    if (chunk_size) *chunk_size = cs;
    return PBS_OK;
}

extern "C" int pbs_fidx_chunk_info(uint64_t size, uint64_t chunk_size, size_t pos, uint64_t* start,
                                   uint64_t* end) {
    if (chunk_size == 0 || pos >= count64(size, chunk_size)) return PBS_ERR_INVALID;  // None
    const uint64_t s = (uint64_t)pos * chunk_size;
    uint64_t e = size - s > chunk_size ? s + chunk_size : size;  // if end > self.size { end = self.size }
    if (start) *start = s;
    if (end) *end = e;
    return PBS_OK;
}

extern "C" int pbs_fidx_chunk_from_offset(uint64_t size, uint64_t chunk_size, uint64_t offset, size_t* idx,
                                          uint64_t* within) {
    if (chunk_size == 0) return PBS_ERR_INVALID;
    if (!pow2(chunk_size)) return PBS_ERR_NOT_POW2;
    if (offset >= size) return PBS_ERR_INVALID;  // None
    if (idx) *idx = (size_t)(offset / chunk_size);
    if (within) *within = offset & (chunk_size - 1);  // "fast modulo, valid for 2^x chunk_size"
    return PBS_OK;
}

extern "C" int pbs_fidx_check_chunk_alignment(uint64_t size, uint64_t chunk_size, uint64_t end_offset,
                                              uint64_t chunk_len, size_t* idx) {
    if (chunk_size == 0) return PBS_ERR_INVALID;
    if (!pow2(chunk_size)) return PBS_ERR_NOT_POW2;
    if (end_offset < chunk_len) return PBS_ERR_INVALID;  // :365 "got chunk with small offset"
    const uint64_t pos = end_offset - chunk_len;         // :369
    if (end_offset > size) return PBS_ERR_INVALID;       // :371 "chunk data exceeds size"
    // :376-378 "chunk with unexpected length": the last chunk can be smaller
    if ((end_offset != size && chunk_len != chunk_size) || chunk_len > chunk_size || chunk_len == 0)
        return PBS_ERR_INVALID;
    if (pos & (chunk_size - 1)) return PBS_ERR_INVALID;  // :387 "got unaligned chunk"
    if (idx) *idx = (size_t)(pos / chunk_size);          // :391
    return PBS_OK;
}

extern "C" int pbs_fixed_dirty_host(const uint8_t* prev, const uint8_t* cur, uint64_t size, uint64_t chunk_size,
                                    uint8_t* dirty, size_t* n_dirty) {
    if (n_dirty) *n_dirty = 0;
    if (chunk_size == 0) return PBS_ERR_INVALID;
    if (size == 0) return PBS_OK;
    if (!prev || !cur || !dirty) return PBS_ERR_INVALID;
    size_t cnt = 0, i = 0;
    for (uint64_t s = 0; s < size; s += chunk_size, ++i) {
        const uint64_t l = size - s < chunk_size ? size - s : chunk_size;
        dirty[i] = std::memcmp(prev + s, cur + s, (size_t)l) != 0 ? 1 : 0;
        cnt += dirty[i];
        if (size - s <= chunk_size) break;  // (s += chunk_size cannot wrap)
    }
    if (n_dirty) *n_dirty = cnt;
    return PBS_OK;
}
