// Host side of the restore path (include/pbs_restore.h): the dynamic index reader
// (DynamicIndexReader, pbs-datastore/src/dynamic_index.rs:82-275) over the image that
// pbs_didx.cpp writes, and the host mirror of the digest lookup.  Plain C++: no device code,
// so the sanitizer program of tests/cpp/restore_sanitize.cpp builds it with the host compiler.
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <numeric>
#include <vector>

#include "pbs_chunker.h"
#include "pbs_digest.h"
#include "pbs_restore.h"

namespace {

// DYNAMIC_SIZED_CHUNK_INDEX_1_0 (pbs-datastore/src/file_formats.rs:24)
constexpr uint8_t kDidxMagic[8] = {28, 145, 78, 165, 25, 186, 179, 205};
constexpr size_t kHeader = 4096;
constexpr size_t kEntry = 40;

inline uint64_t get_le64(const uint8_t* p) {
    uint64_t v = 0;
    for (int i = 0; i < 8; ++i) v |= (uint64_t)p[i] << (8 * i);
    return v;
}

}  // namespace

extern "C" size_t pbs_didx_count(size_t image_len) {
    if (image_len < kHeader || (image_len - kHeader) % kEntry) return (size_t)-1;
    return (image_len - kHeader) / kEntry;
}

extern "C" int pbs_didx_parse(const uint8_t* image, size_t len, uint8_t uuid[16], int64_t* ctime,
                              uint8_t header_csum[32], uint8_t computed_csum[32], uint64_t* ends,
                              uint8_t* digests, size_t cap, size_t* n) {
    if (n) *n = 0;
    if (!image || len < kHeader) return PBS_ERR_INVALID;               // "index too small"
    if (std::memcmp(image, kDidxMagic, 8) != 0) return PBS_ERR_INVALID;  // "got unknown magic number"
    const size_t cnt = pbs_didx_count(len);
    if (cnt == (size_t)-1) return PBS_ERR_INVALID;                     // "got unexpected file size"
    if (n) *n = cnt;
    if (cap < cnt) return PBS_ERR_CAPACITY;
    if (cnt && (!ends || !digests)) return PBS_ERR_INVALID;
    const uint8_t* e = image + kHeader;
    uint64_t prev = 0;
    for (size_t i = 0; i < cnt; ++i, e += kEntry) {
        const uint64_t end = get_le64(e);
        if (end < prev) return PBS_ERR_INVALID;
        prev = end;
    }
    e = image + kHeader;
    for (size_t i = 0; i < cnt; ++i, e += kEntry) {
        ends[i] = get_le64(e);
        std::memcpy(digests + 32 * i, e + 8, 32);
    }
    if (uuid) std::memcpy(uuid, image + 8, 16);
    if (ctime) *ctime = (int64_t)get_le64(image + 24);
    if (header_csum) std::memcpy(header_csum, image + 32, 32);
    // the entries are end_le || digest already: compute_csum hashes the body as it stands
    if (computed_csum) pbs_sha256(image + kHeader, cnt * kEntry, computed_csum);
    return PBS_OK;
}

extern "C" int pbs_didx_chunk_from_offset(const uint64_t* ends, size_t n, uint64_t offset, size_t* idx,
                                          uint64_t* within) {
    if (!ends || n == 0) return PBS_ERR_INVALID;
    // binary_search(start_idx, start, end_idx, end, offset), :172-195, as a loop: every step
    // of the recursion is a tail call
    size_t start_idx = 0, end_idx = n - 1;
    uint64_t start = 0, end = ends[n - 1];
    for (;;) {
        if (offset >= end || offset < start) return PBS_ERR_INVALID;  // "offset out of range"
        if (end_idx == start_idx) break;
        const size_t middle_idx = (start_idx + end_idx) / 2;
        const uint64_t middle_end = ends[middle_idx];
        if (offset < middle_end) {
            end_idx = middle_idx;
            end = middle_end;
        } else {
            start_idx = middle_idx + 1;
            start = middle_end;
        }
    }
    if (idx) *idx = start_idx;
    if (within) *within = offset - (start_idx == 0 ? 0 : ends[start_idx - 1]);
    return PBS_OK;
}

extern "C" int pbs_digest_lookup_host(const uint8_t* digests, size_t n, const uint8_t* store, size_t m,
                                      uint32_t* store_pos, uint32_t* first, size_t* n_missing,
                                      size_t* n_unique) {
    if (n_missing) *n_missing = 0;
    if (n_unique) *n_unique = 0;
    if (n == 0) return PBS_OK;
    if (!digests || !store_pos || !first || (m && !store) || n > 0xFFFFFFF0u || m > 0xFFFFFFF0u)
        return PBS_ERR_INVALID;
    // positions sorted by digest, equal digests in ascending position
    auto sorted = [](const uint8_t* d, size_t k) {
        std::vector<uint32_t> o(k);
        std::iota(o.begin(), o.end(), 0u);
        std::stable_sort(o.begin(), o.end(), [d](uint32_t a, uint32_t b) {
            return std::memcmp(d + 32 * (size_t)a, d + 32 * (size_t)b, 32) < 0;
        });
        return o;
    };
    const std::vector<uint32_t> so = sorted(store, m);
    const std::vector<uint32_t> io = sorted(digests, n);
    size_t missing = 0, unique = 0;
    for (size_t p = 0; p < n;) {
        const uint8_t* d = digests + 32 * (size_t)io[p];
        size_t q = p;
        while (q < n && std::memcmp(digests + 32 * (size_t)io[q], d, 32) == 0) ++q;
        const auto it = std::lower_bound(so.begin(), so.end(), d, [store](uint32_t a, const uint8_t* key) {
            return std::memcmp(store + 32 * (size_t)a, key, 32) < 0;
        });
        const uint32_t pos = it != so.end() && std::memcmp(store + 32 * (size_t)*it, d, 32) == 0
                                 ? *it
                                 : PBS_LOOKUP_MISSING;
        for (size_t r = p; r < q; ++r) {
            store_pos[io[r]] = pos;
            first[io[r]] = io[p];
        }
        ++unique;
        if (pos == PBS_LOOKUP_MISSING) missing += q - p;
        p = q;
    }
    if (n_missing) *n_missing = missing;
    if (n_unique) *n_unique = unique;
    return PBS_OK;
}
