// What the device side (pbs_gc.hip) and the host mirror (pbs_gc_host.cpp) of include/pbs_gc.h
// share: the argument rules, the table's size and hash, and the layout of an index image.
// Plain C++, no device code.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cstring>

#include "pbs_chunker.h"
#include "pbs_gc.h"

namespace pbs {
namespace gc {

constexpr uint64_t kGcMaxEntries = 0xFFFFFFF0ull;  // n, m < 2^32 - 16
constexpr uint64_t kGcHashMul = 0x9E3779B97F4A7C15ull;

// smallest L with 2^L >= max(2 m, 64)
inline uint32_t table_log2_for(uint64_t m) {
    uint32_t l = 6;
    while ((1ull << l) < 2 * m) ++l;
    return l;
}

inline uint64_t get_le64(const uint8_t* p) {
    uint64_t v = 0;
    for (int i = 0; i < 8; ++i) v |= (uint64_t)p[i] << (8 * i);
    return v;
}

inline bool flags_valid(const uint8_t* flags, size_t m) {
    for (size_t j = 0; j < m; ++j)
        if (flags[j] & ~(PBS_GC_BAD | PBS_GC_FOREIGN)) return false;
    return true;
}

// the rules of pbs_gc_mark_device's arguments
inline bool mark_args_valid(const void* base, size_t stride, size_t n, const uint32_t* missing_pos, size_t cap) {
    if (stride < 32 || (stride & 7) || ((uintptr_t)base & 7) || n >= kGcMaxEntries) return false;
    if ((n && !base) || (cap && !missing_pos)) return false;
    if (n > 1 && (n - 1) > (SIZE_MAX - 32) / stride) return false;
    return true;
}

// min_atime of sweep_unused_chunks (chunk_store.rs:363-369); false when the times are not legal
inline bool sweep_min_atime(int64_t phase1_start, int64_t oldest_writer, int64_t* min_atime) {
    if (oldest_writer > phase1_start || phase1_start < INT64_MIN + 86400 + 300 || oldest_writer < INT64_MIN + 300)
        return false;
    int64_t t = phase1_start - 86400;
    if (oldest_writer < t) t = oldest_writer;
    *min_atime = t - 300;
    return true;
}

// Where the digests of an index image lie: entry i at image + off + i * stride.
struct IndexLayout {
    size_t off = 0, stride = 0, n = 0;
    uint64_t index_bytes = 0;
};

// DYNAMIC_SIZED_CHUNK_INDEX_1_0 / FIXED_SIZED_CHUNK_INDEX_1_0 (pbs-datastore/src/file_formats.rs:20-24)
constexpr uint8_t kDidxMagic[8] = {28, 145, 78, 165, 25, 186, 179, 205};
constexpr uint8_t kFidxMagic[8] = {47, 127, 65, 237, 145, 253, 15, 205};

// The checks of pbs_didx_parse (pbs_didx_read.cpp) and pbs_fidx_parse (pbs_fidx.cpp), in their
// order and with their codes, without copying anything out.
inline int index_layout(const uint8_t* image, size_t len, IndexLayout* out) {
    constexpr size_t kHeader = 4096;
    if (!image || len < kHeader) return PBS_ERR_INVALID;
    IndexLayout lo;
    if (std::memcmp(image, kDidxMagic, 8) == 0) {
        if ((len - kHeader) % 40) return PBS_ERR_INVALID;
        lo.off = kHeader + 8;
        lo.stride = 40;
        lo.n = (len - kHeader) / 40;
        uint64_t prev = 0;
        const uint8_t* e = image + kHeader;
        for (size_t i = 0; i < lo.n; ++i, e += 40) {
            const uint64_t end = get_le64(e);
            if (end < prev) return PBS_ERR_INVALID;
            prev = end;
        }
        lo.index_bytes = prev;
    } else if (std::memcmp(image, kFidxMagic, 8) == 0) {
        const uint64_t sz = get_le64(image + 64), cs = get_le64(image + 72);
        if (cs == 0) return PBS_ERR_INVALID;
        const uint64_t cnt = sz / cs + (sz % cs ? 1 : 0);
        if (cnt > (SIZE_MAX - kHeader) / 32 || cnt * 32 != len - kHeader) return PBS_ERR_INVALID;
        if (sz == 0) return PBS_ERR_INVALID;
        if (cs & (cs - 1)) return PBS_ERR_NOT_POW2;
        lo.off = kHeader;
        lo.stride = 32;
        lo.n = (size_t)cnt;
        lo.index_bytes = sz;
    } else {
        return PBS_ERR_INVALID;
    }
    if (lo.n >= kGcMaxEntries) return PBS_ERR_INVALID;
    *out = lo;
    return PBS_OK;
}

}  // namespace gc
}  // namespace pbs
