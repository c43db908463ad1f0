// Host mirror of garbage collection (include/pbs_gc.h, pbs_gc_*_host): the same calls by a sort
// of the store's digests and a binary search per index entry.  Plain C++: no device code, so the
// sanitizer program of tests/cpp/gc_sanitize.cpp builds it with the host compiler.  It is what
// the GPU is compared against, and the library's GC where there is no device.
#include <stdint.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <new>
#include <vector>

#include "gc_common.h"
#include "live_handles.h"
#include "pbs_chunker.h"
#include "pbs_gc.h"

using namespace pbs::gc;

struct pbs_gc_host {
    std::vector<uint8_t> digests, flags, ref;
    // store positions in digest order: `key` is the digest's first 8 bytes, big-endian
    struct Ent {
        uint64_t key;
        uint32_t pos;
    };
    std::vector<Ent> order;
    uint64_t index_file_count = 0, index_data_bytes = 0;
};

namespace {

using Clock = std::chrono::steady_clock;
inline double ms_since(Clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
}

inline uint64_t be64(const uint8_t* p) {
    uint64_t v = 0;
    for (int i = 0; i < 8; ++i) v = (v << 8) | p[i];
    return v;
}

using Handles = pbs::Live<pbs_gc_host>;

// calls f(j) for every store entry j that carries the digest `d`
template <class F>
inline void for_each_match(const pbs_gc_host& h, const uint8_t* d, F f) {
    const uint64_t key = be64(d);
    auto it = std::lower_bound(h.order.begin(), h.order.end(), key,
                               [](const pbs_gc_host::Ent& e, uint64_t k) { return e.key < k; });
    for (; it != h.order.end() && it->key == key; ++it)
        if (std::memcmp(h.digests.data() + 32 * (size_t)it->pos, d, 32) == 0) f(it->pos);
}

int mark(pbs_gc_host* h, const uint8_t* base, size_t stride, size_t n, bool whole, uint64_t index_bytes,
         uint32_t* missing_pos, size_t cap, size_t* n_missing, double* mark_ms) {
    const Clock::time_point t0 = Clock::now();
    if (n_missing) *n_missing = 0;
    if (mark_ms) *mark_ms = 0;
    if (!Handles::alive(h) || !mark_args_valid(base, stride, n, missing_pos, cap)) return PBS_ERR_INVALID;
    size_t missing = 0;
    for (size_t i = 0; i < n; ++i) {
        bool chunk = false;
        for_each_match(*h, base + i * stride, [&](uint32_t j) {
            h->ref[j] = 1;
            if (h->flags[j] == 0) chunk = true;
        });
        if (!chunk) {
            if (missing < cap) missing_pos[missing] = (uint32_t)i;
            ++missing;
        }
    }
    if (whole) {
        h->index_file_count += 1;
        h->index_data_bytes += index_bytes;
    }
    if (n_missing) *n_missing = missing;
    if (mark_ms) *mark_ms = ms_since(t0);
    return PBS_OK;
}

bool entry_touched(const pbs_gc_host& h, size_t j) {
    const uint8_t f = h.flags[j];
    if (!h.ref[j] || (f & PBS_GC_FOREIGN)) return false;
    if (f == 0) return true;
    bool chunk = false;
    for_each_match(h, h.digests.data() + 32 * j, [&](uint32_t k) {
        if (h.flags[k] == 0) chunk = true;
    });
    return !chunk;
}

}  // namespace

extern "C" uint64_t pbs_gc_home_slot(const uint8_t digest[32], uint32_t table_log2) {
    if (!digest || table_log2 < 1 || table_log2 > 63) return 0;
    return (be64(digest) * kGcHashMul) >> (64 - table_log2);
}

extern "C" int pbs_gc_begin_host(const uint8_t* store_digests, const uint8_t* flags, size_t m, pbs_gc_host** out,
                                 double* build_ms) {
    const Clock::time_point t0 = Clock::now();
    if (out) *out = nullptr;
    if (build_ms) *build_ms = 0;
    if (!out || (m && (!store_digests || !flags)) || m >= kGcMaxEntries || !flags_valid(flags, m))
        return PBS_ERR_INVALID;
    pbs_gc_host* h = new (std::nothrow) pbs_gc_host;
    if (!h) return PBS_ERR_NOMEM;
    try {
        if (m) {
            h->digests.assign(store_digests, store_digests + 32 * m);
            h->flags.assign(flags, flags + m);
        }
        h->ref.assign(m, 0);
        h->order.resize(m);
        for (size_t j = 0; j < m; ++j) h->order[j] = {be64(store_digests + 32 * j), (uint32_t)j};
        std::sort(h->order.begin(), h->order.end(), [](const pbs_gc_host::Ent& a, const pbs_gc_host::Ent& b) {
            return a.key != b.key ? a.key < b.key : a.pos < b.pos;
        });
    } catch (const std::bad_alloc&) {
        delete h;
        return PBS_ERR_NOMEM;
    }
    Handles::add(h);
    *out = h;
    if (build_ms) *build_ms = ms_since(t0);
    return PBS_OK;
}

extern "C" int pbs_gc_mark_host(pbs_gc_host* h, const uint8_t* base, size_t stride, size_t n, uint64_t index_bytes,
                                uint32_t* missing_pos, size_t cap, size_t* n_missing, double* mark_ms) {
    return mark(h, base, stride, n, true, index_bytes, missing_pos, cap, n_missing, mark_ms);
}

extern "C" int pbs_gc_mark_piece_host(pbs_gc_host* h, const uint8_t* base, size_t stride, size_t n,
                                      uint32_t* missing_pos, size_t cap, size_t* n_missing, double* mark_ms) {
    return mark(h, base, stride, n, false, 0, missing_pos, cap, n_missing, mark_ms);
}

extern "C" int pbs_gc_mark_index_image_host(pbs_gc_host* h, const uint8_t* image, size_t len, uint32_t* missing_pos,
                                            size_t cap, size_t* n_missing, double* mark_ms) {
    if (n_missing) *n_missing = 0;
    if (mark_ms) *mark_ms = 0;
    if (!Handles::alive(h)) return PBS_ERR_INVALID;
    IndexLayout lo;
    const int rc = index_layout(image, len, &lo);
    if (rc != PBS_OK) return rc;
    return mark(h, image + lo.off, lo.stride, lo.n, true, lo.index_bytes, missing_pos, cap, n_missing, mark_ms);
}

extern "C" int pbs_gc_touched_host(pbs_gc_host* h, uint8_t* touched, size_t* n_touched) {
    if (n_touched) *n_touched = 0;
    if (!Handles::alive(h)) return PBS_ERR_INVALID;
    const size_t m = h->flags.size();
    if (m && !touched) return PBS_ERR_INVALID;
    size_t cnt = 0;
    for (size_t j = 0; j < m; ++j) cnt += (touched[j] = entry_touched(*h, j) ? 1 : 0);
    if (n_touched) *n_touched = cnt;
    return PBS_OK;
}

extern "C" int pbs_gc_sweep_host(pbs_gc_host* h, const uint64_t* sizes, const int64_t* atimes, int64_t phase1_start,
                                 int64_t oldest_writer, uint8_t* actions, pbs_gc_status* status, double* sweep_ms) {
    const Clock::time_point t0 = Clock::now();
    if (sweep_ms) *sweep_ms = 0;
    if (!Handles::alive(h)) return PBS_ERR_INVALID;
    const size_t m = h->flags.size();
    int64_t min_atime = 0;
    if ((m && (!sizes || !atimes)) || !sweep_min_atime(phase1_start, oldest_writer, &min_atime)) return PBS_ERR_INVALID;
    pbs_gc_status s;
    std::memset(&s, 0, sizeof(s));
    s.index_file_count = h->index_file_count;
    s.index_data_bytes = h->index_data_bytes;
    for (size_t j = 0; j < m; ++j) {
        uint8_t act = PBS_GC_KEEP;
        if (sizes[j] != PBS_GC_VANISHED) {
            const bool bad = (h->flags[j] & PBS_GC_BAD) != 0;
            // (min_atime < oldest_writer: only an entry older than oldest_writer needs the question)
            const bool touched = atimes[j] < oldest_writer && entry_touched(*h, j);
            if (!touched && atimes[j] < min_atime) {
                act = PBS_GC_REMOVE;
                if (bad)
                    s.removed_bad += 1;
                else
                    s.removed_chunks += 1;
                s.removed_bytes += sizes[j];
            } else if (!touched && atimes[j] < oldest_writer) {
                act = PBS_GC_PENDING;
                if (bad)
                    s.still_bad += 1;
                else
                    s.pending_chunks += 1;
                s.pending_bytes += sizes[j];
            } else {
                if (!bad) s.disk_chunks += 1;
                s.disk_bytes += sizes[j];
            }
        }
        if (actions) actions[j] = act;
    }
    if (status) *status = s;
    if (sweep_ms) *sweep_ms = ms_since(t0);
    return PBS_OK;
}

extern "C" void pbs_gc_end_host(pbs_gc_host* h) {
    if (h && Handles::remove(h)) delete h;
}
