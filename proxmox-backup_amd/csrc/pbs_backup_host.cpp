// Host mirror of the backup session (include/pbs_backup.h, pbs_backup_*_host): the sequential
// rules of the header, item by item over a hash map from digest to lowest entry position, and a
// blob at a time through the verify mirror's verdict with the stored CRC left unjudged
// (pbs_verify_host.cpp).  The table itself is not kept, only its L by the rules of
// sync_common.h, so the mirror and the device agree on it.  The writers, the counters and the
// closes are backup_common.h's, the same code the device side runs.  Plain C++: no device code,
// so the sanitizer program of tests/cpp/backup_sanitize.cpp builds it with the host compiler.
#include <stdint.h>

#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "backup_common.h"
#include "pbs_backup.h"
#include "sync_common.h"
#include "verify_common.h"

namespace {

using namespace pbs::backup;

inline std::string key(const uint8_t* d) { return std::string(reinterpret_cast<const char*>(d), 32); }

struct HostEntries {
    std::vector<uint8_t> digests, present, kind, known;  // 32, 1, 1 and 1 per entry
    std::vector<uint64_t> size;
    std::vector<uint32_t> ksize;
    std::unordered_map<std::string, uint32_t> lowest;  // digest -> the lowest entry position carrying it
    uint32_t l2 = 0;
    double last_ms = -1;  // (the device side's kernel time: the mirror reports its host clock)

    size_t count() const { return present.size(); }
    uint32_t log2() const { return l2; }

    // the digest's entry, appended with present = 0 if new
    uint32_t entry(const uint8_t* d) {
        auto it = lowest.find(key(d));
        if (it != lowest.end()) return it->second;
        const uint32_t c = (uint32_t)count();
        digests.insert(digests.end(), d, d + 32);
        present.push_back(0);
        kind.push_back(PBS_BLOB_KIND_NONE);
        known.push_back(0);
        size.push_back(0);
        ksize.push_back(0);
        lowest.emplace(key(d), c);
        return c;
    }

    int listing(uint8_t* d, uint8_t* p, uint64_t* s, uint8_t* k, uint8_t* kn, uint32_t* ks, size_t n) const {
        if (d) std::memcpy(d, digests.data(), 32 * n);
        if (p) std::memcpy(p, present.data(), n);
        if (s) std::memcpy(s, size.data(), 8 * n);
        if (k) std::memcpy(k, kind.data(), n);
        if (kn) std::memcpy(kn, known.data(), n);
        if (ks) std::memcpy(ks, ksize.data(), 4 * n);
        return PBS_OK;
    }

    int lookup(const uint8_t* d, bool* is_known, uint32_t* sz) const {
        auto it = lowest.find(key(d));
        *is_known = it != lowest.end() && known[it->second];
        *sz = *is_known ? ksize[it->second] : 0;
        return PBS_OK;
    }

    int register_previous(const uint8_t* d, const uint32_t* sizes, size_t n) {
        l2 = pbs::sync::plan_log2(count(), n, l2);
        for (size_t i = 0; i < n; ++i) {
            const uint32_t c = entry(d + 32 * i);
            known[c] = 1;
            ksize[c] = sizes[i];
        }
        return PBS_OK;
    }

    int verdicts(const uint8_t* blobs, const uint64_t* off, const uint8_t* d, const uint32_t* sizes, size_t k,
                 const uint8_t* pre, uint8_t* kinds, uint8_t* status, uint32_t* crc, pbs_backup_timing* tm) {
        const Clock::time_point t0 = Clock::now();
        for (size_t t = 0; t < k; ++t) {
            if (pre[t]) continue;
            const size_t len = (size_t)(off[t + 1] - off[t]);
            status[t] = pbs::verify::host_blob_verdict_upload(blobs + off[t], len, d + 32 * t, sizes[t], &kinds[t], &crc[t]);
            tm->decoded += 1;
            if (kinds[t] != PBS_BLOB_KIND_NONE && kinds[t] >= 2) tm->encrypted += 1;
            else tm->scratch_bytes += sizes[t];
        }
        tm->decode_ms = ms_since(t0);
        return PBS_OK;
    }

    int insert_batch(const uint8_t* d, const uint8_t* status, const uint8_t* kinds, const uint32_t* lens,
                     const uint32_t* sizes, size_t k, bool fixed, uint64_t chunk_size, uint64_t small, uint8_t* ins,
                     uint8_t* action, uint8_t* dup, uint32_t* comp, uint8_t* reg, double* ms) {
        const Clock::time_point t0 = Clock::now();
        l2 = pbs::sync::plan_log2(count(), k, l2);
        for (size_t t = 0; t < k; ++t) {
            ins[t] = PBS_BACKUP_INS_NONE;
            reg[t] = PBS_BACKUP_REG_NONE;
            if (status[t] != PBS_BLOB_ST_OK) continue;
            const uint32_t c = entry(d + 32 * t);
            EntryState e{size[c], present[c], kind[c]};
            ins[t] = insert_step(e, lens[t], kinds[t], &action[t], &dup[t], &comp[t]);
            present[c] = e.present;
            size[c] = e.size;
            kind[c] = e.kind;
            if (!ins_ok(ins[t])) continue;
            if (fixed && sizes[t] < chunk_size) small += 1;
            reg[t] = register_rule(fixed, chunk_size, sizes[t], small);
            if (reg[t] == PBS_BACKUP_REG_OK) {
                known[c] = 1;
                ksize[c] = sizes[t];
            }
        }
        *ms = ms_since(t0);
        return PBS_OK;
    }

    int append_dynamic(const uint8_t* d, const uint64_t* offsets, size_t n, uint64_t start, size_t* n_done, int* err,
                       uint64_t* ends) const {
        uint64_t offset = start;
        size_t i = 0;
        *err = PBS_BACKUP_E_NONE;
        for (; i < n; ++i) {
            bool kn;
            uint32_t ks;
            lookup(d + 32 * i, &kn, &ks);
            if ((*err = dynamic_append_code(kn, offsets[i], offset)) != PBS_BACKUP_E_NONE) break;
            offset += ks;
            ends[i] = offset;
        }
        *n_done = i;
        return PBS_OK;
    }

    int append_fixed(const uint8_t* d, const uint64_t* offsets, size_t n, uint64_t sz, uint64_t chunk_size,
                     uint64_t index_length, size_t* n_done, int* err, uint64_t* idx) const {
        size_t i = 0;
        *err = PBS_BACKUP_E_NONE;
        for (; i < n; ++i) {
            bool kn;
            uint32_t ks;
            lookup(d + 32 * i, &kn, &ks);
            if (!kn) {
                *err = PBS_BACKUP_E_NO_SUCH_CHUNK;
                break;
            }
            size_t at = 0;  // check_chunk_alignment itself: the device runs backup_common.h's copy of it
            const int rc = pbs_fidx_check_chunk_alignment(sz, chunk_size, offsets[i] + ks, ks, &at);
            if (rc != PBS_OK) {
                *err = rc;
                break;
            }
            if (at >= index_length) {
                *err = PBS_BACKUP_E_INDEX_RANGE;
                break;
            }
            idx[i] = at;
        }
        *n_done = i;
        return PBS_OK;
    }
};

struct NoGuard {
    bool ok = true;
    explicit NoGuard(const void*) {}
};

}  // namespace

struct pbs_backup_host {
    pbs::backup::Session<HostEntries> s;
};

extern "C" int pbs_backup_begin_host(const uint8_t* store_digests, const uint64_t* store_sizes, const uint8_t* store_kinds,
                                     size_t m, size_t reserve, pbs_backup_host** out, double* build_ms) {
    const Clock::time_point t0 = Clock::now();
    if (out) *out = nullptr;
    if (build_ms) *build_ms = 0;
    if (!begin_args_valid(store_digests, store_sizes, store_kinds, m, reserve, out)) return PBS_ERR_INVALID;
    pbs_backup_host* h = new (std::nothrow) pbs_backup_host;
    if (!h) return PBS_ERR_NOMEM;
    try {
        HostEntries& e = h->s.e;
        if (m) {
            e.digests.assign(store_digests, store_digests + 32 * m);
            e.size.assign(store_sizes, store_sizes + m);
            e.kind.assign(store_kinds, store_kinds + m);
        }
        e.present.assign(m, 1);
        e.known.assign(m, 0);
        e.ksize.assign(m, 0);
        e.lowest.reserve(m + reserve);
        for (size_t j = 0; j < m; ++j) e.lowest.emplace(key(store_digests + 32 * j), (uint32_t)j);  // (the first stays)
        e.l2 = pbs::sync::begin_log2(m, reserve);
    } catch (const std::bad_alloc&) {
        delete h;
        return PBS_ERR_NOMEM;
    }
    pbs::Live<pbs_backup_host>::add(h);
    *out = h;
    if (build_ms) *build_ms = ms_since(t0);
    return PBS_OK;
}

extern "C" void pbs_backup_end_host(pbs_backup_host* h) {
    if (h && pbs::Live<pbs_backup_host>::remove(h)) delete h;
}

PBS_BACKUP_DEFINE_ABI(_host, pbs_backup_host, NoGuard)
