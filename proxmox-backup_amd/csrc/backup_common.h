// What the device side (pbs_backup.hip) and the host mirror (pbs_backup_host.cpp) of
// include/pbs_backup.h share: the insert rule and the append checks as functions both a lane and
// the host can call, the argument rules, the index writers (they live on the host in both), the
// session's counters, the closes and the C ABI over a session.  A session is a `Session<Entries>`:
// `Entries` is what differs -- the digest list with its table and the per-entry state, in device
// memory (pbs_backup.hip) or in vectors (pbs_backup_host.cpp).  Plain C++ unless a .hip file
// includes it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <chrono>
#include <cstring>
#include <map>
#include <new>
#include <vector>

#include "gc_common.h"
#include "live_handles.h"
#include "pbs_backup.h"
#include "pbs_blob.h"
#include "pbs_chunker.h"
#include "pbs_digest.h"
#include "pbs_fixed.h"
#include "sync_common.h"
#include "verify_common.h"

#ifdef __HIPCC__
#define PBS_HD __host__ __device__
#else
#define PBS_HD
#endif

namespace pbs {
namespace backup {

using gc::kGcMaxEntries;

constexpr uint32_t kMaxWriters = 256;
constexpr uint32_t kMaxEncoded = PBS_BACKUP_MAX_CHUNK + PBS_BLOB_ENC_HEADER_SIZE;  // 16 MiB + 44

// ---- rules a lane and the host share -------------------------------------------------------------

struct EntryState {
    uint64_t size;
    uint8_t present, kind;
};

PBS_HD inline bool ins_ok(uint8_t ins) { return ins >= PBS_BACKUP_INS_NEW && ins <= PBS_BACKUP_INS_REPLACE_BIGGER; }
PBS_HD inline bool ins_writes(uint8_t ins) {
    return ins == PBS_BACKUP_INS_NEW || ins == PBS_BACKUP_INS_OVERWRITE_EMPTY || ins == PBS_BACKUP_INS_REPLACE_BIGGER;
}

// insert_chunk (chunk_store.rs:457-497) for a blob of `len` bytes and magic `bkind` against the
// file the entry describes: the outcome, first clause first
PBS_HD inline uint8_t insert_rule(const EntryState& e, uint32_t len, uint8_t bkind) {
    if (!e.present) return PBS_BACKUP_INS_NEW;
    if (e.kind == PBS_BACKUP_KIND_NOT_FILE) return PBS_BACKUP_INS_ERR_TYPE;
    if (len == e.size) return PBS_BACKUP_INS_DUP_SAME;
    if (e.size == 0) return PBS_BACKUP_INS_OVERWRITE_EMPTY;
    if (bkind >= 2) {
        if (e.kind == PBS_BLOB_KIND_NONE) return PBS_BACKUP_INS_ERR_READ;
        if (e.kind < 2) return PBS_BACKUP_INS_ERR_UNENC_TO_ENC;
        if (e.kind == PBS_BLOB_KIND_ENCRYPTED && bkind == PBS_BLOB_KIND_ENCRYPTED) return PBS_BACKUP_INS_ERR_ENC_UNCOMPRESSED;
        return PBS_BACKUP_INS_DUP_KEEP_FIRST;
    }
    if (e.size < len) return PBS_BACKUP_INS_DUP_KEEP_SMALLER;
    return PBS_BACKUP_INS_REPLACE_BIGGER;
}

// one upload against its entry: the outcome, what the caller does and what register_*_chunk is
// told; the entry changes where the file is written
PBS_HD inline uint8_t insert_step(EntryState& e, uint32_t len, uint8_t bkind, uint8_t* action, uint8_t* dup,
                                  uint32_t* comp) {
    const uint8_t ins = insert_rule(e, len, bkind);
    *action = PBS_BACKUP_ACT_NONE;
    *dup = 0;
    *comp = 0;
    if (ins_writes(ins)) {
        e.present = 1;
        e.size = len;
        e.kind = bkind;
        *action = PBS_BACKUP_ACT_WRITE;
        *comp = len;
    } else if (ins_ok(ins)) {
        *action = PBS_BACKUP_ACT_TOUCH;
        *dup = 1;
        *comp = (uint32_t)e.size;
    }
    return ins;
}

// register_fixed_chunk's checks (environment.rs:187-204) with `smalls` chunks under chunk_size
// registered or refused so far, this one included
PBS_HD inline uint8_t register_rule(bool fixed, uint64_t chunk_size, uint32_t size, uint64_t smalls) {
    if (!fixed) return PBS_BACKUP_REG_OK;
    if (size > chunk_size) return PBS_BACKUP_REG_ERR_LARGE;
    if (size < chunk_size && smalls > 1) return PBS_BACKUP_REG_ERR_MULTI_SMALL;
    return PBS_BACKUP_REG_OK;
}

// one dynamic append (environment.rs:336-343 after mod.rs' lookup)
PBS_HD inline int dynamic_append_code(bool known, uint64_t offset, uint64_t expected) {
    if (!known) return PBS_BACKUP_E_NO_SUCH_CHUNK;
    return offset == expected ? PBS_BACKUP_E_NONE : PBS_BACKUP_E_STRANGE_OFFSET;
}

// one fixed append: pbs_fidx_check_chunk_alignment clause by clause (pbs_fidx.cpp; the tests hold
// the two together), then add_digest's range check
PBS_HD inline int fixed_append_code(bool known, uint32_t ksize, uint64_t offset, uint64_t size, uint64_t chunk_size,
                                    uint64_t index_length, uint64_t* idx) {
    if (!known) return PBS_BACKUP_E_NO_SUCH_CHUNK;
    const uint64_t end = offset + ksize, len = ksize;  // (a wrapped sum is "small offset")
    if (chunk_size & (chunk_size - 1)) return PBS_ERR_NOT_POW2;
    if (end < len) return PBS_ERR_INVALID;
    if (end > size) return PBS_ERR_INVALID;
    if ((end != size && len != chunk_size) || len > chunk_size || len == 0) return PBS_ERR_INVALID;
    const uint64_t pos = end - len;
    if (pos & (chunk_size - 1)) return PBS_ERR_INVALID;
    *idx = pos / chunk_size;
    return *idx >= index_length ? PBS_BACKUP_E_INDEX_RANGE : PBS_BACKUP_E_NONE;
}

// the API schema of one upload and its length check (upload_chunk.rs:123-142, :62-74): 0 or a status
inline uint8_t upload_pre(uint32_t size, const uint32_t* encoded_size, uint64_t len) {
    const uint64_t enc = encoded_size ? *encoded_size : len;
    if (size < 1 || size > PBS_BACKUP_MAX_CHUNK || enc < PBS_BLOB_HEADER_SIZE + 1 || enc > kMaxEncoded)
        return PBS_BACKUP_ST_BAD_PARAM;
    return len == enc ? 0 : PBS_BACKUP_ST_WRONG_LENGTH;
}

inline bool begin_args_valid(const uint8_t* digests, const uint64_t* sizes, const uint8_t* kinds, size_t m, size_t reserve,
                             const void* out) {
    if (m && (!sizes || !kinds)) return false;
    return sync::begin_args_valid(digests, m, reserve, out);
}

// ---- the writers and the session's counters (host, in both sessions) -----------------------------

struct UploadStat {
    uint64_t count = 0, size = 0, compressed_size = 0, duplicates = 0;
    void add(const UploadStat& o) {
        count += o.count;
        size += o.size;
        compressed_size += o.compressed_size;
        duplicates += o.duplicates;
    }
};

struct Writer {
    bool fixed = false, incremental = false;
    uint8_t uuid[16] = {};
    int64_t ctime = 0;
    uint64_t offset = 0, chunk_count = 0;                            // dynamic: the running end
    uint64_t size = 0, chunk_size = 0, index_length = 0, small = 0;  // fixed
    UploadStat stat;
    std::vector<uint64_t> ends;    // dynamic: one per entry
    std::vector<uint8_t> digests;  // dynamic: 32 per entry; fixed: 32 index_length, zeros where nothing was added
};

// log_upload_stat (environment.rs:380-428)
inline void writer_stat(const UploadStat& u, uint64_t size, uint64_t chunk_count, pbs_backup_writer_stat* s) {
    std::memset(s, 0, sizeof(*s));
    s->count = u.count;
    s->size = u.size;
    s->compressed_size = u.compressed_size;
    s->duplicates = u.duplicates;
    s->chunk_count = chunk_count;
    s->archive_size = size;
    if (size == 0 || chunk_count == 0) return;
    s->logged = 1;
    s->upload_percent = u.size * 100 / size;
    s->client_duplicates = chunk_count < u.count ? 0 : chunk_count - u.count;
    s->server_duplicates = u.duplicates;
    if (s->client_duplicates + s->server_duplicates > 0)
        s->duplicate_percent = (s->client_duplicates + s->server_duplicates) * 100 / chunk_count;
    if (u.size > 0) s->compression_percent = u.compressed_size * 100 / u.size;
}

using Clock = std::chrono::steady_clock;
inline double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

// What `Entries` provides (E below):
//   size_t count();  uint32_t log2();
//   int listing(digests, present, size, kind, known, known_size, k)      the first k entries
//   int lookup(digest, bool* known, uint32_t* size)
//   int register_previous(digests, sizes, n)
//   double last_ms       the kernels of the last register or append by HIP events, or < 0: none
//   int verdicts(blobs, off, digests, sizes, k, pre, kinds, status, crc, tm)
//        for the items with pre[t] == 0: kind, status (encrypted blobs that load: NO_CONFIG or OK) and
//        the payload's CRC; the others keep what the arrays hold
//   int insert_batch(digests, status, kinds, lens, sizes, k, fixed, chunk_size, small_before,
//                    ins, action, dup, comp, reg, ms)
//   int append_dynamic(digests, offsets, n, start, n_done, err, ends)
//   int append_fixed(digests, offsets, n, size, chunk_size, index_length, n_done, err, idx)
template <class E>
struct Session {
    E e;
    bool finished = false;
    uint32_t uid = 0;
    uint64_t file_counter = 0, backup_size = 0;
    UploadStat backup_stat;
    std::map<uint32_t, Writer> writers;
    // (work arrays of a batch, kept between calls)
    std::vector<uint8_t> pre, kinds, status, ins, action, dup, reg;
    std::vector<uint32_t> crc, comp, lens;
    std::vector<uint64_t> tmp64;

    void stats(pbs_backup_stat* s) const {
        std::memset(s, 0, sizeof(*s));
        s->file_counter = file_counter;
        s->backup_size = backup_size;
        s->count = backup_stat.count;
        s->size = backup_stat.size;
        s->compressed_size = backup_stat.compressed_size;
        s->duplicates = backup_stat.duplicates;
        s->open_writers = (uint32_t)writers.size();
        s->finished = finished;
    }

    int finish(pbs_backup_stat* s) {
        if (finished) return PBS_BACKUP_E_FINISHED;
        if (!writers.empty()) return PBS_BACKUP_E_OPEN_WRITER;
        if (file_counter == 0) return PBS_BACKUP_E_NO_FILES;
        finished = true;
        if (s) stats(s);
        return PBS_OK;
    }

    int lookup(const uint8_t* digest, uint32_t* size) {
        if (!digest || !size) return PBS_ERR_INVALID;
        *size = 0;
        if (finished) return PBS_BACKUP_E_FINISHED;
        bool known = false;
        const int rc = e.lookup(digest, &known, size);
        if (rc != PBS_OK) return rc;
        return known ? PBS_OK : PBS_BACKUP_E_NO_SUCH_CHUNK;
    }

    int listing(uint8_t* digests, uint8_t* present, uint64_t* size, uint8_t* kind, uint8_t* known, uint32_t* ksize,
                size_t cap, size_t* count) {
        if (count) *count = e.count();
        const size_t k = cap < e.count() ? cap : e.count();
        if (k == 0) return PBS_OK;
        return e.listing(digests, present, size, kind, known, ksize, k);
    }

    int register_previous(const uint8_t* digests, const uint32_t* sizes, size_t n, double* ms) {
        const Clock::time_point t0 = Clock::now();
        if (ms) *ms = 0;
        if (!sync::entries_fit(e.count(), n) || (n && (!digests || !sizes))) return PBS_ERR_INVALID;
        if (finished) return PBS_BACKUP_E_FINISHED;
        if (n == 0) return PBS_OK;
        const int rc = e.register_previous(digests, sizes, n);
        if (ms) *ms = e.last_ms >= 0 ? e.last_ms : ms_since(t0);
        return rc;
    }

    // download_previous of an index (mod.rs:859-863): every chunk of a .didx / .fidx image with
    // the length its chunk_info states.  Recognised and checked as pbs_gc_mark_index_image does it.
    int register_index_image(const uint8_t* image, size_t len, size_t* n_entries, double* ms) {
        if (n_entries) *n_entries = 0;
        if (ms) *ms = 0;
        gc::IndexLayout lo;
        const int rc = gc::index_layout(image, len, &lo);
        if (rc != PBS_OK) return rc;
        std::vector<uint8_t> digests;
        std::vector<uint64_t> sizes;
        verify::index_entries(image, lo, digests, sizes);
        std::vector<uint32_t> s32(lo.n);
        for (size_t i = 0; i < lo.n; ++i) {
            if (sizes[i] > UINT32_MAX) return PBS_ERR_INVALID;  // (register_chunk takes a u32)
            s32[i] = (uint32_t)sizes[i];
        }
        if (n_entries) *n_entries = lo.n;
        return register_previous(digests.data(), s32.data(), lo.n, ms);
    }

    int new_wid(uint32_t* wid) {
        if (uid >= kMaxWriters) return PBS_BACKUP_E_TOO_MANY_WRITERS;
        *wid = ++uid;
        return PBS_OK;
    }

    int create_dynamic(const uint8_t* uuid, int64_t ctime, uint32_t* wid) {
        if (!wid) return PBS_ERR_INVALID;
        *wid = 0;
        if (finished) return PBS_BACKUP_E_FINISHED;
        Writer w;
        if (uuid) std::memcpy(w.uuid, uuid, 16);
        w.ctime = ctime;
        const int rc = new_wid(wid);
        if (rc != PBS_OK) return rc;
        writers.emplace(*wid, std::move(w));
        return PBS_OK;
    }

    int create_fixed(uint64_t size, uint64_t chunk_size, const uint8_t* uuid, int64_t ctime, const uint8_t* reuse_image,
                     size_t reuse_len, const uint8_t* reuse_csum, uint32_t* wid) {
        if (!wid) return PBS_ERR_INVALID;
        *wid = 0;
        if (chunk_size == 0) return PBS_ERR_INVALID;
        const uint64_t n = pbs_fidx_count(size, chunk_size);
        if (n >= kGcMaxEntries) return PBS_ERR_INVALID;
        if (finished) return PBS_BACKUP_E_FINISHED;
        Writer w;
        w.fixed = true;
        if (uuid) std::memcpy(w.uuid, uuid, 16);
        w.ctime = ctime;
        w.size = size;
        w.chunk_size = chunk_size;
        w.index_length = n;
        w.digests.assign(32 * (size_t)n, 0);
        if (reuse_csum) {  // mod.rs:471-507
            w.incremental = true;
            size_t pn = 0;
            uint8_t csum[32];
            if (pbs_fidx_parse(reuse_image, reuse_len, nullptr, nullptr, nullptr, csum, nullptr, nullptr, nullptr, SIZE_MAX,
                               &pn) != PBS_OK)
                return PBS_BACKUP_E_REUSE_NO_IMAGE;
            if (std::memcmp(csum, reuse_csum, 32) != 0) return PBS_BACKUP_E_REUSE_CSUM;
            if (pn != n) return PBS_BACKUP_E_REUSE_LENGTH;  // clone_data_from
            if (n) std::memcpy(w.digests.data(), reuse_image + 4096, 32 * (size_t)n);
        }
        const int rc = new_wid(wid);
        if (rc != PBS_OK) return rc;
        writers.emplace(*wid, std::move(w));
        return PBS_OK;
    }

    Writer* writer(uint32_t wid, bool fixed) {
        auto it = writers.find(wid);
        return it != writers.end() && it->second.fixed == fixed ? &it->second : nullptr;
    }

    int upload(uint32_t wid, const uint8_t* digests, const uint32_t* sizes, const uint32_t* encoded_sizes,
               const uint8_t* blobs, const uint64_t* off, size_t k, uint8_t* status_out, uint32_t* crc_out, uint8_t* ins_out,
               uint8_t* action_out, uint8_t* dup_out, uint32_t* comp_out, uint8_t* reg_out, uint64_t* first_failed,
               pbs_backup_timing* timing) {
        const Clock::time_point t0 = Clock::now();
        if (timing) std::memset(timing, 0, sizeof(*timing));
        if (first_failed) *first_failed = PBS_BACKUP_NONE;
        if (!sync::entries_fit(e.count(), k) || (k && (!digests || !sizes || !off))) return PBS_ERR_INVALID;
        for (size_t t = 0; t < k; ++t)
            if (off[t] > off[t + 1]) return PBS_ERR_INVALID;
        if (k && !blobs && off[k] != off[0]) return PBS_ERR_INVALID;
        if (finished) return PBS_BACKUP_E_FINISHED;
        auto it = writers.find(wid);
        if (it == writers.end()) return PBS_BACKUP_E_NO_WRITER;
        if (k == 0) return PBS_OK;
        Writer& w = it->second;
        pbs_backup_timing tm;
        std::memset(&tm, 0, sizeof(tm));
        tm.blobs = k;
        pre.assign(k, 0);
        kinds.assign(k, PBS_BLOB_KIND_NONE);
        status.assign(k, 0);
        crc.assign(k, 0);
        lens.assign(k, 0);
        for (auto* v : {&ins, &action, &dup, &reg}) v->assign(k, 0);
        comp.assign(k, 0);
        for (size_t t = 0; t < k; ++t) {
            const uint64_t len = off[t + 1] - off[t];
            status[t] = pre[t] = upload_pre(sizes[t], encoded_sizes ? encoded_sizes + t : nullptr, len);
            if (!pre[t]) lens[t] = (uint32_t)len;
        }
        int rc = e.verdicts(blobs, off, digests, sizes, k, pre.data(), kinds.data(), status.data(), crc.data(), &tm);
        if (rc != PBS_OK) return rc;
        for (size_t t = 0; t < k; ++t)
            if (status[t] == PBS_BLOB_ST_NO_CONFIG) status[t] = PBS_BLOB_ST_OK;  // accepted after from_raw
        double ims = 0;
        rc = e.insert_batch(digests, status.data(), kinds.data(), lens.data(), sizes, k, w.fixed, w.chunk_size, w.small,
                            ins.data(), action.data(), dup.data(), comp.data(), reg.data(), &ims);
        if (rc != PBS_OK) return rc;
        tm.insert_ms = ims;
        for (size_t t = 0; t < k; ++t) {
            if (w.fixed && ins_ok(ins[t]) && sizes[t] < w.chunk_size) w.small += 1;
            if (reg[t] == PBS_BACKUP_REG_OK) {
                w.stat.count += 1;
                w.stat.size += sizes[t];
                w.stat.compressed_size += comp[t];
                w.stat.duplicates += dup[t];
            } else if (first_failed && *first_failed == PBS_BACKUP_NONE) {
                *first_failed = t;
            }
        }
        if (status_out) std::memcpy(status_out, status.data(), k);
        if (crc_out) std::memcpy(crc_out, crc.data(), 4 * k);
        if (ins_out) std::memcpy(ins_out, ins.data(), k);
        if (action_out) std::memcpy(action_out, action.data(), k);
        if (dup_out) std::memcpy(dup_out, dup.data(), k);
        if (comp_out) std::memcpy(comp_out, comp.data(), 4 * k);
        if (reg_out) std::memcpy(reg_out, reg.data(), k);
        tm.total_ms = ms_since(t0);
        if (timing) *timing = tm;
        return PBS_OK;
    }

    int append(bool fixed, uint32_t wid, const uint8_t* digests, const uint64_t* offsets, size_t n, size_t* n_done,
               int* err, double* ms) {
        const Clock::time_point t0 = Clock::now();
        if (n_done) *n_done = 0;
        if (err) *err = PBS_BACKUP_E_NONE;
        if (ms) *ms = 0;
        if (!n_done || !err || n >= kGcMaxEntries || (n && (!digests || !offsets))) return PBS_ERR_INVALID;
        if (finished) return PBS_BACKUP_E_FINISHED;
        Writer* w = writer(wid, fixed);
        if (!w) return PBS_BACKUP_E_NO_WRITER;
        if (n == 0) return PBS_OK;
        tmp64.assign(n, 0);
        size_t done = 0;
        int code = PBS_BACKUP_E_NONE;
        const int rc = fixed ? e.append_fixed(digests, offsets, n, w->size, w->chunk_size, w->index_length, &done, &code,
                                              tmp64.data())
                             : e.append_dynamic(digests, offsets, n, w->offset, &done, &code, tmp64.data());
        if (rc != PBS_OK) return rc;
        if (done > n || (done < n) != (code != PBS_BACKUP_E_NONE)) return PBS_ERR_HIP;  // (never)
        if (fixed) {
            for (size_t i = 0; i < done; ++i) {
                if (tmp64[i] >= w->index_length) return PBS_ERR_HIP;  // (never)
                std::memcpy(&w->digests[32 * (size_t)tmp64[i]], digests + 32 * i, 32);
            }
        } else if (done) {
            w->ends.insert(w->ends.end(), tmp64.begin(), tmp64.begin() + done);
            w->digests.insert(w->digests.end(), digests, digests + 32 * done);
            w->offset = tmp64[done - 1];
        }
        w->chunk_count += done;
        *n_done = done;
        *err = code;
        if (ms) *ms = e.last_ms >= 0 ? e.last_ms : ms_since(t0);
        return PBS_OK;
    }

    int close(bool fixed, uint32_t wid, uint64_t chunk_count, uint64_t size, const uint8_t* csum, uint8_t* image_out,
              size_t cap, int* result, pbs_backup_writer_stat* stat) {
        if (stat) std::memset(stat, 0, sizeof(*stat));
        if (!result || !csum) return PBS_ERR_INVALID;
        *result = PBS_BACKUP_E_NONE;
        if (finished) return PBS_BACKUP_E_FINISHED;
        Writer* w = writer(wid, fixed);
        if (!w) {
            *result = PBS_BACKUP_E_NO_WRITER;
            return PBS_OK;
        }
        const size_t entries = fixed ? (size_t)w->index_length : w->ends.size();
        const size_t need = fixed ? pbs_fidx_size(entries) : pbs_didx_size(entries);
        if (image_out && cap < need) return PBS_ERR_CAPACITY;
        std::vector<uint8_t> image(need);
        uint8_t expect[32];
        const int brc = fixed ? pbs_fidx_build(w->digests.data(), w->size, w->chunk_size, w->uuid, w->ctime, image.data(),
                                               need, expect)
                              : pbs_didx_build(w->ends.data(), w->digests.data(), entries, w->uuid, w->ctime, image.data(),
                                               need, expect);
        if (brc != PBS_OK) return brc;
        const Writer data = std::move(*w);
        writers.erase(wid);  // (removed before the checks, :442 / :504)
        if (data.chunk_count != chunk_count) *result = PBS_BACKUP_E_CHUNK_COUNT;
        else if (!fixed && data.offset != size) *result = PBS_BACKUP_E_SIZE;
        else if (fixed && !data.incremental && chunk_count != data.index_length) *result = PBS_BACKUP_E_EXPECTED_COUNT;
        else if (fixed && !data.incremental && size != data.size) *result = PBS_BACKUP_E_SIZE;
        else if (std::memcmp(csum, expect, 32) != 0) *result = PBS_BACKUP_E_CSUM;
        if (*result != PBS_BACKUP_E_NONE) return PBS_OK;
        if (image_out) std::memcpy(image_out, image.data(), need);
        if (stat) writer_stat(data.stat, size, chunk_count, stat);
        file_counter += 1;
        backup_size += size;
        backup_stat.add(data.stat);
        return PBS_OK;
    }

    // add_blob (:566-591): DataBlob::load_from_reader = from_raw + verify_crc
    int add_blob(const uint8_t* raw, size_t len, uint8_t* status_out) {
        if (!status_out || (len && !raw)) return PBS_ERR_INVALID;
        *status_out = PBS_BLOB_ST_TOO_SMALL;
        if (finished) return PBS_BACKUP_E_FINISHED;
        uint8_t kind;
        uint8_t st = verify::host_blob_load(raw, len, &kind);
        if (st == PBS_BLOB_ST_NO_CONFIG) st = PBS_BLOB_ST_OK;  // (nothing is decoded here)
        *status_out = st;
        if (st != PBS_BLOB_ST_OK) return PBS_OK;
        file_counter += 1;
        backup_size += len;
        backup_stat.size += len;
        return PBS_OK;
    }
};

}  // namespace backup
}  // namespace pbs

// The C ABI over a handle type H with a member `s` (a Session) and a scope guard G(h) that is
// `ok` when the call may run (the device side sets the handle's device with it).  begin, end
// and release are written out by each side.
#define PBS_BACKUP_CALL(H, G, expr)                    \
    if (!pbs::Live<H>::alive(h)) return PBS_ERR_INVALID; \
    G guard(h);                                        \
    if (!guard.ok) return PBS_ERR_NO_DEVICE;           \
    try {                                              \
        return h->s.expr;                              \
    } catch (const std::bad_alloc&) {                  \
        return PBS_ERR_NOMEM;                          \
    }

#define PBS_BACKUP_DEFINE_ABI(SFX, H, G)                                                                                  \
    extern "C" size_t pbs_backup_count##SFX(H* h) { return pbs::Live<H>::alive(h) ? h->s.e.count() : 0; }          \
    extern "C" uint32_t pbs_backup_table_log2##SFX(H* h) { return pbs::Live<H>::alive(h) ? h->s.e.log2() : 0; }    \
    extern "C" int pbs_backup_listing##SFX(H* h, uint8_t* digests_out, uint8_t* present_out, uint64_t* size_out,           \
                                           uint8_t* kind_out, uint8_t* known_out, uint32_t* known_size_out, size_t cap,    \
                                           size_t* count) {                                                                \
        if (count) *count = 0;                                                                                             \
        PBS_BACKUP_CALL(H, G, listing(digests_out, present_out, size_out, kind_out, known_out, known_size_out, cap, count)) \
    }                                                                                                                      \
    extern "C" int pbs_backup_lookup##SFX(H* h, const uint8_t* digest, uint32_t* size) {                                   \
        PBS_BACKUP_CALL(H, G, lookup(digest, size))                                                                        \
    }                                                                                                                      \
    extern "C" int pbs_backup_stats##SFX(H* h, pbs_backup_stat* stat) {                                                    \
        if (!pbs::Live<H>::alive(h) || !stat) return PBS_ERR_INVALID;                                              \
        h->s.stats(stat);                                                                                                  \
        return PBS_OK;                                                                                                     \
    }                                                                                                                      \
    extern "C" int pbs_backup_finish##SFX(H* h, pbs_backup_stat* stat) { PBS_BACKUP_CALL(H, G, finish(stat)) }             \
    extern "C" int pbs_backup_register_previous##SFX(H* h, const uint8_t* digests, const uint32_t* sizes, size_t n,        \
                                                     double* ms) {                                                         \
        PBS_BACKUP_CALL(H, G, register_previous(digests, sizes, n, ms))                                                    \
    }                                                                                                                      \
    extern "C" int pbs_backup_register_index_image##SFX(H* h, const uint8_t* image, size_t len, size_t* n_entries,         \
                                                        double* ms) {                                                      \
        PBS_BACKUP_CALL(H, G, register_index_image(image, len, n_entries, ms))                                             \
    }                                                                                                                      \
    extern "C" int pbs_backup_upload##SFX(H* h, uint32_t wid, const uint8_t* digests, const uint32_t* sizes,               \
                                          const uint32_t* encoded_sizes, const uint8_t* blobs, const uint64_t* blob_offsets, \
                                          size_t k, uint8_t* status, uint32_t* crc_out, uint8_t* ins, uint8_t* action,     \
                                          uint8_t* is_duplicate, uint32_t* compressed_size, uint8_t* reg,                  \
                                          uint64_t* first_failed, pbs_backup_timing* timing) {                             \
        PBS_BACKUP_CALL(H, G, upload(wid, digests, sizes, encoded_sizes, blobs, blob_offsets, k, status, crc_out, ins,     \
                                     action, is_duplicate, compressed_size, reg, first_failed, timing))                    \
    }                                                                                                                      \
    extern "C" int pbs_backup_create_dynamic##SFX(H* h, const uint8_t* uuid, int64_t ctime, uint32_t* wid) {               \
        PBS_BACKUP_CALL(H, G, create_dynamic(uuid, ctime, wid))                                                            \
    }                                                                                                                      \
    extern "C" int pbs_backup_create_fixed##SFX(H* h, uint64_t size, uint64_t chunk_size, const uint8_t* uuid,             \
                                                int64_t ctime, const uint8_t* reuse_image, size_t reuse_len,               \
                                                const uint8_t* reuse_csum, uint32_t* wid) {                                \
        PBS_BACKUP_CALL(H, G, create_fixed(size, chunk_size, uuid, ctime, reuse_image, reuse_len, reuse_csum, wid))        \
    }                                                                                                                      \
    extern "C" int pbs_backup_dynamic_append##SFX(H* h, uint32_t wid, const uint8_t* digests, const uint64_t* offsets,     \
                                                  size_t n, size_t* n_done, int* err, double* ms) {                        \
        PBS_BACKUP_CALL(H, G, append(false, wid, digests, offsets, n, n_done, err, ms))                                    \
    }                                                                                                                      \
    extern "C" int pbs_backup_fixed_append##SFX(H* h, uint32_t wid, const uint8_t* digests, const uint64_t* offsets,       \
                                                size_t n, size_t* n_done, int* err, double* ms) {                          \
        PBS_BACKUP_CALL(H, G, append(true, wid, digests, offsets, n, n_done, err, ms))                                     \
    }                                                                                                                      \
    extern "C" int pbs_backup_dynamic_close##SFX(H* h, uint32_t wid, uint64_t chunk_count, uint64_t size,                  \
                                                 const uint8_t* csum, uint8_t* image_out, size_t cap, int* result,         \
                                                 pbs_backup_writer_stat* stat) {                                           \
        PBS_BACKUP_CALL(H, G, close(false, wid, chunk_count, size, csum, image_out, cap, result, stat))                    \
    }                                                                                                                      \
    extern "C" int pbs_backup_fixed_close##SFX(H* h, uint32_t wid, uint64_t chunk_count, uint64_t size,                    \
                                               const uint8_t* csum, uint8_t* image_out, size_t cap, int* result,           \
                                               pbs_backup_writer_stat* stat) {                                             \
        PBS_BACKUP_CALL(H, G, close(true, wid, chunk_count, size, csum, image_out, cap, result, stat))                     \
    }                                                                                                                      \
    extern "C" int pbs_backup_add_blob##SFX(H* h, const uint8_t* raw, size_t len, uint8_t* status) {                       \
        PBS_BACKUP_CALL(H, G, add_blob(raw, len, status))                                                                  \
    }
