// Host mirror of the verify job (include/pbs_verify.h, pbs_verify_*_host) and pbs_verify_blob_host:
// the same calls by a sort of the store's digests and a binary search per index entry, a blob at
// a time.  Plain C++: no device code, so the sanitizer program of tests/cpp/verify_sanitize.cpp
// builds it with the host compiler next to pbs_inflate_host.cpp and pbs_didx.cpp.  A blob is
// read as pbs_blob_decode_host reads it without a config (from_raw's checks, the CRC), restated
// here because that call lives in a device translation unit; the frames go through the host
// inflater and the digests through pbs_sha256.  It is what the GPU is compared against, and
// verify where there is no device.
#include <stdint.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <exception>
#include <new>
#include <vector>

#include "gc_common.h"
#include "live_handles.h"
#include "pbs_blob.h"
#include "pbs_chunker.h"
#include "pbs_digest.h"
#include "pbs_verify.h"
#include "verify_common.h"

using namespace pbs::gc;
using namespace pbs::verify;

struct pbs_verify_host {
    std::vector<uint8_t> digests, state;
    struct Ent {
        uint64_t key;  // the digest's first 8 bytes, big-endian
        uint32_t pos;
    };
    std::vector<Ent> order;      // store positions in (key, position) order
    std::vector<uint32_t> pos;   // of the open index: entry -> lowest store position, kAbsent
    IndexRun run;
};

namespace {

constexpr uint32_t kAbsent = 0xFFFFFFFFu;

using Clock = std::chrono::steady_clock;
inline double ms_since(Clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
}

inline uint64_t be64(const uint8_t* p) {
    uint64_t v = 0;
    for (int i = 0; i < 8; ++i) v = (v << 8) | p[i];
    return v;
}

using Handles = pbs::Live<pbs_verify_host>;

// the lowest store position carrying the digest `d`
inline uint32_t lowest(const pbs_verify_host& h, const uint8_t* d) {
    const uint64_t key = be64(d);
    auto it = std::lower_bound(h.order.begin(), h.order.end(), key,
                               [](const pbs_verify_host::Ent& e, uint64_t k) { return e.key < k; });
    for (; it != h.order.end() && it->key == key; ++it)
        if (std::memcmp(h.digests.data() + 32 * (size_t)it->pos, d, 32) == 0) return it->pos;
    return kAbsent;
}

// CRC-32/ISO-HDLC (crc32fast), bytewise: the mirror is not a fast path
uint32_t crc32_bytes(const uint8_t* p, size_t n) {
    static const std::vector<uint32_t> table = [] {
        std::vector<uint32_t> t(256);
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1)));
            t[i] = c;
        }
        return t;
    }();
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) c = table[(c ^ p[i]) & 0xFF] ^ (c >> 8);
    return ~c;
}

const uint8_t kMagics[4][8] = {{66, 171, 56, 7, 190, 131, 112, 161},
                               {49, 185, 88, 66, 111, 182, 163, 127},
                               {123, 103, 133, 190, 34, 45, 76, 240},
                               {230, 89, 27, 191, 11, 191, 216, 11}};

// DataBlob::load_from_reader without a config: from_raw (data_blob.rs:268-290) and verify_crc.
// kind, header length, and the first failing check (OK; an encrypted blob that passes is
// NO_CONFIG, as pbs_blob_decode_host says it).  crc_out != NULL: the payload's CRC goes there
// and the stored one is not judged (the backup session's upload, upload_chunk.rs:77-85)
uint8_t load(const uint8_t* p, size_t len, uint8_t* kind, size_t* hdr, uint32_t* crc_out = nullptr) {
    *kind = PBS_BLOB_KIND_NONE;
    *hdr = 0;
    if (len < PBS_BLOB_HEADER_SIZE) return PBS_BLOB_ST_TOO_SMALL;
    for (int k = 0; k < 4; ++k)
        if (std::memcmp(p, kMagics[k], 8) == 0) *kind = (uint8_t)k;
    if (*kind == PBS_BLOB_KIND_NONE) return PBS_BLOB_ST_BAD_MAGIC;
    const size_t h = *kind >= 2 ? PBS_BLOB_ENC_HEADER_SIZE : PBS_BLOB_HEADER_SIZE;
    if (len < h) return PBS_BLOB_ST_TOO_SMALL;
    *hdr = h;
    const uint32_t stored = (uint32_t)p[8] | (uint32_t)p[9] << 8 | (uint32_t)p[10] << 16 | (uint32_t)p[11] << 24;
    const uint32_t crc = crc32_bytes(p + h, len - h);
    if (crc_out) *crc_out = crc;
    else if (stored != crc) return PBS_BLOB_ST_BAD_CRC;
    return *kind >= 2 ? PBS_BLOB_ST_NO_CONFIG : PBS_BLOB_ST_OK;
}

// pbs_blob_decode_inflate_device's verdict for one blob with no config, the digest `want` and a
// slot of exactly `size` bytes (sizes_exact): load, decode_all, verify_digest, then the length
uint8_t decode_one(const uint8_t* p, size_t len, const uint8_t* want, uint64_t size, uint8_t* kind,
                   uint32_t* crc_out = nullptr) {
    size_t hdr = 0;
    const uint8_t st = load(p, len, kind, &hdr, crc_out);
    if (st != PBS_BLOB_ST_OK) return st;
    const uint8_t* pay = p + hdr;
    const size_t plen = len - hdr;
    std::vector<uint8_t> slot;
    const uint8_t* content = pay;
    uint64_t clen = plen;
    if (*kind == PBS_BLOB_KIND_COMPRESSED) {
        if (size > (uint64_t)SIZE_MAX - 1) return PBS_BLOB_ST_BAD_DIGEST;
        slot.resize((size_t)size + 1);  // (+1: never an empty buffer)
        size_t olen = 0;
        uint8_t zst = PBS_ZST_OK;
        if (pbs_zstd_inflate_host(pay, plen, slot.data(), (size_t)size, &olen, &zst) != PBS_OK) return PBS_BLOB_ST_BAD_FRAME;
        if (zst == PBS_ZST_BAD_FRAME) return PBS_BLOB_ST_BAD_FRAME;
        if (zst == PBS_ZST_UNSUPPORTED) return PBS_BLOB_ST_UNSUPPORTED_FRAME;
        // content that overflows its slot: a message of another length cannot have the digest
        if (zst == PBS_ZST_TOO_LARGE) return PBS_BLOB_ST_BAD_DIGEST;
        content = slot.data();
        clen = olen;
    } else if (plen > size) {
        return PBS_BLOB_ST_BAD_DIGEST;
    }
    uint8_t d[32];
    pbs_sha256(content, (size_t)clen, d);
    if (std::memcmp(d, want, 32) != 0) return PBS_BLOB_ST_BAD_DIGEST;
    return clen == size ? PBS_BLOB_ST_OK : PBS_BLOB_ST_BAD_SIZE;
}

int submit(pbs_verify_host* h, const uint8_t* blobs, const uint64_t* blob_offsets, const uint8_t* load_failed,
           size_t k, uint8_t* kinds, uint8_t* status, pbs_verify_timing* timing) {
    const Clock::time_point t0 = Clock::now();
    if (timing) std::memset(timing, 0, sizeof(*timing));
    if (!Handles::alive(h) || !submit_args_valid(h->run, blobs, blob_offsets, k)) return PBS_ERR_INVALID;
    IndexRun& run = h->run;
    pbs_verify_timing tm;
    std::memset(&tm, 0, sizeof(tm));
    tm.blobs = k;
    for (size_t t = 0; t < k; ++t) {
        const size_t item = run.done;
        const uint64_t len = blob_offsets[t + 1] - blob_offsets[t];
        uint8_t kind = PBS_BLOB_KIND_NONE, st = PBS_VERIFY_ST_LOAD_FAILED;
        if (!load_failed || !load_failed[t]) {
            try {
                st = decode_one(len ? blobs + blob_offsets[t] : kMagics[0], (size_t)len, &run.todo_digests[32 * item],
                                run.todo_sizes[item], &kind);
            } catch (const std::exception&) {  // (no memory for a slot of the index's size: the items before stay consumed)
                return PBS_ERR_NOMEM;
            }
            if (st == PBS_BLOB_ST_NO_CONFIG) st = PBS_BLOB_ST_OK;
            tm.decoded += 1;
            const bool enc = kind == PBS_BLOB_KIND_ENCRYPTED || kind == PBS_BLOB_KIND_ENCR_COMPR;
            tm.encrypted += enc;
            if (!enc) tm.scratch_bytes += run.todo_sizes[item];
        }
        h->state[run.todo_store[item]] = account(run, kind, st, len);
        if (kinds) kinds[t] = kind;
        if (status) status[t] = st;
    }
    tm.decode_ms = tm.total_ms = ms_since(t0);
    if (timing) *timing = tm;
    return PBS_OK;
}

int finish(pbs_verify_host* h, pbs_verify_result* res, uint32_t* corrupt_store, size_t ccap, size_t* n_corrupt,
           uint32_t* missing_pos, size_t mcap, size_t* n_missing) {
    if (n_corrupt) *n_corrupt = 0;
    if (n_missing) *n_missing = 0;
    if (!Handles::alive(h) || !finish_args_valid(h->run, corrupt_store, ccap, missing_pos, mcap)) return PBS_ERR_INVALID;
    uint64_t failing = 0;
    for (size_t i = 0; i < h->run.n; ++i) {
        const uint32_t j = h->pos[i];
        failing += j == kAbsent || h->state[j] == PBS_VERIFY_CORRUPT;
    }
    close_run(h->run, failing, res, corrupt_store, ccap, n_corrupt, missing_pos, mcap, n_missing);
    return PBS_OK;
}

int plan(pbs_verify_host* h, const uint8_t* digests, const uint64_t* sizes, size_t n, int index_mode,
         uint32_t* todo_store, uint32_t* todo_entry, size_t cap, size_t* n_todo, double* plan_ms) {
    const Clock::time_point t0 = Clock::now();
    if (n_todo) *n_todo = 0;
    if (plan_ms) *plan_ms = 0;
    if (!Handles::alive(h) || h->run.open ||
        !plan_args_valid(digests, sizes, n, index_mode, todo_store, todo_entry, cap, n_todo))
        return PBS_ERR_INVALID;
    IndexRun& run = h->run;
    try {
        run.clear();
        const size_t m = h->state.size();
        std::vector<uint32_t> first(m, kAbsent);
        h->pos.assign(n, kAbsent);
        for (size_t i = 0; i < n; ++i) {
            const uint32_t j = lowest(*h, digests + 32 * i);
            h->pos[i] = j;
            if (j == kAbsent) {
                run.missing.push_back((uint32_t)i);
                continue;
            }
            if (first[j] == kAbsent) first[j] = (uint32_t)i;
            run.res.skipped_verified += h->state[j] == PBS_VERIFY_VERIFIED;
            run.res.skipped_corrupt += h->state[j] == PBS_VERIFY_CORRUPT;
        }
        for (size_t j = 0; j < m; ++j)
            if (first[j] != kAbsent && h->state[j] == PBS_VERIFY_UNKNOWN) {
                run.todo_store.push_back((uint32_t)j);
                run.todo_entry.push_back(first[j]);
            }
        run.gather(digests, sizes);
    } catch (const std::bad_alloc&) {
        run.clear();
        return PBS_ERR_NOMEM;
    }
    run.open = true;
    run.mode = index_mode;
    run.n = n;
    run.res.entries = n;
    run.res.missing = run.missing.size();
    const size_t k = run.todo_store.size();
    for (size_t t = 0; t < k && t < cap; ++t) {
        todo_store[t] = run.todo_store[t];
        todo_entry[t] = run.todo_entry[t];
    }
    *n_todo = k;
    if (plan_ms) *plan_ms = ms_since(t0);
    return PBS_OK;
}

}  // namespace

uint8_t pbs::verify::host_blob_verdict(const uint8_t* p, size_t len, const uint8_t* want, uint64_t size, uint8_t* kind) {
    return decode_one(len ? p : kMagics[0], len, want, size, kind);
}

uint8_t pbs::verify::host_blob_verdict_upload(const uint8_t* p, size_t len, const uint8_t* want, uint64_t size,
                                              uint8_t* kind, uint32_t* crc) {
    *crc = 0;
    return decode_one(len ? p : kMagics[0], len, want, size, kind, crc);
}

uint8_t pbs::verify::host_blob_load(const uint8_t* p, size_t len, uint8_t* kind) {
    size_t hdr = 0;
    return load(len ? p : kMagics[0], len, kind, &hdr);
}

extern "C" int pbs_verify_begin_host(const uint8_t* store_digests, size_t m, pbs_verify_host** out, double* build_ms) {
    const Clock::time_point t0 = Clock::now();
    if (out) *out = nullptr;
    if (build_ms) *build_ms = 0;
    if (!out || (m && !store_digests) || m >= kGcMaxEntries) return PBS_ERR_INVALID;
    pbs_verify_host* h = new (std::nothrow) pbs_verify_host;
    if (!h) return PBS_ERR_NOMEM;
    try {
        if (m) h->digests.assign(store_digests, store_digests + 32 * m);
        h->state.assign(m, PBS_VERIFY_UNKNOWN);
        h->order.resize(m);
        for (size_t j = 0; j < m; ++j) h->order[j] = {be64(store_digests + 32 * j), (uint32_t)j};
        std::sort(h->order.begin(), h->order.end(), [](const pbs_verify_host::Ent& a, const pbs_verify_host::Ent& b) {
            return a.key != b.key ? a.key < b.key : a.pos < b.pos;
        });
        h->run.clear();
    } catch (const std::bad_alloc&) {
        delete h;
        return PBS_ERR_NOMEM;
    }
    Handles::add(h);
    *out = h;
    if (build_ms) *build_ms = ms_since(t0);
    return PBS_OK;
}

extern "C" int pbs_verify_states_host(pbs_verify_host* h, uint8_t* states_host, size_t m) {
    if (!Handles::alive(h) || m != h->state.size() || (m && !states_host)) return PBS_ERR_INVALID;
    if (m) std::memcpy(states_host, h->state.data(), m);
    return PBS_OK;
}

extern "C" void pbs_verify_end_host(pbs_verify_host* h) {
    if (h && Handles::remove(h)) delete h;
}

extern "C" int pbs_verify_plan_host(pbs_verify_host* h, const uint8_t* digests, const uint64_t* sizes, size_t n,
                                    int index_mode, uint32_t* todo_store, uint32_t* todo_entry, size_t cap,
                                    size_t* n_todo, double* plan_ms) {
    return plan(h, digests, sizes, n, index_mode, todo_store, todo_entry, cap, n_todo, plan_ms);
}

extern "C" int pbs_verify_abort_index_host(pbs_verify_host* h) {
    if (!Handles::alive(h)) return PBS_ERR_INVALID;
    h->run.clear();
    return PBS_OK;
}

extern "C" int pbs_verify_submit_host(pbs_verify_host* h, const uint8_t* blobs, const uint64_t* blob_offsets,
                                      const uint8_t* load_failed, size_t k, uint8_t* kinds, uint8_t* status,
                                      pbs_verify_timing* timing) {
    return submit(h, blobs, blob_offsets, load_failed, k, kinds, status, timing);
}

extern "C" int pbs_verify_finish_host(pbs_verify_host* h, pbs_verify_result* res, uint32_t* corrupt_store, size_t ccap,
                                      size_t* n_corrupt, uint32_t* missing_pos, size_t mcap, size_t* n_missing) {
    return finish(h, res, corrupt_store, ccap, n_corrupt, missing_pos, mcap, n_missing);
}

extern "C" int pbs_verify_index_host(pbs_verify_host* h, const uint8_t* image, size_t len, int index_mode,
                                     const uint64_t* info_size, const uint8_t* info_csum, const uint8_t* store_blobs,
                                     const uint64_t* store_offsets, size_t budget_bytes, pbs_verify_result* res,
                                     uint32_t* corrupt_store, size_t ccap, size_t* n_corrupt, uint32_t* missing_pos,
                                     size_t mcap, size_t* n_missing) {
    if (res) std::memset(res, 0, sizeof(*res));
    if (n_corrupt) *n_corrupt = 0;
    if (n_missing) *n_missing = 0;
    if (!Handles::alive(h) || h->run.open || !mode_valid(index_mode) || (ccap && !corrupt_store) || (mcap && !missing_pos))
        return PBS_ERR_INVALID;
    const size_t m = h->state.size();
    if (m && !store_offsets) return PBS_ERR_INVALID;
    for (size_t j = 0; j < m; ++j)
        if (store_offsets[j] > store_offsets[j + 1]) return PBS_ERR_INVALID;
    if (m && store_offsets[m] > store_offsets[0] && !store_blobs) return PBS_ERR_INVALID;
    IndexLayout lo;
    int rc = index_layout(image, len, &lo);
    if (rc != PBS_OK) return rc;
    const uint32_t chk = index_check(image, lo, info_size, info_csum);
    if (chk != PBS_VERIFY_INDEX_OK) {
        if (res) {
            res->entries = lo.n;
            res->index_check = chk;
        }
        return PBS_OK;
    }
    std::vector<uint8_t> digests, enc;
    std::vector<uint64_t> sizes, offs;
    size_t k = 0;
    try {
        index_entries(image, lo, digests, sizes);
        rc = plan(h, digests.data(), sizes.data(), lo.n, index_mode, nullptr, nullptr, 0, &k, nullptr);
        if (rc != PBS_OK) return rc;
        const IndexRun& run = h->run;
        auto blob_len = [&](size_t t) { return store_offsets[run.todo_store[t] + 1] - store_offsets[run.todo_store[t]]; };
        enc.resize(k);
        for (size_t t = 0; t < k; ++t) {
            const uint8_t* p = blob_len(t) ? store_blobs + store_offsets[run.todo_store[t]] : kMagics[0];
            enc[t] = blob_len(t) >= PBS_BLOB_HEADER_SIZE &&
                     (std::memcmp(p, kMagics[2], 8) == 0 || std::memcmp(p, kMagics[3], 8) == 0);
        }
        std::vector<uint8_t> packed;
        for (size_t t0 = 0; t0 < k;) {
            const size_t t1 = batch_end(run, t0, budget_bytes, enc.data(), blob_len);
            packed.clear();
            offs.assign(1, 0);
            for (size_t t = t0; t < t1; ++t) {
                if (blob_len(t)) {
                    const uint8_t* p = store_blobs + store_offsets[run.todo_store[t]];
                    packed.insert(packed.end(), p, p + blob_len(t));
                }
                offs.push_back(packed.size());
            }
            packed.push_back(0);  // (never an empty buffer)
            rc = submit(h, packed.data(), offs.data(), nullptr, t1 - t0, nullptr, nullptr, nullptr);
            if (rc != PBS_OK) break;
            t0 = t1;
        }
    } catch (const std::bad_alloc&) {
        rc = PBS_ERR_NOMEM;
    }
    if (rc != PBS_OK) {
        h->run.clear();  // (the states of the blobs already submitted stay: they were verified)
        return rc;
    }
    return finish(h, res, corrupt_store, ccap, n_corrupt, missing_pos, mcap, n_missing);
}

extern "C" int pbs_verify_blob_host(const uint8_t* raw, size_t len, uint64_t info_size, const uint8_t info_csum[32],
                                    int* result) {
    if (!result || !info_csum || (len && !raw)) return PBS_ERR_INVALID;
    static const uint8_t none = 0;
    if (!raw) raw = &none;
    *result = PBS_VERIFY_BLOB_OK;
    if ((uint64_t)len != info_size) {
        *result = PBS_VERIFY_BLOB_WRONG_SIZE;
        return PBS_OK;
    }
    uint8_t c[32];
    pbs_sha256(raw, len, c);
    if (std::memcmp(c, info_csum, 32) != 0) {
        *result = PBS_VERIFY_BLOB_WRONG_CSUM;
        return PBS_OK;
    }
    uint8_t kind = PBS_BLOB_KIND_NONE;
    size_t hdr = 0;
    const uint8_t st = load(raw, len, &kind, &hdr);
    if (st != PBS_BLOB_ST_OK && st != PBS_BLOB_ST_NO_CONFIG) {
        *result = PBS_VERIFY_BLOB_LOAD;
        return PBS_OK;
    }
    if (kind != PBS_BLOB_KIND_COMPRESSED) return PBS_OK;  // encrypted: Ok; uncompressed: decode copies
    // decode(None, None) of a compressed blob: decode_all, to whatever length it has (the frame
    // need not say; MAX_BLOB_SIZE, 128 MiB, bounds what a blob holds)
    const size_t kMax = (size_t)128 << 20;
    std::vector<uint8_t> out;
    for (size_t cap = std::max<size_t>(65536, 8 * (len - hdr));; cap *= 2) {
        cap = std::min(cap, kMax);
        try {
            out.resize(cap);
        } catch (const std::bad_alloc&) {
            return PBS_ERR_NOMEM;
        }
        size_t olen = 0;
        uint8_t zst = PBS_ZST_OK;
        if (pbs_zstd_inflate_host(raw + hdr, len - hdr, out.data(), cap, &olen, &zst) != PBS_OK) zst = PBS_ZST_BAD_FRAME;
        if (zst == PBS_ZST_TOO_LARGE && cap < kMax) continue;
        if (zst != PBS_ZST_OK) *result = PBS_VERIFY_BLOB_DECODE;
        return PBS_OK;
    }
}
