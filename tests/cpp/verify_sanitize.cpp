// The host mirror of the verify job (proxmox-backup_amd/csrc/pbs_verify_host.cpp, with the host
// inflater and pbs_sha256) under ASan + UBSan (make -C proxmox-backup_amd/csrc sanitize-verify):
// every buffer a heap block of exactly its size -- a small store of three blob kinds with a
// known answer, by hand and through the whole-index call at three budgets, verify_blob, then the
// error cases: plan during plan, oversubmit, early finish, a bad mode, descending offsets,
// truncated and ragged index images, an empty store, calls on a handle that has ended.
#include <cstdio>
#include <cstring>
#include <vector>

#include "pbs_blob.h"
#include "pbs_chunker.h"
#include "pbs_digest.h"
#include "pbs_verify.h"

static int g_fail = 0;
#define CHECK(x)                                                      \
    do {                                                              \
        if (!(x)) {                                                   \
            std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #x); \
            ++g_fail;                                                 \
        }                                                             \
    } while (0)

typedef std::vector<uint8_t> Bytes;

static void put_le64(uint8_t* p, uint64_t v) {
    for (int i = 0; i < 8; ++i) p[i] = (uint8_t)(v >> (8 * i));
}

static uint32_t crc32(const uint8_t* p, size_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1)));
    }
    return ~c;
}

static const uint8_t kMagic[4][8] = {{66, 171, 56, 7, 190, 131, 112, 161},
                                     {49, 185, 88, 66, 111, 182, 163, 127},
                                     {123, 103, 133, 190, 34, 45, 76, 240},
                                     {230, 89, 27, 191, 11, 191, 216, 11}};

// magic || crc || [iv, tag] || payload
static Bytes blob(int kind, const Bytes& payload) {
    Bytes b(kMagic[kind], kMagic[kind] + 8);
    const uint32_t c = crc32(payload.data(), payload.size());
    for (int i = 0; i < 4; ++i) b.push_back((uint8_t)(c >> (8 * i)));
    if (kind >= 2) b.insert(b.end(), 32, 0x5A);
    b.insert(b.end(), payload.begin(), payload.end());
    return b;
}

// a zstd frame of one raw block (single segment, 1-byte content size): data.size() < 256
static Bytes raw_frame(const Bytes& data) {
    Bytes f = {0x28, 0xB5, 0x2F, 0xFD, 0x20, (uint8_t)data.size()};
    const uint32_t bh = ((uint32_t)data.size() << 3) | 1;
    f.push_back((uint8_t)bh);
    f.push_back((uint8_t)(bh >> 8));
    f.push_back((uint8_t)(bh >> 16));
    f.insert(f.end(), data.begin(), data.end());
    return f;
}

static Bytes chunk(unsigned k, size_t n) {
    Bytes c(n);
    for (size_t i = 0; i < n; ++i) c[i] = (uint8_t)(k * 31 + i * 7);
    return c;
}

static Bytes sha(const Bytes& d) {
    static const uint8_t none = 0;
    Bytes o(32);
    pbs_sha256(d.empty() ? &none : d.data(), d.size(), o.data());
    return o;
}

struct Store {
    Bytes digests, blobs;
    std::vector<uint64_t> off{0};
    void add(const Bytes& dig, const Bytes& b) {
        digests.insert(digests.end(), dig.begin(), dig.end());
        blobs.insert(blobs.end(), b.begin(), b.end());
        off.push_back(blobs.size());
    }
    size_t m() const { return off.size() - 1; }
};

// a .didx image of (digest, size) entries
static Bytes didx(const std::vector<Bytes>& digs, const std::vector<uint64_t>& sizes) {
    static const uint8_t magic[8] = {28, 145, 78, 165, 25, 186, 179, 205};
    Bytes img(4096 + 40 * digs.size(), 0);
    std::memcpy(img.data(), magic, 8);
    uint64_t end = 0;
    for (size_t i = 0; i < digs.size(); ++i) {
        end += sizes[i];
        put_le64(&img[4096 + 40 * i], end);
        std::memcpy(&img[4096 + 40 * i + 8], digs[i].data(), 32);
    }
    return img;
}

int main() {
    // the store: 0 good plain, 1 good compressed, 2 encrypted (any digest), 3 stale CRC, 4 a blob
    // under another chunk's name, 5 eleven bytes, 6 digest 0 again (garbage: never read), 7 empty chunk
    const Bytes c0 = chunk(0, 100), c1 = chunk(1, 200), c4 = chunk(4, 50), c7;
    Bytes d2 = chunk(2, 32), d3 = chunk(3, 32), d4 = chunk(40, 32), d5 = chunk(5, 32), absent = chunk(9, 32);
    Store s;
    s.add(sha(c0), blob(0, c0));
    s.add(sha(c1), blob(1, raw_frame(c1)));
    s.add(d2, blob(2, chunk(2, 77)));
    Bytes stale = blob(0, chunk(3, 60));
    stale.back() ^= 1;
    s.add(d3, stale);
    s.add(d4, blob(0, c4));
    const Bytes b0 = blob(0, c0);
    s.add(d5, Bytes(b0.begin(), b0.begin() + 11));
    s.add(sha(c0), Bytes(5, 0xEE));
    s.add(sha(c7), blob(0, c7));
    const size_t m = s.m();

    // the index: 1, 0, absent, 3, 0 (wrong size: the first one's decides), 2, 4, 5, 3, 7
    const std::vector<Bytes> digs = {sha(c1), sha(c0), absent, d3, sha(c0), d2, d4, d5, d3, sha(c7)};
    const std::vector<uint64_t> sizes = {200, 100, 10, 60, 101, 77, 50, 100, 60, 0};
    const size_t n = digs.size();
    Bytes flat;
    for (const Bytes& d : digs) flat.insert(flat.end(), d.begin(), d.end());

    pbs_verify_host* h = nullptr;
    double ms = 0;
    CHECK(pbs_verify_begin_host(s.digests.data(), m, &h, &ms) == PBS_OK && h);
    std::vector<uint32_t> ts(m), te(m);
    size_t nt = 0;
    CHECK(pbs_verify_plan_host(h, flat.data(), sizes.data(), n, PBS_VERIFY_MODE_NONE, ts.data(), te.data(), m, &nt,
                               &ms) == PBS_OK);
    const uint32_t want_ts[7] = {0, 1, 2, 3, 4, 5, 7}, want_te[7] = {1, 0, 5, 3, 6, 7, 9};
    CHECK(nt == 7 && std::memcmp(ts.data(), want_ts, 28) == 0 && std::memcmp(te.data(), want_te, 28) == 0);
    // error cases on an open plan: nothing may change it
    CHECK(pbs_verify_plan_host(h, flat.data(), sizes.data(), n, PBS_VERIFY_MODE_NONE, ts.data(), te.data(), m, &nt,
                               nullptr) == PBS_ERR_INVALID);
    CHECK(pbs_verify_finish_host(h, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr) == PBS_ERR_INVALID);
    {
        std::vector<uint64_t> eight(9, 0);
        CHECK(pbs_verify_submit_host(h, s.blobs.data(), eight.data(), nullptr, 8, nullptr, nullptr, nullptr) ==
              PBS_ERR_INVALID);
        const uint64_t down[2] = {5, 3};
        CHECK(pbs_verify_submit_host(h, s.blobs.data(), down, nullptr, 1, nullptr, nullptr, nullptr) == PBS_ERR_INVALID);
        CHECK(pbs_verify_submit_host(h, s.blobs.data(), nullptr, nullptr, 1, nullptr, nullptr, nullptr) == PBS_ERR_INVALID);
        CHECK(pbs_verify_index_host(h, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr,
                                    nullptr, 0, nullptr) == PBS_ERR_INVALID);
    }
    // submit: the first six store entries are contiguous in the stream; entry 5 as a load failure;
    // then entry 7 alone, each batch a heap block of its own
    {
        Bytes part(s.blobs.begin(), s.blobs.begin() + s.off[6]);
        std::vector<uint64_t> off(s.off.begin(), s.off.begin() + 7);
        std::vector<uint8_t> lf = {0, 0, 0, 0, 0, 1}, kinds(6), st(6);
        pbs_verify_timing tm;
        CHECK(pbs_verify_submit_host(h, part.data(), off.data(), lf.data(), 6, kinds.data(), st.data(), &tm) == PBS_OK);
        const uint8_t want_k[6] = {0, 1, 2, 0, 0, 255};
        const uint8_t want_s[6] = {0, 0, 0, PBS_BLOB_ST_BAD_CRC, PBS_BLOB_ST_BAD_DIGEST, PBS_VERIFY_ST_LOAD_FAILED};
        CHECK(std::memcmp(kinds.data(), want_k, 6) == 0 && std::memcmp(st.data(), want_s, 6) == 0);
        CHECK(tm.blobs == 6 && tm.decoded == 5 && tm.encrypted == 1 && tm.scratch_bytes == 100 + 200 + 60 + 50);
        Bytes last(s.blobs.begin() + s.off[7], s.blobs.begin() + s.off[8]);
        const uint64_t off1[2] = {0, last.size()};
        CHECK(pbs_verify_submit_host(h, last.data(), off1, nullptr, 1, kinds.data(), st.data(), nullptr) == PBS_OK);
        CHECK(kinds[0] == 0 && st[0] == PBS_BLOB_ST_OK);
        CHECK(pbs_verify_submit_host(h, last.data(), off1, nullptr, 1, nullptr, nullptr, nullptr) == PBS_ERR_INVALID);
    }
    pbs_verify_result r;
    std::vector<uint32_t> cs(3), mp(1);
    size_t nc = 0, nm = 0;
    CHECK(pbs_verify_finish_host(h, &r, cs.data(), 1, &nc, nullptr, 1, &nm) == PBS_ERR_INVALID);  // cap without list
    CHECK(pbs_verify_finish_host(h, &r, cs.data(), 3, &nc, mp.data(), 1, &nm) == PBS_OK);
    CHECK(nc == 3 && cs[0] == 3 && cs[1] == 4 && cs[2] == 5 && nm == 1 && mp[0] == 2);
    // errors: absent (1) + d3 twice + d4 + d5 + the encrypted chunk under a NONE index (1 mismatch)
    CHECK(r.entries == 10 && r.missing == 1 && r.loaded == 5 && r.newly_verified == 4 && r.newly_corrupt == 3);
    CHECK(r.mode_mismatch == 1 && r.errors == 6 && r.ok == 0 && r.index_check == PBS_VERIFY_INDEX_OK);
    CHECK(r.decoded_bytes == 100 + 200 + 77 + 50 + 0 && r.skipped_verified == 0 && r.skipped_corrupt == 0);
    std::vector<uint8_t> states(m);
    CHECK(pbs_verify_states_host(h, states.data(), m) == PBS_OK);
    const uint8_t want_st[8] = {1, 1, 1, 2, 2, 2, 0, 1};
    CHECK(std::memcmp(states.data(), want_st, m) == 0);
    CHECK(pbs_verify_states_host(h, states.data(), m - 1) == PBS_ERR_INVALID);

    // the same index again, as an image: nothing is loaded; then the manifest's checks
    const Bytes img = didx(digs, sizes);
    Bytes csum(32);
    pbs_sha256(img.data() + 4096, img.size() - 4096, csum.data());
    const uint64_t isz = 758, wrong = 759;
    CHECK(pbs_verify_index_host(h, img.data(), img.size(), PBS_VERIFY_MODE_NONE, &isz, csum.data(), s.blobs.data(),
                                s.off.data(), 0, &r, cs.data(), 3, &nc, mp.data(), 1, &nm) == PBS_OK);
    CHECK(r.loaded == 0 && r.skipped_verified == 5 && r.skipped_corrupt == 4 && r.errors == 5 && nc == 0 && nm == 1);
    CHECK(pbs_verify_index_host(h, img.data(), img.size(), PBS_VERIFY_MODE_NONE, &wrong, csum.data(), s.blobs.data(),
                                s.off.data(), 0, &r, nullptr, 0, nullptr, nullptr, 0, nullptr) == PBS_OK);
    CHECK(r.index_check == PBS_VERIFY_INDEX_WRONG_SIZE && r.ok == 0 && r.entries == 10);
    csum[0] ^= 1;
    CHECK(pbs_verify_index_host(h, img.data(), img.size(), PBS_VERIFY_MODE_NONE, &isz, csum.data(), s.blobs.data(),
                                s.off.data(), 0, &r, nullptr, 0, nullptr, nullptr, 0, nullptr) == PBS_OK);
    CHECK(r.index_check == PBS_VERIFY_INDEX_WRONG_CSUM && r.ok == 0);
    CHECK(pbs_verify_index_host(h, img.data(), img.size(), 7, nullptr, nullptr, s.blobs.data(), s.off.data(), 0, &r,
                                nullptr, 0, nullptr, nullptr, 0, nullptr) == PBS_ERR_INVALID);
    {
        Bytes cut(img.begin(), img.begin() + 4095), ragged(img.begin(), img.end() - 1), magic = img;
        magic[0] ^= 1;
        for (const Bytes* b : {&cut, &ragged, &magic})
            CHECK(pbs_verify_index_host(h, b->data(), b->size(), 0, nullptr, nullptr, s.blobs.data(), s.off.data(), 0, &r,
                                        nullptr, 0, nullptr, nullptr, 0, nullptr) == PBS_ERR_INVALID);
    }

    // fresh workers through the whole-index call at three budgets: one blob a batch, a few, all
    for (size_t budget : {(size_t)1, (size_t)400, (size_t)0}) {
        pbs_verify_host* w = nullptr;
        CHECK(pbs_verify_begin_host(s.digests.data(), m, &w, nullptr) == PBS_OK);
        CHECK(pbs_verify_index_host(w, img.data(), img.size(), PBS_VERIFY_MODE_ENCRYPT, nullptr, nullptr, s.blobs.data(),
                                    s.off.data(), budget, &r, cs.data(), 3, &nc, mp.data(), 1, &nm) == PBS_OK);
        // (entry 5 is eleven bytes here, not a load failure: TOO_SMALL, corrupt all the same)
        CHECK(r.loaded == 5 && r.newly_corrupt == 3 && r.mode_mismatch == 4 && r.errors == 5 + 4 && nc == 3 && nm == 1);
        CHECK(pbs_verify_states_host(w, states.data(), m) == PBS_OK && std::memcmp(states.data(), want_st, m) == 0);
        pbs_verify_end_host(w);
    }

    // an empty store and an empty index
    {
        pbs_verify_host* e = nullptr;
        CHECK(pbs_verify_begin_host(nullptr, 0, &e, nullptr) == PBS_OK && e);
        CHECK(pbs_verify_plan_host(e, flat.data(), sizes.data(), n, 0, nullptr, nullptr, 0, &nt, nullptr) == PBS_OK && nt == 0);
        CHECK(pbs_verify_submit_host(e, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr) == PBS_OK);
        CHECK(pbs_verify_finish_host(e, &r, nullptr, 0, &nc, nullptr, 0, &nm) == PBS_OK && nm == 10 && r.errors == 10);
        CHECK(pbs_verify_plan_host(e, nullptr, nullptr, 0, 0, nullptr, nullptr, 0, &nt, nullptr) == PBS_OK && nt == 0);
        CHECK(pbs_verify_abort_index_host(e) == PBS_OK && pbs_verify_abort_index_host(e) == PBS_OK);
        CHECK(pbs_verify_finish_host(e, &r, nullptr, 0, nullptr, nullptr, 0, nullptr) == PBS_ERR_INVALID);
        CHECK(pbs_verify_states_host(e, nullptr, 0) == PBS_OK);
        CHECK(pbs_verify_plan_host(e, flat.data(), sizes.data(), n, 2, nullptr, nullptr, 0, &nt, nullptr) == PBS_ERR_INVALID);
        CHECK(pbs_verify_plan_host(e, flat.data(), sizes.data(), n, 0, nullptr, nullptr, 1, &nt, nullptr) == PBS_ERR_INVALID);
        CHECK(pbs_verify_plan_host(e, flat.data(), sizes.data(), n, 0, nullptr, nullptr, 0, nullptr, nullptr) == PBS_ERR_INVALID);
        pbs_verify_end_host(e);
        pbs_verify_end_host(e);
        CHECK(pbs_verify_states_host(e, nullptr, 0) == PBS_ERR_INVALID);
    }

    // verify_blob
    {
        const Bytes good = blob(1, raw_frame(c1)), enc = blob(2, chunk(8, 9));
        Bytes bad = good, frame = raw_frame(c1);
        bad.back() ^= 1;
        frame[0] ^= 1;
        const Bytes badframe = blob(1, frame);
        int res = -1;
        CHECK(pbs_verify_blob_host(good.data(), good.size(), good.size(), sha(good).data(), &res) == PBS_OK && res == PBS_VERIFY_BLOB_OK);
        CHECK(pbs_verify_blob_host(enc.data(), enc.size(), enc.size(), sha(enc).data(), &res) == PBS_OK && res == PBS_VERIFY_BLOB_OK);
        CHECK(pbs_verify_blob_host(good.data(), good.size(), good.size() + 1, sha(good).data(), &res) == PBS_OK && res == PBS_VERIFY_BLOB_WRONG_SIZE);
        CHECK(pbs_verify_blob_host(good.data(), good.size(), good.size(), sha(bad).data(), &res) == PBS_OK && res == PBS_VERIFY_BLOB_WRONG_CSUM);
        CHECK(pbs_verify_blob_host(bad.data(), bad.size(), bad.size(), sha(bad).data(), &res) == PBS_OK && res == PBS_VERIFY_BLOB_LOAD);
        CHECK(pbs_verify_blob_host(badframe.data(), badframe.size(), badframe.size(), sha(badframe).data(), &res) == PBS_OK && res == PBS_VERIFY_BLOB_DECODE);
        CHECK(pbs_verify_blob_host(nullptr, 0, 0, sha(Bytes()).data(), &res) == PBS_OK && res == PBS_VERIFY_BLOB_LOAD);
        CHECK(pbs_verify_blob_host(good.data(), good.size(), good.size(), nullptr, &res) == PBS_ERR_INVALID);
    }

    // after the end every call is rejected
    pbs_verify_end_host(h);
    CHECK(pbs_verify_plan_host(h, flat.data(), sizes.data(), n, 0, ts.data(), te.data(), m, &nt, nullptr) == PBS_ERR_INVALID);
    CHECK(pbs_verify_finish_host(h, &r, nullptr, 0, nullptr, nullptr, 0, nullptr) == PBS_ERR_INVALID);
    CHECK(pbs_verify_abort_index_host(h) == PBS_ERR_INVALID);
    CHECK(pbs_verify_index_host(h, img.data(), img.size(), 0, nullptr, nullptr, s.blobs.data(), s.off.data(), 0, &r, nullptr,
                                0, nullptr, nullptr, 0, nullptr) == PBS_ERR_INVALID);
    pbs_verify_end_host(nullptr);

    std::printf(g_fail ? "verify_sanitize: %d checks failed\n" : "verify_sanitize ok\n", g_fail);
    return g_fail ? 1 : 0;
}
