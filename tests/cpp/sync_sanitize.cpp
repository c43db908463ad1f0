// The host mirror of the sync job (proxmox-backup_amd/csrc/pbs_sync_host.cpp, over the verify
// mirror's blob verdict, the host inflater and pbs_sha256) under ASan + UBSan (make -C
// proxmox-backup_amd/csrc sanitize-sync): every buffer a heap block of exactly its size -- a small
// store with a known answer through two groups and a table growth, by hand and through the index
// image call, then the error cases: plan during plan, oversubmit, early finish, new_group with an
// index open, count + n at the limit, truncated and ragged index images, a lying manifest, an
// empty store, calls on a handle that has ended.
#include <cstdio>
#include <cstring>
#include <vector>

#include "pbs_blob.h"
#include "pbs_chunker.h"
#include "pbs_digest.h"
#include "pbs_sync.h"

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

static Bytes flat(const std::vector<Bytes>& v) {
    Bytes f;
    for (const Bytes& d : v) f.insert(f.end(), d.begin(), d.end());
    return f;
}

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
    // the local store lists L0, L1, L0 again; the index: N0 (new, good plain), L0, N1 (new, good
    // compressed), N0 again, N2 (new, stale CRC), N3 (new, cannot be fetched), L1, N4 (new, encrypted)
    const Bytes c0 = chunk(0, 100), c1 = chunk(1, 200), c2 = chunk(2, 60);
    const Bytes L0 = chunk(50, 32), L1 = chunk(51, 32), N3 = chunk(53, 32), N4 = chunk(54, 32);
    const Bytes N0 = sha(c0), N1 = sha(c1), N2 = sha(c2);
    const Bytes store = flat({L0, L1, L0});
    const std::vector<Bytes> digs = {N0, L0, N1, N0, N2, N3, L1, N4};
    const std::vector<uint64_t> sizes = {100, 5, 200, 100, 60, 9, 5, 77};
    const size_t n = digs.size();
    const Bytes fl = flat(digs);

    pbs_sync_host* h = nullptr;
    double ms = 0;
    CHECK(pbs_sync_begin_host(store.data(), 3, 0, &h, &ms) == PBS_OK && h);
    CHECK(pbs_sync_count_host(h) == 3 && pbs_sync_table_log2_host(h) == 6);
    std::vector<uint8_t> vd(n);
    std::vector<uint32_t> fs(n), fe(n), ts(n);
    size_t nf = 0, nt = 0;
    CHECK(pbs_sync_plan_host(h, fl.data(), sizes.data(), n, vd.data(), fs.data(), fe.data(), n, &nf, ts.data(), n, &nt,
                             &ms) == PBS_OK);
    const uint8_t want_v[8] = {2, 1, 2, 0, 2, 2, 1, 2};
    const uint32_t want_fs[5] = {3, 4, 5, 6, 7}, want_fe[5] = {0, 2, 4, 5, 7}, want_ts[2] = {0, 1};
    CHECK(std::memcmp(vd.data(), want_v, 8) == 0 && nf == 5 && nt == 2);
    CHECK(std::memcmp(fs.data(), want_fs, 20) == 0 && std::memcmp(fe.data(), want_fe, 20) == 0);
    CHECK(std::memcmp(ts.data(), want_ts, 8) == 0 && pbs_sync_count_host(h) == 8);
    // error cases on an open plan: nothing may change it
    CHECK(pbs_sync_plan_host(h, fl.data(), sizes.data(), n, nullptr, nullptr, nullptr, 0, &nf, nullptr, 0, &nt, nullptr) ==
          PBS_ERR_INVALID);
    CHECK(pbs_sync_new_group_host(h) == PBS_ERR_INVALID);
    CHECK(pbs_sync_finish_host(h, nullptr) == PBS_ERR_INVALID);
    {
        std::vector<uint32_t> a(2), b(2), c(1);
        CHECK(pbs_sync_lists_host(h, a.data(), b.data(), 2, &nf, c.data(), 1, &nt) == PBS_OK && nf == 5 && nt == 2);
        CHECK(a[1] == 4 && b[1] == 2 && c[0] == 0);
        CHECK(pbs_sync_lists_host(h, nullptr, nullptr, 1, &nf, nullptr, 0, &nt) == PBS_ERR_INVALID);
        std::vector<uint64_t> six(7, 0);
        const Bytes one(1, 0);
        CHECK(pbs_sync_submit_host(h, one.data(), six.data(), nullptr, 6, nullptr, nullptr, nullptr) == PBS_ERR_INVALID);
        const uint64_t down[2] = {5, 3};
        CHECK(pbs_sync_submit_host(h, one.data(), down, nullptr, 1, nullptr, nullptr, nullptr) == PBS_ERR_INVALID);
        CHECK(pbs_sync_submit_host(h, one.data(), nullptr, nullptr, 1, nullptr, nullptr, nullptr) == PBS_ERR_INVALID);
    }
    // submit: four items in one heap block (the fourth a load failure), then the encrypted one alone
    Bytes stale = blob(0, c2);
    stale.back() ^= 1;
    {
        const std::vector<Bytes> bl = {blob(0, c0), blob(1, raw_frame(c1)), stale, Bytes()};
        const Bytes part = flat(bl);
        std::vector<uint64_t> off = {0};
        for (const Bytes& b : bl) off.push_back(off.back() + b.size());
        std::vector<uint8_t> lf = {0, 0, 0, 1}, kinds(4), st(4);
        pbs_sync_timing tm;
        CHECK(pbs_sync_submit_host(h, part.data(), off.data(), lf.data(), 4, kinds.data(), st.data(), &tm) == PBS_OK);
        const uint8_t want_k[4] = {0, 1, 0, 255}, want_s[4] = {0, 0, PBS_BLOB_ST_BAD_CRC, PBS_SYNC_ST_LOAD_FAILED};
        CHECK(std::memcmp(kinds.data(), want_k, 4) == 0 && std::memcmp(st.data(), want_s, 4) == 0);
        CHECK(tm.blobs == 4 && tm.decoded == 3 && tm.encrypted == 0);
        CHECK(pbs_sync_finish_host(h, nullptr) == PBS_ERR_INVALID);  // one item is left
        const Bytes enc = blob(2, chunk(8, 30));
        const uint64_t off1[2] = {0, enc.size()};
        CHECK(pbs_sync_submit_host(h, enc.data(), off1, nullptr, 1, kinds.data(), st.data(), nullptr) == PBS_OK);
        CHECK(kinds[0] == 2 && st[0] == PBS_BLOB_ST_OK);  // verified by its CRC alone
        CHECK(pbs_sync_submit_host(h, enc.data(), off1, nullptr, 1, nullptr, nullptr, nullptr) == PBS_ERR_INVALID);
    }
    pbs_sync_result r;
    CHECK(pbs_sync_finish_host(h, &r) == PBS_OK);
    CHECK(r.entries == 8 && r.dup == 1 && r.exists == 2 && r.fetch == 5 && r.appended == 5 && r.inserted == 3);
    CHECK(r.failed == 1 && r.load_failed == 1 && r.chunk_count == 4 && r.first_failed == 2 && r.ok == 0);
    CHECK(r.bytes == 112 + (12 + 9 + 200) + 72 + (44 + 30));
    CHECK(pbs_sync_finish_host(h, &r) == PBS_ERR_INVALID);
    {
        Bytes dg(32 * 8), pr(8);
        size_t cnt = 0;
        CHECK(pbs_sync_listing_host(h, dg.data(), pr.data(), 8, &cnt) == PBS_OK && cnt == 8);
        const uint8_t want_p[8] = {1, 1, 1, 1, 1, 0, 0, 1};
        CHECK(std::memcmp(pr.data(), want_p, 8) == 0 && std::memcmp(&dg[32 * 3], N0.data(), 32) == 0 &&
              std::memcmp(&dg[32 * 7], N4.data(), 32) == 0);
        Bytes two(2);
        CHECK(pbs_sync_listing_host(h, nullptr, two.data(), 2, &cnt) == PBS_OK && cnt == 8 && two[1] == 1);
    }
    // the same group: everything is filtered; a new group: the absent ones are fetched again at their positions
    CHECK(pbs_sync_plan_host(h, fl.data(), sizes.data(), n, vd.data(), nullptr, nullptr, 0, &nf, nullptr, 0, &nt, nullptr) ==
              PBS_OK && nf == 0 && nt == 0 && vd[0] == 0 && vd[7] == 0);
    CHECK(pbs_sync_finish_host(h, &r) == PBS_OK && r.dup == 8 && r.ok == 1 && r.first_failed == PBS_SYNC_NONE);
    CHECK(pbs_sync_new_group_host(h) == PBS_OK);
    const Bytes img = didx(digs, sizes);
    Bytes csum(32);
    pbs_sha256(img.data() + 4096, img.size() - 4096, csum.data());
    const uint64_t isz = 556, wrong = 557;
    uint32_t chk = 9;
    size_t ne = 0;
    // a lying manifest: nothing is claimed, no plan is open
    CHECK(pbs_sync_index_image_host(h, img.data(), img.size(), &wrong, csum.data(), &chk, &ne, nullptr, 0, nullptr, nullptr, 0,
                                    &nf, nullptr, 0, &nt, nullptr) == PBS_OK && chk == PBS_VERIFY_INDEX_WRONG_SIZE && ne == 8);
    csum[0] ^= 1;
    CHECK(pbs_sync_index_image_host(h, img.data(), img.size(), &isz, csum.data(), &chk, &ne, nullptr, 0, nullptr, nullptr, 0,
                                    &nf, nullptr, 0, &nt, nullptr) == PBS_OK && chk == PBS_VERIFY_INDEX_WRONG_CSUM);
    csum[0] ^= 1;
    CHECK(pbs_sync_finish_host(h, &r) == PBS_ERR_INVALID);
    {
        Bytes cut(img.begin(), img.begin() + 4095), ragged(img.begin(), img.end() - 1), magic = img;
        magic[0] ^= 1;
        for (const Bytes* b : {&cut, &ragged, &magic})
            CHECK(pbs_sync_index_image_host(h, b->data(), b->size(), nullptr, nullptr, &chk, nullptr, nullptr, 0, nullptr,
                                            nullptr, 0, &nf, nullptr, 0, &nt, nullptr) == PBS_ERR_INVALID);
        CHECK(pbs_sync_index_image_host(h, img.data(), img.size(), nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr,
                                        nullptr, 0, &nf, nullptr, 0, &nt, nullptr) == PBS_ERR_INVALID);
    }
    Bytes v3(3);
    CHECK(pbs_sync_index_image_host(h, img.data(), img.size(), &isz, csum.data(), &chk, &ne, v3.data(), 3, fs.data(), fe.data(),
                                    n, &nf, ts.data(), n, &nt, &ms) == PBS_OK && chk == PBS_VERIFY_INDEX_OK);
    CHECK(v3[0] == 1 && v3[1] == 1 && v3[2] == 1 && nf == 2 && fs[0] == 5 && fs[1] == 6 && fe[0] == 4 && fe[1] == 5 && nt == 5);
    CHECK(pbs_sync_count_host(h) == 8);
    // abort: the claims stay
    CHECK(pbs_sync_abort_index_host(h) == PBS_OK && pbs_sync_abort_index_host(h) == PBS_OK);
    CHECK(pbs_sync_plan_host(h, fl.data(), sizes.data(), n, vd.data(), nullptr, nullptr, 0, &nf, nullptr, 0, &nt, nullptr) ==
              PBS_OK && nf == 0 && nt == 0);
    CHECK(pbs_sync_abort_index_host(h) == PBS_OK);

    // growth: 8 entries in 64 slots; 25 new ones make 2 (8 + 25) = 66 > 64: L = table_log2_for(33) + 1 = 8
    {
        std::vector<Bytes> more;
        for (unsigned k = 0; k < 25; ++k) more.push_back(chunk(100 + k, 32));
        const Bytes mf = flat(more);
        const std::vector<uint64_t> ms25(25, 7);
        CHECK(pbs_sync_new_group_host(h) == PBS_OK);
        CHECK(pbs_sync_plan_host(h, mf.data(), ms25.data(), 24, nullptr, nullptr, nullptr, 0, &nf, nullptr, 0, &nt, nullptr) ==
                  PBS_OK && nf == 24 && pbs_sync_table_log2_host(h) == 6 && pbs_sync_count_host(h) == 32);
        CHECK(pbs_sync_abort_index_host(h) == PBS_OK);
        CHECK(pbs_sync_plan_host(h, mf.data() + 32 * 24, ms25.data(), 1, nullptr, nullptr, nullptr, 0, &nf, nullptr, 0, &nt,
                                 nullptr) == PBS_OK && nf == 1 && pbs_sync_table_log2_host(h) == 8);
        std::vector<uint32_t> one(1), ent(1);
        CHECK(pbs_sync_lists_host(h, one.data(), ent.data(), 1, &nf, nullptr, 0, &nt) == PBS_OK && one[0] == 32);
        CHECK(pbs_sync_abort_index_host(h) == PBS_OK);
    }

    // the limits, an empty store and an empty index
    {
        CHECK(pbs_sync_plan_host(h, fl.data(), sizes.data(), (size_t)0xFFFFFFF0u - 33, nullptr, nullptr, nullptr, 0, &nf,
                                 nullptr, 0, &nt, nullptr) == PBS_ERR_INVALID);
        pbs_sync_host* e = nullptr;
        CHECK(pbs_sync_begin_host(store.data(), 3, (size_t)0xFFFFFFF0u - 3, &e, nullptr) == PBS_ERR_INVALID && !e);
        CHECK(pbs_sync_begin_host(nullptr, 1, 0, &e, nullptr) == PBS_ERR_INVALID);
        CHECK(pbs_sync_begin_host(nullptr, 0, 0, &e, nullptr) == PBS_OK && e);
        CHECK(pbs_sync_plan_host(e, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, &nf, nullptr, 0, &nt, nullptr) == PBS_OK);
        CHECK(pbs_sync_submit_host(e, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr) == PBS_OK);
        CHECK(pbs_sync_finish_host(e, &r) == PBS_OK && r.entries == 0 && r.ok == 1);
        CHECK(pbs_sync_plan_host(e, fl.data(), sizes.data(), n, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, &nt,
                                 nullptr) == PBS_ERR_INVALID);
        CHECK(pbs_sync_plan_host(e, fl.data(), sizes.data(), n, nullptr, nullptr, nullptr, 1, &nf, nullptr, 0, &nt, nullptr) ==
              PBS_ERR_INVALID);
        CHECK(pbs_sync_listing_host(e, nullptr, nullptr, 0, nullptr) == PBS_OK);
        pbs_sync_end_host(e);
        pbs_sync_end_host(e);
        CHECK(pbs_sync_listing_host(e, nullptr, nullptr, 0, nullptr) == PBS_ERR_INVALID);
    }

    // after the end every call is rejected
    pbs_sync_end_host(h);
    CHECK(pbs_sync_plan_host(h, fl.data(), sizes.data(), n, nullptr, nullptr, nullptr, 0, &nf, nullptr, 0, &nt, nullptr) ==
          PBS_ERR_INVALID);
    CHECK(pbs_sync_finish_host(h, &r) == PBS_ERR_INVALID && pbs_sync_abort_index_host(h) == PBS_ERR_INVALID);
    CHECK(pbs_sync_new_group_host(h) == PBS_ERR_INVALID && pbs_sync_count_host(h) == 0 && pbs_sync_table_log2_host(h) == 0);
    CHECK(pbs_sync_index_image_host(h, img.data(), img.size(), nullptr, nullptr, &chk, nullptr, nullptr, 0, nullptr, nullptr, 0,
                                    &nf, nullptr, 0, &nt, nullptr) == PBS_ERR_INVALID);
    pbs_sync_end_host(nullptr);

    std::printf(g_fail ? "sync_sanitize: %d checks failed\n" : "sync_sanitize ok\n", g_fail);
    return g_fail ? 1 : 0;
}
