// The host mirror of the backup session (proxmox-backup_amd/csrc/pbs_backup_host.cpp with
// backup_common.h, over the verify mirror's blob verdict, the host inflater, pbs_sha256 and both
// index writers) under ASan + UBSan (make -C proxmox-backup_amd/csrc sanitize-backup): every
// buffer a heap block of exactly its size -- a small session with a known answer (register, an
// upload with a chain of one digest and a wrong stored CRC, a dynamic and a fixed writer, an
// incremental one, closes, add_blob, finish), then the error cases: unknown wid, bad blob offsets,
// every close check, truncated reuse and index images, a table growth, calls after finish, calls
// on a handle that has ended.
#include <cstdio>
#include <cstring>
#include <vector>

#include "pbs_backup.h"
#include "pbs_blob.h"
#include "pbs_chunker.h"
#include "pbs_digest.h"
#include "pbs_fixed.h"

static int g_fail = 0;
#define CHECK(x)                                                      \
    do {                                                              \
        if (!(x)) {                                                   \
            std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #x); \
            ++g_fail;                                                 \
        }                                                             \
    } while (0)

typedef std::vector<uint8_t> Bytes;

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

static Bytes digest_of(const Bytes& c) {
    Bytes d(32);
    pbs_sha256(c.data(), c.size(), d.data());
    return d;
}

struct Batch {
    Bytes digests, blobs;
    std::vector<uint32_t> sizes;
    std::vector<uint64_t> off{0};
    void add(const Bytes& dg, uint32_t size, const Bytes& b) {
        digests.insert(digests.end(), dg.begin(), dg.end());
        sizes.push_back(size);
        blobs.insert(blobs.end(), b.begin(), b.end());
        off.push_back(blobs.size());
    }
    size_t k() const { return sizes.size(); }
};

struct Result {
    Bytes status, ins, action, dup, reg;
    std::vector<uint32_t> crc, comp;
    uint64_t first = 0;
    explicit Result(size_t k) : status(k), ins(k), action(k), dup(k), reg(k), crc(k), comp(k) {}
};

static int upload(pbs_backup_host* h, uint32_t wid, const Batch& b, Result& r) {
    return pbs_backup_upload_host(h, wid, b.digests.data(), b.sizes.data(), nullptr, b.blobs.data(), b.off.data(), b.k(),
                                  r.status.data(), r.crc.data(), r.ins.data(), r.action.data(), r.dup.data(), r.comp.data(),
                                  r.reg.data(), &r.first, nullptr);
}

int main() {
    // a listing of three: a kind-0 file, an empty file, something that is no file
    const Bytes c0 = chunk(1, 100), c1 = chunk(2, 120), c2 = chunk(3, 64), c3 = chunk(4, 64), c4 = chunk(5, 30);
    const Bytes d0 = digest_of(c0), d1 = digest_of(c1), d2 = digest_of(c2), d3 = digest_of(c3), d4 = digest_of(c4);
    Bytes listing;
    for (const Bytes* d : {&d0, &d1, &d2}) listing.insert(listing.end(), d->begin(), d->end());
    std::vector<uint64_t> lsize = {blob(0, c0).size(), 0, 10};
    Bytes lkind = {0, PBS_BLOB_KIND_NONE, PBS_BACKUP_KIND_NOT_FILE};
    pbs_backup_host* h = nullptr;
    CHECK(pbs_backup_begin_host(listing.data(), lsize.data(), lkind.data(), 3, 0, &h, nullptr) == PBS_OK);
    CHECK(pbs_backup_count_host(h) == 3 && pbs_backup_table_log2_host(h) == 6);

    uint32_t wd = 0, wf = 0;
    CHECK(pbs_backup_create_dynamic_host(h, nullptr, 7, &wd) == PBS_OK && wd == 1);
    CHECK(pbs_backup_create_fixed_host(h, 64 * 2 + 30, 64, nullptr, 7, nullptr, 0, nullptr, &wf) == PBS_OK && wf == 2);

    // uploads: DUP_SAME, OVERWRITE_EMPTY, ERR_TYPE, a chain of one new digest (a frame, then the
    // shorter kind-0 blob with a wrong stored CRC, then an encrypted copy), a bad digest
    {
        Batch b;
        b.add(d0, 100, blob(0, c0));
        b.add(d1, 120, blob(0, c1));
        b.add(d2, 64, blob(0, c2));
        b.add(d3, 64, blob(1, raw_frame(c3)));
        Bytes wrong = blob(0, c3);
        wrong[9] ^= 4;
        b.add(d3, 64, wrong);
        b.add(d3, 64, blob(2, c3));
        b.add(d4, 30, blob(0, c3));
        Result r(b.k());
        CHECK(upload(h, wd, b, r) == PBS_OK);
        const uint8_t want_ins[] = {PBS_BACKUP_INS_DUP_SAME, PBS_BACKUP_INS_OVERWRITE_EMPTY, PBS_BACKUP_INS_ERR_TYPE,
                                    PBS_BACKUP_INS_NEW, PBS_BACKUP_INS_REPLACE_BIGGER, PBS_BACKUP_INS_ERR_UNENC_TO_ENC,
                                    PBS_BACKUP_INS_NONE};
        for (size_t t = 0; t < b.k(); ++t) CHECK(r.ins[t] == want_ins[t]);
        CHECK(r.status[4] == PBS_BLOB_ST_OK && r.crc[4] == crc32(c3.data(), c3.size()));
        CHECK(r.status[6] == PBS_BLOB_ST_BAD_DIGEST && r.first == 2);
        CHECK(pbs_backup_count_host(h) == 4);
        uint32_t sz = 0;
        CHECK(pbs_backup_lookup_host(h, d3.data(), &sz) == PBS_OK && sz == 64);
        CHECK(pbs_backup_lookup_host(h, d2.data(), &sz) == PBS_BACKUP_E_NO_SUCH_CHUNK);
    }
    // the fixed writer: a full chunk, the small last one, a second small one, a large one
    {
        Batch b;
        b.add(d2, 64, blob(2, c2));   // (NOT_FILE: the insert fails, nothing is registered)
        b.add(d3, 64, blob(0, c3));
        b.add(d4, 30, blob(0, c4));
        b.add(digest_of(chunk(6, 20)), 20, blob(0, chunk(6, 20)));
        b.add(d0, 100, blob(0, c0));
        Result r(b.k());
        CHECK(upload(h, wf, b, r) == PBS_OK);
        CHECK(r.reg[0] == PBS_BACKUP_REG_NONE && r.reg[1] == PBS_BACKUP_REG_OK && r.reg[2] == PBS_BACKUP_REG_OK);
        CHECK(r.reg[3] == PBS_BACKUP_REG_ERR_MULTI_SMALL && r.reg[4] == PBS_BACKUP_REG_ERR_LARGE);
        Result none(0);
        Batch empty;
        CHECK(upload(h, wf, empty, none) == PBS_OK && upload(h, 9, empty, none) == PBS_BACKUP_E_NO_WRITER);
        Batch bad = b;
        bad.off[1] = bad.off[2] + 1;
        CHECK(upload(h, wf, bad, r) == PBS_ERR_INVALID);
    }
    // appends and closes
    Bytes fimage;
    uint8_t fcsum[32];
    {
        Bytes dd;
        for (const Bytes* d : {&d3, &d0, &d3}) dd.insert(dd.end(), d->begin(), d->end());
        std::vector<uint64_t> offs = {0, 64, 164};
        size_t done = 0;
        int err = 0;
        CHECK(pbs_backup_dynamic_append_host(h, wd, dd.data(), offs.data(), 3, &done, &err, nullptr) == PBS_OK);
        CHECK(done == 3 && err == 0);
        offs[1] = 1;
        CHECK(pbs_backup_dynamic_append_host(h, wd, dd.data(), offs.data(), 3, &done, &err, nullptr) == PBS_OK);
        CHECK(done == 0 && err == PBS_BACKUP_E_STRANGE_OFFSET);
        std::vector<uint64_t> ends = {64, 164, 228};
        Bytes image(pbs_didx_size(3)), got(pbs_didx_size(3));
        uint8_t csum[32];
        CHECK(pbs_didx_build(ends.data(), dd.data(), 3, nullptr, 7, image.data(), image.size(), csum) == PBS_OK);
        int result = -1;
        pbs_backup_writer_stat st;
        Bytes small(pbs_didx_size(3) - 1);
        CHECK(pbs_backup_dynamic_close_host(h, wd, 3, 228, csum, small.data(), small.size(), &result, &st) == PBS_ERR_CAPACITY);
        CHECK(pbs_backup_dynamic_close_host(h, wd, 3, 228, csum, got.data(), got.size(), &result, &st) == PBS_OK);
        CHECK(result == PBS_BACKUP_E_NONE && got == image && st.logged == 1 && st.count == 4 && st.client_duplicates == 0);
        CHECK(pbs_backup_dynamic_close_host(h, wd, 3, 228, csum, got.data(), got.size(), &result, &st) == PBS_OK);
        CHECK(result == PBS_BACKUP_E_NO_WRITER);

        Bytes fd;
        for (const Bytes* d : {&d4, &d3, &d3}) fd.insert(fd.end(), d->begin(), d->end());
        std::vector<uint64_t> foffs = {128, 64, 0};
        CHECK(pbs_backup_fixed_append_host(h, wf, fd.data(), foffs.data(), 3, &done, &err, nullptr) == PBS_OK);
        CHECK(done == 3 && err == 0);
        foffs[0] = 129;
        CHECK(pbs_backup_fixed_append_host(h, wf, fd.data(), foffs.data(), 1, &done, &err, nullptr) == PBS_OK);
        CHECK(done == 0 && err == PBS_ERR_INVALID);
        Bytes want;
        for (const Bytes* d : {&d3, &d3, &d4}) want.insert(want.end(), d->begin(), d->end());
        fimage.resize(pbs_fidx_size(3));
        CHECK(pbs_fidx_build(want.data(), 158, 64, nullptr, 7, fimage.data(), fimage.size(), fcsum) == PBS_OK);
        Bytes fgot(fimage.size());
        CHECK(pbs_backup_fixed_close_host(h, wf, 3, 158, fcsum, fgot.data(), fgot.size(), &result, &st) == PBS_OK);
        CHECK(result == PBS_BACKUP_E_NONE && fgot == fimage);
    }
    // the incremental writer, truncated images, register from images
    {
        uint32_t w = 0;
        Bytes cut(fimage.begin(), fimage.end() - 1);
        CHECK(pbs_backup_create_fixed_host(h, 158, 64, nullptr, 0, cut.data(), cut.size(), fcsum, &w) == PBS_BACKUP_E_REUSE_NO_IMAGE);
        uint8_t other[32] = {};
        CHECK(pbs_backup_create_fixed_host(h, 158, 64, nullptr, 0, fimage.data(), fimage.size(), other, &w) == PBS_BACKUP_E_REUSE_CSUM);
        CHECK(pbs_backup_create_fixed_host(h, 300, 64, nullptr, 0, fimage.data(), fimage.size(), fcsum, &w) == PBS_BACKUP_E_REUSE_LENGTH);
        CHECK(pbs_backup_create_fixed_host(h, 158, 0, nullptr, 0, nullptr, 0, nullptr, &w) == PBS_ERR_INVALID);
        CHECK(pbs_backup_create_fixed_host(h, 158, 64, nullptr, 0, fimage.data(), fimage.size(), fcsum, &w) == PBS_OK && w == 3);
        int result = -1;
        Bytes fgot(fimage.size());
        CHECK(pbs_backup_fixed_close_host(h, w, 0, 0, fcsum, fgot.data(), fgot.size(), &result, nullptr) == PBS_OK);
        CHECK(result == PBS_BACKUP_E_NONE && std::memcmp(fgot.data() + 4096, fimage.data() + 4096, 96) == 0);
        size_t n = 0;
        CHECK(pbs_backup_register_index_image_host(h, fimage.data(), fimage.size(), &n, nullptr) == PBS_OK && n == 3);
        CHECK(pbs_backup_register_index_image_host(h, cut.data(), cut.size(), &n, nullptr) == PBS_ERR_INVALID);
        CHECK(pbs_backup_register_index_image_host(h, cut.data(), 100, &n, nullptr) == PBS_ERR_INVALID);
        uint32_t sz = 0;
        CHECK(pbs_backup_lookup_host(h, d4.data(), &sz) == PBS_OK && sz == 30);
    }
    // a growth of the table: 100 new digests registered over 6 entries
    {
        Bytes dd(32 * 100);
        std::vector<uint32_t> sizes(100, 9);
        for (size_t i = 0; i < dd.size(); ++i) dd[i] = (uint8_t)(i * 13 + i / 32);
        CHECK(pbs_backup_register_previous_host(h, dd.data(), sizes.data(), 100, nullptr) == PBS_OK);
        CHECK(pbs_backup_count_host(h) == 106 && pbs_backup_table_log2_host(h) == 9);
        Bytes out(32 * 106), present(106), kind(106), known(106);
        std::vector<uint64_t> size(106);
        std::vector<uint32_t> ks(106);
        size_t cnt = 0;
        CHECK(pbs_backup_listing_host(h, out.data(), present.data(), size.data(), kind.data(), known.data(), ks.data(), 106,
                                      &cnt) == PBS_OK);
        CHECK(cnt == 106 && present[105] == 0 && known[105] == 1 && ks[105] == 9);
        CHECK(pbs_backup_listing_host(h, out.data(), nullptr, nullptr, nullptr, nullptr, nullptr, 2, &cnt) == PBS_OK);
    }
    // add_blob, finish, and everything after
    {
        uint8_t st = 0;
        pbs_backup_stat bs;
        const Bytes m = blob(0, chunk(9, 40));
        Bytes bad = m;
        bad[20] ^= 1;
        CHECK(pbs_backup_add_blob_host(h, bad.data(), bad.size(), &st) == PBS_OK && st == PBS_BLOB_ST_BAD_CRC);
        CHECK(pbs_backup_add_blob_host(h, m.data(), 5, &st) == PBS_OK && st == PBS_BLOB_ST_TOO_SMALL);
        CHECK(pbs_backup_add_blob_host(h, nullptr, 0, &st) == PBS_OK && st == PBS_BLOB_ST_TOO_SMALL);
        CHECK(pbs_backup_add_blob_host(h, m.data(), m.size(), &st) == PBS_OK && st == PBS_BLOB_ST_OK);
        uint32_t w = 0;
        CHECK(pbs_backup_create_dynamic_host(h, nullptr, 0, &w) == PBS_OK);
        CHECK(pbs_backup_finish_host(h, &bs) == PBS_BACKUP_E_OPEN_WRITER);
        int result = 0;
        uint8_t none[32] = {};
        CHECK(pbs_backup_dynamic_close_host(h, w, 1, 0, none, nullptr, 0, &result, nullptr) == PBS_OK);
        CHECK(result == PBS_BACKUP_E_CHUNK_COUNT);
        CHECK(pbs_backup_finish_host(h, &bs) == PBS_OK && bs.finished == 1 && bs.file_counter == 4 && bs.open_writers == 0);
        CHECK(pbs_backup_finish_host(h, &bs) == PBS_BACKUP_E_FINISHED);
        CHECK(pbs_backup_create_dynamic_host(h, nullptr, 0, &w) == PBS_BACKUP_E_FINISHED);
        CHECK(pbs_backup_add_blob_host(h, m.data(), m.size(), &st) == PBS_BACKUP_E_FINISHED);
        CHECK(pbs_backup_stats_host(h, &bs) == PBS_OK && bs.finished == 1);
    }
    pbs_backup_end_host(h);
    pbs_backup_end_host(h);  // (a dead handle: nothing)
    uint32_t w = 0;
    CHECK(pbs_backup_create_dynamic_host(h, nullptr, 0, &w) == PBS_ERR_INVALID);
    CHECK(pbs_backup_count_host(h) == 0 && pbs_backup_count_host(nullptr) == 0);
    // an empty listing
    CHECK(pbs_backup_begin_host(nullptr, nullptr, nullptr, 0, 0, &h, nullptr) == PBS_OK);
    pbs_backup_stat bs;
    CHECK(pbs_backup_finish_host(h, &bs) == PBS_BACKUP_E_NO_FILES);
    pbs_backup_end_host(h);
    CHECK(pbs_backup_begin_host(nullptr, nullptr, nullptr, 1, 0, &h, nullptr) == PBS_ERR_INVALID);
    if (g_fail) {
        std::printf("backup_sanitize: %d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("backup_sanitize ok\n");
    return 0;
}
