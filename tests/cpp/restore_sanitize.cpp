// The host code of the restore path (proxmox-backup_amd/csrc/pbs_didx_read.cpp) under ASan +
// UBSan (make -C proxmox-backup_amd/csrc sanitize-restore): the index reader, chunk_from_offset
// and the lookup mirror on exactly sized heap buffers, good inputs and every error case.
#include <cstdio>
#include <cstring>
#include <vector>

#include "pbs_chunker.h"
#include "pbs_digest.h"
#include "pbs_restore.h"

static int g_fail = 0;
#define CHECK(x)                                                  \
    do {                                                          \
        if (!(x)) {                                               \
            std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #x); \
            ++g_fail;                                             \
        }                                                         \
    } while (0)

static std::vector<uint8_t> build(const std::vector<uint64_t>& ends, const std::vector<uint8_t>& dig) {
    std::vector<uint8_t> img(pbs_didx_size(ends.size()));
    uint8_t uuid[16];
    for (int i = 0; i < 16; ++i) uuid[i] = (uint8_t)(i + 1);
    CHECK(pbs_didx_build(ends.data(), dig.data(), ends.size(), uuid, 1234567, img.data(), img.size(), nullptr) == PBS_OK);
    return img;
}

static int parse(const std::vector<uint8_t>& img, size_t cap, size_t* n_out = nullptr) {
    std::vector<uint64_t> ends(cap);
    std::vector<uint8_t> dig(32 * cap);
    uint8_t uuid[16], hc[32], cc[32];
    int64_t ctime = 0;
    size_t n = 0;
    const int rc = pbs_didx_parse(img.data(), img.size(), uuid, &ctime, hc, cc, cap ? ends.data() : nullptr,
                                  cap ? dig.data() : nullptr, cap, &n);
    if (rc == PBS_OK) CHECK(std::memcmp(hc, cc, 32) == 0 && ctime == 1234567 && uuid[15] == 16);
    if (n_out) *n_out = n;
    return rc;
}

int main() {
    for (size_t n : {(size_t)0, (size_t)1, (size_t)3, (size_t)1000}) {
        std::vector<uint64_t> ends(n);
        std::vector<uint8_t> dig(32 * n);
        for (size_t i = 0; i < n; ++i) {
            ends[i] = (i / 2) * 1000 + 7;  // every second entry is empty
            for (int b = 0; b < 32; ++b) dig[32 * i + b] = (uint8_t)(i * 131 + b * 7);
        }
        const std::vector<uint8_t> img = build(ends, dig);
        size_t got = 0;
        CHECK(pbs_didx_count(img.size()) == n);
        CHECK(parse(img, n, &got) == PBS_OK && got == n);
        if (n) CHECK(parse(img, n - 1, &got) == PBS_ERR_CAPACITY && got == n);
        // every offset around every end
        for (size_t i = 0; i < n; ++i)
            for (uint64_t off : {ends[i] - 1, ends[i], ends[i] + 1}) {
                size_t idx = 0;
                uint64_t within = 0;
                const int rc = pbs_didx_chunk_from_offset(ends.data(), n, off, &idx, &within);
                if (off >= ends[n - 1]) {
                    CHECK(rc == PBS_ERR_INVALID);
                } else {
                    CHECK(rc == PBS_OK && idx < n && off < ends[idx] && (idx == 0 || ends[idx - 1] <= off));
                    CHECK(within == off - (idx ? ends[idx - 1] : 0));
                }
            }
        CHECK(pbs_didx_chunk_from_offset(ends.data(), n, n ? ends[n - 1] : 0, nullptr, nullptr) == PBS_ERR_INVALID);
        // the error cases, each in a buffer of exactly its size
        std::vector<uint8_t> cut(img.begin(), img.begin() + 4095);
        CHECK(parse(cut, n) == PBS_ERR_INVALID && pbs_didx_count(4095) == (size_t)-1);
        std::vector<uint8_t> magic = img;
        magic[7] ^= 1;
        CHECK(parse(magic, n) == PBS_ERR_INVALID);
        std::vector<uint8_t> ragged = img;
        ragged.push_back(0);
        CHECK(parse(ragged, n + 1) == PBS_ERR_INVALID && pbs_didx_count(ragged.size()) == (size_t)-1);
        if (n >= 3) {
            std::vector<uint8_t> dec = img;
            std::memset(&dec[4096 + 40 * (n - 1)], 0, 8);  // the last end: 0, below its neighbour
            CHECK(parse(dec, n) == PBS_ERR_INVALID);
        }
        // the lookup mirror: the index against itself reversed, plus misses
        std::vector<uint8_t> store;
        for (size_t i = n; i-- > 0;)
            if (i % 3) store.insert(store.end(), dig.begin() + 32 * i, dig.begin() + 32 * i + 32);
        const size_t m = store.size() / 32;
        std::vector<uint32_t> pos(n), first(n);
        size_t nm = 0, nu = 0;
        CHECK(pbs_digest_lookup_host(dig.data(), n, store.data(), m, pos.data(), first.data(), &nm, &nu) == PBS_OK);
        for (size_t i = 0; i < n; ++i) {
            CHECK(first[i] <= i && std::memcmp(&dig[32 * first[i]], &dig[32 * i], 32) == 0);
            if (pos[i] == PBS_LOOKUP_MISSING)
                CHECK(i % 3 == 0 || n > 256);  // (digests repeat with period 256 * k: only then may others match)
            else
                CHECK(pos[i] < m && std::memcmp(&store[32 * pos[i]], &dig[32 * i], 32) == 0);
        }
        CHECK(pbs_digest_lookup_host(dig.data(), n, nullptr, 0, pos.data(), first.data(), &nm, &nu) == PBS_OK && nm == n);
    }
    std::printf(g_fail ? "restore_sanitize: %d checks failed\n" : "restore_sanitize ok\n", g_fail);
    return g_fail ? 1 : 0;
}
