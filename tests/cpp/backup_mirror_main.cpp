// pbs::BackupSession of the C++ host mirror (host/pbs_chunker.hpp) over the session's host
// mirror: a snapshot of kind-0 chunks read from a file goes through create / upload / append /
// close / add_blob / finish, and every result is printed as "key value" lines for
// tests/test_backup_mirror_cpp.py.
//   backup_mirror <data file> <chunk length> <out .didx>
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "pbs_chunker.hpp"

static std::string hex(const uint8_t* p, size_t n) {
    static const char* d = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; ++i) {
        s += d[p[i] >> 4];
        s += d[p[i] & 15];
    }
    return s;
}

static std::vector<uint8_t> plain_blob(const uint8_t* c, size_t n) {
    static const uint8_t magic[8] = {66, 171, 56, 7, 190, 131, 112, 161};
    std::vector<uint8_t> b(magic, magic + 8);
    const uint32_t crc = pbs::crc32(c, n);
    for (int i = 0; i < 4; ++i) b.push_back((uint8_t)(crc >> (8 * i)));
    b.insert(b.end(), c, c + n);
    return b;
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    try {
        std::ifstream in(argv[1], std::ios::binary);
        const std::vector<uint8_t> data((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        const size_t len = std::stoul(argv[2]);
        std::vector<uint8_t> digests, blobs;
        std::vector<uint32_t> sizes;
        std::vector<uint64_t> boff{0}, starts, ends;
        for (size_t at = 0; at < data.size(); at += len) {
            const size_t n = std::min(len, data.size() - at);
            const pbs::Digest dg = pbs::sha256(data.data() + at, n);
            digests.insert(digests.end(), dg.begin(), dg.end());
            sizes.push_back((uint32_t)n);
            const std::vector<uint8_t> b = plain_blob(data.data() + at, n);
            blobs.insert(blobs.end(), b.begin(), b.end());
            boff.push_back(blobs.size());
            starts.push_back(at);
            ends.push_back(at + n);
        }
        const size_t k = sizes.size();
        pbs::BackupSession s({}, {}, {}, 0, false);
        std::printf("finish_empty %d\n", s.finish());
        const auto w = s.create_dynamic();
        std::printf("wid %d %u\n", w.first, w.second);
        const auto up = s.upload(w.second, digests, sizes, blobs.data(), boff);
        std::printf("upload %d %llu\n", up.code, (unsigned long long)up.first_failed);
        for (size_t t = 0; t < k; ++t)
            std::printf("item%zu %u %u %u %u %u %u\n", t, up.status[t], up.ins[t], up.action[t], up.is_duplicate[t],
                        up.compressed_size[t], up.reg[t]);
        const auto unknown = s.lookup(std::vector<uint8_t>(32, 7).data());
        std::printf("lookup %d %u\n", unknown ? 1 : 0, k ? *s.lookup(digests.data()) : 0);
        std::vector<uint64_t> wrong = starts;
        if (k > 1) wrong[1] += 1;
        const auto bad = s.dynamic_append(w.second, digests, wrong);
        std::printf("append_bad %d %zu %d\n", bad.code, bad.n_done, bad.err);
        const std::vector<uint8_t> rest(digests.begin() + 32 * bad.n_done, digests.end());
        const std::vector<uint64_t> rest_off(starts.begin() + bad.n_done, starts.end());
        const auto ok = s.dynamic_append(w.second, rest, rest_off);
        std::printf("append %d %zu %d\n", ok.code, ok.n_done, ok.err);
        pbs::Digest csum;  // what the client's DynamicIndexWriter ends with
        std::vector<uint8_t> client(pbs_didx_size(k));
        if (pbs_didx_build(ends.data(), digests.data(), k, nullptr, 0, client.data(), client.size(), csum.data()) != PBS_OK)
            return 4;
        const auto cl = s.dynamic_close(w.second, k, data.size(), csum.data());
        std::printf("close %d %d %llu %llu\n", cl.code, cl.result, (unsigned long long)cl.stat.count,
                    (unsigned long long)cl.stat.upload_percent);
        std::ofstream(argv[3], std::ios::binary).write(reinterpret_cast<const char*>(cl.image.data()), (std::streamsize)cl.image.size());
        const auto again = s.dynamic_close(w.second, k, data.size(), csum.data());
        std::printf("close_again %d %d\n", again.code, again.result);
        const std::vector<uint8_t> m = plain_blob(data.data(), std::min<size_t>(data.size(), 10));
        const auto ab = s.add_blob(m.data(), m.size());
        std::printf("add_blob %d %u\n", ab.first, ab.second);
        std::printf("finish %d\n", s.finish());
        const pbs_backup_stat st = s.stats();
        std::printf("stats %llu %llu %llu %u\n", (unsigned long long)st.file_counter, (unsigned long long)st.backup_size,
                    (unsigned long long)st.count, st.finished);
        std::printf("count %zu %u\n", s.count(), s.table_log2());
        std::printf("after %d\n", s.create_dynamic().first);
    } catch (const std::exception& e) {
        std::printf("error %s\n", e.what());
        return 3;
    }
    return 0;
}
