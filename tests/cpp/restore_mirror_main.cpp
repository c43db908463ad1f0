// pbs::DynamicIndexReader of the C++ host mirror (proxmox-backup_amd/host/pbs_chunker.hpp) on
// the host: opens the .didx file argv[1] and prints what the reader knows; every further
// argument is an archive offset to look up (tests/test_restore_mirror_cpp.py compares with the
// builder's inputs).  A file that the reader refuses prints "error" and exits 3.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "pbs_chunker.hpp"

static void hex(const char* tag, const uint8_t* p, size_t n) {
    std::printf("%s ", tag);
    for (size_t i = 0; i < n; ++i) std::printf("%02x", p[i]);
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    try {
        const pbs::DynamicIndexReader r{std::string(argv[1])};
        std::printf("count %zu\nbytes %llu\nsize %zu\nctime %lld\n", r.index_count(),
                    (unsigned long long)r.index_bytes(), r.size, (long long)r.ctime);
        hex("uuid", r.uuid.data(), 16);
        hex("index_csum", r.index_csum.data(), 32);
        const auto cs = r.compute_csum();
        hex("computed_csum", cs.first.data(), 32);
        std::printf("csum_end %llu\n", (unsigned long long)cs.second);
        for (size_t i = 0; i < r.index_count(); ++i) {
            const pbs::ChunkReadInfo ci = *r.chunk_info(i);
            std::printf("chunk%zu %llu %llu ", i, (unsigned long long)ci.start, (unsigned long long)ci.end);
            hex("", ci.digest.data(), 32);
            if (ci.end != r.chunk_end(i) || *r.index_digest(i) != ci.digest) return 4;
        }
        if (r.chunk_info(r.index_count()) || r.index_digest(r.index_count())) return 4;
        for (int a = 2; a < argc; ++a) {
            const unsigned long long off = std::strtoull(argv[a], nullptr, 0);
            const auto f = r.chunk_from_offset(off);
            if (f)
                std::printf("offset%llu %zu %llu\n", off, f->first, (unsigned long long)f->second);
            else
                std::printf("offset%llu none\n", off);
        }
    } catch (const std::exception& e) {
        std::printf("error %s\n", e.what());
        return 3;
    }
    return 0;
}
