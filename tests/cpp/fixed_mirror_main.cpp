// Drives the fixed-path mirrors of host/pbs_chunker.hpp for tests/test_fixed_mirror_cpp.py:
//   fixed_mirror read FILE [OFFSET...]     FixedIndexReader over a .fidx file
//   fixed_mirror stream C PIECE FILE       FixedChunkStream over a file fed in PIECE-byte reads
//   fixed_mirror write FILE OUT            FixedIndexWriter: clone FILE, entries added out of
//                                          order through add_chunk, errors probed
#include <cstdio>
#include <cstdlib>
#include <string>

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

static std::vector<uint8_t> slurp(const char* path) {
    std::vector<uint8_t> v;
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return v;
    uint8_t buf[65536];
    for (size_t k; (k = std::fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + k);
    std::fclose(f);
    return v;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const std::string mode = argv[1];
    try {
        if (mode == "read") {
            pbs::FixedIndexReader r{std::string(argv[2])};
            std::printf("count %zu\nbytes %llu\nchunk_size %llu\nctime %lld\n", r.index_count(),
                        (unsigned long long)r.index_bytes(), (unsigned long long)r.chunk_size, (long long)r.ctime);
            std::printf("uuid %s\nindex_csum %s\n", hex(r.uuid.data(), 16).c_str(), hex(r.index_csum.data(), 32).c_str());
            const auto cs = r.compute_csum();
            std::printf("computed_csum %s\ncsum_end %llu\n", hex(cs.first.data(), 32).c_str(), (unsigned long long)cs.second);
            for (size_t i = 0; i < r.index_count(); ++i) {
                const auto ci = *r.chunk_info(i);
                std::printf("chunk%zu %llu %llu %s\n", i, (unsigned long long)ci.start, (unsigned long long)ci.end,
                            hex(ci.digest.data(), 32).c_str());
            }
            std::printf("past %d %d\n", r.chunk_info(r.index_count()).has_value(), r.index_digest(r.index_count()).has_value());
            for (int a = 3; a < argc; ++a) {
                const auto p = r.chunk_from_offset(std::strtoull(argv[a], nullptr, 10));
                if (p)
                    std::printf("offset%s %zu %llu\n", argv[a], p->first, (unsigned long long)p->second);
                else
                    std::printf("offset%s none\n", argv[a]);
            }
        } else if (mode == "stream" && argc >= 5) {
            const size_t c = std::strtoull(argv[2], nullptr, 10), piece = std::strtoull(argv[3], nullptr, 10);
            const std::vector<uint8_t> data = slurp(argv[4]);
            pbs::FixedChunkStream s(c);
            size_t k = 0;
            auto show = [&](const std::vector<std::vector<uint8_t>>& v) {
                for (const auto& ch : v) {
                    uint8_t d[32];
                    pbs_sha256(ch.data(), ch.size(), d);
                    std::printf("chunk%zu %zu %s\n", k++, ch.size(), hex(d, 32).c_str());
                }
            };
            for (size_t at = 0; at < data.size(); at += piece) show(s.feed(data.data() + at, std::min(piece, data.size() - at)));
            show(s.finish());
            std::printf("chunks %zu\n", k);
        } else if (mode == "write" && argc >= 4) {
            pbs::FixedIndexReader r{std::string(argv[2])};
            const size_t n = r.index_count();
            // out of order through add_chunk: odd entries descending, then even ones
            pbs::FixedIndexWriter w(r.size, r.chunk_size, r.uuid, r.ctime);
            auto add = [&](size_t i) {
                const auto ci = *r.chunk_info(i);
                w.add_chunk(ci.end, ci.end - ci.start, ci.digest);
            };
            for (size_t i = n; i-- > 0;)
                if (i % 2) add(i);
            for (size_t i = 0; i < n; i += 2) add(i);
            int errs = 0;
            try { w.add_digest(n, pbs::Digest{}); } catch (const std::out_of_range&) { errs |= 1; }
            try { w.add_chunk(r.size + 1, 1, pbs::Digest{}); } catch (const std::runtime_error&) { errs |= 2; }
            const pbs::Digest cs = w.close();
            try { w.close(); } catch (const std::runtime_error&) { errs |= 4; }
            pbs::FixedIndexWriter w2(r.size + r.chunk_size, r.chunk_size, r.uuid, r.ctime);
            try { w2.clone_data_from(r); } catch (const std::runtime_error&) { errs |= 8; }
            pbs::FixedIndexWriter w3(r.size, r.chunk_size, r.uuid, r.ctime);
            w3.clone_data_from(r);
            const pbs::Digest cs3 = w3.close();
            std::printf("csum %s\nclone_csum %s\nerrors %d\nsame %d\n", hex(cs.data(), 32).c_str(), hex(cs3.data(), 32).c_str(),
                        errs, (int)(w.image() == w3.image()));
            std::FILE* f = std::fopen(argv[3], "wb");
            if (!f) return 2;
            std::fwrite(w.image().data(), 1, w.image().size(), f);
            std::fclose(f);
        } else {
            return 2;
        }
    } catch (const std::exception& e) {
        std::printf("error %s\n", e.what());
        return 3;
    }
    return 0;
}
