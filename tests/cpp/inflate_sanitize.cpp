// The zstd format code (csrc/zstd_dec.h) under AddressSanitizer + UndefinedBehaviorSanitizer,
// through its host mirror pbs_zstd_inflate_host (csrc/pbs_inflate_host.cpp): the bounds proof
// of the code the GPU kernel shares.  Stand-alone: `make -C proxmox-backup_amd/csrc
// sanitize-inflate INFLATE_CORPUS=<dir>`; <dir> holds the corpus of tests/iplanted.py, one
// file per frame named <index>_<slot bytes>.zst, bad frames included.
//
// Every frame is copied into a heap buffer of exactly its length and inflated into heap
// buffers of exactly the slot's size, of half of it and of none, so a read or write one byte
// outside either is a report; then every prefix of its first 96 bytes and its last 32 is
// inflated too (truncations inside every header field).  A status is never an error here:
// only a sanitizer report (halt_on_error) or a failed call fails the run.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <string>
#include <vector>

#include "pbs_blob.h"
#include "pbs_chunker.h"

static int failures = 0;
static unsigned long calls = 0, not_ok = 0;

static void run(const uint8_t* src, size_t len, size_t cap) {
    uint8_t* frame = static_cast<uint8_t*>(std::malloc(len ? len : 1));
    uint8_t* out = static_cast<uint8_t*>(std::malloc(cap ? cap : 1));
    if (len) std::memcpy(frame, src, len);
    size_t out_len = ~(size_t)0;
    uint8_t status = 0xEE;
    const int rc = pbs_zstd_inflate_host(frame, len, cap ? out : nullptr, cap, &out_len, &status);
    ++calls;
    if (rc != PBS_OK || status > PBS_ZST_UNSUPPORTED || out_len > cap) {
        std::fprintf(stderr, "FAIL: rc %d status %u out_len %zu cap %zu (frame of %zu bytes)\n", rc, status, out_len,
                     cap, len);
        ++failures;
    }
    not_ok += status != PBS_ZST_OK;
    std::free(out);
    std::free(frame);
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s <corpus directory>\n", argv[0]);
        return 2;
    }
    unsigned long files = 0;
    for (const auto& e : std::filesystem::directory_iterator(argv[1])) {
        const std::string name = e.path().filename().string();
        const size_t us = name.find('_'), dot = name.find(".zst");
        if (us == std::string::npos || dot == std::string::npos) continue;
        const size_t cap = std::strtoull(name.c_str() + us + 1, nullptr, 10);
        std::ifstream f(e.path(), std::ios::binary);
        const std::vector<char> buf((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        const uint8_t* p = reinterpret_cast<const uint8_t*>(buf.data());
        const size_t len = buf.size();
        ++files;
        run(p, len, cap);
        run(p, len, cap / 2);
        run(p, len, 0);
        for (size_t cut = 0; cut < len && cut < 96; ++cut) run(p, cut, cap);
        for (size_t back = 1; back <= 32 && back < len; ++back) run(p, len - back, cap);
    }
    if (files == 0) {
        std::fprintf(stderr, "no frames in %s\n", argv[1]);
        return 2;
    }
    std::printf("inflate_sanitize ok (%d failures): %lu frames, %lu calls, %lu not OK\n", failures, files, calls, not_ok);
    return failures ? 1 : 0;
}
