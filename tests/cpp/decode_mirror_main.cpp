// The read side of the C++ host mirror (proxmox-backup_amd/host/pbs_chunker.hpp) on the host:
// reads one blob image as hex on the command line (argv[1]; "-" for the empty blob), an
// optional expected digest (argv[2], 64 hex digits or "-") and size (argv[3] or "-"), opens it
// under the key [1; 32] and prints kind, status and the payload; then seals and opens `len`
// bytes through CryptConfig (tests/test_decode_mirror_cpp.py compares with the reference).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "pbs_chunker.hpp"

static std::vector<uint8_t> unhex(const char* s) {
    std::vector<uint8_t> v;
    if (std::strcmp(s, "-") == 0) return v;
    for (size_t i = 0; s[i] && s[i + 1]; i += 2) v.push_back((uint8_t)std::stoul(std::string(s + i, 2), nullptr, 16));
    return v;
}

static void hex(const char* tag, const uint8_t* p, size_t n) {
    std::printf("%s ", tag);
    for (size_t i = 0; i < n; ++i) std::printf("%02x", p[i]);
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::vector<uint8_t> blob = unhex(argv[1]);
    std::array<uint8_t, 32> key;
    key.fill(1);
    pbs::CryptConfig cfg(key);
    pbs::Digest dig;
    const pbs::Digest* dp = nullptr;
    if (argc > 2 && std::strcmp(argv[2], "-") != 0) {
        const std::vector<uint8_t> d = unhex(argv[2]);
        if (d.size() != 32) return 2;
        std::memcpy(dig.data(), d.data(), 32);
        dp = &dig;
    }
    uint64_t size = 0;
    const uint64_t* sp = nullptr;
    if (argc > 3 && std::strcmp(argv[3], "-") != 0) {
        size = std::strtoull(argv[3], nullptr, 0);
        sp = &size;
    }
    const pbs::DecodedBlob r = pbs::blob_decode_host(blob.data(), blob.size(), &cfg, dp, sp);
    std::printf("kind %u\nstatus %u\n", (unsigned)r.kind, (unsigned)r.status);
    hex("payload", r.payload.data(), r.payload.size());
    const pbs::DecodedBlob nc = pbs::blob_decode_host(blob.data(), blob.size());
    std::printf("status_without_config %u\n", (unsigned)nc.status);

    // seal, open, and open with one tag bit flipped
    std::array<uint8_t, 16> iv, tag;
    for (int i = 0; i < 16; ++i) iv[i] = (uint8_t)(0x40 + i);
    std::vector<uint8_t> data(77);
    for (size_t i = 0; i < data.size(); ++i) data[i] = (uint8_t)(i % 255);
    const std::vector<uint8_t> ct = cfg.encrypt_host(iv, data.data(), data.size(), tag);
    bool ok = false;
    const std::vector<uint8_t> back = cfg.decrypt_host(iv, ct.data(), ct.size(), tag, ok);
    std::printf("roundtrip %d\n", ok && back == data ? 1 : 0);
    tag[5] ^= 0x10;
    const std::vector<uint8_t> none = cfg.decrypt_host(iv, ct.data(), ct.size(), tag, ok);
    std::printf("forged %d\n", !ok && none.empty() ? 1 : 0);
    return 0;
}
