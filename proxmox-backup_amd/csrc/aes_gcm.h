// AES-256 and GF(2^128) helpers shared by the host side of the crypt config and the GCM
// kernels (pbs_crypt.hip): what `Crypter::new(aes_256_gcm, Encrypt, key, Some(iv16))` with
// empty AAD computes (NIST SP 800-38D; pbs-datastore/src/data_blob.rs:107-131 calls it
// through pbs-tools/src/crypt_config.rs:127-150).
//
// A GCM block is kept as B128: `hi` = bytes 0..7 and `lo` = bytes 8..15, both read big
// endian, so the field's x^0 is bit 63 of `hi` and multiplying by x is a right shift.
// AES state words are the big-endian columns of FIPS 197; the round function is the one
// 256-entry table Te0[x] = {02,01,01,03} * S[x] with the other three columns by rotation
// and the last round's S-box from Te0's second byte.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PBS_HD __host__ __device__ __forceinline__
#else
#define PBS_HD inline
#endif

namespace pbs {
namespace gcm {

struct B128 {
    uint64_t hi, lo;
};

// x * y in GF(2^128), GCM bit order (SP 800-38D algorithm 1), constant time
PBS_HD B128 gf_mul(B128 x, B128 y) {
    uint64_t zh = 0, zl = 0, vh = y.hi, vl = y.lo;
    for (int half = 0; half < 2; ++half) {
        uint64_t xb = half ? x.lo : x.hi;
        for (int i = 0; i < 64; ++i) {
            const uint64_t m = 0 - (xb >> 63);
            xb <<= 1;
            zh ^= vh & m;
            zl ^= vl & m;
            const uint64_t c = 0 - (vl & 1);
            vl = (vl >> 1) | (vh << 63);
            vh = (vh >> 1) ^ (c & 0xE100000000000000ull);
        }
    }
    return B128{zh, zl};
}

PBS_HD B128 gf_xor(B128 a, B128 b) { return B128{a.hi ^ b.hi, a.lo ^ b.lo}; }

PBS_HD uint64_t load_be64(const uint8_t* p) {
    uint64_t v = 0;
    for (int i = 0; i < 8; ++i) v = v << 8 | p[i];
    return v;
}
PBS_HD void store_be64(uint8_t* p, uint64_t v) {
    for (int i = 0; i < 8; ++i) p[i] = (uint8_t)(v >> (56 - 8 * i));
}
PBS_HD B128 load_block(const uint8_t* p) { return B128{load_be64(p), load_be64(p + 8)}; }
PBS_HD void store_block(uint8_t* p, B128 v) {
    store_be64(p, v.hi);
    store_be64(p + 8, v.lo);
}

// J0 of a 16-byte IV: GHASH_H(IV || 0^64 || [128]_64) = ((IV * H) ^ 128) * H
PBS_HD B128 j0_of_iv16(B128 iv, B128 h) {
    B128 y = gf_mul(iv, h);
    y.lo ^= 128;
    return gf_mul(y, h);
}

PBS_HD uint32_t ror32(uint32_t v, int r) { return (v >> r) | (v << (32 - r)); }

// One AES-256 block: `s` = the four big-endian columns, in place.  `te0(x)` returns Te0[x].
template <class Te0>
PBS_HD void aes256_encrypt(const uint32_t* rk, const Te0& te0, uint32_t s[4]) {
    uint32_t s0 = s[0] ^ rk[0], s1 = s[1] ^ rk[1], s2 = s[2] ^ rk[2], s3 = s[3] ^ rk[3];
#pragma unroll
    for (int r = 1; r < 14; ++r) {
        const uint32_t t0 = te0(s0 >> 24) ^ ror32(te0((s1 >> 16) & 255), 8) ^ ror32(te0((s2 >> 8) & 255), 16) ^
                            ror32(te0(s3 & 255), 24) ^ rk[4 * r];
        const uint32_t t1 = te0(s1 >> 24) ^ ror32(te0((s2 >> 16) & 255), 8) ^ ror32(te0((s3 >> 8) & 255), 16) ^
                            ror32(te0(s0 & 255), 24) ^ rk[4 * r + 1];
        const uint32_t t2 = te0(s2 >> 24) ^ ror32(te0((s3 >> 16) & 255), 8) ^ ror32(te0((s0 >> 8) & 255), 16) ^
                            ror32(te0(s1 & 255), 24) ^ rk[4 * r + 2];
        const uint32_t t3 = te0(s3 >> 24) ^ ror32(te0((s0 >> 16) & 255), 8) ^ ror32(te0((s1 >> 8) & 255), 16) ^
                            ror32(te0(s2 & 255), 24) ^ rk[4 * r + 3];
        s0 = t0;
        s1 = t1;
        s2 = t2;
        s3 = t3;
    }
    // last round: SubBytes + ShiftRows + AddRoundKey; S[x] is Te0[x]'s second byte
    const uint32_t m1 = 0x0000FF00u;
    s[0] = ((te0(s0 >> 24) & m1) << 16 | (te0((s1 >> 16) & 255) & m1) << 8 | (te0((s2 >> 8) & 255) & m1) |
            (te0(s3 & 255) & m1) >> 8) ^ rk[56];
    s[1] = ((te0(s1 >> 24) & m1) << 16 | (te0((s2 >> 16) & 255) & m1) << 8 | (te0((s3 >> 8) & 255) & m1) |
            (te0(s0 & 255) & m1) >> 8) ^ rk[57];
    s[2] = ((te0(s2 >> 24) & m1) << 16 | (te0((s3 >> 16) & 255) & m1) << 8 | (te0((s0 >> 8) & 255) & m1) |
            (te0(s1 & 255) & m1) >> 8) ^ rk[58];
    s[3] = ((te0(s3 >> 24) & m1) << 16 | (te0((s0 >> 16) & 255) & m1) << 8 | (te0((s1 >> 8) & 255) & m1) |
            (te0(s2 & 255) & m1) >> 8) ^ rk[59];
}

// Te0 from a plain array (host, and the device's rare per-blob blocks)
struct Te0Array {
    const uint32_t* t;
    PBS_HD uint32_t operator()(uint32_t x) const { return t[x]; }
};

// ---- host only: tables and the key schedule

inline uint8_t xtime(uint8_t v) { return (uint8_t)((v << 1) ^ ((v & 0x80) ? 0x1B : 0)); }

// S-box by the field inverse and the affine map (FIPS 197 5.1.1), then Te0
inline void make_te0(uint32_t te0[256]) {
    uint8_t sbox[256];
    uint8_t p = 1, q = 1;
    do {
        p = (uint8_t)(p ^ xtime(p));  // p *= 3
        q ^= (uint8_t)(q << 1);       // q /= 3
        q ^= (uint8_t)(q << 2);
        q ^= (uint8_t)(q << 4);
        if (q & 0x80) q ^= 0x09;
        const uint8_t r = (uint8_t)(q ^ (uint8_t)(q << 1 | q >> 7) ^ (uint8_t)(q << 2 | q >> 6) ^
                                    (uint8_t)(q << 3 | q >> 5) ^ (uint8_t)(q << 4 | q >> 4));
        sbox[p] = (uint8_t)(r ^ 0x63);
    } while (p != 1);
    sbox[0] = 0x63;
    for (int x = 0; x < 256; ++x) {
        const uint8_t s = sbox[x], s2 = xtime(s);
        te0[x] = (uint32_t)s2 << 24 | (uint32_t)s << 16 | (uint32_t)s << 8 | (uint32_t)(uint8_t)(s2 ^ s);
    }
}

// FIPS 197 5.2 for Nk = 8: 60 words
inline void aes256_expand_key(const uint8_t key[32], const uint32_t te0[256], uint32_t rk[60]) {
    auto sub = [&](uint32_t w) {
        return ((te0[w >> 24] >> 8) & 255) << 24 | ((te0[(w >> 16) & 255] >> 8) & 255) << 16 |
               ((te0[(w >> 8) & 255] >> 8) & 255) << 8 | ((te0[w & 255] >> 8) & 255);
    };
    for (int i = 0; i < 8; ++i)
        rk[i] = (uint32_t)key[4 * i] << 24 | (uint32_t)key[4 * i + 1] << 16 | (uint32_t)key[4 * i + 2] << 8 |
                key[4 * i + 3];
    uint32_t rcon = 1;
    for (int i = 8; i < 60; ++i) {
        uint32_t t = rk[i - 1];
        if (i % 8 == 0) {
            t = sub(t << 8 | t >> 24) ^ rcon << 24;
            rcon = xtime((uint8_t)rcon);
        } else if (i % 8 == 4) {
            t = sub(t);
        }
        rk[i] = rk[i - 8] ^ t;
    }
}

}  // namespace gcm
}  // namespace pbs
