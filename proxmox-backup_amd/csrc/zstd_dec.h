// zstd frame format, reading side (RFC 8878), shared by the GPU inflater (pbs_inflate.hip)
// and its serial host mirror (pbs_zstd_inflate_host, the same file): every function here is
// PBS_HD, so the kernel and the mirror run the same code, and the mirror is what runs under
// the sanitizers (tests/cpp/inflate_sanitize.cpp).
//
// What is read: the frame header (magic, descriptor, window descriptor, dictionary id, every
// content-size width and its absence, single segment), block headers, the literals section
// header (four types, all size formats), the Huffman tree description (direct 4-bit weights
// and FSE-compressed weights with two interleaved states, last weight deduced, at most 11
// bits), the FSE table description (repeat-zero flags, the -1 "less than one" probabilities,
// accuracy limits 9 / 9 / 8, the RFC's spread step), the sequences header (three nbSeq
// encodings, four modes per table) and the sequence bitstream with the offset rule (repeat
// codes 1-3, the shift when the literal length is 0, "repeat 1 minus 1"; the repeat offsets
// start at 1, 4, 8 and carry across blocks).  The code baselines are zstd_enc.h's.
//
// Every reader takes an explicit end pointer (or a length) and returns an error rather than
// reading past it; every table index is masked or checked against the table's size before
// it is used, whatever the frame says.
#pragma once
#include "zstd_enc.h"

namespace pbs {
namespace zstd {
namespace dec {

// per-frame status (include/pbs_blob.h: PBS_ZST_*)
constexpr uint8_t kOk = 0, kBadFrame = 1, kTooLarge = 2, kUnsupported = 3;

constexpr uint64_t kWindowMax = 128ull << 20;  // libzstd's default limit and MAX_BLOB_SIZE
constexpr uint64_t kSizeUnknown = ~0ull;
constexpr int kHufMaxBits = 11;
constexpr uint32_t kHufTableSize = 1u << kHufMaxBits;
constexpr int kHufWeightLog = 6;  // accuracy limit of the FSE table of the Huffman weights
// a sequence regenerates at least 3 bytes and a block at most 128 KiB
constexpr uint32_t kMaxSeq = kBlockMax / 3;

PBS_HD inline uint32_t le16(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
PBS_HD inline uint32_t le24(const uint8_t* p) { return le16(p) | (uint32_t)p[2] << 16; }
PBS_HD inline uint32_t le32(const uint8_t* p) { return le24(p) | (uint32_t)p[3] << 24; }
PBS_HD inline uint64_t le64(const uint8_t* p) { return (uint64_t)le32(p) | (uint64_t)le32(p + 4) << 32; }

// ---- frame header (RFC 8878 3.1.1.1) --------------------------------------------------
struct FrameHeader {
    uint32_t size;     // bytes of the header, magic included
    uint64_t window;   // Window_Size (the content size for a single-segment frame)
    uint64_t content;  // Frame_Content_Size or kSizeUnknown
    bool checksum;     // a 4-byte Content_Checksum follows the last block
};

PBS_HD inline uint8_t parse_frame_header(const uint8_t* p, const uint8_t* end, FrameHeader* h) {
    if (end - p < 5) return kBadFrame;
    const uint32_t magic = le32(p);
    if ((magic & 0xFFFFFFF0u) == 0x184D2A50u) return kUnsupported;  // skippable frame
    if (magic != kMagic) return kBadFrame;
    const uint32_t d = p[4];
    const uint32_t fcs_flag = d >> 6, single = (d >> 5) & 1, did_flag = d & 3;
    if (d & 0x08) return kBadFrame;  // Reserved_Bit
    h->checksum = (d >> 2) & 1;
    const uint32_t did_len = did_flag == 3 ? 4 : did_flag;
    const uint32_t fcs_len = fcs_flag == 0 ? single : 1u << fcs_flag;
    const uint32_t size = 5 + (single ? 0 : 1) + did_len + fcs_len;
    if ((uint64_t)(end - p) < size) return kBadFrame;
    const uint8_t* q = p + 5;
    uint64_t window = 0;
    if (!single) {
        const uint32_t wd = *q++;
        const uint32_t wlog = 10 + (wd >> 3);
        if (wlog > 41) return kUnsupported;
        const uint64_t base = 1ull << wlog;
        window = base + (base >> 3) * (wd & 7);
    }
    uint32_t did = 0;
    for (uint32_t i = 0; i < did_len; ++i) did |= (uint32_t)q[i] << (8 * i);
    q += did_len;
    if (did != 0) return kUnsupported;
    uint64_t fcs = kSizeUnknown;
    if (fcs_len == 1) fcs = q[0];
    if (fcs_len == 2) fcs = (uint64_t)le16(q) + 256;
    if (fcs_len == 4) fcs = le32(q);
    if (fcs_len == 8) fcs = le64(q);
    if (single) window = fcs;
    if (window > kWindowMax) return kUnsupported;
    h->size = size;
    h->window = window;
    h->content = fcs;
    return kOk;
}

// ---- block header (3.1.1.2) ------------------------------------------------------------
struct BlockHeader {
    bool last;
    uint32_t type;  // 0 raw, 1 RLE, 2 compressed
    uint32_t size;  // Block_Size: bytes of the block's content (1 for RLE), or the run length for RLE
};

PBS_HD inline uint8_t parse_block_header(const uint8_t* p, const uint8_t* end, uint64_t block_max, BlockHeader* b) {
    if (end - p < 3) return kBadFrame;
    const uint32_t v = le24(p);
    b->last = v & 1;
    b->type = (v >> 1) & 3;
    b->size = v >> 3;
    if (b->type == 3) return kBadFrame;  // reserved
    if (b->size > block_max) return kBadFrame;
    const uint64_t content = b->type == 1 ? 1 : b->size;
    if ((uint64_t)(end - p) - 3 < content) return kBadFrame;
    // (libzstd refuses a compressed block under 3 bytes, the smallest it writes)
    if (b->type == 2 && b->size < 3) return kBadFrame;
    return kOk;
}

// ---- literals section header (3.1.1.3.1.1) ----------------------------------------------
struct LitHeader {
    uint32_t type;     // 0 raw, 1 RLE, 2 compressed, 3 treeless
    uint32_t regen;    // Regenerated_Size
    uint32_t comp;     // Compressed_Size (types 2, 3: tree description + streams)
    uint32_t streams;  // 1 or 4
    uint32_t size;     // bytes of this header
};

PBS_HD inline uint8_t parse_literals_header(const uint8_t* p, const uint8_t* end, LitHeader* h) {
    if (end - p < 1) return kBadFrame;
    const uint32_t b0 = p[0];
    const uint32_t type = b0 & 3, sf = (b0 >> 2) & 3;
    h->type = type;
    h->streams = 1;
    h->comp = 0;
    if (type < 2) {
        h->size = (sf & 1) == 0 ? 1 : sf == 1 ? 2 : 3;
        if ((uint64_t)(end - p) < h->size) return kBadFrame;
        h->regen = h->size == 1 ? b0 >> 3 : h->size == 2 ? le16(p) >> 4 : le24(p) >> 4;
    } else {
        h->size = sf < 2 ? 3 : sf + 2;
        if ((uint64_t)(end - p) < h->size) return kBadFrame;
        h->streams = sf == 0 ? 1 : 4;
        if (sf < 2) {
            const uint32_t v = le24(p);
            h->regen = (v >> 4) & 0x3FF;
            h->comp = v >> 14;
        } else if (sf == 2) {
            const uint32_t v = le32(p);
            h->regen = (v >> 4) & 0x3FFF;
            h->comp = v >> 18;
        } else {
            const uint64_t v = (uint64_t)le32(p) | (uint64_t)p[4] << 32;
            h->regen = (uint32_t)(v >> 4) & 0x3FFFF;
            h->comp = (uint32_t)(v >> 22);
        }
    }
    if (h->regen > kBlockMax || h->comp > kBlockMax) return kBadFrame;
    const uint64_t body = type == 0 ? h->regen : type == 1 ? 1 : h->comp;
    if ((uint64_t)(end - p) - h->size < body) return kBadFrame;
    return kOk;
}

// ---- backward bitstream (4.1) -------------------------------------------------------------
// The stream is [p, p + len); its last byte holds the end mark.  `pos` is the number of
// unread bits; bits below the stream's first are zeros (pos goes negative: the caller
// decides whether that is an error).
struct BitR {
    const uint8_t* p;
    int64_t pos;
    uint64_t w;  // unread bits, the next one at bit 63
    int avail;   // valid bits of w
};

// the 64 bits below bit `pos` of the stream, the next unread bit at bit 63 (at least 57 are
// valid; zeros below the stream's start).  Reads only [p, p + ceil(pos / 8)).
PBS_HD inline uint64_t bit_window(const uint8_t* p, int64_t pos) {
    if (pos <= 0) return 0;
    const int64_t e = (pos + 7) >> 3;  // the byte after the last one needed
    uint64_t l = 0;
    if (e >= 8) {
        l = le64(p + e - 8);
    } else {
        for (int64_t i = 0; i < e; ++i) l |= (uint64_t)p[i] << (8 * (8 - e + i));
    }
    return l << (8 * e - pos);
}

PBS_HD inline bool bitr_init(BitR* r, const uint8_t* p, uint64_t len) {
    if (len == 0 || p[len - 1] == 0) return false;
    r->p = p;
    r->pos = (int64_t)(len - 1) * 8 + (int64_t)highbit(p[len - 1]);
    r->w = bit_window(p, r->pos);
    r->avail = 57;
    return true;
}
PBS_HD inline void bitr_need(BitR* r, int n) {  // n <= 57
    if (r->avail < n) {
        r->w = bit_window(r->p, r->pos);
        r->avail = 57;
    }
}
PBS_HD inline uint32_t bitr_peek(const BitR* r, int n) {  // 0 <= n <= 32, after bitr_need
    return n ? (uint32_t)(r->w >> (64 - n)) : 0u;
}
PBS_HD inline void bitr_skip(BitR* r, int n) {
    r->w = n >= 64 ? 0 : r->w << n;
    r->avail -= n;
    r->pos -= n;
}
PBS_HD inline uint32_t bitr_read(BitR* r, int n) {
    bitr_need(r, n);
    const uint32_t v = bitr_peek(r, n);
    bitr_skip(r, n);
    return v;
}

// ---- FSE table description (4.1.1) --------------------------------------------------------
// `norm[0 .. *nsym)` (-1: "less than one"), the accuracy log and the bytes read.  `max_sym`:
// the alphabet's last symbol (35 / 31 / 52, 255 for Huffman weights).
PBS_HD inline uint8_t read_ncount(const uint8_t* p, const uint8_t* end, int max_log, uint32_t max_sym, int16_t* norm,
                                  uint32_t* nsym, int* log, uint32_t* used) {
    const uint64_t nbits = (uint64_t)(end - p) * 8;
    uint64_t at = 0;  // bit position, forward, least significant bit first
    auto get = [&](int n, uint32_t* v) -> bool {  // n <= 16
        if (at + (uint64_t)n > nbits) return false;
        uint32_t x = 0;
        const uint64_t b = at >> 3;
        for (int i = 0; i < 3 && b + i < (uint64_t)(end - p); ++i) x |= (uint32_t)p[b + i] << (8 * i);
        *v = (x >> (at & 7)) & ((1u << n) - 1);
        return true;
    };
    uint32_t v;
    if (!get(4, &v)) return kBadFrame;
    at += 4;
    const int alog = (int)v + 5;
    if (alog > max_log) return kBadFrame;
    int32_t remaining = 1 << alog;
    uint32_t s = 0;
    while (remaining > 0 && s <= max_sym) {
        const int bits = (int)highbit((uint32_t)remaining + 1) + 1;
        // the last bit may lie past the end when the short form is taken
        uint32_t val;
        if (!get(bits - 1, &val)) return kBadFrame;
        const uint32_t lower = (1u << (bits - 1)) - 1;
        const uint32_t threshold = (1u << bits) - 1 - ((uint32_t)remaining + 1);
        if ((val & lower) < threshold) {
            at += bits - 1;
        } else {
            if (!get(bits, &val)) return kBadFrame;
            at += bits;
            if (val > lower) val -= threshold;
        }
        const int32_t proba = (int32_t)val - 1;
        remaining -= proba < 0 ? 1 : proba;
        norm[s++] = (int16_t)proba;
        if (proba == 0) {
            for (;;) {
                uint32_t rep;
                if (!get(2, &rep)) return kBadFrame;
                at += 2;
                for (uint32_t i = 0; i < rep; ++i) {
                    if (s > max_sym) return kBadFrame;
                    norm[s++] = 0;
                }
                if (rep != 3) break;
            }
        }
    }
    if (remaining != 0) return kBadFrame;
    *nsym = s;
    *log = alog;
    *used = (uint32_t)((at + 7) >> 3);
    return kOk;
}

// Decoding table entry: symbol | bits << 8 | baseline << 16.
// `table` has 1 << log entries; `next` is scratch of nsym entries.
PBS_HD inline uint8_t build_fse_table(const int16_t* norm, uint32_t nsym, int log, uint32_t* table, uint16_t* next) {
    const uint32_t size = 1u << log, mask = size - 1;
    uint32_t high = size;
    uint32_t total = 0;
    for (uint32_t s = 0; s < nsym; ++s) {
        total += norm[s] < 0 ? 1u : (uint32_t)norm[s];
        if (norm[s] == -1) {
            if (high == 0) return kBadFrame;
            table[--high] = s;
            next[s] = 1;
        } else {
            next[s] = (uint16_t)norm[s];
        }
    }
    if (total != size) return kBadFrame;
    const uint32_t step = (size >> 1) + (size >> 3) + 3;
    uint32_t pos = 0;
    for (uint32_t s = 0; s < nsym; ++s)
        for (int i = 0; i < norm[s]; ++i) {
            table[pos] = s;
            // (total == size bounds the walk: every cell below `high` is visited once)
            do pos = (pos + step) & mask;
            while (pos >= high);
        }
    if (pos != 0) return kBadFrame;
    for (uint32_t i = 0; i < size; ++i) {
        const uint32_t s = table[i];
        const uint32_t x = next[s]++;
        const uint32_t nb = (uint32_t)log - highbit(x);
        table[i] = s | nb << 8 | ((x << nb) - size) << 16;
    }
    return kOk;
}
PBS_HD inline uint32_t fse_sym(uint32_t e) { return e & 0xFF; }
PBS_HD inline int fse_nb(uint32_t e) { return (int)((e >> 8) & 0xFF); }
PBS_HD inline uint32_t fse_base(uint32_t e) { return e >> 16; }

// ---- Huffman tree description (4.2.1) -----------------------------------------------------
// Reads the transmitted weights of [p, end) into w[0 .. *nw) (w holds 256; the deduced last
// weight is added by build_huf_table) and returns the bytes of the description.  `fse`:
// scratch of 64 entries, `next` of 16.
PBS_HD inline uint8_t read_huf_weights(const uint8_t* p, const uint8_t* end, uint8_t* w, uint32_t* nw, uint32_t* used,
                                       uint32_t* fse, uint16_t* next) {
    if (end - p < 1) return kBadFrame;
    const uint32_t hb = p[0];
    uint32_t n = 0;
    if (hb >= 128) {  // direct: 4 bits per weight
        n = hb - 127;
        const uint32_t bytes = (n + 1) / 2;
        if ((uint64_t)(end - p) - 1 < bytes) return kBadFrame;
        for (uint32_t i = 0; i < n; ++i) w[i] = (i & 1) ? p[1 + i / 2] & 15 : p[1 + i / 2] >> 4;
        *used = 1 + bytes;
    } else {  // FSE-compressed, two interleaved states
        if (hb == 0 || (uint64_t)(end - p) - 1 < hb) return kBadFrame;
        const uint8_t* const q = p + 1;
        int16_t norm[16];
        uint32_t nsym, hdr;
        int log;
        // weights 0 .. 11: anything above is no valid weight
        const uint8_t r = read_ncount(q, q + hb, kHufWeightLog, kHufMaxBits, norm, &nsym, &log, &hdr);
        if (r != kOk) return r;
        if (build_fse_table(norm, nsym, log, fse, next) != kOk) return kBadFrame;
        BitR br;
        if (hdr >= hb || !bitr_init(&br, q + hdr, hb - hdr)) return kBadFrame;
        const uint32_t mask = (1u << log) - 1;
        uint32_t s1 = bitr_read(&br, log), s2 = bitr_read(&br, log);
        if (br.pos < 0) return kBadFrame;
        for (;;) {
            if (n > 253) return kBadFrame;
            const uint32_t e1 = fse[s1 & mask];
            w[n++] = (uint8_t)fse_sym(e1);
            s1 = fse_base(e1) + bitr_read(&br, fse_nb(e1));
            if (br.pos < 0) {
                w[n++] = (uint8_t)fse_sym(fse[s2 & mask]);
                break;
            }
            const uint32_t e2 = fse[s2 & mask];
            w[n++] = (uint8_t)fse_sym(e2);
            s2 = fse_base(e2) + bitr_read(&br, fse_nb(e2));
            if (br.pos < 0) {
                w[n++] = (uint8_t)fse_sym(fse[s1 & mask]);
                break;
            }
        }
        *used = 1 + hb;
    }
    *nw = n;
    return kOk;
}

// The decoding table of the weights w[0 .. n) plus the deduced last one (written to w[n]):
// entry = symbol | bits << 8; 1 << *max_bits of them, at most 2^11.
PBS_HD inline uint8_t build_huf_table(uint8_t* w, uint32_t n, uint16_t* table, int* max_bits) {
    if (n == 0 || n > 255) return kBadFrame;
    // the last weight completes the sum to a power of two
    uint32_t total = 0, ones = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (w[i] > kHufMaxBits) return kBadFrame;
        if (w[i]) total += 1u << (w[i] - 1);
        ones += w[i] == 1;
    }
    if (total == 0) return kBadFrame;
    const int mb = (int)highbit(total) + 1;
    if (mb > kHufMaxBits) return kBadFrame;
    const uint32_t rest = (1u << mb) - total;
    if (rest & (rest - 1)) return kBadFrame;
    w[n] = (uint8_t)(highbit(rest) + 1);
    ones += w[n] == 1;
    ++n;
    if (ones < 2 || (ones & 1)) return kBadFrame;  // (as libzstd: an odd count cannot fill the table)
    // symbols in order of weight, then of value: the lowest weights take the lowest cells
    uint32_t start[kHufMaxBits + 2];
    for (int k = 0; k <= kHufMaxBits + 1; ++k) start[k] = 0;
    for (uint32_t i = 0; i < n; ++i) start[w[i] + 1u] += w[i] ? 1u << (w[i] - 1) : 0u;
    start[1] = 0;
    for (int k = 2; k <= kHufMaxBits + 1; ++k) start[k] += start[k - 1];
    for (uint32_t i = 0; i < n; ++i) {
        if (!w[i]) continue;
        const uint32_t cnt = 1u << (w[i] - 1), at = start[w[i]];
        if (at + cnt > (1u << mb)) return kBadFrame;
        const uint16_t e = (uint16_t)(i | (uint32_t)(mb + 1 - w[i]) << 8);
        for (uint32_t k = 0; k < cnt; ++k) table[at + k] = e;
        start[w[i]] = at + cnt;
    }
    *max_bits = mb;
    return kOk;
}

// One Huffman stream [p, p + len) into dst[0 .. n): every bit must be used, none more.
PBS_HD inline uint8_t huf_decode_stream(const uint8_t* p, uint64_t len, const uint16_t* table, int max_bits,
                                        uint8_t* dst, uint32_t n) {
    BitR br;
    if (!bitr_init(&br, p, len)) return kBadFrame;
    const uint32_t mask = (1u << max_bits) - 1;
    for (uint32_t i = 0; i < n; ++i) {
        bitr_need(&br, max_bits);
        const uint32_t e = table[bitr_peek(&br, max_bits) & mask];
        bitr_skip(&br, (int)(e >> 8));
        dst[i] = (uint8_t)e;
        if (br.pos < 0) return kBadFrame;
    }
    return br.pos == 0 ? kOk : kBadFrame;
}

// The spans of the Huffman streams of a compressed literals section: `body` = the bytes
// after the tree description, `regen` symbols in all.
struct HufStreams {
    uint32_t off[4], len[4], dst[4], cnt[4];
};
PBS_HD inline uint8_t split_huf_streams(const uint8_t* body, uint32_t body_len, uint32_t streams, uint32_t regen,
                                        HufStreams* s) {
    for (int k = 0; k < 4; ++k) s->off[k] = s->len[k] = s->dst[k] = s->cnt[k] = 0;
    if (streams == 1) {
        s->len[0] = body_len;
        s->cnt[0] = regen;
        return body_len ? kOk : kBadFrame;
    }
    if (body_len < 10) return kBadFrame;  // jump table and one byte per stream
    const uint32_t l0 = le16(body), l1 = le16(body + 2), l2 = le16(body + 4);
    if ((uint64_t)6 + l0 + l1 + l2 >= body_len) return kBadFrame;
    const uint32_t seg = (regen + 3) / 4;
    if (3 * seg > regen) return kBadFrame;
    s->off[0] = 6;
    s->len[0] = l0;
    s->off[1] = 6 + l0;
    s->len[1] = l1;
    s->off[2] = 6 + l0 + l1;
    s->len[2] = l2;
    s->off[3] = 6 + l0 + l1 + l2;
    s->len[3] = body_len - s->off[3];
    for (uint32_t k = 0; k < 4; ++k) {
        s->dst[k] = k * seg;
        s->cnt[k] = k < 3 ? seg : regen - 3 * seg;
        if (s->len[k] == 0) return kBadFrame;
    }
    return kOk;
}

// ---- sequences section (3.1.1.3.2) --------------------------------------------------------
struct SeqHeader {
    uint32_t nseq;
    uint32_t mode[3];  // LL, OF, ML: 0 predefined, 1 RLE, 2 FSE-compressed, 3 repeat
    uint32_t size;     // bytes of the header (count + modes byte)
};

PBS_HD inline uint8_t parse_seq_header(const uint8_t* p, const uint8_t* end, SeqHeader* h) {
    if (end - p < 1) return kBadFrame;
    const uint32_t b0 = p[0];
    h->mode[0] = h->mode[1] = h->mode[2] = 0;
    if (b0 == 0) {
        h->nseq = 0;
        h->size = 1;
        // (nothing may follow: the block ends here)
        return end - p == 1 ? kOk : kBadFrame;
    }
    uint32_t n, sz;
    if (b0 < 128) {
        n = b0;
        sz = 1;
    } else if (b0 < 255) {
        if (end - p < 2) return kBadFrame;
        n = ((b0 - 128) << 8) + p[1];
        sz = 2;
    } else {
        if (end - p < 3) return kBadFrame;
        n = le16(p + 1) + 0x7F00;
        sz = 3;
    }
    if ((uint64_t)(end - p) < sz + 1) return kBadFrame;
    const uint32_t m = p[sz];
    if (m & 3) return kBadFrame;  // reserved
    h->mode[0] = m >> 6;
    h->mode[1] = (m >> 4) & 3;
    h->mode[2] = (m >> 2) & 3;
    h->nseq = n;
    h->size = sz + 1;
    if (n > kMaxSeq) return kBadFrame;
    return kOk;
}

// The description of one of a block's three tables (`which`: 0 LL, 1 OF, 2 ML), read from
// `p` as its mode says: the normalised counts for FSE_Compressed_Mode, the symbol (norm[0])
// for RLE_Mode, nothing otherwise.  Returns the bytes used.
struct SeqTableDesc {
    int16_t norm[56];
    uint32_t nsym;
    int log;
};
PBS_HD inline uint8_t read_seq_table_desc(int which, uint32_t mode, const uint8_t* p, const uint8_t* end,
                                          SeqTableDesc* d, uint32_t* used) {
    const uint32_t max_sym = which == 0 ? 35u : which == 1 ? 31u : 52u;
    *used = 0;
    if (mode == 1) {
        if (end - p < 1 || p[0] > max_sym) return kBadFrame;
        d->norm[0] = (int16_t)p[0];
        *used = 1;
    } else if (mode == 2) {
        const int max_log = which == 0 ? kLLMaxLog : which == 1 ? kOFMaxLog : kMLMaxLog;
        return read_ncount(p, end, max_log, max_sym, d->norm, &d->nsym, &d->log, used);
    }
    return kOk;
}
// The table itself (512 / 256 / 512 entries) from the description; *log persists across the
// frame's blocks, and Repeat_Mode (3) leaves table and log as they are.  `next`: scratch of 64.
PBS_HD inline uint8_t build_seq_table(int which, uint32_t mode, const SeqTableDesc* d, uint32_t* table, int* log,
                                      uint16_t* next) {
    if (mode == 3) return kOk;
    if (mode == 1) {
        table[0] = (uint32_t)d->norm[0];  // 0 bits, baseline 0
        *log = 0;
        return kOk;
    }
    if (mode == 0) {
        const int16_t* const norm = which == 0 ? kLLNorm : which == 1 ? kOFNorm : kMLNorm;
        const uint32_t n = which == 0 ? 36u : which == 1 ? 29u : 53u;
        *log = which == 0 ? kLLLog : which == 1 ? kOFLog : kMLLog;
        return build_fse_table(norm, n, *log, table, next);
    }
    *log = d->log;
    return build_fse_table(d->norm, d->nsym, d->log, table, next);
}

// Everything a compressed block's headers say, found in one serial pass over them (short:
// the table builds, the Huffman streams and the sequence stream, which are the long chains,
// come afterwards and may run side by side).
struct BlockDesc {
    LitHeader lit;
    const uint8_t* lit_body;  // raw bytes, the RLE byte, or the Huffman streams (after the tree)
    uint32_t lit_body_len;
    HufStreams hs;
    uint32_t nw;     // transmitted weights (type 2)
    uint8_t w[256];
    SeqHeader sh;
    SeqTableDesc td[3];
    const uint8_t* seq;  // the sequence bitstream
    uint32_t seq_len;
};

// [p, end) is the block's content.  `huf_valid` / `seq_valid[3]`: whether an earlier block of
// the frame left a Huffman tree / each sequence table (treeless literals and Repeat_Mode
// need them); updated for the next block.
PBS_HD inline uint8_t parse_block_desc(const uint8_t* p, const uint8_t* end, uint64_t block_max, bool* huf_valid,
                                       bool* seq_valid, BlockDesc* d, uint32_t* fse, uint16_t* next) {
    uint8_t r = parse_literals_header(p, end, &d->lit);
    if (r != kOk) return r;
    if (d->lit.regen > block_max) return kBadFrame;
    const uint8_t* q = p + d->lit.size;
    d->nw = 0;
    if (d->lit.type < 2) {
        d->lit_body = q;
        d->lit_body_len = d->lit.type == 0 ? d->lit.regen : 1;
        q += d->lit_body_len;
    } else {
        const uint8_t* const lend = q + d->lit.comp;
        uint32_t used = 0;
        if (d->lit.type == 2) {
            r = read_huf_weights(q, lend, d->w, &d->nw, &used, fse, next);
            if (r != kOk) return r;
            *huf_valid = true;
        } else if (!*huf_valid) {
            return kBadFrame;
        }
        d->lit_body = q + used;
        d->lit_body_len = d->lit.comp - used;
        r = split_huf_streams(d->lit_body, d->lit_body_len, d->lit.streams, d->lit.regen, &d->hs);
        if (r != kOk) return r;
        q = lend;
    }
    r = parse_seq_header(q, end, &d->sh);
    if (r != kOk) return r;
    q += d->sh.size;
    d->seq = q;
    d->seq_len = 0;
    if (d->sh.nseq == 0) return kOk;
    for (int k = 0; k < 3; ++k) {
        const uint32_t mode = d->sh.mode[k];
        if (mode == 3) {
            if (!seq_valid[k]) return kBadFrame;
            continue;
        }
        uint32_t used = 0;
        r = read_seq_table_desc(k, mode, q, end, &d->td[k], &used);
        if (r != kOk) return r;
        seq_valid[k] = true;
        q += used;
    }
    if (q >= end) return kBadFrame;
    d->seq = q;
    d->seq_len = (uint32_t)(end - q);
    return kOk;
}

// One decoded sequence, positions relative to the block: the literal run starts at `dst` in
// the block's output and at `lit` in its literals; its length is the next entry's `lit`
// less this one's; the match of `ml` bytes at distance `off` follows it.  Entry nseq closes
// the list: {output bytes of the sequences, literals used, 0, 0}.
struct Seq {
    uint32_t dst, lit, ml, off;
};

// The sequence bitstream [p, p + len) into seq[0 .. nseq]; `rep` (the three repeat offsets)
// is updated only when the block is good.  `produced`: content bytes before this block (an
// offset reaching before the frame's first byte is an error); `lit_size`: the block's
// literals; *block_out: the block's regenerated size, last literals included.
PBS_HD inline uint8_t decode_sequences(const uint8_t* p, uint64_t len, uint32_t nseq, const uint32_t* ll_t, int ll_log,
                                       const uint32_t* of_t, int of_log, const uint32_t* ml_t, int ml_log,
                                       uint32_t* rep, uint64_t produced, uint32_t lit_size, Seq* seq,
                                       uint32_t* block_out) {
    BitR br;
    if (!bitr_init(&br, p, len)) return kBadFrame;
    const uint32_t ll_m = (1u << ll_log) - 1, of_m = (1u << of_log) - 1, ml_m = (1u << ml_log) - 1;
    uint32_t ll_s = bitr_read(&br, ll_log);
    uint32_t of_s = bitr_read(&br, of_log);
    uint32_t ml_s = bitr_read(&br, ml_log);
    if (br.pos < 0) return kBadFrame;
    uint32_t r1 = rep[0], r2 = rep[1], r3 = rep[2];
    uint32_t dst = 0, lit = 0;
    for (uint32_t i = 0; i < nseq; ++i) {
        const uint32_t le = ll_t[ll_s & ll_m], oe = of_t[of_s & of_m], me = ml_t[ml_s & ml_m];
        const uint32_t lc = fse_sym(le), oc = fse_sym(oe), mc = fse_sym(me);
        if (lc > 35 || oc > 31 || mc > 52) return kBadFrame;
        const uint64_t ov = (1ull << oc) + bitr_read(&br, (int)oc);
        const uint32_t ml = ml_base(mc) + bitr_read(&br, (int)ml_bits(mc));
        const uint32_t ll = ll_base(lc) + bitr_read(&br, (int)ll_bits(lc));
        if (br.pos < 0) return kBadFrame;
        uint64_t off;
        if (ov > 3) {
            off = ov - 3;
            r3 = r2;
            r2 = r1;
            r1 = (uint32_t)off;
        } else {
            const uint32_t idx = (uint32_t)ov - 1 + (ll == 0 ? 1u : 0u);  // 0 .. 3
            if (idx == 0) {
                off = r1;
            } else {
                off = idx == 1 ? r2 : idx == 2 ? r3 : r1 - 1;
                if (off == 0) return kBadFrame;
                if (idx != 1) r3 = r2;
                r2 = r1;
                r1 = (uint32_t)off;
            }
        }
        if (off > kWindowMax) return kBadFrame;
        seq[i].dst = dst;
        seq[i].lit = lit;
        seq[i].ml = ml;
        seq[i].off = (uint32_t)off;
        if (ll > lit_size - lit) return kBadFrame;
        lit += ll;
        dst += ll;
        if (off > produced + dst) return kBadFrame;  // before the frame's first byte
        if (dst > kBlockMax || ml > kBlockMax - dst) return kBadFrame;  // a block regenerates at most 128 KiB
        dst += ml;
        if (i + 1 < nseq) {
            ll_s = fse_base(le) + bitr_read(&br, fse_nb(le));
            ml_s = fse_base(me) + bitr_read(&br, fse_nb(me));
            of_s = fse_base(oe) + bitr_read(&br, fse_nb(oe));
            if (br.pos < 0) return kBadFrame;
        }
    }
    if (br.pos != 0) return kBadFrame;  // 3.1.1.3.2.1.1: the stream is used up exactly
    seq[nseq].dst = dst;
    seq[nseq].lit = lit;
    seq[nseq].ml = 0;
    seq[nseq].off = 0;
    const uint32_t total = dst + (lit_size - lit);
    if (total > kBlockMax) return kBadFrame;
    *block_out = total;
    rep[0] = r1;
    rep[1] = r2;
    rep[2] = r3;
    return kOk;
}

// ---- frame-level rules shared by the kernel and the mirror ---------------------------------
// Whether a block regenerating `block_out` bytes after `produced` may be written: into a slot
// of `cap` bytes, within the block limit and the header's content size.
PBS_HD inline uint8_t block_fits(uint32_t block_out, uint64_t produced, uint64_t cap, uint64_t block_max,
                                 uint64_t content) {
    if (block_out > block_max) return kBadFrame;
    if (block_out > cap - produced) return kTooLarge;
    if (content != kSizeUnknown && block_out > content - produced) return kBadFrame;
    return kOk;
}

// After the last block at `p`: the optional checksum field (consumed, not verified), the
// content size, and whatever follows the frame.
PBS_HD inline uint8_t frame_end_status(const uint8_t* p, const uint8_t* end, const FrameHeader& fh,
                                       uint64_t produced) {
    if (fh.checksum) {
        if (end - p < 4) return kBadFrame;
        p += 4;
    }
    if (fh.content != kSizeUnknown && produced != fh.content) return kBadFrame;
    if (p == end) return kOk;
    if (end - p >= 4) {
        const uint32_t magic = le32(p);
        if (magic == kMagic || (magic & 0xFFFFFFF0u) == 0x184D2A50u) return kUnsupported;  // another frame
    }
    return kBadFrame;
}

}  // namespace dec
}  // namespace zstd
}  // namespace pbs
