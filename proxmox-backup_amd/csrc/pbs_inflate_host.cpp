// pbs_zstd_inflate_host: the serial zstd decoder over zstd_dec.h -- the mirror the GPU
// inflater (pbs_inflate.hip) is compared against, and what runs under the sanitizers
// (tests/cpp/inflate_sanitize.cpp).  Plain host C++, no device pass.  Not a fast path.
//
// The order of checks is the kernel's: a block is parsed and checked completely (headers,
// tables, literals, the whole sequence stream, the slot's capacity) before its first byte is
// written, so both stop at the same block with the same status and the same bytes.
#include <cstring>
#include <vector>

#include "pbs_blob.h"
#include "pbs_chunker.h"
#include "zstd_dec.h"

using namespace pbs::zstd;
using namespace pbs::zstd::dec;

extern "C" int pbs_zstd_frame_content_size(const uint8_t* frame, size_t len, uint64_t* size) {
    if (!frame || !size) return PBS_ERR_ARG;
    FrameHeader fh;
    if (parse_frame_header(frame, frame + len, &fh) != kOk) return PBS_ERR_ARG;
    *size = fh.content;
    return PBS_OK;
}

extern "C" int pbs_zstd_inflate_host(const uint8_t* frame, size_t len, uint8_t* out, size_t cap, size_t* out_len,
                                     uint8_t* status) {
    if (!out_len || !status || (len && !frame) || (cap && !out)) return PBS_ERR_ARG;
    *out_len = 0;
    const uint8_t* const end = frame + len;
    FrameHeader fh;
    uint8_t r = parse_frame_header(frame, end, &fh);
    if (r == kOk && fh.content != kSizeUnknown && fh.content > cap) r = kTooLarge;
    if (r != kOk) {
        *status = r;
        return PBS_OK;
    }
    const uint64_t block_max = fh.window < kBlockMax ? fh.window : kBlockMax;
    struct State {
        uint32_t ll[512], of[256], ml[512];
        uint16_t huf[kHufTableSize];
        int log[3] = {0, 0, 0};
        bool seq_valid[3] = {false, false, false};
        bool huf_valid = false;
        int huf_bits = 0;
        uint32_t rep[3] = {1, 4, 8};
        uint32_t fse[64];
        uint16_t next[64];
        BlockDesc d;
    };
    std::vector<State> stv(1);
    State& s = stv[0];
    std::vector<uint8_t> lit;  // sized at the first compressed block
    std::vector<Seq> seq;
    const uint8_t* p = frame + fh.size;
    uint64_t produced = 0;
    for (;;) {
        BlockHeader bh;
        r = parse_block_header(p, end, block_max, &bh);
        if (r != kOk) break;
        p += 3;
        if (bh.type < 2) {
            r = block_fits(bh.size, produced, cap, block_max, fh.content);
            if (r != kOk) break;
            if (bh.type == 0) {
                if (bh.size) std::memcpy(out + produced, p, bh.size);
                p += bh.size;
            } else {
                if (bh.size) std::memset(out + produced, p[0], bh.size);
                p += 1;
            }
            produced += bh.size;
        } else {
            const uint8_t* const bend = p + bh.size;
            if (lit.empty()) {
                lit.resize(kBlockMax);
                seq.resize(kMaxSeq + 1);
            }
            BlockDesc& d = s.d;
            r = parse_block_desc(p, bend, block_max, &s.huf_valid, s.seq_valid, &d, s.fse, s.next);
            if (r != kOk) break;
            if (d.lit.type == 2) r = build_huf_table(d.w, d.nw, s.huf, &s.huf_bits);
            uint32_t* const tabs[3] = {s.ll, s.of, s.ml};
            for (int k = 0; k < 3 && r == kOk && d.sh.nseq; ++k)
                r = build_seq_table(k, d.sh.mode[k], &d.td[k], tabs[k], &s.log[k], s.next);
            if (r != kOk) break;
            const uint8_t* lp = lit.data();
            if (d.lit.type == 0) {
                lp = d.lit_body;
            } else if (d.lit.type == 1) {
                std::memset(lit.data(), d.lit_body[0], d.lit.regen);
            } else {
                for (uint32_t k = 0; k < d.lit.streams && r == kOk; ++k)
                    r = huf_decode_stream(d.lit_body + d.hs.off[k], d.hs.len[k], s.huf, s.huf_bits,
                                          lit.data() + d.hs.dst[k], d.hs.cnt[k]);
                if (r != kOk) break;
            }
            uint32_t block_out = d.lit.regen;
            seq[0] = Seq{0, 0, 0, 0};
            if (d.sh.nseq) {
                r = decode_sequences(d.seq, d.seq_len, d.sh.nseq, s.ll, s.log[0], s.of, s.log[1], s.ml, s.log[2],
                                     s.rep, produced, d.lit.regen, seq.data(), &block_out);
                if (r != kOk) break;
            }
            r = block_fits(block_out, produced, cap, block_max, fh.content);
            if (r != kOk) break;
            uint8_t* const o = out + produced;
            for (uint32_t i = 0; i < d.sh.nseq; ++i) {
                const uint32_t ll = seq[i + 1].lit - seq[i].lit;
                if (ll) std::memcpy(o + seq[i].dst, lp + seq[i].lit, ll);
                uint8_t* const m = o + seq[i].dst + ll;
                const uint8_t* const src = m - seq[i].off;
                for (uint32_t j = 0; j < seq[i].ml; ++j) m[j] = src[j];
            }
            const uint32_t used = seq[d.sh.nseq].lit, at = seq[d.sh.nseq].dst;
            if (d.lit.regen > used) std::memcpy(o + at, lp + used, d.lit.regen - used);
            produced += block_out;
            p = bend;
        }
        if (bh.last) {
            r = frame_end_status(p, end, fh, produced);
            break;
        }
    }
    *out_len = (size_t)produced;
    *status = r;
    return PBS_OK;
}
