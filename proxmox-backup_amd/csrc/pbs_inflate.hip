// Inflating zstd frames on the GPU: `zstd::stream::decode_all` (pbs-datastore/src/data_blob.rs
// :214, :238) for a batch of frames.  C ABI: include/pbs_blob.h, "Inflating zstd frames".  The
// format code is zstd_dec.h, shared with the serial host mirror (pbs_inflate_host.cpp).
//
// inflate_kernel: one workgroup of five waves owns one frame from its header to its last
// block; it takes frames from an atomic counter, longest first through the order list.  No
// workgroup waits on another and nothing spins: every loop is bounded by a length that was
// read from the frame and checked against the block's end (zstd_dec.h).  The window is the
// output itself: a match reads the slot's earlier bytes in HBM, and Window_Size only validates.
//
// Per compressed block:
//  1. lane 0 reads the headers (parse_block_desc: literals header, Huffman weights, sequences
//     header, the three table descriptions) into LDS -- short;
//  2. the four table builds run side by side, one per wave (Huffman, LL, OF, ML), into LDS:
//     2^11 Huffman entries, 512 + 256 + 512 FSE entries.  Treeless literals and Repeat_Mode
//     keep what the previous block left there;
//  3. the long chains run side by side: the Huffman streams one per wave (waves 0-3, so four
//     chains at once, not four lanes of one divergent wave) into the workgroup's literal
//     scratch, and the backward sequence stream on wave 4 -- its position is known from the
//     literals header, so it does not wait for the literals.  The sequence wave resolves the
//     repeat offsets (a serial rule) and keeps the running sums of literal and match lengths
//     as it goes -- the chain is bound by its table look-ups, the two additions are free --
//     so each sequence leaves as {output position, literal position, match length, offset}
//     and no separate prefix sum is needed; it also checks every offset against the bytes
//     produced so far, so a bad block is refused before its first byte is written;
//  4. all five waves place the literal runs (they depend on nothing): a lane per sequence
//     for short runs, the whole wave on each long one;
//  5. __syncthreads(), then wave 0 does the match copies in sequence order, lanes side by
//     side within a match (src[i mod offset] when offset < length).
//
// Status words.  Every stage that can fail has its own LDS word (Shared::err[stage]), and the
// rule is: a word is written only in the interval before the barrier after which it is read,
// and not again until every wave has passed a later barrier.  The frame word is written
// before the frame's first barrier; the block-header word at the top of a block, after the
// barrier that ends the previous block; the headers word in step 1, where lane 0 also clears
// the words of steps 2 and 3 -- one barrier before their writers (atomicMax from the building
// and the decoding lanes) and two before their readers.  So no wave can see a later stage's
// status in place of the one it is checking: all waves of a workgroup leave a bad block at
// the same barrier, whatever the frame says, and the next frame starts from a workgroup in
// step.  (One shared word would not do: a fast lane's failure in step 2 could land before a
// slow wave's read of step 1's verdict.)
//
// Ordering of step 5.  A match may read (a) bytes of earlier blocks, (b) literals of this
// block, (c) bytes of earlier matches of this block.  (a) and (b) were stored before the
// barrier between steps 4 and 5, which makes a workgroup's global stores visible to all its
// waves.  (c) are stores of other lanes of the same wave with no barrier in between: before a
// match whose source range reaches into [first byte stored by a match since the last fence,
// here), the wave executes a workgroup-scope release + acquire fence, which orders its earlier
// stores before its later loads in the CU's vector cache (all waves of a workgroup share one).
// Within one match no lane reads what another lane of that match stores: for offset < length
// every lane reads from the `offset` bytes before the match.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <numeric>
#include <vector>

#include "dev_arena.h"
#include "dev_copy.h"
#include "pbs_blob.h"
#include "pbs_chunker.h"
#include "pbs_chunker_internal.h"
#include "pbs_digest.h"
#include "zstd_dec.h"

namespace pbs {
namespace inflate {
namespace {

using namespace zstd;
using namespace zstd::dec;

constexpr int kWaves = 5;
constexpr int kThreads = 64 * kWaves;
constexpr int kGroupsPerCuMax = 4;  // the launch keeps what the occupancy query allows, at most this
// per-workgroup scratch: the block's literals, then its sequences (entry nseq closes the list)
constexpr uint64_t kLitBytes = kBlockMax + 256;
constexpr uint64_t kScratchStride = (kLitBytes + (uint64_t)(kMaxSeq + 2) * sizeof(Seq) + 255) & ~(uint64_t)255;

// the stages that report a status, each into its own LDS word
enum Stage : int { kStFrame, kStBlockHeader, kStDesc, kStBuild, kStChains, kStages };

struct Shared {
    uint32_t ll[512], of[256], ml[512];
    uint16_t huf[kHufTableSize];
    uint32_t fse[64];
    uint16_t next[4][64];
    BlockDesc d;
    FrameHeader fh;
    BlockHeader bh;
    int log[3];
    int huf_bits;
    bool seq_valid[3];
    bool huf_valid;
    uint32_t rep[3];
    uint32_t block_out;
    uint32_t err[kStages];  // one word per stage: see "Status words" in the header comment
    unsigned long long item;
};

__device__ inline void wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// step 4: literal runs of the block into o[0 .. block_out); lp = the block's literals
__device__ inline void literal_pass(const Seq* seq, uint32_t nseq, const uint8_t* lp, uint32_t regen, uint8_t* o,
                                    uint32_t tid) {
    const uint32_t wave = tid >> 6, lane = tid & 63u;
    for (uint32_t base = wave * 64u; base < nseq; base += 64u * kWaves) {
        const uint32_t i = base + lane;
        uint32_t dst = 0, lit = 0, ll = 0;
        if (i < nseq) {
            const Seq e = seq[i];
            dst = e.dst;
            lit = e.lit;
            ll = seq[i + 1].lit - e.lit;
        }
        if (ll <= 16)
            for (uint32_t j = 0; j < ll; ++j) o[dst + j] = lp[lit + j];
        uint64_t m = __ballot(ll > 16);
        while (m) {
            const int l = __ffsll((unsigned long long)m) - 1;
            m &= m - 1;
            const uint32_t d = __shfl(dst, l), s = __shfl(lit, l), n = __shfl(ll, l);
            for (uint32_t j = lane; j < n; j += 64) o[d + j] = lp[s + j];
        }
    }
    const uint32_t used = seq[nseq].lit, at = seq[nseq].dst;
    for (uint32_t j = tid; j < regen - used; j += kThreads) o[at + j] = lp[used + j];
}

// step 5 (one wave): `content` = the frame's output, `produced` = its bytes before this block
__device__ inline void match_pass(const Seq* seq, uint32_t nseq, uint8_t* content, uint64_t produced, uint32_t lane) {
    constexpr uint64_t kClean = ~0ull;
    uint64_t dirty = kClean;  // first content position a match stored to since the last fence
    for (uint32_t base = 0; base < nseq; base += 64) {
        const uint32_t i = base + lane;
        uint32_t md = 0, ml = 0, off = 1;
        if (i < nseq) {
            const Seq e = seq[i];
            md = e.dst + (seq[i + 1].lit - e.lit);
            ml = e.ml;
            off = e.off;
        }
        const uint32_t cnt = nseq - base < 64 ? nseq - base : 64;
        for (uint32_t k = 0; k < cnt; ++k) {
            const uint32_t d = __shfl(md, (int)k), n = __shfl(ml, (int)k), f = __shfl(off, (int)k);
            const uint64_t mpos = produced + d;  // (decode_sequences: f <= mpos, d + n <= block_out)
            const uint64_t rd_end = mpos - f + (n < f ? n : f);
            if (rd_end > dirty) {
                wave_fence();
                dirty = kClean;
            }
            uint8_t* const m = content + mpos;
            const uint8_t* const s = m - f;
            if (f >= n) {
                for (uint32_t j = lane; j < n; j += 64) m[j] = s[j];
            } else {
                for (uint32_t j = lane; j < n; j += 64) m[j] = s[j % f];
            }
            if (dirty == kClean) dirty = mpos;
        }
    }
}

__global__ __launch_bounds__(kThreads) void inflate_kernel(const uint8_t* __restrict__ frames,
                                                           const uint64_t* __restrict__ foff,
                                                           const uint64_t* __restrict__ ooff,
                                                           const uint32_t* __restrict__ order, uint64_t n,
                                                           unsigned long long* counter, uint8_t* out, uint8_t* scratch,
                                                           uint64_t* __restrict__ out_lens,
                                                           uint8_t* __restrict__ status) {
    __shared__ Shared S;
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    uint8_t* const lit = scratch + (uint64_t)blockIdx.x * kScratchStride;
    Seq* const seq = reinterpret_cast<Seq*>(lit + kLitBytes);
    for (;;) {
        if (tid == 0) S.item = atomicAdd(counter, 1ull);
        __syncthreads();
        const uint64_t item = S.item;
        if (item >= n) break;
        const uint32_t fi = order[item];
        const uint8_t* const f = frames + foff[fi];
        const uint8_t* const end = frames + foff[fi + 1];
        const uint64_t cap = ooff[fi + 1] - ooff[fi];
        uint8_t* const content = out + ooff[fi];
        if (tid == 0) {
            uint8_t r = parse_frame_header(f, end, &S.fh);
            if (r == kOk && S.fh.content != kSizeUnknown && S.fh.content > cap) r = kTooLarge;
            S.err[kStFrame] = r;
            S.rep[0] = 1;
            S.rep[1] = 4;
            S.rep[2] = 8;
            S.huf_valid = false;
            S.seq_valid[0] = S.seq_valid[1] = S.seq_valid[2] = false;
            S.log[0] = S.log[1] = S.log[2] = 0;
            S.huf_bits = 0;
        }
        __syncthreads();
        uint8_t st = (uint8_t)S.err[kStFrame];
        uint64_t produced = 0;
        if (st == kOk) {
            const FrameHeader fh = S.fh;
            const uint64_t block_max = fh.window < kBlockMax ? fh.window : kBlockMax;
            const uint8_t* p = f + fh.size;
            for (;;) {
                if (tid == 0) S.err[kStBlockHeader] = parse_block_header(p, end, block_max, &S.bh);
                __syncthreads();
                st = (uint8_t)S.err[kStBlockHeader];
                if (st != kOk) break;
                const BlockHeader bh = S.bh;
                p += 3;
                if (bh.type < 2) {
                    st = block_fits(bh.size, produced, cap, block_max, fh.content);
                    if (st != kOk) break;
                    uint8_t* const o = content + produced;
                    if (bh.type == 0) {
                        for (uint32_t j = tid; j < bh.size; j += kThreads) o[j] = p[j];
                        p += bh.size;
                    } else {
                        const uint8_t v = p[0];
                        for (uint32_t j = tid; j < bh.size; j += kThreads) o[j] = v;
                        p += 1;
                    }
                    produced += bh.size;
                } else {
                    const uint8_t* const bend = p + bh.size;
                    // 1. headers
                    if (tid == 0) {
                        S.err[kStDesc] =
                            parse_block_desc(p, bend, block_max, &S.huf_valid, S.seq_valid, &S.d, S.fse, S.next[0]);
                        S.err[kStBuild] = kOk;  // the words of the later stages, cleared a barrier before their writers
                        S.err[kStChains] = kOk;
                    }
                    __syncthreads();
                    st = (uint8_t)S.err[kStDesc];
                    if (st != kOk) break;
                    const uint32_t nseq = S.d.sh.nseq, regen = S.d.lit.regen, ltype = S.d.lit.type;
                    // 2. table builds, one per wave
                    if (lane == 0 && wave < 4) {
                        uint8_t r = kOk;
                        if (wave == 0) {
                            if (ltype == 2) r = build_huf_table(S.d.w, S.d.nw, S.huf, &S.huf_bits);
                        } else if (nseq) {
                            const int k = (int)wave - 1;
                            uint32_t* const tab = k == 0 ? S.ll : k == 1 ? S.of : S.ml;
                            r = build_seq_table(k, S.d.sh.mode[k], &S.d.td[k], tab, &S.log[k], S.next[wave]);
                        }
                        if (r != kOk) atomicMax(&S.err[kStBuild], (uint32_t)r);
                    }
                    __syncthreads();
                    st = (uint8_t)S.err[kStBuild];
                    if (st != kOk) break;
                    // 3. literals (waves 0-3) beside the sequence stream (wave 4)
                    if (wave < 4) {
                        if (ltype == 1) {
                            const uint8_t v = S.d.lit_body[0];
                            for (uint32_t j = tid; j < regen; j += 256) lit[j] = v;
                        } else if (ltype >= 2 && lane == 0 && wave < S.d.lit.streams) {
                            const uint8_t r = huf_decode_stream(S.d.lit_body + S.d.hs.off[wave], S.d.hs.len[wave], S.huf,
                                                                S.huf_bits, lit + S.d.hs.dst[wave], S.d.hs.cnt[wave]);
                            if (r != kOk) atomicMax(&S.err[kStChains], (uint32_t)r);
                        }
                    } else if (lane == 0) {
                        if (nseq) {
                            uint32_t bo = 0;
                            const uint8_t r = decode_sequences(S.d.seq, S.d.seq_len, nseq, S.ll, S.log[0], S.of, S.log[1],
                                                               S.ml, S.log[2], S.rep, produced, regen, seq, &bo);
                            S.block_out = bo;
                            if (r != kOk) atomicMax(&S.err[kStChains], (uint32_t)r);
                        } else {
                            seq[0] = Seq{0, 0, 0, 0};
                            S.block_out = regen;
                        }
                    }
                    __syncthreads();
                    st = (uint8_t)S.err[kStChains];
                    if (st != kOk) break;
                    const uint32_t block_out = S.block_out;
                    st = block_fits(block_out, produced, cap, block_max, fh.content);
                    if (st != kOk) break;
                    // 4. literal runs
                    const uint8_t* const lp = ltype == 0 ? S.d.lit_body : lit;
                    literal_pass(seq, nseq, lp, regen, content + produced, tid);
                    __syncthreads();
                    // 5. matches, in order
                    if (wave == 0) match_pass(seq, nseq, content, produced, lane);
                    produced += block_out;
                    p = bend;
                }
                // the block's bytes are visible to the workgroup, and S may be written again
                __syncthreads();
                if (bh.last) {
                    st = frame_end_status(p, end, fh, produced);
                    break;
                }
            }
        }
        if (tid == 0) {
            out_lens[fi] = produced;
            status[fi] = st;
        }
        __syncthreads();  // S.item and S.err[kStFrame] are written again
    }
}


// ---- pbs_blob_decode_inflate_device: payloads into the caller's slots ---------------------
ArenaPool& ipool() {
    static ArenaPool* p = new ArenaPool;  // never destroyed (HIP may be torn down first at exit)
    return *p;
}
enum ISlot : unsigned { kIsFoff, kIsOoff, kIsOrder, kIsLens, kIsStatus, kIsCounter, kIsScratch, kIsPacked, kIsItems,
                       kIsBounds2, kIsDigOrd, kIsDig, kIsWipe };

}  // namespace

// Asynchronous core on `st`: offsets, order, out_lens and status are device memory.
int inflate_async(const uint8_t* frames_dev, const uint64_t* foff_dev, const uint64_t* ooff_dev,
                  const uint32_t* order_dev, size_t n, uint8_t* out_dev, uint64_t* lens_dev, uint8_t* status_dev,
                  DevArena& ar, unsigned slot0, int ncu, hipStream_t st, unsigned* grid_out) {
    // as many workgroups as can be resident (the registers decide: DESIGN.md section 10), no more:
    // each brings 811 KiB of scratch
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, inflate_kernel, kThreads, 0) != hipSuccess || per_cu < 1) {
        (void)hipGetLastError();
        per_cu = 1;
    }
    per_cu = std::min(per_cu, kGroupsPerCuMax);
    const unsigned grid = (unsigned)std::min<uint64_t>(n, (uint64_t)ncu * per_cu);
    if (grid_out) *grid_out = grid;
    unsigned long long* counter = ar.get<unsigned long long>(slot0, 8);
    uint8_t* scratch = ar.get<uint8_t>(slot0 + 1, (size_t)grid * kScratchStride, false);
    if (!counter || !scratch) return PBS_ERR_NOMEM;
    if (hipMemsetAsync(counter, 0, 8, st) != hipSuccess) return PBS_ERR_HIP;
    hipLaunchKernelGGL(inflate_kernel, dim3(grid), dim3(kThreads), 0, st, frames_dev, foff_dev, ooff_dev, order_dev,
                       (uint64_t)n, counter, out_dev, scratch, lens_dev, status_dev);
    return hipGetLastError() == hipSuccess ? PBS_OK : PBS_ERR_HIP;
}

void inflate_release() { ipool().clear(); }

}  // namespace inflate
}  // namespace pbs

using namespace pbs;
using namespace pbs::inflate;

extern "C" int pbs_zstd_inflate_device(const uint8_t* frames_dev, const uint64_t* frame_offsets, size_t n,
                                       uint8_t* out_dev, const uint64_t* out_offsets, uint64_t* out_lens,
                                       uint8_t* status, pbs_zstd_inflate_timing* timing, void* hip_stream) {
    const HClock::time_point t0 = HClock::now();
    if (timing) std::memset(timing, 0, sizeof(*timing));
    if (n == 0) return PBS_OK;
    if (!frames_dev || !frame_offsets || !out_offsets || !out_lens || !status || n >= 0x7FFFFFFFull) return PBS_ERR_ARG;
    for (size_t i = 0; i < n; ++i)
        if (frame_offsets[i] > frame_offsets[i + 1] || out_offsets[i] > out_offsets[i + 1]) return PBS_ERR_ARG;
    if (out_offsets[n] > out_offsets[0] && !out_dev) return PBS_ERR_ARG;
    hipStream_t st = (hipStream_t)hip_stream;
    const StreamDevice sd(st);
    if (!sd.ok) return PBS_ERR_NO_DEVICE;
    DeviceGuard dg(sd.dev);
    if (!dg.ok) return PBS_ERR_NO_DEVICE;

    // longest frame first: the tail of the batch is made of short ones
    std::vector<uint32_t> order(n);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        return frame_offsets[a + 1] - frame_offsets[a] > frame_offsets[b + 1] - frame_offsets[b];
    });

    ArenaLease ar(ipool(), sd.dev);
    uint64_t* d_foff = ar->get<uint64_t>(kIsFoff, (n + 1) * 8);
    uint64_t* d_ooff = ar->get<uint64_t>(kIsOoff, (n + 1) * 8);
    uint32_t* d_order = ar->get<uint32_t>(kIsOrder, n * 4);
    uint64_t* d_lens = ar->get<uint64_t>(kIsLens, n * 8);
    uint8_t* d_status = ar->get<uint8_t>(kIsStatus, n);
    hipEvent_t e0 = ar->event(0), e1 = ar->event(1);
    if (!d_foff || !d_ooff || !d_order || !d_lens || !d_status) return PBS_ERR_NOMEM;
    if (!e0 || !e1) return PBS_ERR_HIP;
    int rc = PBS_OK;
    unsigned grid = 0;
    (void)hipGetLastError();
    if (hipMemcpyAsync(d_foff, frame_offsets, (n + 1) * 8, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(d_ooff, out_offsets, (n + 1) * 8, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(d_order, order.data(), n * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipEventRecord(e0, st) != hipSuccess)
        rc = PBS_ERR_HIP;
    if (rc == PBS_OK)
        rc = inflate_async(frames_dev, d_foff, d_ooff, d_order, n, out_dev, d_lens, d_status, *ar, kIsCounter, sd.ncu, st, &grid);
    if (rc == PBS_OK &&
        (hipEventRecord(e1, st) != hipSuccess ||
         hipMemcpyAsync(out_lens, d_lens, n * 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
         hipMemcpyAsync(status, d_status, n, hipMemcpyDeviceToHost, st) != hipSuccess))
        rc = PBS_ERR_HIP;
    // (also on failure: the arena and `order` go back only when the stream is idle)
    if (hipStreamSynchronize(st) != hipSuccess && rc == PBS_OK) rc = PBS_ERR_HIP;
    if (rc == PBS_OK && timing) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, e0, e1);
        timing->inflate_ms = ms;
        timing->frames = n;
        timing->workgroups = grid;
        timing->bytes_in = frame_offsets[n] - frame_offsets[0];
        for (size_t i = 0; i < n; ++i) {
            timing->bytes_out += out_lens[i];
            timing->failed += status[i] != PBS_ZST_OK;
        }
    }
    if (timing) timing->total_ms = hms(t0);
    return rc;
}

// DataBlob::load_from_reader + decode + verify for a stream of blobs, the inflate included:
// pbs_blob_decode_device (classify, CRC, GCM open; its contract and code unchanged) packs the
// payloads into arena scratch; kinds 0 and 2 are copied and kinds 1 and 3 inflated into the
// caller's slots (the copies as items of segment_copy_kernel, dev_copy.h: the slots are
// disjoint, so are the items of a launch); the digests of all four kinds are taken over
// [slot, slot + out_len); the verdict follows the reference's order (decrypt, decode_all,
// verify_digest, the length); the slot of every encrypted blob that failed is zeroed by zero
// items of the same kernel, in a later launch.
extern "C" int pbs_blob_decode_inflate_device(const uint8_t* blobs_dev, const uint64_t* blob_offsets, size_t n,
                                              const pbs_crypt_config* cfg, const uint8_t* expect_digests,
                                              const uint64_t* chunk_sizes, int sizes_exact, uint8_t* out_dev,
                                              size_t out_cap, uint64_t* out_offsets, uint64_t* out_lens,
                                              uint8_t* kinds, uint8_t* status,
                                              pbs_blob_decode_inflate_timing* timing, void* hip_stream) {
    return pbs::inflate::decode_inflate_impl(blobs_dev, blob_offsets, n, cfg, expect_digests, chunk_sizes, sizes_exact,
                                             out_dev, out_cap, out_offsets, out_lens, kinds, status, timing, hip_stream,
                                             nullptr);
}

// pbs_blob_decode_inflate_device; crc_out != NULL is the internal mode of decode_device_impl
// (pbs_decode.hip), reachable from the backup session's upload alone.
int pbs::inflate::decode_inflate_impl(const uint8_t* blobs_dev, const uint64_t* blob_offsets, size_t n,
                                      const pbs_crypt_config* cfg, const uint8_t* expect_digests,
                                      const uint64_t* chunk_sizes, int sizes_exact, uint8_t* out_dev, size_t out_cap,
                                      uint64_t* out_offsets, uint64_t* out_lens, uint8_t* kinds, uint8_t* status,
                                      pbs_blob_decode_inflate_timing* timing, void* hip_stream, uint32_t* crc_out) {
    const HClock::time_point t0 = HClock::now();
    if (timing) std::memset(timing, 0, sizeof(*timing));
    if (!out_offsets) return PBS_ERR_ARG;
    out_offsets[0] = 0;
    if (n == 0) return PBS_OK;
    if (!blob_offsets || !blobs_dev || !chunk_sizes || !out_lens || !kinds || !status || n >= 0x7FFFFFFFull)
        return PBS_ERR_ARG;
    for (size_t i = 0; i < n; ++i) {
        if (blob_offsets[i] > blob_offsets[i + 1]) return PBS_ERR_ARG;
        if (chunk_sizes[i] > (uint64_t)out_cap - out_offsets[i]) return PBS_ERR_CAPACITY;
        out_offsets[i + 1] = out_offsets[i] + chunk_sizes[i];
    }
    if (out_offsets[n] && !out_dev) return PBS_ERR_ARG;
    hipStream_t st = (hipStream_t)hip_stream;
    const StreamDevice sd(st);
    if (!sd.ok) return PBS_ERR_NO_DEVICE;
    DeviceGuard dg(sd.dev);
    if (!dg.ok) return PBS_ERR_NO_DEVICE;

    ArenaLease ar(ipool(), sd.dev);
    // 1. classify / CRC / GCM open: the packed payloads (frames for kinds 1 and 3) in scratch
    const size_t bound = pbs_blob_decode_bound(blob_offsets, n);
    uint8_t* packed = ar->get<uint8_t>(kIsPacked, bound);
    if (!packed) return PBS_ERR_NOMEM;
    std::vector<uint64_t> poff(n + 1);
    std::vector<uint8_t> st1(n);
    pbs_blob_decode_timing t1;
    CallRc call;
    if (!call.fail(decode_device_impl(blobs_dev, blob_offsets, n, cfg, nullptr, nullptr, packed, bound, poff.data(), kinds,
                                      st1.data(), &t1, hip_stream, crc_out)))
        return call.rc;

    // 2. copy or inflate into the slots
    // (both item lists live until the last synchronisation; a slot may be copied into by the
    // first launch and zeroed by the later one, never both in one)
    std::vector<CopyItem> items, wipe;
    std::vector<uint32_t> inf;
    const uint64_t out0 = (uint64_t)(uintptr_t)out_dev;
    auto wipe_slot = [&](size_t i) {
        out_lens[i] = 0;
        add_items(wipe, 0, out0 + out_offsets[i], chunk_sizes[i]);
    };
    std::vector<uint8_t> over(n, 0);
    for (size_t i = 0; i < n; ++i) {
        const uint64_t plen = poff[i + 1] - poff[i];
        status[i] = st1[i];
        out_lens[i] = 0;
        const uint8_t k = kinds[i];
        if (k == PBS_BLOB_KIND_NONE) continue;
        if (st1[i] != PBS_BLOB_ST_OK) {
            if (k >= 2) wipe_slot(i);
            if (k != PBS_BLOB_KIND_UNCOMPRESSED) continue;  // (kind 0 keeps its payload bytes, as in the packed call)
        }
        if (k == PBS_BLOB_KIND_UNCOMPRESSED || k == PBS_BLOB_KIND_ENCRYPTED) {
            const uint64_t len = plen < chunk_sizes[i] ? plen : chunk_sizes[i];
            over[i] = plen > chunk_sizes[i];
            out_lens[i] = len;
            add_items(items, (uint64_t)(uintptr_t)packed + poff[i], out0 + out_offsets[i], len);
        } else {
            inf.push_back((uint32_t)i);
        }
    }
    std::stable_sort(inf.begin(), inf.end(), [&](uint32_t a, uint32_t b) {
        return poff[a + 1] - poff[a] > poff[b + 1] - poff[b];
    });
    const size_t ninf = inf.size();
    uint64_t* d_poff = ar->get<uint64_t>(kIsFoff, (n + 1) * 8);
    uint64_t* d_ooff = ar->get<uint64_t>(kIsOoff, (n + 1) * 8);
    uint32_t* d_order = ar->get<uint32_t>(kIsOrder, n * 4);
    uint64_t* d_lens = ar->get<uint64_t>(kIsLens, n * 8);
    uint8_t* d_zst = ar->get<uint8_t>(kIsStatus, n);
    hipEvent_t e0 = ar->event(0), e1 = ar->event(1), e2 = ar->event(2);
    if (!d_poff || !d_ooff || !d_order || !d_lens || !d_zst) return PBS_ERR_NOMEM;
    if (!e0 || !e1 || !e2) return PBS_ERR_HIP;
    (void)hipGetLastError();
    std::vector<uint64_t> zlens(n, 0);
    std::vector<uint8_t> zst(n, 0);
    call.ok(hipMemcpyAsync(d_poff, poff.data(), (n + 1) * 8, hipMemcpyHostToDevice, st)) &&
        call.ok(hipMemcpyAsync(d_ooff, out_offsets, (n + 1) * 8, hipMemcpyHostToDevice, st)) &&
        (!ninf || call.ok(hipMemcpyAsync(d_order, inf.data(), ninf * 4, hipMemcpyHostToDevice, st))) &&
        call.ok(hipEventRecord(e0, st)) && call.fail(copy_items_async(items, *ar, kIsItems, sd.ncu, st));
    if (call.rc == PBS_OK && ninf)
        call.fail(inflate_async(packed, d_poff, d_ooff, d_order, ninf, out_dev, d_lens, d_zst, *ar, kIsCounter, sd.ncu, st,
                                nullptr)) &&
            call.ok(hipMemcpyAsync(zlens.data(), d_lens, n * 8, hipMemcpyDeviceToHost, st)) &&
            call.ok(hipMemcpyAsync(zst.data(), d_zst, n, hipMemcpyDeviceToHost, st));
    if (call.rc == PBS_OK) call.ok(hipEventRecord(e1, st));
    call.ok(hipStreamSynchronize(st));  // (whatever came before: the arena and the item lists need an idle stream)
    if (call.rc != PBS_OK) return call.rc;
    for (uint32_t i : inf) {
        out_lens[i] = zlens[i];
        if (zst[i] == PBS_ZST_BAD_FRAME) status[i] = PBS_BLOB_ST_BAD_FRAME;
        else if (zst[i] == PBS_ZST_UNSUPPORTED) status[i] = PBS_BLOB_ST_UNSUPPORTED_FRAME;
        else if (zst[i] == PBS_ZST_TOO_LARGE) over[i] = 1;
    }
    // content that overflows its slot: a message of another length cannot have the digest
    for (size_t i = 0; i < n; ++i)
        if (over[i] && status[i] == PBS_BLOB_ST_OK)
            status[i] = expect_digests ? PBS_BLOB_ST_BAD_DIGEST : PBS_BLOB_ST_BAD_SIZE;

    // 3. digests of all four kinds over [slot, slot + out_len): the spans as every second
    //    chunk of a bounds list (the digest call's chunks are contiguous)
    if (expect_digests) {
        std::vector<uint64_t> b2(2 * n + 1);
        std::vector<uint32_t> ord;
        std::vector<uint8_t> cls(n, 0);  // digest_order: kinds 0 and 1 plain, kinds 2 and 3 with the id_key
        for (size_t i = 0; i < n; ++i) {
            b2[2 * i] = out_offsets[i];
            b2[2 * i + 1] = out_offsets[i] + out_lens[i];
            if (status[i] == PBS_BLOB_ST_OK && kinds[i] != PBS_BLOB_KIND_NONE) cls[i] = kinds[i] >= 2 ? 2 : 1;
        }
        b2[2 * n] = out_offsets[n];
        const size_t nplain = digest_order(cls.data(), b2.data(), 2, n, ord);
        std::vector<uint8_t> dig(64 * n);
        if (!ord.empty()) {
            uint64_t* d_b2 = ar->get<uint64_t>(kIsBounds2, (2 * n + 1) * 8);
            uint32_t* d_ord = ar->get<uint32_t>(kIsDigOrd, n * 4);
            uint8_t* d_dig = ar->get<uint8_t>(kIsDig, 64 * n);
            if (!d_b2 || !d_ord || !d_dig) return PBS_ERR_NOMEM;
            call.ok(hipMemcpyAsync(d_b2, b2.data(), (2 * n + 1) * 8, hipMemcpyHostToDevice, st)) &&
                call.ok(hipMemcpyAsync(d_ord, ord.data(), ord.size() * 4, hipMemcpyHostToDevice, st)) &&
                call.fail(digest_in_order(out_dev, out_offsets[n], d_b2, d_ord, nplain, ord.size(), cfg, d_dig, st)) &&
                call.ok(hipMemcpyAsync(dig.data(), d_dig, 64 * n, hipMemcpyDeviceToHost, st));
            call.ok(hipStreamSynchronize(st));
            if (call.rc != PBS_OK) return call.rc;
            for (uint32_t c : ord) {
                const size_t i = c / 2;
                if (std::memcmp(dig.data() + 32 * (size_t)c, expect_digests + 32 * i, 32) != 0)
                    status[i] = PBS_BLOB_ST_BAD_DIGEST;
            }
        }
    }
    // 4. verify_unencrypted's length (both unencrypted magics), then the wipe
    for (size_t i = 0; i < n; ++i) {
        if (sizes_exact && status[i] == PBS_BLOB_ST_OK && kinds[i] < 2 && out_lens[i] != chunk_sizes[i])
            status[i] = PBS_BLOB_ST_BAD_SIZE;
        if (kinds[i] != PBS_BLOB_KIND_NONE && kinds[i] >= 2 && status[i] != PBS_BLOB_ST_OK && st1[i] == PBS_BLOB_ST_OK)
            wipe_slot(i);
    }
    call.fail(copy_items_async(wipe, *ar, kIsWipe, sd.ncu, st)) && call.ok(hipEventRecord(e2, st));
    call.ok(hipStreamSynchronize(st));  // (whatever came before: the arena and the item lists need an idle stream)
    if (call.rc == PBS_OK && timing) {
        float a = 0, b = 0;
        (void)hipEventElapsedTime(&a, e0, e1);
        (void)hipEventElapsedTime(&b, e1, e2);
        timing->base = t1;
        timing->base.digest_ms = b;
        timing->inflate_ms = a;
        timing->frames = ninf;
        timing->base.bytes_out = 0;
        timing->base.failed = 0;
        for (size_t i = 0; i < n; ++i) {
            timing->base.bytes_out += out_lens[i];
            timing->base.failed += status[i] != PBS_BLOB_ST_OK;
        }
    }
    if (timing) timing->base.total_ms = hms(t0);
    return call.rc;
}
