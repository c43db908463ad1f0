// The blob verdict of a submit, shared by every job that takes chunk blobs (verify, sync, the
// backup session's upload): the magic read that tells the encrypted blobs apart, and the walk
// over the runs of accepted items with one decode-inflate call each.  Include it from a .hip file
// only; everything is in an unnamed namespace, so each translation unit gets kernels of its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "dev_arena.h"
#include "gc_table_dev.h"
#include "pbs_blob.h"
#include "pbs_chunker_internal.h"
#include "verify_common.h"

namespace pbs {
namespace verify {
namespace {

using namespace pbs::gc;

// One lane per submitted blob: is its magic one of the two encrypted ones?  spans[2 t] is the
// blob's start in `blobs`, spans[2 t + 1] its length; a blob under a header has no magic.
__global__ __launch_bounds__(kGcThreads) void verify_magic_kernel(const uint8_t* __restrict__ blobs,
                                                                  const uint64_t* __restrict__ spans, uint64_t k,
                                                                  uint8_t* __restrict__ enc) {
    const uint64_t t = (uint64_t)blockIdx.x * kGcThreads + threadIdx.x;
    if (t >= k) return;
    uint8_t e = 0;
    if (spans[2 * t + 1] >= PBS_BLOB_HEADER_SIZE) {
        const uint8_t* p = blobs + spans[2 * t];
        uint64_t v = 0;
#pragma unroll
        for (int b = 0; b < 8; ++b) v |= (uint64_t)p[b] << (8 * b);  // (a blob starts at any alignment)
        e = v == kEncMagicLe || v == kEncComprMagicLe;
    }
    enc[t] = e;
}

// the arena slots the verdict works in: the spans, the encrypted flags, the decoder's output
// scratch, and one byte to stand for `blobs_dev` when a call has only empty blobs
struct BlobSlots {
    unsigned spans, enc, out, pack;
};

// what a verdict adds to the job's timing record
struct BlobTiming {
    double magic_ms = 0, decode_ms = 0;
    uint64_t decoded = 0, encrypted = 0, scratch_bytes = 0;
};

// enc[t] for k blobs given as (start, length) pairs in `blobs_dev`; synchronous.  Events 2 and 3
// of the arena time the kernel.
inline int magic_flags(DevArena& ar, const BlobSlots& sl, hipStream_t st, const uint8_t* blobs_dev,
                       const std::vector<uint64_t>& spans, size_t k, std::vector<uint8_t>& enc, double* ms_out) {
    enc.assign(k, 0);
    if (k == 0) return PBS_OK;
    uint64_t* d_spans = ar.get<uint64_t>(sl.spans, 16 * k);
    uint8_t* d_enc = ar.get<uint8_t>(sl.enc, k);
    hipEvent_t e0 = ar.event(2), e1 = ar.event(3);
    if (!d_spans || !d_enc) return PBS_ERR_NOMEM;
    if (!e0 || !e1) return PBS_ERR_HIP;
    CallRc rc;
    (void)hipGetLastError();
    if (rc.ok(hipMemcpyAsync(d_spans, spans.data(), 16 * k, hipMemcpyHostToDevice, st)) && rc.ok(hipEventRecord(e0, st))) {
        hipLaunchKernelGGL(verify_magic_kernel, dim3(blocks_for(k)), dim3(kGcThreads), 0, st, blobs_dev, d_spans,
                           (uint64_t)k, d_enc);
        rc.ok(hipGetLastError()) && rc.ok(hipEventRecord(e1, st)) &&
            rc.ok(hipMemcpyAsync(enc.data(), d_enc, k, hipMemcpyDeviceToHost, st));
    }
    if (hipStreamSynchronize(st) != hipSuccess) rc.fail(PBS_ERR_HIP);
    if (rc.rc == PBS_OK && ms_out) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, e0, e1);
        *ms_out = ms;
    }
    return rc.rc;
}

// The verdict of k submitted blobs (blob t = [off[t], off[t + 1]) of blobs_dev, which may be NULL
// when all are empty): kind and status of every item with skip[t] == 0 (skip may be NULL: none is
// skipped), through the decode-inflate path with no config, the announced digests (32 k bytes),
// the announced sizes (size_of(t)) and sizes_exact = 1.  The skipped items keep what the arrays
// hold.  The magic of every blob is read first: an encrypted blob is verified by its CRC alone,
// gets a zero-length output slot, and its NO_CONFIG becomes OK (load_chunk + verify_unencrypted:
// Ok for an encrypted chunk).  The decoder takes blobs that follow one another, so a run of items
// between two skipped ones goes per call.  crc == NULL: the stored CRC is judged; crc (k words):
// the payloads' CRCs are handed out instead (the backup session's upload).  Synchronous.
template <class SizeOf>
int blob_verdicts(DevArena& ar, const BlobSlots& sl, hipStream_t st, const uint8_t* blobs_dev, const uint64_t* off,
                  const uint8_t* skip, const uint8_t* digests, SizeOf size_of, size_t k, uint8_t* kinds, uint8_t* status,
                  uint32_t* crc, BlobTiming* tm) {
    if (k == 0) return PBS_OK;
    if (!blobs_dev) {  // (k empty blobs: the kernels still want an address)
        blobs_dev = ar.get<uint8_t>(sl.pack, 1);
        if (!blobs_dev) return PBS_ERR_NOMEM;
    }
    std::vector<uint64_t> spans(2 * k);
    for (size_t t = 0; t < k; ++t) {
        spans[2 * t] = off[t];
        spans[2 * t + 1] = skip && skip[t] ? 0 : off[t + 1] - off[t];
    }
    std::vector<uint8_t> enc;
    int rc = magic_flags(ar, sl, st, blobs_dev, spans, k, enc, &tm->magic_ms);
    if (rc != PBS_OK) return rc;
    std::vector<uint64_t> csz, ooff, olens;
    for (size_t a = 0; a < k;) {
        if (skip && skip[a]) {
            ++a;
            continue;
        }
        size_t b = a;
        while (b < k && !(skip && skip[b])) ++b;
        const size_t cnt = b - a;
        csz.assign(cnt, 0);
        uint64_t total = 0;
        bool plain = false;
        for (size_t t = a; t < b; ++t) {
            tm->encrypted += enc[t];
            if (enc[t]) continue;
            plain = true;
            csz[t - a] = size_of(t);
            if (csz[t - a] > UINT64_MAX - total) return PBS_ERR_NOMEM;
            total += csz[t - a];
        }
        if (total > SIZE_MAX) return PBS_ERR_NOMEM;
        // (an all-encrypted run takes no output scratch at all)
        uint8_t* d_out = plain ? ar.get<uint8_t>(sl.out, (size_t)total, false) : nullptr;
        if (plain && !d_out) return PBS_ERR_NOMEM;
        ooff.assign(cnt + 1, 0);
        olens.assign(cnt, 0);
        pbs_blob_decode_inflate_timing dt;
        rc = pbs::inflate::decode_inflate_impl(blobs_dev, off + a, cnt, nullptr, digests + 32 * a, csz.data(), 1, d_out,
                                               (size_t)total, ooff.data(), olens.data(), kinds + a, status + a, &dt, st,
                                               crc ? crc + a : nullptr);
        if (rc != PBS_OK) return rc;
        tm->decode_ms += dt.base.total_ms;
        tm->decoded += cnt;
        tm->scratch_bytes += total;
        for (size_t t = a; t < b; ++t)
            if (status[t] == PBS_BLOB_ST_NO_CONFIG) status[t] = PBS_BLOB_ST_OK;
        a = b;
    }
    return PBS_OK;
}

}  // namespace
}  // namespace verify
}  // namespace pbs
