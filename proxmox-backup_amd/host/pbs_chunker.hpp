// C++ host mirror of proxmox-backup's chunker interface over the C ABI
// (include/pbs_chunker.h).  Header-only; link with libpbschunk.so.
//
//   pbs::Chunker            pbs-datastore/src/chunker.rs:18-186   (new / scan)
//   pbs::ChunkStream        pbs-client/src/chunk_stream.rs:12-78  (pull iterator of chunks)
//   pbs::DynamicChunkWriter pbs-datastore/src/dynamic_index.rs:397-523 (write / close)
//   pbs::DynamicIndexWriter pbs-datastore/src/dynamic_index.rs:297-391 (add_chunk / close)
//   pbs::DynamicIndexReader pbs-datastore/src/dynamic_index.rs:82-275 (open / chunk_from_offset)
//   pbs::digest_chunks_device  DataChunkBuilder::digest (data_blob.rs:516-536) per chunk, GPU
//   pbs::sha256             openssl::sha::sha256 (host; index checksum)
//   pbs::crc32_chunks_device DataBlob::compute_crc (data_blob.rs:70-75) per chunk, GPU
//   pbs::crc32 / pbs::blob_encode_uncompressed  crc32fast::Hasher, DataBlob::encode(.., false)
//   pbs::CryptConfig / pbs::blob_encode_chunks_encrypted_device  CryptConfig::new,
//                           DataBlob::encode(.., Some(config), ..) per chunk, AES-256-GCM on the GPU
//   pbs::digest_chunks_host  the per-chunk digest on host cores (SHA extensions)
//   pbs::pipeline_host      ChunkStream + the upload stream's per-chunk digest
//                           (chunk_stream.rs:40-77, backup_writer.rs:671-678) over a host buffer
//
// Same names, argument meaning and error behaviour as the reference: a non-power-of-two
// average throws std::invalid_argument with the reference's panic text; `scan` is
// infallible in the reference, so a device error throws std::runtime_error (the Rust
// shim in INTEGRATION.md panics at the same point).  The hash scan runs on the GPU.
#pragma once

#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <ctime>
#include <functional>
#include <map>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "pbs_chunker.h"
#include "pbs_blob.h"
#include "pbs_digest.h"
#include "pbs_restore.h"
#include "pbs_fixed.h"
#include "pbs_gc.h"
#include "pbs_verify.h"
#include "pbs_sync.h"
#include "pbs_backup.h"

namespace pbs {

class Chunker {
  public:
    explicit Chunker(size_t chunk_size_avg) {
        int err = 0;
        h_ = pbs_chunker_new(chunk_size_avg, &err);
        if (!h_) {
            if (err == PBS_ERR_NOT_POW2)
                throw std::invalid_argument("got unexpected chunk size - not a power of two.");
            throw std::runtime_error(std::string("pbs_chunker_new: ") + pbs_strerror(err));
        }
    }
    Chunker(const Chunker&) = delete;
    Chunker& operator=(const Chunker&) = delete;
    Chunker(Chunker&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    Chunker& operator=(Chunker&& o) noexcept {
        if (this != &o) {
            reset_handle();
            h_ = std::exchange(o.h_, nullptr);
        }
        return *this;
    }
    ~Chunker() { reset_handle(); }

    // chunker.rs:112 -- 0 if no boundary in `data` (all consumed), else the position
    // just after the cut byte, relative to `data`.
    size_t scan(const uint8_t* data, size_t len) {
        const size_t r = pbs_chunker_scan(h_, data, len);
        if (r == SIZE_MAX)
            throw std::runtime_error(std::string("pbs_chunker_scan: ") +
                                     pbs_strerror(pbs_chunker_last_error(h_)));
        return r;
    }
    size_t scan(const std::vector<uint8_t>& v) { return scan(v.data(), v.size()); }

    // All chunk END offsets (absolute) decided inside `data`; with is_final the tail too.
    std::vector<uint64_t> find_cuts(const uint8_t* data, size_t len, bool is_final = false) {
        std::vector<uint64_t> out(pbs_chunker_cuts_bound(h_, len));
        size_t n = 0;
        const int rc = pbs_chunker_find_cuts(h_, data, len, is_final ? 1 : 0, out.data(),
                                             out.size(), &n);
        if (rc != PBS_OK)
            throw std::runtime_error(std::string("pbs_chunker_find_cuts: ") + pbs_strerror(rc));
        out.resize(n);
        return out;
    }

    pbs_chunker* handle() const { return h_; }

  private:
    void reset_handle() {
        if (h_) pbs_chunker_free(h_);
        h_ = nullptr;
    }
    pbs_chunker* h_ = nullptr;
};

// ChunkStream: `next()` pulls input pieces from `source` (returns false at EOF) and
// yields chunks; the remainder is yielded at EOF (chunk_stream.rs:64-68).
class ChunkStream {
  public:
    using Source = std::function<bool(std::vector<uint8_t>&)>;
    explicit ChunkStream(Source source, std::optional<size_t> chunk_size = std::nullopt)
        : source_(std::move(source)), chunker_(chunk_size.value_or(4 * 1024 * 1024)) {}

    std::optional<std::vector<uint8_t>> next() {
        for (;;) {
            // gather at least min_scan unscanned bytes before a scan: each scan is a
            // host->device round trip (~30 us), so scanning every 8 KiB read piece would
            // cap the stream near 250 MB/s.  The cuts are those of the whole stream either
            // way (the chunker is a pure function of the bytes); only latency changes.
            while (!eof_ && buffer_.size() - head_ - scan_pos_ < std::max<size_t>(min_scan_, 1)) pull();
            const size_t avail = buffer_.size() - head_;
            if (scan_pos_ < avail) {
                const uint8_t* base = buffer_.data() + head_;
                const size_t boundary = chunker_.scan(base + scan_pos_, avail - scan_pos_);
                const size_t chunk_size = scan_pos_ + boundary;
                if (boundary == 0) {
                    scan_pos_ = avail;
                } else if (chunk_size <= avail) {
                    // BytesMut::split_to (chunk_stream.rs:51) is O(1): advance a head
                    // offset instead of moving the remainder
                    std::vector<uint8_t> out(base, base + chunk_size);
                    head_ += chunk_size;
                    scan_pos_ = 0;
                    return out;
                } else {
                    throw std::logic_error("got unexpected chunk boundary from chunker");
                }
                continue;
            }
            // everything buffered is scanned and the source is exhausted: the tail
            scan_pos_ = 0;
            if (head_ == buffer_.size()) return std::nullopt;
            std::vector<uint8_t> out(buffer_.begin() + (ptrdiff_t)head_, buffer_.end());
            buffer_.clear();
            head_ = 0;
            return out;
        }
    }

    // bytes gathered per device scan (default 4 MiB; 0 scans every piece as it arrives)
    void set_min_scan(size_t bytes) { min_scan_ = bytes; }

  private:
    Source source_;
    Chunker chunker_;
    std::vector<uint8_t> buffer_;
    size_t head_ = 0;      // bytes of buffer_ already handed out
    size_t scan_pos_ = 0;  // relative to head_
    size_t min_scan_ = 4u << 20;
    bool eof_ = false;

    void pull() {
        std::vector<uint8_t> piece;
        if (!source_(piece)) {
            eof_ = true;
            return;
        }
        if (head_ && head_ * 2 >= buffer_.size()) {  // compact before growing
            buffer_.erase(buffer_.begin(), buffer_.begin() + (ptrdiff_t)head_);
            head_ = 0;
        }
        buffer_.insert(buffer_.end(), piece.begin(), piece.end());
    }
};

// DynamicChunkWriter: `write` returns the bytes consumed (the caller re-submits the
// rest, as write_all does); every finished chunk goes to sink(chunk_end_offset, bytes)
// in place of the digest/compress/insert/add_chunk step (dynamic_index.rs:444-490).
class DynamicChunkWriter {
  public:
    using Sink = std::function<void(uint64_t, const std::vector<uint8_t>&)>;
    DynamicChunkWriter(Sink sink, size_t chunk_size) : sink_(std::move(sink)), chunker_(chunk_size) {
        chunk_buffer_.reserve(chunk_size * 4);
    }

    size_t write(const uint8_t* data, size_t len) {
        const size_t pos = chunker_.scan(data, len);
        if (pos > 0) {
            chunk_buffer_.insert(chunk_buffer_.end(), data, data + pos);
            chunk_offset_ += pos;
            write_chunk_buffer();
            return pos;
        }
        chunk_offset_ += len;
        chunk_buffer_.insert(chunk_buffer_.end(), data, data + len);
        return len;
    }

    void write_all(const uint8_t* data, size_t len) {
        while (len) {
            const size_t k = write(data, len);
            data += k;
            len -= k;
        }
    }

    void close() {
        if (closed_) return;
        closed_ = true;
        write_chunk_buffer();
    }

    uint64_t chunk_count() const { return chunk_count_; }

  private:
    void write_chunk_buffer() {
        if (chunk_buffer_.empty()) return;
        if (chunk_offset_ - last_chunk_ != chunk_buffer_.size())
            throw std::logic_error("wrong chunk size");
        ++chunk_count_;
        last_chunk_ = chunk_offset_;
        sink_(chunk_offset_, chunk_buffer_);
        chunk_buffer_.clear();
    }

    Sink sink_;
    Chunker chunker_;
    std::vector<uint8_t> chunk_buffer_;
    uint64_t chunk_offset_ = 0, last_chunk_ = 0, chunk_count_ = 0;
    bool closed_ = false;
};

using Digest = std::array<uint8_t, 32>;

inline Digest sha256(const uint8_t* data, size_t len) {
    Digest d;
    pbs_sha256(data, len, d.data());
    return d;
}

// SHA-256 of every chunk [bounds[i], bounds[i+1]) of a device-resident stream (stream
// bytes [base, base + len) at dev), optionally keyed (SHA-256(chunk || id_key)).
inline std::vector<Digest> digest_chunks_device(const uint8_t* dev, size_t len, uint64_t base,
                                                const std::vector<uint64_t>& bounds,
                                                const std::vector<uint8_t>& key = {},
                                                void* hip_stream = nullptr) {
    const size_t n = bounds.size() > 1 ? bounds.size() - 1 : 0;
    std::vector<Digest> out(n);
    if (!n) return out;
    const int rc = pbs_digest_chunks_device(dev, len, base, bounds.data(), n,
                                            key.empty() ? nullptr : key.data(), key.size(),
                                            out[0].data(), hip_stream);
    if (rc != PBS_OK) throw std::runtime_error(std::string("pbs_digest_chunks_device: ") + pbs_strerror(rc));
    return out;
}

// CRC-32 (crc32fast) of every chunk [bounds[i], bounds[i+1]) of a device-resident stream:
// the blob CRC of an uncompressed chunk blob (DataBlob::compute_crc, data_blob.rs:70-75).
inline std::vector<uint32_t> crc32_chunks_device(const uint8_t* dev, size_t len, uint64_t base,
                                                 const std::vector<uint64_t>& bounds,
                                                 void* hip_stream = nullptr) {
    const size_t n = bounds.size() > 1 ? bounds.size() - 1 : 0;
    std::vector<uint32_t> out(n);
    if (!n) return out;
    const int rc = pbs_crc32_chunks_device(dev, len, base, bounds.data(), n, out.data(), hip_stream);
    if (rc != PBS_OK) throw std::runtime_error(std::string("pbs_crc32_chunks_device: ") + pbs_strerror(rc));
    return out;
}

// Host CRC-32, continuable like crc32fast::Hasher::update (crc = 0 to start).
inline uint32_t crc32(const uint8_t* data, size_t len, uint32_t crc = 0) { return pbs_crc32(crc, data, len); }

// DataBlob::encode(data, None, compress = false) (data_blob.rs:159-174) with a known CRC:
// UNCOMPRESSED_BLOB_MAGIC_1_0 || crc LE || data; throws above MAX_BLOB_SIZE like the
// reference's bail! (data_blob.rs:92-94).
inline std::vector<uint8_t> blob_encode_uncompressed(const uint8_t* data, size_t len, uint32_t crc) {
    std::vector<uint8_t> out(len + PBS_BLOB_HEADER_SIZE);
    if (pbs_blob_encode_uncompressed(data, len, crc, out.data(), out.size()) != out.size())
        throw std::invalid_argument("data blob too large (" + std::to_string(len) + " bytes).");
    return out;
}

// CryptConfig::new(enc_key) (pbs-tools/src/crypt_config.rs:42-61): owns the C handle; the key
// material is zeroed when it goes out of scope.  id_key() is the digest key of an encrypted
// backup (pass it as `key` to the digest calls above).
class CryptConfig {
  public:
    explicit CryptConfig(const std::array<uint8_t, 32>& enc_key) {
        const int rc = pbs_crypt_config_new(enc_key.data(), &h_);
        if (rc != PBS_OK) throw std::runtime_error(std::string("pbs_crypt_config_new: ") + pbs_strerror(rc));
    }
    ~CryptConfig() { pbs_crypt_config_free(h_); }
    CryptConfig(const CryptConfig&) = delete;
    CryptConfig& operator=(const CryptConfig&) = delete;
    const pbs_crypt_config* handle() const { return h_; }
    std::vector<uint8_t> id_key() const {
        const uint8_t* k = pbs_crypt_config_id_key(h_);
        return std::vector<uint8_t>(k, k + 32);
    }
    // AES-256-GCM of `data` under a 16-byte IV on the host: ciphertext, and the tag in `tag`
    std::vector<uint8_t> encrypt_host(const std::array<uint8_t, 16>& iv, const uint8_t* data, size_t len,
                                      std::array<uint8_t, 16>& tag) const {
        std::vector<uint8_t> out(len);
        const int rc = pbs_aes256gcm_encrypt_host(h_, iv.data(), data, len, out.data(), tag.data());
        if (rc != PBS_OK) throw std::runtime_error(std::string("pbs_aes256gcm_encrypt_host: ") + pbs_strerror(rc));
        return out;
    }
    // Opens what encrypt_host seals: the plaintext and `ok` true, or an empty vector and `ok`
    // false when the tag does not match (nothing unauthenticated is returned)
    std::vector<uint8_t> decrypt_host(const std::array<uint8_t, 16>& iv, const uint8_t* data, size_t len,
                                      const std::array<uint8_t, 16>& tag, bool& ok) const {
        std::vector<uint8_t> out(len);
        const int rc = pbs_aes256gcm_decrypt_host(h_, iv.data(), data, len, tag.data(), out.data());
        if (rc != PBS_OK && rc != PBS_ERR_TAG)
            throw std::runtime_error(std::string("pbs_aes256gcm_decrypt_host: ") + pbs_strerror(rc));
        ok = rc == PBS_OK;
        if (!ok) out.clear();
        return out;
    }

  private:
    pbs_crypt_config* h_ = nullptr;
};

// DataBlob::load_from_reader + decode (+ verify_unencrypted's length) of one blob on the host
// (pbs_blob_decode_host): the payload -- chunk bytes, or the zstd frame of a compressed kind,
// which the caller inflates -- with the blob's kind (PBS_BLOB_KIND_*) and status
// (PBS_BLOB_ST_*: the first check that fails).  `crypt`, `expect_digest`, `expect_size`: null
// where there is none.
struct DecodedBlob {
    std::vector<uint8_t> payload;
    uint8_t kind = PBS_BLOB_KIND_NONE;
    uint8_t status = PBS_BLOB_ST_OK;
};
inline DecodedBlob blob_decode_host(const uint8_t* blob, size_t len, const CryptConfig* crypt = nullptr,
                                    const Digest* expect_digest = nullptr, const uint64_t* expect_size = nullptr) {
    DecodedBlob r;
    r.payload.resize(len);
    size_t n = 0;
    const int rc = pbs_blob_decode_host(blob, len, crypt ? crypt->handle() : nullptr,
                                        expect_digest ? expect_digest->data() : nullptr, expect_size,
                                        r.payload.data(), r.payload.size(), &n, &r.kind, &r.status);
    if (rc != PBS_OK) throw std::runtime_error(std::string("pbs_blob_decode_host: ") + pbs_strerror(rc));
    r.payload.resize(n);
    return r;
}

// The same for n blobs [offsets[i], offsets[i+1]) of a device buffer, any mix of kinds, on the
// GPU (pbs_blob_decode_device): the payloads back to back at `out_dev` (out_cap >=
// pbs_blob_decode_bound), payload i at [out_offsets[i], out_offsets[i+1]).  `expect_digests`
// (empty or n; kinds 0 and 2) and `expect_sizes` (empty or n; kind 0).  A bad blob is a status,
// never an exception; a failed encrypted blob leaves zeros in the output.
struct DecodedBlobs {
    std::vector<uint64_t> out_offsets;
    std::vector<uint8_t> kinds, status;
    pbs_blob_decode_timing timing;
};
inline DecodedBlobs blob_decode_device(const uint8_t* blobs_dev, const std::vector<uint64_t>& offsets,
                                       const CryptConfig* crypt, uint8_t* out_dev, size_t out_cap,
                                       const std::vector<Digest>& expect_digests = {},
                                       const std::vector<uint64_t>& expect_sizes = {}, void* hip_stream = nullptr) {
    const size_t n = offsets.size() > 1 ? offsets.size() - 1 : 0;
    if ((!expect_digests.empty() && expect_digests.size() != n) || (!expect_sizes.empty() && expect_sizes.size() != n))
        throw std::invalid_argument("expectations must hold one entry per blob");
    DecodedBlobs r;
    r.out_offsets.assign(n + 1, 0);
    r.kinds.resize(n);
    r.status.resize(n);
    const int rc = pbs_blob_decode_device(blobs_dev, offsets.data(), n, crypt ? crypt->handle() : nullptr,
                                          expect_digests.empty() ? nullptr : expect_digests[0].data(),
                                          expect_sizes.empty() ? nullptr : expect_sizes.data(), out_dev, out_cap,
                                          r.out_offsets.data(), r.kinds.data(), r.status.data(), &r.timing, hip_stream);
    if (rc != PBS_OK) throw std::runtime_error(std::string("pbs_blob_decode_device: ") + pbs_strerror(rc));
    return r;
}

// zstd frames (`zstd::stream::decode_all`).  zstd_frame_content_size: the header's content size,
// PBS_ZSTD_SIZE_UNKNOWN when it carries none.  zstd_inflate_host: the serial mirror of the GPU
// inflater -- `cap` bytes of room, the status PBS_ZST_* in `status`.  zstd_inflate_device: frame
// i = [frame_offsets[i], frame_offsets[i+1]) of a device buffer into the caller's slot
// [out_offsets[i], out_offsets[i+1]) of `out_dev`; a bad frame is a status, never an exception.
inline uint64_t zstd_frame_content_size(const uint8_t* frame, size_t len) {
    uint64_t v = 0;
    if (pbs_zstd_frame_content_size(frame, len, &v) != PBS_OK) throw std::invalid_argument("no zstd frame header");
    return v;
}
inline std::vector<uint8_t> zstd_inflate_host(const uint8_t* frame, size_t len, size_t cap, uint8_t& status) {
    std::vector<uint8_t> out(cap);
    size_t n = 0;
    const int rc = pbs_zstd_inflate_host(frame, len, out.data(), cap, &n, &status);
    if (rc != PBS_OK) throw std::runtime_error(std::string("pbs_zstd_inflate_host: ") + pbs_strerror(rc));
    out.resize(n);
    return out;
}
struct InflatedFrames {
    std::vector<uint64_t> out_lens;
    std::vector<uint8_t> status;
    pbs_zstd_inflate_timing timing;
};
inline InflatedFrames zstd_inflate_device(const uint8_t* frames_dev, const std::vector<uint64_t>& frame_offsets,
                                          uint8_t* out_dev, const std::vector<uint64_t>& out_offsets,
                                          void* hip_stream = nullptr) {
    const size_t n = frame_offsets.size() > 1 ? frame_offsets.size() - 1 : 0;
    if (out_offsets.size() != n + 1) throw std::invalid_argument("out_offsets must hold one slot per frame");
    InflatedFrames r;
    r.out_lens.assign(n, 0);
    r.status.assign(n, 0);
    const int rc = pbs_zstd_inflate_device(frames_dev, frame_offsets.data(), n, out_dev, out_offsets.data(),
                                           r.out_lens.data(), r.status.data(), &r.timing, hip_stream);
    if (rc != PBS_OK) throw std::runtime_error(std::string("pbs_zstd_inflate_device: ") + pbs_strerror(rc));
    return r;
}

// The read path in one call (pbs_blob_decode_inflate_device): blob i's chunk -- copied, opened,
// inflated -- in the slot of chunk_sizes[i] bytes at out_offsets[i] of `out_dev`, its length in
// out_lens[i]; `expect_digests` (empty or n) is checked for all four kinds.
struct InflatedBlobs {
    std::vector<uint64_t> out_offsets, out_lens;
    std::vector<uint8_t> kinds, status;
    pbs_blob_decode_inflate_timing timing;
};
inline InflatedBlobs blob_decode_inflate_device(const uint8_t* blobs_dev, const std::vector<uint64_t>& offsets,
                                                const CryptConfig* crypt, const std::vector<uint64_t>& chunk_sizes,
                                                uint8_t* out_dev, size_t out_cap,
                                                const std::vector<Digest>& expect_digests = {},
                                                bool sizes_exact = false, void* hip_stream = nullptr) {
    const size_t n = offsets.size() > 1 ? offsets.size() - 1 : 0;
    if (chunk_sizes.size() != n || (!expect_digests.empty() && expect_digests.size() != n))
        throw std::invalid_argument("chunk_sizes and expectations must hold one entry per blob");
    InflatedBlobs r;
    r.out_offsets.assign(n + 1, 0);
    r.out_lens.assign(n, 0);
    r.kinds.resize(n);
    r.status.resize(n);
    const int rc = pbs_blob_decode_inflate_device(
        blobs_dev, offsets.data(), n, crypt ? crypt->handle() : nullptr,
        expect_digests.empty() ? nullptr : expect_digests[0].data(), chunk_sizes.data(), sizes_exact ? 1 : 0, out_dev,
        out_cap, r.out_offsets.data(), r.out_lens.data(), r.kinds.data(), r.status.data(), &r.timing, hip_stream);
    if (rc != PBS_OK) throw std::runtime_error(std::string("pbs_blob_decode_inflate_device: ") + pbs_strerror(rc));
    return r;
}

// DataBlob::encode(chunk, Some(config), compress) of every chunk [bounds[i], bounds[i+1]) of a
// device-resident stream, on the GPU (pbs_blob_encode_chunks_encrypted_device): the blobs
// back to back at `blobs_dev` (blobs_cap >= pbs_blob_stream_bound_encrypted), blob i at
// [offsets[i], offsets[i+1]).  `ivs` empty: the library draws a fresh IV per blob; 16 n bytes:
// the caller's IVs, for reproducible tests only -- reusing an IV under one key breaks GCM.
struct EncryptedBlobs {
    std::vector<uint64_t> offsets;
    std::vector<uint32_t> crcs;
    std::vector<uint8_t> compressed;
    pbs_blob_encode_timing_crypt timing;
};
inline EncryptedBlobs blob_encode_chunks_encrypted_device(const uint8_t* dev, size_t len, uint64_t base,
                                                          const std::vector<uint64_t>& bounds, bool compress,
                                                          const CryptConfig& crypt, uint8_t* blobs_dev,
                                                          size_t blobs_cap, const std::vector<uint8_t>& ivs = {},
                                                          void* hip_stream = nullptr) {
    const size_t n = bounds.size() > 1 ? bounds.size() - 1 : 0;
    if (!ivs.empty() && ivs.size() != 16 * n) throw std::invalid_argument("ivs must hold 16 bytes per chunk");
    EncryptedBlobs r;
    r.offsets.assign(n + 1, 0);
    r.crcs.resize(n);
    r.compressed.resize(n);
    const int rc = pbs_blob_encode_chunks_encrypted_device(
        dev, len, base, bounds.data(), n, compress ? 1 : 0, crypt.handle(), ivs.empty() ? nullptr : ivs.data(),
        blobs_dev, blobs_cap, r.offsets.data(), r.crcs.data(), r.compressed.data(), &r.timing, hip_stream);
    if (rc != PBS_OK)
        throw std::runtime_error(std::string("pbs_blob_encode_chunks_encrypted_device: ") + pbs_strerror(rc));
    return r;
}

// SHA-256 of every chunk [bounds[i], bounds[i+1]) of a host buffer (stream bytes
// [base, base + len)) on `threads` host threads (0: all), optionally keyed.
inline std::vector<Digest> digest_chunks_host(const uint8_t* data, size_t len, uint64_t base,
                                              const std::vector<uint64_t>& bounds,
                                              const std::vector<uint8_t>& key = {}, int threads = 0) {
    const size_t n = bounds.size() > 1 ? bounds.size() - 1 : 0;
    std::vector<Digest> out(n);
    if (!n) return out;
    const int rc = pbs_digest_chunks_host(data, len, base, bounds.data(), n, key.empty() ? nullptr : key.data(),
                                          key.size(), out[0].data(), threads);
    if (rc != PBS_OK) throw std::runtime_error(std::string("pbs_digest_chunks_host: ") + pbs_strerror(rc));
    return out;
}

// The client's upload path over a whole host buffer (pbs_pipeline_host): chunk END
// offsets (the tail included), the per-chunk digests and, with crc, the uncompressed
// blobs' CRC-32s; copies to HBM, chunking and digests overlapped on the GPU and host cores.
struct PipelineResult {
    std::vector<uint64_t> ends;
    std::vector<Digest> digests;
    std::vector<uint32_t> crcs;
    pbs_pipeline_timing timing;
};
inline PipelineResult pipeline_host(const uint8_t* data, size_t len, size_t avg, size_t piece = (size_t)1 << 30,
                                    const std::vector<uint8_t>& key = {}, bool crc = true, int digest_cus = 64) {
    // pbs_chunker_cuts_bound without a handle: every chunk but the tail >= max(avg / 4, 65)
    const size_t cap = len / std::max<size_t>(avg >> 2, 65) + 4;
    PipelineResult r;
    r.ends.resize(cap);
    r.digests.resize(cap);
    if (crc) r.crcs.resize(cap);
    size_t n = 0;
    const int rc = pbs_pipeline_host(avg, data, len, piece, key.empty() ? nullptr : key.data(), key.size(),
                                     digest_cus, r.ends.data(), r.digests[0].data(),
                                     crc ? r.crcs.data() : nullptr, cap, &n, &r.timing);
    if (rc == PBS_ERR_NOT_POW2) throw std::invalid_argument("chunk size is not a power of two");
    if (rc != PBS_OK) throw std::runtime_error(std::string("pbs_pipeline_host: ") + pbs_strerror(rc));
    r.ends.resize(n);
    r.digests.resize(n);
    if (crc) r.crcs.resize(n);
    return r;
}

// DynamicIndexWriter (dynamic_index.rs:297-391): add_chunk(end offset, digest) per chunk,
// close() writes the .didx file (tmp file + rename) and returns index_csum.
class DynamicIndexWriter {
  public:
    explicit DynamicIndexWriter(std::string path, std::array<uint8_t, 16> uuid = {},
                                int64_t ctime = (int64_t)std::time(nullptr))
        : path_(std::move(path)), uuid_(uuid), ctime_(ctime) {}

    void add_chunk(uint64_t offset, const Digest& digest) {
        if (closed_) throw std::runtime_error("cannot write to closed dynamic index file " + path_);
        ends_.push_back(offset);
        digests_.insert(digests_.end(), digest.begin(), digest.end());
    }

    Digest close() {
        if (closed_) throw std::runtime_error("cannot close already closed archive index file " + path_);
        closed_ = true;
        std::vector<uint8_t> image(pbs_didx_size(ends_.size()));
        Digest csum;
        const int rc = pbs_didx_build(ends_.data(), digests_.data(), ends_.size(), uuid_.data(),
                                      ctime_, image.data(), image.size(), csum.data());
        if (rc != PBS_OK) throw std::runtime_error(std::string("pbs_didx_build: ") + pbs_strerror(rc));
        std::string tmp = path_;
        const size_t dot = tmp.find_last_of('.');
        tmp = (dot == std::string::npos ? tmp : tmp.substr(0, dot)) + ".tmp_didx";
        std::FILE* f = std::fopen(tmp.c_str(), "wb");
        if (!f) throw std::runtime_error("cannot create " + tmp);
        const bool ok = std::fwrite(image.data(), 1, image.size(), f) == image.size();
        if (std::fclose(f) != 0 || !ok) throw std::runtime_error("write failed: " + tmp);
        if (std::rename(tmp.c_str(), path_.c_str()) != 0)
            throw std::runtime_error("Atomic rename file " + path_ + " failed");
        return csum;
    }

  private:
    std::string path_;
    std::array<uint8_t, 16> uuid_;
    int64_t ctime_;
    std::vector<uint64_t> ends_;
    std::vector<uint8_t> digests_;
    bool closed_ = false;
};

// DynamicIndexReader (dynamic_index.rs:82-275) over pbs_didx_parse: from the bytes of a .didx
// image or from a file.  Throws where the reference's `new` bails (short image, wrong magic,
// ragged body) and for chunk ends that decrease.  index_csum is the header's checksum,
// compute_csum() the one over the entries; opening does not compare them.
struct ChunkReadInfo {
    uint64_t start, end;
    Digest digest;
};
class DynamicIndexReader {
  public:
    DynamicIndexReader(const uint8_t* image, size_t len) { parse(image, len); }
    explicit DynamicIndexReader(const std::string& path) {
        std::FILE* f = std::fopen(path.c_str(), "rb");
        if (!f) throw std::runtime_error("Unable to open dynamic index " + path);
        std::vector<uint8_t> image;
        uint8_t buf[65536];
        for (size_t k; (k = std::fread(buf, 1, sizeof buf, f)) > 0;) image.insert(image.end(), buf, buf + k);
        std::fclose(f);
        parse(image.data(), image.size());
    }

    std::array<uint8_t, 16> uuid{};
    int64_t ctime = 0;
    Digest index_csum{};
    size_t size = 0;  // bytes of the image

    size_t index_count() const { return ends_.size(); }
    uint64_t index_bytes() const { return ends_.empty() ? 0 : ends_.back(); }
    uint64_t chunk_end(size_t pos) const {
        if (pos >= ends_.size()) throw std::out_of_range("chunk index out of range");
        return ends_[pos];
    }
    std::optional<Digest> index_digest(size_t pos) const {
        if (pos >= ends_.size()) return std::nullopt;
        Digest d;
        std::memcpy(d.data(), digests_.data() + 32 * pos, 32);
        return d;
    }
    std::optional<ChunkReadInfo> chunk_info(size_t pos) const {
        if (pos >= ends_.size()) return std::nullopt;
        return ChunkReadInfo{pos ? ends_[pos - 1] : 0, ends_[pos], *index_digest(pos)};
    }
    // (entry, offset inside it) of an archive byte; nullopt at or past the end
    std::optional<std::pair<size_t, uint64_t>> chunk_from_offset(uint64_t offset) const {
        size_t idx = 0;
        uint64_t within = 0;
        if (pbs_didx_chunk_from_offset(ends_.data(), ends_.size(), offset, &idx, &within) != PBS_OK) return std::nullopt;
        return std::make_pair(idx, within);
    }
    std::pair<Digest, uint64_t> compute_csum() const { return {csum_, index_bytes()}; }
    const std::vector<uint64_t>& ends() const { return ends_; }
    const std::vector<uint8_t>& digests() const { return digests_; }  // 32 bytes per entry

  private:
    void parse(const uint8_t* image, size_t len) {
        const size_t cnt = pbs_didx_count(len);
        const size_t cap = cnt == (size_t)-1 ? 0 : cnt;
        ends_.resize(cap);
        digests_.resize(32 * cap);
        size_t n = 0;
        const int rc = pbs_didx_parse(image, len, uuid.data(), &ctime, index_csum.data(), csum_.data(), ends_.data(),
                                      digests_.data(), cap, &n);
        if (rc != PBS_OK) throw std::runtime_error(std::string("pbs_didx_parse: ") + pbs_strerror(rc));
        size = len;
    }
    std::vector<uint64_t> ends_;
    std::vector<uint8_t> digests_;
    Digest csum_{};
};

// ---- the fixed-size chunk path (include/pbs_fixed.h) ----

// FixedChunkStream (pbs-client/src/chunk_stream.rs:80-134): feed bytes in any pieces; chunks of
// exactly chunk_size come out and, at the end, one last chunk of any non-zero length.
class FixedChunkStream {
  public:
    explicit FixedChunkStream(size_t chunk_size) : chunk_size_(chunk_size) {
        if (!chunk_size) throw std::invalid_argument("chunk_size must be positive");
    }
    // the chunks `data` completes
    std::vector<std::vector<uint8_t>> feed(const uint8_t* data, size_t len) {
        std::vector<std::vector<uint8_t>> out;
        while (len) {
            const size_t k = std::min(len, chunk_size_ - buf_.size());
            buf_.insert(buf_.end(), data, data + k);
            data += k;
            len -= k;
            if (buf_.size() == chunk_size_) {
                out.push_back(std::move(buf_));
                buf_.clear();
            }
        }
        return out;
    }
    // the last, shorter chunk (:118-130); nothing after an exact multiple or an empty input
    std::vector<std::vector<uint8_t>> finish() {
        std::vector<std::vector<uint8_t>> out;
        if (!buf_.empty()) out.push_back(std::move(buf_));
        buf_.clear();
        return out;
    }

  private:
    size_t chunk_size_;
    std::vector<uint8_t> buf_;
};

// FixedIndexReader (pbs-datastore/src/fixed_index.rs:59-215) over pbs_fidx_parse.
class FixedIndexReader {
  public:
    FixedIndexReader(const uint8_t* image, size_t len) { parse(image, len); }
    explicit FixedIndexReader(const std::string& path) {
        std::FILE* f = std::fopen(path.c_str(), "rb");
        if (!f) throw std::runtime_error("Unable to open fixed index " + path);
        std::vector<uint8_t> image;
        uint8_t buf[65536];
        for (size_t k; (k = std::fread(buf, 1, sizeof buf, f)) > 0;) image.insert(image.end(), buf, buf + k);
        std::fclose(f);
        parse(image.data(), image.size());
    }

    std::array<uint8_t, 16> uuid{};
    int64_t ctime = 0;
    Digest index_csum{};
    uint64_t size = 0;        // bytes of the archive
    uint64_t chunk_size = 0;

    size_t index_count() const { return digests_.size() / 32; }
    uint64_t index_bytes() const { return size; }
    std::optional<Digest> index_digest(size_t pos) const {
        if (pos >= index_count()) return std::nullopt;
        Digest d;
        std::memcpy(d.data(), digests_.data() + 32 * pos, 32);
        return d;
    }
    std::optional<ChunkReadInfo> chunk_info(size_t pos) const {
        uint64_t s = 0, e = 0;
        if (pbs_fidx_chunk_info(size, chunk_size, pos, &s, &e) != PBS_OK) return std::nullopt;
        return ChunkReadInfo{s, e, *index_digest(pos)};
    }
    std::optional<std::pair<size_t, uint64_t>> chunk_from_offset(uint64_t offset) const {
        size_t idx = 0;
        uint64_t within = 0;
        if (pbs_fidx_chunk_from_offset(size, chunk_size, offset, &idx, &within) != PBS_OK) return std::nullopt;
        return std::make_pair(idx, within);
    }
    std::pair<Digest, uint64_t> compute_csum() const { return {csum_, size}; }
    const std::vector<uint8_t>& digests() const { return digests_; }  // 32 bytes per entry

  private:
    void parse(const uint8_t* image, size_t len) {
        const size_t cap = len > 4096 ? (len - 4096) / 32 : 0;
        digests_.resize(32 * cap);
        size_t n = 0;
        const int rc = pbs_fidx_parse(image, len, uuid.data(), &ctime, index_csum.data(), csum_.data(), &size,
                                      &chunk_size, digests_.data(), cap, &n);
        if (rc != PBS_OK) throw std::runtime_error(std::string("pbs_fidx_parse: ") + pbs_strerror(rc));
        digests_.resize(32 * n);
    }
    std::vector<uint8_t> digests_;
    Digest csum_{};
};

// FixedIndexWriter (fixed_index.rs:243-461) in memory: digests in any order (:394), close()
// returns index_csum and image() the .fidx bytes.  A slot never written holds zeros.
class FixedIndexWriter {
  public:
    FixedIndexWriter(uint64_t size, uint64_t chunk_size, const std::array<uint8_t, 16>& uuid, int64_t ctime)
        : size_(size), chunk_size_(chunk_size), uuid_(uuid), ctime_(ctime) {
        if (!chunk_size || (chunk_size & (chunk_size - 1))) throw std::invalid_argument("chunk_size: not a power of two");
        if (!size) throw std::invalid_argument("invalid index size");
        digests_.assign(32 * pbs_fidx_count(size, chunk_size), 0);
    }
    size_t index_length() const { return digests_.size() / 32; }
    size_t check_chunk_alignment(uint64_t end_offset, uint64_t chunk_len) const {
        size_t idx = 0;
        if (pbs_fidx_check_chunk_alignment(size_, chunk_size_, end_offset, chunk_len, &idx) != PBS_OK)
            throw std::runtime_error("chunk with unexpected offset or length");
        return idx;
    }
    void add_digest(size_t index, const Digest& digest) {
        if (index >= index_length()) throw std::out_of_range("add digest failed - index out of range");
        if (closed_) throw std::runtime_error("cannot write to closed index file.");
        std::memcpy(digests_.data() + 32 * index, digest.data(), 32);
    }
    void add_chunk(uint64_t end_offset, uint64_t chunk_len, const Digest& digest) {
        add_digest(check_chunk_alignment(end_offset, chunk_len), digest);
    }
    void clone_data_from(const FixedIndexReader& reader) {
        if (index_length() != reader.index_count()) throw std::runtime_error("clone_data_from failed - index sizes not equal");
        for (size_t i = 0; i < index_length(); ++i) add_digest(i, *reader.index_digest(i));
    }
    Digest close() {
        if (closed_) throw std::runtime_error("cannot close already closed index file.");
        closed_ = true;
        image_.resize(pbs_fidx_size(index_length()));
        Digest csum{};
        const int rc = pbs_fidx_build(digests_.data(), size_, chunk_size_, uuid_.data(), ctime_, image_.data(),
                                      image_.size(), csum.data());
        if (rc != PBS_OK) throw std::runtime_error(std::string("pbs_fidx_build: ") + pbs_strerror(rc));
        return csum;
    }
    const std::vector<uint8_t>& image() const {
        if (!closed_) throw std::runtime_error("the index is not closed yet");
        return image_;
    }

  private:
    uint64_t size_, chunk_size_;
    std::array<uint8_t, 16> uuid_;
    int64_t ctime_;
    std::vector<uint8_t> digests_, image_;
    bool closed_ = false;
};

// One garbage collection run (include/pbs_gc.h) over a chunk store's listing: digests (32 bytes
// per entry) and flags (PBS_GC_BAD / PBS_GC_FOREIGN).  device == true: the table lives in the
// memory of hip_stream's device and mark() takes device addresses; false: the host mirror.
class GarbageCollector {
  public:
    struct Sweep {
        std::vector<uint8_t> actions;  // PBS_GC_KEEP / PBS_GC_PENDING / PBS_GC_REMOVE per entry
        pbs_gc_status status;
    };

    GarbageCollector(const std::vector<uint8_t>& digests, const std::vector<uint8_t>& flags, bool device = true,
                     void* hip_stream = nullptr)
        : m_(flags.size()), device_(device) {
        if (digests.size() != 32 * m_) throw std::invalid_argument("32 bytes of digest per flag");
        const int rc = device_ ? pbs_gc_begin(digests.data(), flags.data(), m_, &dev_, &build_ms, hip_stream)
                               : pbs_gc_begin_host(digests.data(), flags.data(), m_, &host_, &build_ms);
        check(rc, "pbs_gc_begin");
    }
    ~GarbageCollector() { close(); }
    GarbageCollector(const GarbageCollector&) = delete;
    GarbageCollector& operator=(const GarbageCollector&) = delete;

    double build_ms = 0, mark_ms = 0, sweep_ms = 0;  // of the last such call

    void close() {
        if (dev_) pbs_gc_end(dev_);
        if (host_) pbs_gc_end_host(host_);
        dev_ = nullptr;
        host_ = nullptr;
    }
    size_t entries() const { return m_; }

    // The positions of the missing entries (ascending, at most `cap`) among the n digests at
    // base + i * stride; *n_missing counts them all.  index_bytes: one index file (counted in the
    // status); std::nullopt: a piece of one.
    std::vector<uint32_t> mark(const uint8_t* base, size_t stride, size_t n, std::optional<uint64_t> index_bytes,
                               size_t cap, size_t* n_missing = nullptr) {
        std::vector<uint32_t> pos(cap);
        size_t nm = 0;
        uint32_t* out = cap ? pos.data() : nullptr;
        int rc;
        if (device_)
            rc = index_bytes ? pbs_gc_mark_device(dev_, base, stride, n, *index_bytes, out, cap, &nm, &mark_ms)
                             : pbs_gc_mark_piece(dev_, base, stride, n, out, cap, &nm, &mark_ms);
        else
            rc = index_bytes ? pbs_gc_mark_host(host_, base, stride, n, *index_bytes, out, cap, &nm, &mark_ms)
                             : pbs_gc_mark_piece_host(host_, base, stride, n, out, cap, &nm, &mark_ms);
        check(rc, "pbs_gc_mark");
        pos.resize(std::min(cap, nm));
        if (n_missing) *n_missing = nm;
        return pos;
    }
    // A whole .didx / .fidx image (host memory): the positions of all its missing entries.
    std::vector<uint32_t> mark_index(const uint8_t* image, size_t len, size_t* n_missing = nullptr) {
        const size_t cap = len > 4096 ? (len - 4096) / 32 : 0;
        std::vector<uint32_t> pos(cap);
        size_t nm = 0;
        uint32_t* out = cap ? pos.data() : nullptr;
        const int rc = device_ ? pbs_gc_mark_index_image(dev_, image, len, out, cap, &nm, &mark_ms)
                               : pbs_gc_mark_index_image_host(host_, image, len, out, cap, &nm, &mark_ms);
        check(rc, "pbs_gc_mark_index_image");
        pos.resize(std::min(cap, nm));
        if (n_missing) *n_missing = nm;
        return pos;
    }
    std::vector<uint8_t> touched() {
        std::vector<uint8_t> t(m_);
        check(device_ ? pbs_gc_touched(dev_, t.data(), nullptr) : pbs_gc_touched_host(host_, t.data(), nullptr),
              "pbs_gc_touched");
        return t;
    }
    Sweep sweep(const std::vector<uint64_t>& sizes, const std::vector<int64_t>& atimes, int64_t phase1_start,
                int64_t oldest_writer) {
        if (sizes.size() != m_ || atimes.size() != m_) throw std::invalid_argument("one size and atime per entry");
        Sweep s;
        s.actions.resize(m_);
        check(device_ ? pbs_gc_sweep(dev_, sizes.data(), atimes.data(), phase1_start, oldest_writer, s.actions.data(),
                                     &s.status, &sweep_ms)
                      : pbs_gc_sweep_host(host_, sizes.data(), atimes.data(), phase1_start, oldest_writer,
                                          s.actions.data(), &s.status, &sweep_ms),
              "pbs_gc_sweep");
        return s;
    }

  private:
    static void check(int rc, const char* what) {
        if (rc != PBS_OK) throw std::runtime_error(std::string(what) + ": " + pbs_strerror(rc));
    }
    size_t m_;
    bool device_;
    pbs_gc* dev_ = nullptr;
    pbs_gc_host* host_ = nullptr;
};

// The verify job's worker (include/pbs_verify.h) over a chunk store's listing (32 bytes of digest
// per chunk file): the states of its chunks live from index to index and snapshot to snapshot.
// device == true: table and states live in the memory of hip_stream's device and the blobs handed
// to submit / verify_index are device memory; false: the host mirror.
class VerifyWorker {
  public:
    struct Outcome {
        pbs_verify_result result;
        std::vector<uint32_t> corrupt_store;  // the store positions that became CORRUPT: the files to rename
        std::vector<uint32_t> missing_pos;    // the index positions whose chunk is absent
    };
    struct Plan {
        std::vector<uint32_t> todo_store, todo_entry;
    };

    explicit VerifyWorker(const std::vector<uint8_t>& digests, bool device = true, void* hip_stream = nullptr)
        : m_(digests.size() / 32), device_(device) {
        if (digests.size() != 32 * m_) throw std::invalid_argument("32 bytes of digest per entry");
        const int rc = device_ ? pbs_verify_begin(digests.data(), m_, &dev_, &build_ms, hip_stream)
                               : pbs_verify_begin_host(digests.data(), m_, &host_, &build_ms);
        check(rc, "pbs_verify_begin");
    }
    ~VerifyWorker() { close(); }
    VerifyWorker(const VerifyWorker&) = delete;
    VerifyWorker& operator=(const VerifyWorker&) = delete;

    double build_ms = 0, plan_ms = 0;  // of the last such call
    pbs_verify_timing timing{};        // of the last submit

    void close() {
        if (dev_) pbs_verify_end(dev_);
        if (host_) pbs_verify_end_host(host_);
        dev_ = nullptr;
        host_ = nullptr;
    }
    size_t entries() const { return m_; }

    std::vector<uint8_t> states() {
        std::vector<uint8_t> s(m_);
        check(device_ ? pbs_verify_states(dev_, s.data(), m_) : pbs_verify_states_host(host_, s.data(), m_),
              "pbs_verify_states");
        return s;
    }
    // The chunk files to read for an index of n entries (digests: 32 n bytes, sizes: n), in read order.
    Plan plan(const std::vector<uint8_t>& digests, const std::vector<uint64_t>& sizes, int index_mode) {
        const size_t n = sizes.size(), cap = std::min(n, m_);
        if (digests.size() != 32 * n) throw std::invalid_argument("32 bytes of digest per size");
        Plan p;
        p.todo_store.resize(cap);
        p.todo_entry.resize(cap);
        size_t k = 0;
        const int rc = device_ ? pbs_verify_plan(dev_, digests.data(), sizes.data(), n, index_mode, p.todo_store.data(),
                                                 p.todo_entry.data(), cap, &k, &plan_ms)
                               : pbs_verify_plan_host(host_, digests.data(), sizes.data(), n, index_mode,
                                                      p.todo_store.data(), p.todo_entry.data(), cap, &k, &plan_ms);
        check(rc, "pbs_verify_plan");
        p.todo_store.resize(std::min(cap, k));
        p.todo_entry.resize(std::min(cap, k));
        return p;
    }
    void abort_index() {
        check(device_ ? pbs_verify_abort_index(dev_) : pbs_verify_abort_index_host(host_), "pbs_verify_abort_index");
    }
    // The plan's next blob_offsets.size() - 1 items as raw blob images; returns their status codes.
    std::vector<uint8_t> submit(const uint8_t* blobs, const std::vector<uint64_t>& blob_offsets,
                                const uint8_t* load_failed = nullptr, std::vector<uint8_t>* kinds = nullptr) {
        const size_t k = blob_offsets.empty() ? 0 : blob_offsets.size() - 1;
        std::vector<uint8_t> status(k), kd(k);
        const int rc = device_ ? pbs_verify_submit(dev_, blobs, blob_offsets.data(), load_failed, k, kd.data(),
                                                   status.data(), &timing)
                               : pbs_verify_submit_host(host_, blobs, blob_offsets.data(), load_failed, k, kd.data(),
                                                        status.data(), &timing);
        check(rc, "pbs_verify_submit");
        if (kinds) *kinds = kd;
        return status;
    }
    // `entries`: the index's length (bounds missing_pos).
    Outcome finish(size_t entries) {
        Outcome o;
        o.corrupt_store.resize(m_);
        o.missing_pos.resize(entries);
        size_t nc = 0, nm = 0;
        const int rc = device_ ? pbs_verify_finish(dev_, &o.result, o.corrupt_store.data(), m_, &nc,
                                                   o.missing_pos.data(), entries, &nm)
                               : pbs_verify_finish_host(host_, &o.result, o.corrupt_store.data(), m_, &nc,
                                                        o.missing_pos.data(), entries, &nm);
        check(rc, "pbs_verify_finish");
        o.corrupt_store.resize(std::min(m_, nc));
        o.missing_pos.resize(std::min(entries, nm));
        return o;
    }
    // A whole .didx / .fidx image against a resident store (store entry j: [store_offsets[j],
    // store_offsets[j + 1]) of store_blobs).  info_size / info_csum: the manifest's, or nullptr.
    Outcome verify_index(const uint8_t* image, size_t len, int index_mode, const uint64_t* info_size,
                         const uint8_t* info_csum, const uint8_t* store_blobs,
                         const std::vector<uint64_t>& store_offsets, size_t budget_bytes = 0) {
        if (store_offsets.size() != m_ + 1) throw std::invalid_argument("one offset per entry and one more");
        Outcome o;
        const size_t entries = len > 4096 ? (len - 4096) / 32 : 0;
        o.corrupt_store.resize(m_);
        o.missing_pos.resize(entries);
        size_t nc = 0, nm = 0;
        const int rc =
            device_ ? pbs_verify_index_device(dev_, image, len, index_mode, info_size, info_csum, store_blobs,
                                              store_offsets.data(), budget_bytes, &o.result, o.corrupt_store.data(), m_,
                                              &nc, o.missing_pos.data(), entries, &nm)
                    : pbs_verify_index_host(host_, image, len, index_mode, info_size, info_csum, store_blobs,
                                            store_offsets.data(), budget_bytes, &o.result, o.corrupt_store.data(), m_, &nc,
                                            o.missing_pos.data(), entries, &nm);
        check(rc, "pbs_verify_index");
        o.corrupt_store.resize(std::min(m_, nc));
        o.missing_pos.resize(std::min(entries, nm));
        return o;
    }

  private:
    static void check(int rc, const char* what) {
        if (rc != PBS_OK) throw std::runtime_error(std::string(what) + ": " + pbs_strerror(rc));
    }
    size_t m_;
    bool device_;
    pbs_verify* dev_ = nullptr;
    pbs_verify_host* host_ = nullptr;
};

// The sync job's worker (include/pbs_sync.h) over the local chunk store's listing (32 bytes of
// digest per chunk file): the store as it grows, and the claims of the current group.
// device == true: table, digest list, present and claimed bytes live in the memory of hip_stream's
// device and the blobs handed to submit are device memory; false: the host mirror.
class SyncWorker {
  public:
    struct Plan {
        uint32_t index_check = PBS_VERIFY_INDEX_OK;  // of plan_index; not OK: nothing was claimed, no index is open
        std::vector<uint8_t> verdict;                // PBS_SYNC_DUP / EXISTS / FETCH per entry
        std::vector<uint32_t> fetch_store, fetch_entry, touch_store;
    };
    struct Listing {
        std::vector<uint8_t> digests, present;  // 32 and 1 per entry
    };

    explicit SyncWorker(const std::vector<uint8_t>& digests, size_t reserve = 0, bool device = true,
                        void* hip_stream = nullptr)
        : device_(device) {
        const size_t m = digests.size() / 32;
        if (digests.size() != 32 * m) throw std::invalid_argument("32 bytes of digest per entry");
        const int rc = device_ ? pbs_sync_begin(digests.data(), m, reserve, &dev_, &build_ms, hip_stream)
                               : pbs_sync_begin_host(digests.data(), m, reserve, &host_, &build_ms);
        check(rc, "pbs_sync_begin");
    }
    ~SyncWorker() { close(); }
    SyncWorker(const SyncWorker&) = delete;
    SyncWorker& operator=(const SyncWorker&) = delete;

    double build_ms = 0, plan_ms = 0;  // of the last such call
    pbs_sync_timing timing{};          // of the last submit

    void close() {
        if (dev_) pbs_sync_end(dev_);
        if (host_) pbs_sync_end_host(host_);
        dev_ = nullptr;
        host_ = nullptr;
    }
    size_t count() { return device_ ? pbs_sync_count(dev_) : pbs_sync_count_host(host_); }
    uint32_t table_log2() { return device_ ? pbs_sync_table_log2(dev_) : pbs_sync_table_log2_host(host_); }
    Listing listing() {
        Listing l;
        const size_t c = count();
        l.digests.resize(32 * c);
        l.present.resize(c);
        check(device_ ? pbs_sync_listing(dev_, l.digests.data(), l.present.data(), c, nullptr)
                      : pbs_sync_listing_host(host_, l.digests.data(), l.present.data(), c, nullptr),
              "pbs_sync_listing");
        return l;
    }
    // A fresh downloaded_chunks: the next group.
    void new_group() { check(device_ ? pbs_sync_new_group(dev_) : pbs_sync_new_group_host(host_), "pbs_sync_new_group"); }
    // The verdicts and the two lists for an index of n entries (digests: 32 n bytes, sizes: n).
    Plan plan(const std::vector<uint8_t>& digests, const std::vector<uint64_t>& sizes) {
        const size_t n = sizes.size();
        if (digests.size() != 32 * n) throw std::invalid_argument("32 bytes of digest per size");
        Plan p;
        p.verdict.resize(n);
        p.fetch_store.resize(n);
        p.fetch_entry.resize(n);
        p.touch_store.resize(n);
        size_t nf = 0, nt = 0;
        const int rc = device_ ? pbs_sync_plan(dev_, digests.data(), sizes.data(), n, p.verdict.data(), p.fetch_store.data(),
                                               p.fetch_entry.data(), n, &nf, p.touch_store.data(), n, &nt, &plan_ms)
                               : pbs_sync_plan_host(host_, digests.data(), sizes.data(), n, p.verdict.data(),
                                                    p.fetch_store.data(), p.fetch_entry.data(), n, &nf,
                                                    p.touch_store.data(), n, &nt, &plan_ms);
        check(rc, "pbs_sync_plan");
        p.fetch_store.resize(nf);
        p.fetch_entry.resize(nf);
        p.touch_store.resize(nt);
        return p;
    }
    // The same for a .didx / .fidx image, after verify_archive against the manifest's FileInfo
    // (info_size / info_csum, or nullptr).
    Plan plan_index(const uint8_t* image, size_t len, const uint64_t* info_size, const uint8_t* info_csum) {
        const size_t cap = len > 4096 ? (len - 4096) / 32 : 0;
        Plan p;
        p.verdict.resize(cap);
        p.fetch_store.resize(cap);
        p.fetch_entry.resize(cap);
        p.touch_store.resize(cap);
        size_t n = 0, nf = 0, nt = 0;
        const int rc =
            device_ ? pbs_sync_index_image(dev_, image, len, info_size, info_csum, &p.index_check, &n, p.verdict.data(), cap,
                                           p.fetch_store.data(), p.fetch_entry.data(), cap, &nf, p.touch_store.data(), cap,
                                           &nt, &plan_ms)
                    : pbs_sync_index_image_host(host_, image, len, info_size, info_csum, &p.index_check, &n,
                                                p.verdict.data(), cap, p.fetch_store.data(), p.fetch_entry.data(), cap, &nf,
                                                p.touch_store.data(), cap, &nt, &plan_ms);
        check(rc, "pbs_sync_index_image");
        p.verdict.resize(p.index_check == PBS_VERIFY_INDEX_OK ? n : 0);
        p.fetch_store.resize(nf);
        p.fetch_entry.resize(nf);
        p.touch_store.resize(nt);
        return p;
    }
    // The next blob_offsets.size() - 1 fetch items as raw blob images; returns their status codes.
    std::vector<uint8_t> submit(const uint8_t* blobs, const std::vector<uint64_t>& blob_offsets,
                                const uint8_t* load_failed = nullptr, std::vector<uint8_t>* kinds = nullptr) {
        const size_t k = blob_offsets.empty() ? 0 : blob_offsets.size() - 1;
        std::vector<uint8_t> status(k), kd(k);
        const int rc = device_ ? pbs_sync_submit(dev_, blobs, blob_offsets.data(), load_failed, k, kd.data(), status.data(),
                                                 &timing)
                               : pbs_sync_submit_host(host_, blobs, blob_offsets.data(), load_failed, k, kd.data(),
                                                      status.data(), &timing);
        check(rc, "pbs_sync_submit");
        if (kinds) *kinds = kd;
        return status;
    }
    pbs_sync_result finish() {
        pbs_sync_result r;
        check(device_ ? pbs_sync_finish(dev_, &r) : pbs_sync_finish_host(host_, &r), "pbs_sync_finish");
        return r;
    }
    void abort_index() {
        check(device_ ? pbs_sync_abort_index(dev_) : pbs_sync_abort_index_host(host_), "pbs_sync_abort_index");
    }

  private:
    static void check(int rc, const char* what) {
        if (rc != PBS_OK) throw std::runtime_error(std::string(what) + ": " + pbs_strerror(rc));
    }
    bool device_;
    pbs_sync* dev_ = nullptr;
    pbs_sync_host* host_ = nullptr;
};

// One backup session on one datastore (include/pbs_backup.h: BackupEnvironment, UploadChunk and
// ChunkStore::insert_chunk) over the store's listing: per chunk file 32 bytes of digest, its
// length and its magic.  device == true: table, digest list and per-entry state live in the
// memory of hip_stream's device and the blobs handed to upload are device memory; false: the
// host mirror.  A call returns 0 or the positive PBS_BACKUP_E_* code with which the reference's
// request fails; a negative code throws.
class BackupSession {
  public:
    struct Listing {
        std::vector<uint8_t> digests, present, kind, known;  // 32, 1, 1 and 1 per entry
        std::vector<uint64_t> size;
        std::vector<uint32_t> known_size;
    };
    struct Uploaded {
        int code = 0;  // PBS_OK or PBS_BACKUP_E_*
        std::vector<uint8_t> status, ins, action, is_duplicate, reg;
        std::vector<uint32_t> crc, compressed_size;
        uint64_t first_failed = PBS_BACKUP_NONE;
    };
    struct Appended {
        int code = 0;
        size_t n_done = 0;
        int err = 0;
    };
    struct Closed {
        int code = 0, result = 0;
        std::vector<uint8_t> image;  // result == 0: the .didx / .fidx image
        pbs_backup_writer_stat stat{};
    };

    BackupSession(const std::vector<uint8_t>& digests, const std::vector<uint64_t>& sizes,
                  const std::vector<uint8_t>& kinds, size_t reserve = 0, bool device = true, void* hip_stream = nullptr)
        : device_(device) {
        const size_t m = sizes.size();
        if (digests.size() != 32 * m || kinds.size() != m) throw std::invalid_argument("32 bytes of digest, a size and a kind per entry");
        const int rc = device_ ? pbs_backup_begin(digests.data(), sizes.data(), kinds.data(), m, reserve, &dev_, &build_ms, hip_stream)
                               : pbs_backup_begin_host(digests.data(), sizes.data(), kinds.data(), m, reserve, &host_, &build_ms);
        check(rc, "pbs_backup_begin");
    }
    ~BackupSession() { close(); }
    BackupSession(const BackupSession&) = delete;
    BackupSession& operator=(const BackupSession&) = delete;

    double build_ms = 0, ms = 0;   // of the begin; of the last register_previous / append
    pbs_backup_timing timing{};    // of the last upload

    void close() {
        if (dev_) pbs_backup_end(dev_);
        if (host_) pbs_backup_end_host(host_);
        dev_ = nullptr;
        host_ = nullptr;
    }
    size_t count() { return device_ ? pbs_backup_count(dev_) : pbs_backup_count_host(host_); }
    uint32_t table_log2() { return device_ ? pbs_backup_table_log2(dev_) : pbs_backup_table_log2_host(host_); }
    Listing listing() {
        Listing l;
        const size_t c = count();
        l.digests.resize(32 * c);
        l.present.resize(c);
        l.kind.resize(c);
        l.known.resize(c);
        l.size.resize(c);
        l.known_size.resize(c);
        check(device_ ? pbs_backup_listing(dev_, l.digests.data(), l.present.data(), l.size.data(), l.kind.data(),
                                           l.known.data(), l.known_size.data(), c, nullptr)
                      : pbs_backup_listing_host(host_, l.digests.data(), l.present.data(), l.size.data(), l.kind.data(),
                                                l.known.data(), l.known_size.data(), c, nullptr),
              "pbs_backup_listing");
        return l;
    }
    // lookup_chunk
    std::optional<uint32_t> lookup(const uint8_t digest[32]) {
        uint32_t size = 0;
        const int rc = check(device_ ? pbs_backup_lookup(dev_, digest, &size) : pbs_backup_lookup_host(host_, digest, &size),
                             "pbs_backup_lookup");
        return rc == PBS_OK ? std::optional<uint32_t>(size) : std::nullopt;
    }
    pbs_backup_stat stats() {
        pbs_backup_stat s;
        check(device_ ? pbs_backup_stats(dev_, &s) : pbs_backup_stats_host(host_, &s), "pbs_backup_stats");
        return s;
    }
    int finish() { return check(device_ ? pbs_backup_finish(dev_, nullptr) : pbs_backup_finish_host(host_, nullptr), "pbs_backup_finish"); }
    int register_previous(const std::vector<uint8_t>& digests, const std::vector<uint32_t>& sizes) {
        if (digests.size() != 32 * sizes.size()) throw std::invalid_argument("32 bytes of digest per size");
        return check(device_ ? pbs_backup_register_previous(dev_, digests.data(), sizes.data(), sizes.size(), &ms)
                             : pbs_backup_register_previous_host(host_, digests.data(), sizes.data(), sizes.size(), &ms),
                     "pbs_backup_register_previous");
    }
    int register_index_image(const uint8_t* image, size_t len, size_t* n_entries = nullptr) {
        return check(device_ ? pbs_backup_register_index_image(dev_, image, len, n_entries, &ms)
                             : pbs_backup_register_index_image_host(host_, image, len, n_entries, &ms),
                     "pbs_backup_register_index_image");
    }
    // k = blob_offsets.size() - 1 chunks for writer wid; encoded_sizes may be empty (as announced)
    Uploaded upload(uint32_t wid, const std::vector<uint8_t>& digests, const std::vector<uint32_t>& sizes, const uint8_t* blobs,
                    const std::vector<uint64_t>& blob_offsets, const std::vector<uint32_t>& encoded_sizes = {}) {
        const size_t k = blob_offsets.empty() ? 0 : blob_offsets.size() - 1;
        if (sizes.size() != k || digests.size() != 32 * k || (!encoded_sizes.empty() && encoded_sizes.size() != k))
            throw std::invalid_argument("a digest and a size per blob");
        Uploaded u;
        for (auto* v : {&u.status, &u.ins, &u.action, &u.is_duplicate, &u.reg}) v->resize(k);
        u.crc.resize(k);
        u.compressed_size.resize(k);
        const uint32_t* es = encoded_sizes.empty() ? nullptr : encoded_sizes.data();
        const int rc =
            device_ ? pbs_backup_upload(dev_, wid, digests.data(), sizes.data(), es, blobs, blob_offsets.data(), k, u.status.data(),
                                        u.crc.data(), u.ins.data(), u.action.data(), u.is_duplicate.data(),
                                        u.compressed_size.data(), u.reg.data(), &u.first_failed, &timing)
                    : pbs_backup_upload_host(host_, wid, digests.data(), sizes.data(), es, blobs, blob_offsets.data(), k,
                                             u.status.data(), u.crc.data(), u.ins.data(), u.action.data(),
                                             u.is_duplicate.data(), u.compressed_size.data(), u.reg.data(), &u.first_failed,
                                             &timing);
        u.code = check(rc, "pbs_backup_upload");
        return u;
    }
    // (code, wid)
    std::pair<int, uint32_t> create_dynamic(const uint8_t* uuid = nullptr, int64_t ctime = 0) {
        uint32_t wid = 0;
        const int rc = check(device_ ? pbs_backup_create_dynamic(dev_, uuid, ctime, &wid)
                                     : pbs_backup_create_dynamic_host(host_, uuid, ctime, &wid),
                             "pbs_backup_create_dynamic");
        if (rc == PBS_OK) entries_[wid] = 0;
        return {rc, wid};
    }
    std::pair<int, uint32_t> create_fixed(uint64_t size, uint64_t chunk_size, const uint8_t* uuid = nullptr, int64_t ctime = 0,
                                          const uint8_t* reuse_image = nullptr, size_t reuse_len = 0,
                                          const uint8_t* reuse_csum = nullptr) {
        uint32_t wid = 0;
        const int rc = check(device_ ? pbs_backup_create_fixed(dev_, size, chunk_size, uuid, ctime, reuse_image, reuse_len,
                                                               reuse_csum, &wid)
                                     : pbs_backup_create_fixed_host(host_, size, chunk_size, uuid, ctime, reuse_image,
                                                                    reuse_len, reuse_csum, &wid),
                             "pbs_backup_create_fixed");
        if (rc == PBS_OK) entries_[wid] = pbs_fidx_count(size, chunk_size);
        return {rc, wid};
    }
    Appended dynamic_append(uint32_t wid, const std::vector<uint8_t>& digests, const std::vector<uint64_t>& offsets) {
        Appended a = append(false, wid, digests, offsets);
        if (a.code == PBS_OK) entries_[wid] += a.n_done;
        return a;
    }
    Appended fixed_append(uint32_t wid, const std::vector<uint8_t>& digests, const std::vector<uint64_t>& offsets) {
        return append(true, wid, digests, offsets);
    }
    Closed dynamic_close(uint32_t wid, uint64_t chunk_count, uint64_t size, const uint8_t csum[32]) {
        return close_writer(false, wid, chunk_count, size, csum);
    }
    Closed fixed_close(uint32_t wid, uint64_t chunk_count, uint64_t size, const uint8_t csum[32]) {
        return close_writer(true, wid, chunk_count, size, csum);
    }
    // (code, PBS_BLOB_ST_* of from_raw + verify_crc)
    std::pair<int, uint8_t> add_blob(const uint8_t* raw, size_t len) {
        uint8_t st = 0;
        const int rc = check(device_ ? pbs_backup_add_blob(dev_, raw, len, &st) : pbs_backup_add_blob_host(host_, raw, len, &st),
                             "pbs_backup_add_blob");
        return {rc, st};
    }

  private:
    static int check(int rc, const char* what) {
        if (rc < 0) throw std::runtime_error(std::string(what) + ": " + pbs_strerror(rc));
        return rc;
    }
    Appended append(bool fixed, uint32_t wid, const std::vector<uint8_t>& digests, const std::vector<uint64_t>& offsets) {
        const size_t n = offsets.size();
        if (digests.size() != 32 * n) throw std::invalid_argument("32 bytes of digest per offset");
        Appended a;
        int rc;
        if (fixed)
            rc = device_ ? pbs_backup_fixed_append(dev_, wid, digests.data(), offsets.data(), n, &a.n_done, &a.err, &ms)
                         : pbs_backup_fixed_append_host(host_, wid, digests.data(), offsets.data(), n, &a.n_done, &a.err, &ms);
        else
            rc = device_ ? pbs_backup_dynamic_append(dev_, wid, digests.data(), offsets.data(), n, &a.n_done, &a.err, &ms)
                         : pbs_backup_dynamic_append_host(host_, wid, digests.data(), offsets.data(), n, &a.n_done, &a.err, &ms);
        a.code = check(rc, fixed ? "pbs_backup_fixed_append" : "pbs_backup_dynamic_append");
        return a;
    }
    Closed close_writer(bool fixed, uint32_t wid, uint64_t chunk_count, uint64_t size, const uint8_t* csum) {
        Closed c;
        auto it = entries_.find(wid);
        const size_t n = it == entries_.end() ? 0 : it->second;
        c.image.resize(fixed ? pbs_fidx_size(n) : pbs_didx_size(n));
        int rc;
        if (fixed)
            rc = device_ ? pbs_backup_fixed_close(dev_, wid, chunk_count, size, csum, c.image.data(), c.image.size(), &c.result, &c.stat)
                         : pbs_backup_fixed_close_host(host_, wid, chunk_count, size, csum, c.image.data(), c.image.size(),
                                                       &c.result, &c.stat);
        else
            rc = device_ ? pbs_backup_dynamic_close(dev_, wid, chunk_count, size, csum, c.image.data(), c.image.size(), &c.result, &c.stat)
                         : pbs_backup_dynamic_close_host(host_, wid, chunk_count, size, csum, c.image.data(), c.image.size(),
                                                         &c.result, &c.stat);
        c.code = check(rc, fixed ? "pbs_backup_fixed_close" : "pbs_backup_dynamic_close");
        if (c.code == PBS_OK && c.result != PBS_BACKUP_E_NO_WRITER) entries_.erase(wid);  // (gone, whatever the checks said)
        if (c.code != PBS_OK || c.result != PBS_BACKUP_E_NONE) c.image.clear();
        return c;
    }
    bool device_;
    pbs_backup* dev_ = nullptr;
    pbs_backup_host* host_ = nullptr;
    std::map<uint32_t, size_t> entries_;  // wid -> index entries (what the close's image holds)
};

}  // namespace pbs
