"""Python host mirror of proxmox-backup's chunker interface over the C ABI
(include/pbs_chunker.h, built as proxmox-backup_amd/csrc/libpbschunk.so).

Mirrors, with the same names, argument meaning and error behaviour:
  * ``Chunker(chunk_size_avg)`` / ``Chunker.scan(data) -> int``
      pbs-datastore/src/chunker.rs:75-106 and :112-168.  A non-power-of-two average
      raises (the reference panics: "got unexpected chunk size - not a power of two.").
  * ``ChunkStream(input, chunk_size=None)`` -- iterator of chunks (bytes)
      pbs-client/src/chunk_stream.rs:12-78 (default average 4 MiB, tail emitted at EOF).
  * ``DynamicChunkWriter(sink, chunk_size)`` -- ``write(data) -> consumed`` / ``close()``
      pbs-datastore/src/dynamic_index.rs:397-523, with the digest/compress/index step
      replaced by a callback ``sink(chunk_end_offset, chunk_bytes)``.
  * ``digest_chunks_device(...)`` -- per-chunk SHA-256 on the GPU,
      ``DataChunkBuilder::digest`` (pbs-datastore/src/data_blob.rs:516-536; with a key,
      ``CryptConfig::compute_digest``, pbs-tools/src/crypt_config.rs:79-84).
  * ``DynamicIndexWriter(path)`` -- ``add_chunk(offset, digest)`` / ``close() -> csum``
      pbs-datastore/src/dynamic_index.rs:297-391 (.didx image built by the C library).
  * ``DynamicIndexReader(bytes or path)`` -- ``index_count`` / ``chunk_info`` / ``chunk_from_offset`` ...
      pbs-datastore/src/dynamic_index.rs:82-275, and ``restore_range_device`` /
      ``restore_stream_device``: the bytes of an archive range from an index and a blob store
      (``BufferedDynamicReader`` :544-673 over ``ReadChunk::read_chunk``; include/pbs_restore.h).

The hash scan always runs on the GPU through the HIP library; there is no CPU path.
Loading fails loudly (``ChunkerLibraryError``) when the library is missing and handle
creation fails when no HIP device is visible.
"""
from __future__ import annotations

import ctypes
import os
from typing import Callable, Iterable, Iterator, Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libpbschunk.so")
# (diagnostics only: an A/B against another build of the same library, e.g. a PMC run of
# the previous round's kernels; the product path loads the in-tree build)
if os.environ.get("PBS_LIBPBSCHUNK_AB"):
    LIB_PATH = os.environ["PBS_LIBPBSCHUNK_AB"]

PBS_OK = 0
PBS_ERR_NOT_POW2 = -1
PBS_ERR_NO_DEVICE = -2
PBS_ERR_HIP = -3
PBS_ERR_NOMEM = -4
PBS_ERR_CAPACITY = -5
PBS_ERR_INVALID = -6

GEN_COUNTER, GEN_RANDOM, GEN_VMIMAGE = 0, 1, 2

EXPORTED_SYMBOLS = (
    "pbs_chunker_new", "pbs_chunker_free", "pbs_chunker_scan", "pbs_chunker_find_cuts",
    "pbs_chunker_find_cuts_device", "pbs_chunker_max_cuts", "pbs_chunker_cuts_bound",
    "pbs_chunker_stream_offset",
    "pbs_chunker_chunk_start", "pbs_chunker_reset", "pbs_chunker_set_stream",
    "pbs_chunker_last_error", "pbs_strerror", "pbs_chunker_last_timing",
    "pbs_candidates_host", "pbs_generate_device", "pbs_device_count", "pbs_table_copy", "pbs_build_id",
    "pbs_chunker_candidates_device", "pbs_chunker_resolve_device",
    # include/pbs_digest.h (chunk digests, dynamic index)
    "pbs_digest_chunks_device", "pbs_digest_chunks_async", "pbs_sha256", "pbs_didx_size",
    "pbs_didx_build", "pbs_known_chunks_device", "pbs_pipeline_host", "pbs_chunker_set_cu_count",
    "pbs_digest_chunks_hybrid", "pbs_digest_chunks_host", "pbs_sha256_host_uses_ni",
    # include/pbs_blob.h (blob CRC)
    "pbs_crc32_chunks_device", "pbs_crc32_chunks_async", "pbs_crc32", "pbs_blob_encode_uncompressed",
    "pbs_blob_encode_chunks_device", "pbs_blob_stream_bound", "pbs_zstd_frame_bound",
    "pbs_blob_encode_release", "pbs_digest_hybrid_release", "pbs_debug_arena_allocs",
    "pbs_pipeline_release", "pbs_blob_encode_spans_device", "pbs_upload_stream_host",
    # encrypted blobs (include/pbs_blob.h: crypt config, AES-256-GCM)
    "pbs_crypt_config_new", "pbs_crypt_config_id_key", "pbs_crypt_config_free", "pbs_aes256gcm_encrypt_host",
    "pbs_blob_encode_chunks_encrypted_device", "pbs_blob_encode_spans_encrypted_device",
    "pbs_blob_stream_bound_encrypted", "pbs_upload_stream_host_crypt",
    # reading blobs (include/pbs_blob.h: CRC, AES-256-GCM open, digests)
    "pbs_blob_decode_device", "pbs_blob_decode_bound", "pbs_aes256gcm_decrypt_host", "pbs_blob_decode_host",
    # inflating zstd frames (include/pbs_blob.h)
    "pbs_zstd_inflate_device", "pbs_zstd_inflate_host", "pbs_zstd_frame_content_size",
    "pbs_blob_decode_inflate_device",
    # restoring a .didx stream (include/pbs_restore.h)
    "pbs_didx_count", "pbs_didx_parse", "pbs_didx_chunk_from_offset", "pbs_digest_lookup_device",
    "pbs_digest_lookup_host", "pbs_copy_segments_device", "pbs_restore_range_device", "pbs_restore_release",
    # the fixed-size chunk path (include/pbs_fixed.h)
    "pbs_fidx_count", "pbs_fidx_size", "pbs_fidx_build", "pbs_fidx_parse", "pbs_fidx_chunk_info",
    "pbs_fidx_chunk_from_offset", "pbs_fidx_check_chunk_alignment", "pbs_fixed_dirty_device", "pbs_fixed_dirty_host",
    "pbs_fixed_digests_device", "pbs_upload_fixed_host", "pbs_upload_fixed_host_crypt",
    "pbs_restore_fixed_range_device",
    # garbage collection (include/pbs_gc.h)
    "pbs_gc_begin", "pbs_gc_mark_device", "pbs_gc_mark_piece", "pbs_gc_mark_index_image", "pbs_gc_touched",
    "pbs_gc_sweep", "pbs_gc_end", "pbs_gc_release", "pbs_gc_table_log2", "pbs_gc_home_slot",
    "pbs_gc_begin_host", "pbs_gc_mark_host", "pbs_gc_mark_piece_host", "pbs_gc_mark_index_image_host",
    "pbs_gc_touched_host", "pbs_gc_sweep_host", "pbs_gc_end_host",
    # the verify job (include/pbs_verify.h)
    "pbs_verify_begin", "pbs_verify_states", "pbs_verify_end", "pbs_verify_release", "pbs_verify_plan",
    "pbs_verify_abort_index", "pbs_verify_submit", "pbs_verify_finish", "pbs_verify_index_device",
    "pbs_verify_blob_host", "pbs_verify_begin_host", "pbs_verify_states_host", "pbs_verify_end_host",
    "pbs_verify_plan_host", "pbs_verify_abort_index_host", "pbs_verify_submit_host", "pbs_verify_finish_host",
    "pbs_verify_index_host",
    # the sync job (include/pbs_sync.h)
    "pbs_sync_begin", "pbs_sync_count", "pbs_sync_table_log2", "pbs_sync_listing", "pbs_sync_new_group",
    "pbs_sync_end", "pbs_sync_release", "pbs_sync_plan", "pbs_sync_lists", "pbs_sync_submit", "pbs_sync_finish",
    "pbs_sync_abort_index", "pbs_sync_index_image",
    "pbs_sync_begin_host", "pbs_sync_count_host", "pbs_sync_table_log2_host", "pbs_sync_listing_host",
    "pbs_sync_new_group_host", "pbs_sync_end_host", "pbs_sync_plan_host", "pbs_sync_lists_host",
    "pbs_sync_submit_host", "pbs_sync_finish_host", "pbs_sync_abort_index_host", "pbs_sync_index_image_host",
    # the backup session (include/pbs_backup.h)
    "pbs_backup_release",
) + tuple(name + sfx for sfx in ("", "_host") for name in (
    "pbs_backup_begin", "pbs_backup_count", "pbs_backup_table_log2", "pbs_backup_listing", "pbs_backup_lookup",
    "pbs_backup_stats", "pbs_backup_finish", "pbs_backup_end", "pbs_backup_register_previous",
    "pbs_backup_register_index_image", "pbs_backup_upload",
    "pbs_backup_create_dynamic", "pbs_backup_create_fixed", "pbs_backup_dynamic_append", "pbs_backup_fixed_append",
    "pbs_backup_dynamic_close", "pbs_backup_fixed_close", "pbs_backup_add_blob"))


class ChunkerLibraryError(RuntimeError):
    pass


class ChunkerError(RuntimeError):
    def __init__(self, code: int, what: str = ""):
        self.code = code
        super().__init__(f"{what}: {strerror(code)} ({code})" if what else f"{strerror(code)} ({code})")


class Timing(ctypes.Structure):
    _fields_ = [
        ("scan_ms", ctypes.c_float), ("exact_ms", ctypes.c_float),
        ("resolve_ms", ctypes.c_float), ("total_ms", ctypes.c_float),
        ("bytes", ctypes.c_uint64), ("suspects", ctypes.c_uint64),
        ("candidates", ctypes.c_uint64), ("cuts", ctypes.c_uint64),
        ("fused", ctypes.c_uint64), ("scan_pass", ctypes.c_uint64),
    ]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class PipelineTiming(ctypes.Structure):
    _fields_ = [
        ("total_ms", ctypes.c_double), ("h2d_ms", ctypes.c_double),
        ("chunk_ms", ctypes.c_double), ("drain_ms", ctypes.c_double),
        ("bytes", ctypes.c_uint64), ("chunks", ctypes.c_uint64), ("pieces", ctypes.c_uint64),
        ("host_chunks", ctypes.c_uint64), ("host_bytes", ctypes.c_uint64),
        ("host_done_ms", ctypes.c_double), ("host_threads", ctypes.c_int),
        ("gpu_jobs", ctypes.c_uint64), ("gpu_claimed", ctypes.c_uint64), ("queue_launches", ctypes.c_uint64),
        ("gpu_done_ms", ctypes.c_double), ("host_work_ms", ctypes.c_double),
    ]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class BlobEncodeTiming(ctypes.Structure):
    _fields_ = [
        ("total_ms", ctypes.c_double), ("compress_ms", ctypes.c_double),
        ("assemble_ms", ctypes.c_double), ("crc_ms", ctypes.c_double),
        ("bytes_in", ctypes.c_uint64), ("bytes_out", ctypes.c_uint64),
        ("blocks", ctypes.c_uint64), ("compressed_chunks", ctypes.c_uint64),
    ]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class BlobEncodeTimingCrypt(ctypes.Structure):
    _fields_ = [("base", BlobEncodeTiming), ("encrypt_ms", ctypes.c_double), ("gcm_segments", ctypes.c_uint64)]

    def as_dict(self) -> dict:
        d = self.base.as_dict()
        d["encrypt_ms"] = self.encrypt_ms
        d["gcm_segments"] = self.gcm_segments
        return d


class BlobDecodeTiming(ctypes.Structure):
    _fields_ = [
        ("total_ms", ctypes.c_double), ("classify_ms", ctypes.c_double), ("crc_ms", ctypes.c_double),
        ("decrypt_ms", ctypes.c_double), ("digest_ms", ctypes.c_double),
        ("bytes_in", ctypes.c_uint64), ("bytes_out", ctypes.c_uint64),
        ("gcm_segments", ctypes.c_uint64), ("failed", ctypes.c_uint64),
    ]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class ZstdInflateTiming(ctypes.Structure):
    _fields_ = [
        ("total_ms", ctypes.c_double), ("inflate_ms", ctypes.c_double),
        ("bytes_in", ctypes.c_uint64), ("bytes_out", ctypes.c_uint64), ("frames", ctypes.c_uint64),
        ("failed", ctypes.c_uint64), ("workgroups", ctypes.c_uint64),
    ]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class BlobDecodeInflateTiming(ctypes.Structure):
    _fields_ = [("base", BlobDecodeTiming), ("inflate_ms", ctypes.c_double), ("frames", ctypes.c_uint64)]

    def as_dict(self) -> dict:
        d = self.base.as_dict()
        d["inflate_ms"] = self.inflate_ms
        d["frames"] = self.frames
        return d


class RestoreTiming(ctypes.Structure):
    _fields_ = [
        ("total_ms", ctypes.c_double), ("lookup_ms", ctypes.c_double), ("pack_ms", ctypes.c_double),
        ("decode_ms", ctypes.c_double), ("scatter_ms", ctypes.c_double),
        ("entries", ctypes.c_uint64), ("unique", ctypes.c_uint64), ("missing", ctypes.c_uint64),
        ("failed", ctypes.c_uint64), ("blob_bytes", ctypes.c_uint64), ("decoded_bytes", ctypes.c_uint64),
        ("out_bytes", ctypes.c_uint64), ("decode", BlobDecodeInflateTiming),
    ]

    def as_dict(self) -> dict:
        return {k: (getattr(self, k).as_dict() if k == "decode" else getattr(self, k)) for k, _ in self._fields_}


class UploadTiming(ctypes.Structure):
    _fields_ = [
        ("pipe", PipelineTiming), ("known_ms", ctypes.c_double), ("encode_ms", ctypes.c_double),
        ("d2h_ms", ctypes.c_double), ("total_ms", ctypes.c_double),
        ("chunk_count", ctypes.c_uint64), ("chunk_reused", ctypes.c_uint64), ("size", ctypes.c_uint64),
        ("size_reused", ctypes.c_uint64), ("size_compressed", ctypes.c_uint64),
        ("compressed_chunks", ctypes.c_uint64), ("blob", BlobEncodeTiming),
    ]

    def as_dict(self) -> dict:
        return {k: (getattr(self, k).as_dict() if k in ("pipe", "blob") else getattr(self, k))
                for k, _ in self._fields_}


class FixedDigestTiming(ctypes.Structure):
    _fields_ = [("total_ms", ctypes.c_double), ("gpu_ms", ctypes.c_double),
                ("hashed_chunks", ctypes.c_uint64), ("hashed_bytes", ctypes.c_uint64)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class UploadFixedTiming(ctypes.Structure):
    _fields_ = [("up", UploadTiming), ("dirty_chunks", ctypes.c_uint64), ("copied_bytes", ctypes.c_uint64)]

    def as_dict(self) -> dict:
        d = self.up.as_dict()
        d["dirty_chunks"] = self.dirty_chunks
        d["copied_bytes"] = self.copied_bytes
        return d


class GcStatus(ctypes.Structure):
    """pbs_gc_status: GarbageCollectionStatus (pbs-api-types/src/datastore.rs:1308-1330) without upid."""
    _fields_ = [(k, ctypes.c_uint64) for k in (
        "index_file_count", "index_data_bytes", "disk_bytes", "disk_chunks", "removed_bytes", "removed_chunks",
        "pending_bytes", "pending_chunks", "removed_bad", "still_bad")]

    def as_dict(self) -> dict:
        """The kebab-case keys the reference serialises into .gc-status."""
        return {k.replace("_", "-"): int(getattr(self, k)) for k, _ in self._fields_}


class VerifyResult(ctypes.Structure):
    """pbs_verify_result: the counts of one verified index."""
    _fields_ = [(k, ctypes.c_uint64) for k in (
        "entries", "skipped_verified", "skipped_corrupt", "loaded", "newly_verified", "newly_corrupt",
        "mode_mismatch", "missing", "read_bytes", "decoded_bytes", "errors")] + [
        ("ok", ctypes.c_uint32), ("index_check", ctypes.c_uint32)]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class VerifyTiming(ctypes.Structure):
    """pbs_verify_timing: one submit."""
    _fields_ = [("total_ms", ctypes.c_double), ("magic_ms", ctypes.c_double), ("decode_ms", ctypes.c_double),
                ("state_ms", ctypes.c_double), ("blobs", ctypes.c_uint64), ("decoded", ctypes.c_uint64),
                ("encrypted", ctypes.c_uint64), ("scratch_bytes", ctypes.c_uint64)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class SyncResult(ctypes.Structure):
    """pbs_sync_result: the counts of one pulled index."""
    _fields_ = [(k, ctypes.c_uint64) for k in (
        "entries", "dup", "exists", "fetch", "appended", "inserted", "failed", "load_failed", "chunk_count",
        "bytes", "first_failed")] + [("ok", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "reserved"}


class BackupWriterStat(ctypes.Structure):
    """pbs_backup_writer_stat: UploadStatistic and the numbers of log_upload_stat."""
    _fields_ = [(k, ctypes.c_uint64) for k in (
        "count", "size", "compressed_size", "duplicates", "chunk_count", "archive_size", "upload_percent",
        "client_duplicates", "server_duplicates", "duplicate_percent", "compression_percent")] + [
        ("logged", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "reserved"}


class BackupStat(ctypes.Structure):
    """pbs_backup_stat: the session's counters."""
    _fields_ = [(k, ctypes.c_uint64) for k in ("file_counter", "backup_size", "count", "size", "compressed_size",
                                               "duplicates")] + [("open_writers", ctypes.c_uint32),
                                                                 ("finished", ctypes.c_uint32)]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class BackupTiming(ctypes.Structure):
    _fields_ = [("total_ms", ctypes.c_double), ("decode_ms", ctypes.c_double), ("insert_ms", ctypes.c_double),
                ("blobs", ctypes.c_uint64), ("decoded", ctypes.c_uint64), ("encrypted", ctypes.c_uint64),
                ("scratch_bytes", ctypes.c_uint64)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class HybridOpts(ctypes.Structure):
    _fields_ = [
        ("host_threads", ctypes.c_int), ("host_min_len", ctypes.c_uint64),
        ("host_mb_s", ctypes.c_double), ("gpu_mb_s", ctypes.c_double),
    ]


class HybridTiming(ctypes.Structure):
    _fields_ = [
        ("total_ms", ctypes.c_double), ("zero_ms", ctypes.c_double),
        ("gpu_ms", ctypes.c_double), ("host_ms", ctypes.c_double),
        ("gpu_chunks", ctypes.c_uint64), ("host_chunks", ctypes.c_uint64),
        ("host_bytes", ctypes.c_uint64), ("zero_chunks", ctypes.c_uint64),
        ("zero_lengths", ctypes.c_uint64), ("threshold", ctypes.c_uint64),
        ("threads", ctypes.c_int),
    ]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


_lib = None


def lib():
    """Load libpbschunk.so (no fallback: raises if it is missing)."""
    global _lib
    if _lib is not None:
        return _lib
    # torch wheels bundle their own libamdhip64.so.7; load it first so this library
    # binds to the same HIP runtime instead of a second copy from /opt/rocm.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise ChunkerLibraryError(
            f"{LIB_PATH} not built; run `make -C proxmox-backup_amd/csrc` or __graft_entry__.build()")
    L = ctypes.CDLL(LIB_PATH)
    p, u64, sz, i = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_int
    dbl = ctypes.POINTER(ctypes.c_double)
    sig = {
        "pbs_chunker_new": ([sz, ctypes.POINTER(i)], p),
        "pbs_chunker_free": ([p], None),
        "pbs_chunker_scan": ([p, p, sz], sz),
        "pbs_chunker_find_cuts": ([p, p, sz, i, p, sz, ctypes.POINTER(sz)], i),
        "pbs_chunker_find_cuts_device": ([p, p, sz, i, p, sz, ctypes.POINTER(sz)], i),
        "pbs_chunker_max_cuts": ([sz], sz),
        "pbs_chunker_cuts_bound": ([p, sz], sz),
        "pbs_chunker_stream_offset": ([p], u64),
        "pbs_chunker_chunk_start": ([p], u64),
        "pbs_chunker_reset": ([p], i),
        "pbs_chunker_set_stream": ([p, p], i),
        "pbs_chunker_last_error": ([p], i),
        "pbs_strerror": ([i], ctypes.c_char_p),
        "pbs_chunker_last_timing": ([p, ctypes.POINTER(Timing)], i),
        "pbs_candidates_host": ([p, sz, sz, p, sz, ctypes.POINTER(sz)], i),
        "pbs_generate_device": ([p, sz, i, u64, u64, p], i),
        "pbs_device_count": ([], i),
        "pbs_table_copy": ([p], i),
        "pbs_build_id": ([], ctypes.c_char_p),
        "pbs_debug_arena_allocs": ([], u64),
        "pbs_chunker_candidates_device": ([p, p, sz, p, sz, u64, p, sz, ctypes.POINTER(sz)], i),
        "pbs_chunker_resolve_device": ([p, p, sz, u64, i, p, sz, ctypes.POINTER(sz)], i),
        "pbs_digest_chunks_device": ([p, sz, u64, p, sz, p, sz, p, p], i),
        "pbs_digest_chunks_async": ([p, sz, u64, p, p, sz, p, sz, p, p], i),
        "pbs_sha256": ([p, sz, p], None),
        "pbs_didx_size": ([sz], sz),
        "pbs_didx_build": ([p, p, sz, p, ctypes.c_int64, p, sz, p], i),
        "pbs_known_chunks_device": ([p, sz, p, sz, p, ctypes.POINTER(sz), p], i),
        "pbs_pipeline_host": ([sz, p, sz, sz, p, sz, i, p, p, p, sz, ctypes.POINTER(sz),
                               ctypes.POINTER(PipelineTiming)], i),
        "pbs_chunker_set_cu_count": ([p, i], i),
        "pbs_digest_chunks_hybrid": ([p, p, sz, u64, p, sz, p, sz, p, ctypes.POINTER(HybridOpts),
                                      ctypes.POINTER(HybridTiming), p], i),
        "pbs_digest_chunks_host": ([p, sz, u64, p, sz, p, sz, p, i], i),
        "pbs_sha256_host_uses_ni": ([], i),
        "pbs_crc32_chunks_device": ([p, sz, u64, p, sz, p, p], i),
        "pbs_crc32_chunks_async": ([p, sz, u64, p, p, sz, p, p], i),
        "pbs_crc32": ([ctypes.c_uint32, p, sz], ctypes.c_uint32),
        "pbs_blob_encode_uncompressed": ([p, sz, ctypes.c_uint32, p, sz], sz),
        "pbs_blob_encode_chunks_device": ([p, sz, u64, p, sz, i, p, sz, p, p, p,
                                           ctypes.POINTER(BlobEncodeTiming), p], i),
        "pbs_blob_encode_spans_device": ([p, sz, u64, p, sz, i, p, sz, p, p, p,
                                          ctypes.POINTER(BlobEncodeTiming), p], i),
        "pbs_upload_stream_host": ([sz, p, sz, sz, p, sz, i, p, sz, i, p, p, p, sz, ctypes.POINTER(sz),
                                    p, sz, p, p, ctypes.POINTER(UploadTiming)], i),
        "pbs_blob_stream_bound": ([p, sz], sz),
        "pbs_crypt_config_new": ([p, ctypes.POINTER(p)], i),
        "pbs_crypt_config_id_key": ([p], p),
        "pbs_crypt_config_free": ([p], None),
        "pbs_aes256gcm_encrypt_host": ([p, p, p, sz, p, p], i),
        "pbs_blob_encode_chunks_encrypted_device": ([p, sz, u64, p, sz, i, p, p, p, sz, p, p, p,
                                                     ctypes.POINTER(BlobEncodeTimingCrypt), p], i),
        "pbs_blob_encode_spans_encrypted_device": ([p, sz, u64, p, sz, i, p, p, p, sz, p, p, p,
                                                    ctypes.POINTER(BlobEncodeTimingCrypt), p], i),
        "pbs_blob_stream_bound_encrypted": ([p, sz], sz),
        "pbs_upload_stream_host_crypt": ([sz, p, sz, sz, p, i, p, sz, i, p, p, p, sz, ctypes.POINTER(sz),
                                          p, sz, p, p, ctypes.POINTER(UploadTiming),
                                          ctypes.POINTER(ctypes.c_double)], i),
        "pbs_blob_decode_device": ([p, p, sz, p, p, p, p, sz, p, p, p, ctypes.POINTER(BlobDecodeTiming), p], i),
        "pbs_blob_decode_bound": ([p, sz], sz),
        "pbs_aes256gcm_decrypt_host": ([p, p, p, sz, p, p], i),
        "pbs_blob_decode_host": ([p, sz, p, p, p, p, sz, ctypes.POINTER(sz), p, p], i),
        "pbs_blob_decode_inflate_device": ([p, p, sz, p, p, p, i, p, sz, p, p, p, p,
                                            ctypes.POINTER(BlobDecodeInflateTiming), p], i),
        "pbs_zstd_inflate_device": ([p, p, sz, p, p, p, p, ctypes.POINTER(ZstdInflateTiming), p], i),
        "pbs_zstd_inflate_host": ([p, sz, p, sz, ctypes.POINTER(sz), p], i),
        "pbs_zstd_frame_content_size": ([p, sz, ctypes.POINTER(u64)], i),
        "pbs_zstd_frame_bound": ([sz], sz),
        "pbs_didx_count": ([sz], sz),
        "pbs_didx_parse": ([p, sz, p, ctypes.POINTER(ctypes.c_int64), p, p, p, p, sz, ctypes.POINTER(sz)], i),
        "pbs_didx_chunk_from_offset": ([p, sz, u64, ctypes.POINTER(sz), ctypes.POINTER(u64)], i),
        "pbs_digest_lookup_device": ([p, sz, p, sz, p, p, ctypes.POINTER(sz), ctypes.POINTER(sz), p], i),
        "pbs_digest_lookup_host": ([p, sz, p, sz, p, p, ctypes.POINTER(sz), ctypes.POINTER(sz)], i),
        "pbs_copy_segments_device": ([p, p, p, p, p, sz, p], i),
        "pbs_restore_range_device": ([p, p, sz, p, p, p, sz, p, u64, u64, p, p, ctypes.POINTER(RestoreTiming), p], i),
        "pbs_restore_release": ([], None),
        "pbs_fidx_count": ([u64, u64], sz),
        "pbs_fidx_size": ([sz], sz),
        "pbs_fidx_build": ([p, u64, u64, p, ctypes.c_int64, p, sz, p], i),
        "pbs_fidx_parse": ([p, sz, p, ctypes.POINTER(ctypes.c_int64), p, p, ctypes.POINTER(u64), ctypes.POINTER(u64),
                            p, sz, ctypes.POINTER(sz)], i),
        "pbs_fidx_chunk_info": ([u64, u64, sz, ctypes.POINTER(u64), ctypes.POINTER(u64)], i),
        "pbs_fidx_chunk_from_offset": ([u64, u64, u64, ctypes.POINTER(sz), ctypes.POINTER(u64)], i),
        "pbs_fidx_check_chunk_alignment": ([u64, u64, u64, u64, ctypes.POINTER(sz)], i),
        "pbs_fixed_dirty_device": ([p, p, u64, u64, p, ctypes.POINTER(sz), p], i),
        "pbs_fixed_dirty_host": ([p, p, u64, u64, p, ctypes.POINTER(sz)], i),
        "pbs_fixed_digests_device": ([p, u64, u64, p, sz, p, p, p, p, ctypes.POINTER(FixedDigestTiming), p], i),
        "pbs_upload_fixed_host": ([u64, p, sz, sz, p, sz, i, p, sz, i, p, p, p, p, p, sz, ctypes.POINTER(sz),
                                   p, sz, p, p, p, ctypes.POINTER(UploadFixedTiming)], i),
        "pbs_upload_fixed_host_crypt": ([u64, p, sz, sz, p, i, p, sz, i, p, p, p, p, p, sz, ctypes.POINTER(sz),
                                         p, sz, p, p, p, ctypes.POINTER(UploadFixedTiming),
                                         ctypes.POINTER(ctypes.c_double)], i),
        "pbs_restore_fixed_range_device": ([p, sz, u64, u64, p, p, p, sz, p, u64, u64, p, p,
                                            ctypes.POINTER(RestoreTiming), p], i),
        "pbs_gc_begin": ([p, p, sz, ctypes.POINTER(p), dbl, p], i),
        "pbs_gc_mark_device": ([p, p, sz, sz, u64, p, sz, ctypes.POINTER(sz), dbl], i),
        "pbs_gc_mark_piece": ([p, p, sz, sz, p, sz, ctypes.POINTER(sz), dbl], i),
        "pbs_gc_mark_index_image": ([p, p, sz, p, sz, ctypes.POINTER(sz), dbl], i),
        "pbs_gc_touched": ([p, p, ctypes.POINTER(sz)], i),
        "pbs_gc_sweep": ([p, p, p, ctypes.c_int64, ctypes.c_int64, p, ctypes.POINTER(GcStatus), dbl], i),
        "pbs_gc_end": ([p], None),
        "pbs_gc_release": ([], None),
        "pbs_gc_table_log2": ([p], ctypes.c_uint32),
        "pbs_gc_home_slot": ([p, ctypes.c_uint32], u64),
        "pbs_gc_begin_host": ([p, p, sz, ctypes.POINTER(p), dbl], i),
        "pbs_gc_mark_host": ([p, p, sz, sz, u64, p, sz, ctypes.POINTER(sz), dbl], i),
        "pbs_gc_mark_piece_host": ([p, p, sz, sz, p, sz, ctypes.POINTER(sz), dbl], i),
        "pbs_gc_mark_index_image_host": ([p, p, sz, p, sz, ctypes.POINTER(sz), dbl], i),
        "pbs_gc_touched_host": ([p, p, ctypes.POINTER(sz)], i),
        "pbs_gc_sweep_host": ([p, p, p, ctypes.c_int64, ctypes.c_int64, p, ctypes.POINTER(GcStatus), dbl], i),
        "pbs_gc_end_host": ([p], None),
        "pbs_verify_begin": ([p, sz, ctypes.POINTER(p), dbl, p], i),
        "pbs_verify_states": ([p, p, sz], i),
        "pbs_verify_end": ([p], None),
        "pbs_verify_release": ([], None),
        "pbs_verify_plan": ([p, p, p, sz, i, p, p, sz, ctypes.POINTER(sz), dbl], i),
        "pbs_verify_abort_index": ([p], i),
        "pbs_verify_submit": ([p, p, p, p, sz, p, p, ctypes.POINTER(VerifyTiming)], i),
        "pbs_verify_finish": ([p, ctypes.POINTER(VerifyResult), p, sz, ctypes.POINTER(sz), p, sz,
                               ctypes.POINTER(sz)], i),
        "pbs_verify_index_device": ([p, p, sz, i, ctypes.POINTER(u64), p, p, p, sz, ctypes.POINTER(VerifyResult),
                                     p, sz, ctypes.POINTER(sz), p, sz, ctypes.POINTER(sz)], i),
        "pbs_verify_blob_host": ([p, sz, u64, p, ctypes.POINTER(i)], i),
        "pbs_verify_begin_host": ([p, sz, ctypes.POINTER(p), dbl], i),
        "pbs_verify_states_host": ([p, p, sz], i),
        "pbs_verify_end_host": ([p], None),
        "pbs_verify_plan_host": ([p, p, p, sz, i, p, p, sz, ctypes.POINTER(sz), dbl], i),
        "pbs_verify_abort_index_host": ([p], i),
        "pbs_verify_submit_host": ([p, p, p, p, sz, p, p, ctypes.POINTER(VerifyTiming)], i),
        "pbs_verify_finish_host": ([p, ctypes.POINTER(VerifyResult), p, sz, ctypes.POINTER(sz), p, sz,
                                    ctypes.POINTER(sz)], i),
        "pbs_verify_index_host": ([p, p, sz, i, ctypes.POINTER(u64), p, p, p, sz, ctypes.POINTER(VerifyResult),
                                   p, sz, ctypes.POINTER(sz), p, sz, ctypes.POINTER(sz)], i),
        "pbs_sync_release": ([], None),
        "pbs_blob_encode_release": ([], None),
        "pbs_digest_hybrid_release": ([], None),
        "pbs_pipeline_release": ([], None),
        # test hooks (not in include/): tile plans and the fused pass's record epoch
        "pbs_test_fused_static_plan": ([u64, u64, ctypes.POINTER(u64)], i),
        "pbs_test_scan_main_plan": ([u64, i, ctypes.POINTER(u64)], i),
        "pbs_test_set_fused_epoch": ([p, ctypes.c_uint32], i),
        "pbs_test_handle_stats": ([p, ctypes.POINTER(u64)], i),
        "pbs_test_gcm_tag_segments_host": ([p, p, p, sz, p], i),
    }
    psz = ctypes.POINTER(sz)
    for sfx, tail in (("", [p]), ("_host", [])):  # (the device calls and the mirror's: the same but for the stream)
        sig.update({
            "pbs_sync_begin" + sfx: ([p, sz, sz, ctypes.POINTER(p), dbl] + tail, i),
            "pbs_sync_count" + sfx: ([p], sz),
            "pbs_sync_table_log2" + sfx: ([p], ctypes.c_uint32),
            "pbs_sync_listing" + sfx: ([p, p, p, sz, psz], i),
            "pbs_sync_new_group" + sfx: ([p], i),
            "pbs_sync_end" + sfx: ([p], None),
            "pbs_sync_plan" + sfx: ([p, p, p, sz, p, p, p, sz, psz, p, sz, psz, dbl], i),
            "pbs_sync_lists" + sfx: ([p, p, p, sz, psz, p, sz, psz], i),
            "pbs_sync_submit" + sfx: ([p, p, p, p, sz, p, p, ctypes.POINTER(VerifyTiming)], i),
            "pbs_sync_finish" + sfx: ([p, ctypes.POINTER(SyncResult)], i),
            "pbs_sync_abort_index" + sfx: ([p], i),
            "pbs_sync_index_image" + sfx: ([p, p, sz, ctypes.POINTER(u64), p, ctypes.POINTER(ctypes.c_uint32), psz, p, sz,
                                            p, p, sz, psz, p, sz, psz, dbl], i),
        })
        u32, i64, pi = ctypes.c_uint32, ctypes.c_int64, ctypes.POINTER(i)
        sig.update({
            "pbs_backup_begin" + sfx: ([p, p, p, sz, sz, ctypes.POINTER(p), dbl] + tail, i),
            "pbs_backup_count" + sfx: ([p], sz),
            "pbs_backup_table_log2" + sfx: ([p], u32),
            "pbs_backup_listing" + sfx: ([p, p, p, p, p, p, p, sz, psz], i),
            "pbs_backup_lookup" + sfx: ([p, p, ctypes.POINTER(u32)], i),
            "pbs_backup_stats" + sfx: ([p, ctypes.POINTER(BackupStat)], i),
            "pbs_backup_finish" + sfx: ([p, ctypes.POINTER(BackupStat)], i),
            "pbs_backup_end" + sfx: ([p], None),
            "pbs_backup_register_previous" + sfx: ([p, p, p, sz, dbl], i),
            "pbs_backup_register_index_image" + sfx: ([p, p, sz, psz, dbl], i),
            "pbs_backup_upload" + sfx: ([p, u32, p, p, p, p, p, sz, p, p, p, p, p, p, p, ctypes.POINTER(u64),
                                         ctypes.POINTER(BackupTiming)], i),
            "pbs_backup_create_dynamic" + sfx: ([p, p, i64, ctypes.POINTER(u32)], i),
            "pbs_backup_create_fixed" + sfx: ([p, u64, u64, p, i64, p, sz, p, ctypes.POINTER(u32)], i),
            "pbs_backup_dynamic_append" + sfx: ([p, u32, p, p, sz, psz, pi, dbl], i),
            "pbs_backup_fixed_append" + sfx: ([p, u32, p, p, sz, psz, pi, dbl], i),
            "pbs_backup_dynamic_close" + sfx: ([p, u32, u64, u64, p, p, sz, pi, ctypes.POINTER(BackupWriterStat)], i),
            "pbs_backup_fixed_close" + sfx: ([p, u32, u64, u64, p, p, sz, pi, ctypes.POINTER(BackupWriterStat)], i),
            "pbs_backup_add_blob" + sfx: ([p, p, sz, p], i),
        })
    sig["pbs_backup_release"] = ([], None)
    for name, (args, res) in sig.items():
        if os.environ.get("PBS_LIBPBSCHUNK_AB") and not hasattr(L, name):
            continue  # (an older build in an A/B run: the symbols it has)
        f = getattr(L, name)
        f.argtypes = args
        f.restype = res
    _lib = L
    return L


def strerror(code: int) -> str:
    return lib().pbs_strerror(code).decode()


def device_count() -> int:
    return int(lib().pbs_device_count())


def table() -> np.ndarray:
    t = np.empty(256, dtype=np.uint32)
    lib().pbs_table_copy(t.ctypes.data)
    return t


def build_id() -> str:
    """Digest of the sources the loaded library was built from (pbs_build_id)."""
    return lib().pbs_build_id().decode()


def max_cuts(length: int) -> int:
    return int(lib().pbs_chunker_max_cuts(length))


def _as_u8(data) -> np.ndarray:
    if isinstance(data, np.ndarray):
        return np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    return np.frombuffer(memoryview(data).cast("B"), dtype=np.uint8)


def _ptr(a: np.ndarray) -> Optional[int]:
    return a.ctypes.data if a.size else None


class Chunker:
    """`pbs_datastore::Chunker` (chunker.rs:18) backed by the gfx950 kernels."""

    def __init__(self, chunk_size_avg: int):
        L = lib()
        err = ctypes.c_int(0)
        h = L.pbs_chunker_new(int(chunk_size_avg), ctypes.byref(err))
        if not h:
            if err.value == PBS_ERR_NOT_POW2:
                # the reference panics here (chunker.rs:87-89)
                raise ValueError("got unexpected chunk size - not a power of two.")
            raise ChunkerError(err.value, "pbs_chunker_new")
        self._h = ctypes.c_void_p(h)
        self.chunk_size_avg = int(chunk_size_avg)

    def close(self):
        if getattr(self, "_h", None):
            lib().pbs_chunker_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc: int, what: str):
        if rc != PBS_OK:
            raise ChunkerError(rc, what)

    def scan(self, data) -> int:
        """chunker.rs:112 -- 0 (no boundary, slice consumed) or the position after the cut."""
        a = _as_u8(data)
        r = lib().pbs_chunker_scan(self._h, _ptr(a), a.size)
        if r == ctypes.c_size_t(-1).value:
            raise ChunkerError(lib().pbs_chunker_last_error(self._h), "pbs_chunker_scan")
        return int(r)

    def cuts_bound(self, length: int) -> int:
        """Output capacity find_cuts needs for ``length`` bytes at this average."""
        return int(lib().pbs_chunker_cuts_bound(self._h, length))

    def _out(self, cap: int) -> np.ndarray:
        # one output array per handle, grown as needed: a fresh multi-MiB array per call
        # would page-fault on every first touch
        buf = getattr(self, "_outbuf", None)
        if buf is None or buf.size < cap:
            buf = self._outbuf = np.empty(cap, dtype=np.uint64)
        return buf

    def find_cuts(self, data, is_final: bool = False) -> np.ndarray:
        """Chunk END offsets (absolute) of every cut decided inside ``data``."""
        a = _as_u8(data)
        cap = self.cuts_bound(a.size)
        out = self._out(cap)
        n = ctypes.c_size_t(0)
        rc = lib().pbs_chunker_find_cuts(self._h, _ptr(a), a.size, int(bool(is_final)),
                                        out.ctypes.data, cap, ctypes.byref(n))
        self._check(rc, "pbs_chunker_find_cuts")
        return out[: n.value].copy()

    def find_cuts_device(self, dev_ptr: int, length: int, is_final: bool = False,
                         out: Optional[np.ndarray] = None) -> np.ndarray:
        """Same over a device (HBM) buffer, e.g. ``tensor.data_ptr()``.  With ``out`` (a
        writeable contiguous uint64 array of at least ``cuts_bound(length)`` entries, ideally
        pinned host memory so the cut list is DMA'd straight into it) the cuts are written
        there and a view of it is returned -- the next call with the same array overwrites
        that view; otherwise a fresh array."""
        cap = self.cuts_bound(length)
        if out is None:
            buf = self._out(cap)
        else:
            if (out.dtype != np.uint64 or not out.flags.c_contiguous or not out.flags.writeable
                    or out.size < cap):
                raise ValueError(f"out must be a writeable contiguous uint64 array of >= {cap} entries")
            buf = out
        n = ctypes.c_size_t(0)
        rc = lib().pbs_chunker_find_cuts_device(self._h, ctypes.c_void_p(dev_ptr), length,
                                               int(bool(is_final)), buf.ctypes.data, cap,
                                               ctypes.byref(n))
        self._check(rc, "pbs_chunker_find_cuts_device")
        return buf[: n.value] if out is not None else buf[: n.value].copy()

    def candidates_device(self, dev_ptr: int, length: int, pre: bytes, base: int,
                          out_dev_ptr: int, cap: int) -> int:
        """Phase A over device bytes [base, base+length) of a stream, given the
        min(base, 63) stream bytes before them (``pre``): sorted absolute candidate
        positions into the device array at ``out_dev_ptr`` (``cap`` u64 entries).
        Returns their number; raises ChunkerError(PBS_ERR_CAPACITY) with
        ``.needed`` set when cap is too small."""
        pre = bytes(pre)
        n = ctypes.c_size_t(0)
        rc = lib().pbs_chunker_candidates_device(
            self._h, ctypes.c_void_p(dev_ptr), length, pre if pre else None, len(pre), base,
            ctypes.c_void_p(out_dev_ptr) if cap else None, cap, ctypes.byref(n))
        if rc == PBS_ERR_CAPACITY:
            e = ChunkerError(rc, "pbs_chunker_candidates_device")
            e.needed = int(n.value)
            raise e
        self._check(rc, "pbs_chunker_candidates_device")
        return int(n.value)

    def resolve_device(self, cand_dev_ptr: int, n: int, end: int, is_final: bool = True) -> np.ndarray:
        """Phase B: cut list of a stream of ``end`` bytes from its complete sorted
        candidate list (device u64 array of ``n`` entries)."""
        cap = self.cuts_bound(end)
        out = np.empty(cap, dtype=np.uint64)
        k = ctypes.c_size_t(0)
        rc = lib().pbs_chunker_resolve_device(self._h, ctypes.c_void_p(cand_dev_ptr), n, end,
                                              int(bool(is_final)), out.ctypes.data, cap,
                                              ctypes.byref(k))
        self._check(rc, "pbs_chunker_resolve_device")
        return out[: k.value].copy()

    def set_stream(self, hip_stream: int):
        self._check(lib().pbs_chunker_set_stream(self._h, ctypes.c_void_p(hip_stream)),
                    "pbs_chunker_set_stream")

    def set_cu_count(self, cus: int):
        self._check(lib().pbs_chunker_set_cu_count(self._h, cus), "pbs_chunker_set_cu_count")

    def reset(self):
        self._check(lib().pbs_chunker_reset(self._h), "pbs_chunker_reset")

    def stats_for_test(self) -> dict:
        """Test hook: scan-server requests sent / served / given up, and the record epoch."""
        out = (ctypes.c_uint64 * 4)()
        self._check(lib().pbs_test_handle_stats(self._h, out), "pbs_test_handle_stats")
        return dict(zip(("requests", "served", "broken", "epoch"), (int(x) for x in out)))

    def set_fused_epoch_for_test(self, v: int):
        """Test hook: the 16-bit tile-record epoch of the last fused / scan pass."""
        self._check(lib().pbs_test_set_fused_epoch(self._h, int(v)), "pbs_test_set_fused_epoch")

    @property
    def stream_offset(self) -> int:
        return int(lib().pbs_chunker_stream_offset(self._h))

    @property
    def chunk_start(self) -> int:
        return int(lib().pbs_chunker_chunk_start(self._h))

    def last_timing(self) -> dict:
        t = Timing()
        self._check(lib().pbs_chunker_last_timing(self._h, ctypes.byref(t)), "last_timing")
        return t.as_dict()


class ChunkStream:
    """pbs-client/src/chunk_stream.rs:12-78: split an iterable of byte pieces into
    dynamic-size chunks (yields ``bytes``); the remainder is emitted at EOF."""

    def __init__(self, input: Iterable, chunk_size: Optional[int] = None):
        self.input = iter(input)
        self.chunker = Chunker(chunk_size if chunk_size is not None else 4 * 1024 * 1024)
        self.buffer = bytearray()
        self.scan_pos = 0
        self.eof = False
        # bytes gathered per device scan: each scan is a host->device round trip, so
        # scanning every small read piece would be latency-bound; the cuts are those of
        # the whole stream either way, only latency changes (0 = scan every piece)
        self.min_scan = 4 * 1024 * 1024

    def __iter__(self) -> Iterator[bytes]:
        return self

    def _pull(self) -> None:
        try:
            self.buffer += bytes(next(self.input))
        except StopIteration:
            self.eof = True

    def __next__(self) -> bytes:
        while True:
            while not self.eof and len(self.buffer) - self.scan_pos < max(self.min_scan, 1):
                self._pull()
            if self.scan_pos < len(self.buffer):
                boundary = self.chunker.scan(memoryview(self.buffer)[self.scan_pos:])
                chunk_size = self.scan_pos + boundary
                if boundary == 0:
                    self.scan_pos = len(self.buffer)
                elif chunk_size <= len(self.buffer):
                    result = bytes(self.buffer[:chunk_size])
                    del self.buffer[:chunk_size]
                    self.scan_pos = 0
                    return result
                else:
                    raise RuntimeError("got unexpected chunk boundary from chunker")
                continue
            self.scan_pos = 0
            if self.buffer:
                result = bytes(self.buffer)
                self.buffer = bytearray()
                return result
            raise StopIteration


class DynamicChunkWriter:
    """dynamic_index.rs:397-523 Write adapter: ``write`` returns the bytes consumed
    (re-submit the rest, as ``write_all`` does); ``close`` flushes the tail.  Each
    finished chunk goes to ``sink(chunk_end_offset, chunk_bytes)``."""

    def __init__(self, sink: Callable[[int, bytes], None], chunk_size: int):
        self.sink = sink
        self.chunker = Chunker(chunk_size)
        self.chunk_offset = 0
        self.last_chunk = 0
        self.chunk_buffer = bytearray()
        self.closed = False
        self.chunk_count = 0

    def _write_chunk_buffer(self):
        if not self.chunk_buffer:
            return
        expected = self.chunk_offset - self.last_chunk
        if expected != len(self.chunk_buffer):
            raise RuntimeError(f"wrong chunk size {expected} != {len(self.chunk_buffer)}")
        self.chunk_count += 1
        self.last_chunk = self.chunk_offset
        self.sink(self.chunk_offset, bytes(self.chunk_buffer))
        self.chunk_buffer = bytearray()

    def write(self, data) -> int:
        mv = memoryview(data).cast("B")
        pos = self.chunker.scan(mv)
        if pos > 0:
            self.chunk_buffer += mv[:pos]
            self.chunk_offset += pos
            self._write_chunk_buffer()
            return pos
        self.chunk_offset += len(mv)
        self.chunk_buffer += mv
        return len(mv)

    def write_all(self, data):
        mv = memoryview(data).cast("B")
        while len(mv):
            k = self.write(mv)
            mv = mv[k:]

    def close(self):
        if self.closed:
            return
        self.closed = True
        self._write_chunk_buffer()


def candidates_host(data, avg: int) -> np.ndarray:
    """Phase-A hook: positions p >= 63 whose window hash passes the cut test (GPU)."""
    a = _as_u8(data)
    cap = max(16, a.size)
    out = np.empty(cap, dtype=np.uint64)
    n = ctypes.c_size_t(0)
    rc = lib().pbs_candidates_host(_ptr(a), a.size, int(avg), out.ctypes.data, cap, ctypes.byref(n))
    if rc != PBS_OK:
        raise ChunkerError(rc, "pbs_candidates_host")
    return out[: n.value].copy()


def plan_fused_static(length: int, nw: int) -> dict:
    """Test hook: the static tile plan of the fused pass over ``nw`` scanner waves."""
    out = (ctypes.c_uint64 * 8)()
    rc = lib().pbs_test_fused_static_plan(int(length), int(nw), out)
    if rc != PBS_OK:
        raise ChunkerError(rc, "pbs_test_fused_static_plan")
    keys = ("ntiles", "seg_q", "t_long", "t_small", "seg_qs", "t_small_long", "covered", "pool")
    return dict(zip(keys, (int(x) for x in out)))


def plan_scan_main(length: int, cu: int) -> dict:
    """Test hook: scan_main's tile plan (tiles [0, t_big) of 64 x seg bytes, then seg / 4)."""
    out = (ctypes.c_uint64 * 5)()
    rc = lib().pbs_test_scan_main_plan(int(length), int(cu), out)
    if rc != PBS_OK:
        raise ChunkerError(rc, "pbs_test_scan_main_plan")
    return dict(zip(("seg", "ntiles", "t_big", "dyn", "covered"), (int(x) for x in out)))


def generate_device(dev_ptr: int, length: int, kind: int, seed: int, offset: int = 0,
                    hip_stream: int = 0):
    rc = lib().pbs_generate_device(ctypes.c_void_p(dev_ptr), length, kind, seed & (2**64 - 1),
                                   offset, ctypes.c_void_p(hip_stream))
    if rc != PBS_OK:
        raise ChunkerError(rc, "pbs_generate_device")


# ---- chunk digests and the dynamic index (include/pbs_digest.h) --------

DIDX_MAGIC = bytes([28, 145, 78, 165, 25, 186, 179, 205])  # file_formats.rs:24
DIDX_HEADER = 4096
DIDX_ENTRY = 40


def sha256(data) -> bytes:
    """Host SHA-256 of the C library (the index checksum's hash)."""
    a = _as_u8(data)
    out = (ctypes.c_uint8 * 32)()
    lib().pbs_sha256(_ptr(a), a.size, out)
    return bytes(out)


def _key_arg(key):
    if key is None:
        return None, 0
    k = bytes(key)
    if len(k) > 64:
        raise ValueError("key longer than PBS_DIGEST_MAX_KEY (64)")
    return ctypes.create_string_buffer(k, len(k) or 1), len(k)


def digest_chunks_device(dev_ptr: int, data_len: int, bounds, base: int = 0, key=None,
                         hip_stream: int = 0) -> np.ndarray:
    """SHA-256 (on the GPU) of every chunk [bounds[i], bounds[i+1]) of the stream whose
    bytes [base, base + data_len) are at device address dev_ptr; (n, 32) uint8 digests.
    ``key``: the crypt config's id_key, appended to every chunk's message."""
    b = np.ascontiguousarray(np.asarray(bounds, dtype=np.uint64))
    n = max(0, b.size - 1)
    out = np.empty((n, 32), dtype=np.uint8)
    if n == 0:
        return out
    kb, kl = _key_arg(key)
    rc = lib().pbs_digest_chunks_device(ctypes.c_void_p(dev_ptr), data_len, base, b.ctypes.data, n,
                                        kb, kl, out.ctypes.data, ctypes.c_void_p(hip_stream))
    if rc != PBS_OK:
        raise ChunkerError(rc, "pbs_digest_chunks_device")
    return out


def digest_chunks_hybrid(dev_ptr: int, data_len: int, bounds, base: int = 0, key=None,
                         host=None, threads: int = 0, host_min_len: int = 0,
                         host_mb_s: float = 0.0, gpu_mb_s: float = 0.0, hip_stream: int = 0):
    """pbs_digest_chunks_hybrid: the digests of digest_chunks_device with the longest
    chunks hashed on ``threads`` host threads (SHA extensions) and all-zero long chunks
    once per length; ``host`` (optional numpy uint8 array, the same bytes as the device
    range) lets the host threads read them without a copy from HBM.  Returns ((n, 32)
    digests, timing dict)."""
    b = np.ascontiguousarray(np.asarray(bounds, dtype=np.uint64))
    n = max(0, b.size - 1)
    out = np.empty((n, 32), dtype=np.uint8)
    t = HybridTiming()
    if n == 0:
        return out, t.as_dict()
    kb, kl = _key_arg(key)
    hp = None
    if host is not None:
        h = _as_u8(host)
        if h.size < data_len:
            raise ValueError("host copy shorter than data_len")
        hp = _ptr(h)
    o = HybridOpts(threads, host_min_len, host_mb_s, gpu_mb_s)
    rc = lib().pbs_digest_chunks_hybrid(ctypes.c_void_p(dev_ptr), hp, data_len, base, b.ctypes.data, n,
                                        kb, kl, out.ctypes.data, ctypes.byref(o), ctypes.byref(t),
                                        ctypes.c_void_p(hip_stream))
    if rc != PBS_OK:
        raise ChunkerError(rc, "pbs_digest_chunks_hybrid")
    return out, t.as_dict()


def digest_chunks_host(data, bounds, base: int = 0, key=None, threads: int = 0) -> np.ndarray:
    """SHA-256(chunk || key) of every chunk of a host buffer on host threads (the C
    library's SHA-extension code); (n, 32) uint8 digests."""
    a = _as_u8(data)
    b = np.ascontiguousarray(np.asarray(bounds, dtype=np.uint64))
    n = max(0, b.size - 1)
    out = np.empty((n, 32), dtype=np.uint8)
    if n == 0:
        return out
    kb, kl = _key_arg(key)
    rc = lib().pbs_digest_chunks_host(_ptr(a), a.size, base, b.ctypes.data, n, kb, kl, out.ctypes.data,
                                      threads)
    if rc != PBS_OK:
        raise ChunkerError(rc, "pbs_digest_chunks_host")
    return out


def sha256_host_uses_ni() -> bool:
    return bool(lib().pbs_sha256_host_uses_ni())


def digest_chunks_async(dev_ptr: int, data_len: int, bounds_dev: int, order_dev: int, n: int,
                        digests_dev: int, base: int = 0, key=None, hip_stream: int = 0):
    """Device-only form (all pointers device memory; order_dev may be 0)."""
    kb, kl = _key_arg(key)
    rc = lib().pbs_digest_chunks_async(ctypes.c_void_p(dev_ptr), data_len, base,
                                       ctypes.c_void_p(bounds_dev), ctypes.c_void_p(order_dev or None),
                                       n, kb, kl, ctypes.c_void_p(digests_dev),
                                       ctypes.c_void_p(hip_stream))
    if rc != PBS_OK:
        raise ChunkerError(rc, "pbs_digest_chunks_async")


def crc32(data, crc: int = 0) -> int:
    """Host CRC-32 of the C library (crc32fast::Hasher: continue ``crc`` over data)."""
    a = _as_u8(data)
    return int(lib().pbs_crc32(crc, _ptr(a), a.size))


def crc32_chunks_device(dev_ptr: int, data_len: int, bounds, base: int = 0, hip_stream: int = 0) -> np.ndarray:
    """DataBlob::compute_crc (data_blob.rs:70-75) on the GPU for every chunk
    [bounds[i], bounds[i+1]) of the stream whose bytes [base, base + data_len) are at
    device address dev_ptr; uint32 CRCs in chunk order."""
    b = np.ascontiguousarray(np.asarray(bounds, dtype=np.uint64))
    n = max(0, b.size - 1)
    out = np.empty(n, dtype=np.uint32)
    if n == 0:
        return out
    rc = lib().pbs_crc32_chunks_device(ctypes.c_void_p(dev_ptr), data_len, base, b.ctypes.data, n,
                                       out.ctypes.data, ctypes.c_void_p(hip_stream))
    if rc != PBS_OK:
        raise ChunkerError(rc, "pbs_crc32_chunks_device")
    return out


BLOB_HEADER_SIZE = 12
BLOB_ENC_HEADER_SIZE = 44  # EncryptedDataBlobHeader
GCM_SEGMENT_BYTES = 65536  # PBS_GCM_SEGMENT_BYTES: one workgroup's share of a payload


class CryptConfig:
    """`CryptConfig::new(enc_key)` (pbs-tools/src/crypt_config.rs:42-61): the handle the
    encrypted blob calls take.  ``id_key`` is the key appended to every chunk's digest
    message.  ``close()`` (or leaving a ``with`` block) zeroes and frees the key material."""

    def __init__(self, enc_key):
        k = bytes(enc_key)
        if len(k) != 32:
            raise ValueError("the encryption key must be 32 bytes")
        h = ctypes.c_void_p()
        rc = lib().pbs_crypt_config_new(ctypes.create_string_buffer(k, 32), ctypes.byref(h))
        if rc != PBS_OK:
            raise ChunkerError(rc, "pbs_crypt_config_new")
        self._h = h

    @property
    def handle(self):
        if self._h is None:
            raise RuntimeError("crypt config is closed")
        return self._h

    @property
    def id_key(self) -> bytes:
        return ctypes.string_at(lib().pbs_crypt_config_id_key(self.handle), 32)

    def encrypt_host(self, iv, data):
        """pbs_aes256gcm_encrypt_host: (ciphertext, tag) of ``data`` under a 16-byte IV."""
        ivb = bytes(iv)
        if len(ivb) != 16:
            raise ValueError("the IV must be 16 bytes")
        a = _as_u8(data)
        out = np.empty(a.size, dtype=np.uint8)
        tag = (ctypes.c_uint8 * 16)()
        rc = lib().pbs_aes256gcm_encrypt_host(self.handle, ctypes.create_string_buffer(ivb, 16), _ptr(a), a.size,
                                              _ptr(out), tag)
        if rc != PBS_OK:
            raise ChunkerError(rc, "pbs_aes256gcm_encrypt_host")
        return out.tobytes(), bytes(tag)

    def decrypt_host(self, iv, data, tag) -> bytes:
        """pbs_aes256gcm_decrypt_host: the plaintext of ciphertext ``data`` under a 16-byte IV;
        raises ChunkerError(PBS_ERR_TAG) when the 16-byte ``tag`` does not match."""
        ivb, tagb = bytes(iv), bytes(tag)
        if len(ivb) != 16 or len(tagb) != 16:
            raise ValueError("the IV and the tag must be 16 bytes each")
        a = _as_u8(data)
        out = np.empty(a.size, dtype=np.uint8)
        rc = lib().pbs_aes256gcm_decrypt_host(self.handle, ctypes.create_string_buffer(ivb, 16), _ptr(a), a.size,
                                              ctypes.create_string_buffer(tagb, 16), _ptr(out))
        if rc != PBS_OK:
            raise ChunkerError(rc, "pbs_aes256gcm_decrypt_host")
        return out.tobytes()

    def close(self):
        if self._h is not None:
            lib().pbs_crypt_config_free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _ivs_arg(ivs, n: int):
    """(keep-alive array, pointer) of n caller-supplied 16-byte IVs, or (None, None): the
    library draws them.  Caller-supplied IVs are for reproducible tests only -- reusing an
    IV under one key breaks GCM."""
    if ivs is None:
        return None, None
    a = np.ascontiguousarray(np.frombuffer(b"".join(bytes(x) for x in ivs), dtype=np.uint8)
                             if isinstance(ivs, (list, tuple)) else np.asarray(ivs, dtype=np.uint8)).reshape(-1)
    if a.size != 16 * n:
        raise ValueError(f"ivs holds {a.size} bytes, {n} blobs need {16 * n}")
    return a, (a.ctypes.data if a.size else None)


def blob_encode_chunks_device(dev_ptr: int, data_len: int, bounds, blobs_dev: int, blobs_cap: int,
                              base: int = 0, compress: bool = True, hip_stream: int = 0,
                              crypt=None, ivs=None):
    """pbs_blob_encode_chunks_device: the DataBlob image of every chunk written back to
    back at device address blobs_dev (data_blob.rs:87-176; zstd frames where shorter).
    Returns (offsets (n + 1), crcs (n), compressed flags (n), timing dict).
    ``crypt`` (a CryptConfig): encrypted blobs (pbs_blob_encode_chunks_encrypted_device;
    44-byte headers, blobs_cap >= blob_stream_bound_encrypted); ``ivs``: None -- the library
    draws a fresh IV per blob -- or n 16-byte IVs, for reproducible tests only."""
    b = np.ascontiguousarray(np.asarray(bounds, dtype=np.uint64))
    n = max(0, b.size - 1)
    offs = np.zeros(n + 1, dtype=np.uint64)
    crcs = np.empty(n, dtype=np.uint32)
    comp = np.empty(n, dtype=np.uint8)
    if crypt is not None:
        iva, ivp = _ivs_arg(ivs, n)
        tc = BlobEncodeTimingCrypt()
        rc = lib().pbs_blob_encode_chunks_encrypted_device(
            ctypes.c_void_p(dev_ptr), data_len, base, b.ctypes.data, n, 1 if compress else 0, crypt.handle, ivp,
            ctypes.c_void_p(blobs_dev), blobs_cap, offs.ctypes.data, crcs.ctypes.data, comp.ctypes.data,
            ctypes.byref(tc), ctypes.c_void_p(hip_stream))
        if rc != PBS_OK:
            raise ChunkerError(rc, "pbs_blob_encode_chunks_encrypted_device")
        return offs, crcs, comp, tc.as_dict()
    if ivs is not None:
        raise ValueError("ivs without crypt")
    t = BlobEncodeTiming()
    rc = lib().pbs_blob_encode_chunks_device(ctypes.c_void_p(dev_ptr), data_len, base, b.ctypes.data, n,
                                             1 if compress else 0, ctypes.c_void_p(blobs_dev), blobs_cap,
                                             offs.ctypes.data, crcs.ctypes.data, comp.ctypes.data,
                                             ctypes.byref(t), ctypes.c_void_p(hip_stream))
    if rc != PBS_OK:
        raise ChunkerError(rc, "pbs_blob_encode_chunks_device")
    return offs, crcs, comp, t.as_dict()


def blob_encode_spans_device(dev_ptr: int, data_len: int, spans, blobs_dev: int, blobs_cap: int,
                             base: int = 0, compress: bool = True, hip_stream: int = 0,
                             crypt=None, ivs=None):
    """pbs_blob_encode_spans_device: as blob_encode_chunks_device for chunks given as
    (start, end) absolute spans in any order (e.g. an upload's new chunks); blob i is
    written for span i.  Returns (offsets (n + 1), crcs (n), compressed flags (n), timing).
    ``crypt`` / ``ivs``: as blob_encode_chunks_device."""
    sp = np.ascontiguousarray(np.asarray(spans, dtype=np.uint64).reshape(-1, 2))
    n = sp.shape[0]
    offs = np.zeros(n + 1, dtype=np.uint64)
    crcs = np.empty(n, dtype=np.uint32)
    comp = np.empty(n, dtype=np.uint8)
    if crypt is not None:
        iva, ivp = _ivs_arg(ivs, n)
        tc = BlobEncodeTimingCrypt()
        rc = lib().pbs_blob_encode_spans_encrypted_device(
            ctypes.c_void_p(dev_ptr), data_len, base, sp.ctypes.data, n, 1 if compress else 0, crypt.handle, ivp,
            ctypes.c_void_p(blobs_dev), blobs_cap, offs.ctypes.data, crcs.ctypes.data, comp.ctypes.data,
            ctypes.byref(tc), ctypes.c_void_p(hip_stream))
        if rc != PBS_OK:
            raise ChunkerError(rc, "pbs_blob_encode_spans_encrypted_device")
        return offs, crcs, comp, tc.as_dict()
    if ivs is not None:
        raise ValueError("ivs without crypt")
    t = BlobEncodeTiming()
    rc = lib().pbs_blob_encode_spans_device(ctypes.c_void_p(dev_ptr), data_len, base, sp.ctypes.data, n,
                                            1 if compress else 0, ctypes.c_void_p(blobs_dev), blobs_cap,
                                            offs.ctypes.data, crcs.ctypes.data, comp.ctypes.data,
                                            ctypes.byref(t), ctypes.c_void_p(hip_stream))
    if rc != PBS_OK:
        raise ChunkerError(rc, "pbs_blob_encode_spans_device")
    return offs, crcs, comp, t.as_dict()


PBS_ERR_TAG = -7  # pbs_aes256gcm_decrypt_host: tag mismatch
BLOB_KIND_UNCOMPRESSED, BLOB_KIND_COMPRESSED, BLOB_KIND_ENCRYPTED, BLOB_KIND_ENCR_COMPR = 0, 1, 2, 3
BLOB_KIND_NONE = 255  # the magic is absent or unknown
(BLOB_ST_OK, BLOB_ST_TOO_SMALL, BLOB_ST_BAD_MAGIC, BLOB_ST_BAD_CRC, BLOB_ST_NO_CONFIG, BLOB_ST_BAD_TAG,
 BLOB_ST_BAD_DIGEST, BLOB_ST_BAD_SIZE) = range(8)


def blob_decode_bound(blob_offsets) -> int:
    """pbs_blob_decode_bound: the most payload bytes the blobs at these offsets can hold."""
    b = np.ascontiguousarray(np.asarray(blob_offsets, dtype=np.uint64))
    return int(lib().pbs_blob_decode_bound(b.ctypes.data, max(0, b.size - 1)))


def _expect_args(n: int, expect_digests, expect_sizes):
    dg = sz = None
    if expect_digests is not None:
        dg = np.ascontiguousarray(np.asarray(expect_digests, dtype=np.uint8)).reshape(-1)
        if dg.size != 32 * n:
            raise ValueError(f"expect_digests holds {dg.size} bytes, {n} blobs need {32 * n}")
    if expect_sizes is not None:
        sz = np.ascontiguousarray(np.asarray(expect_sizes, dtype=np.uint64)).reshape(-1)
        if sz.size != n:
            raise ValueError(f"expect_sizes holds {sz.size} values for {n} blobs")
    return dg, sz


def blob_decode_device(blobs_dev: int, blob_offsets, out_dev: int, out_cap: int, crypt=None,
                       expect_digests=None, expect_sizes=None, hip_stream: int = 0):
    """pbs_blob_decode_device: load, verify and open the blob images [blob_offsets[i],
    blob_offsets[i+1]) at device address blobs_dev (any mix of the four kinds); the payloads
    -- chunk bytes, or the zstd frame of a compressed kind -- go back to back to out_dev.
    ``crypt``: a CryptConfig or None; ``expect_digests``: None or (n, 32) bytes (kinds 0 and 2);
    ``expect_sizes``: None or n lengths (kind 0).  Returns (out_offsets (n + 1), kinds (n),
    status (n, BLOB_ST_*), timing dict).  A bad blob is a status, never an exception."""
    b = np.ascontiguousarray(np.asarray(blob_offsets, dtype=np.uint64))
    n = max(0, b.size - 1)
    offs = np.zeros(n + 1, dtype=np.uint64)
    kinds = np.empty(n, dtype=np.uint8)
    status = np.empty(n, dtype=np.uint8)
    dg, sz = _expect_args(n, expect_digests, expect_sizes)
    t = BlobDecodeTiming()
    rc = lib().pbs_blob_decode_device(
        ctypes.c_void_p(blobs_dev), b.ctypes.data, n, crypt.handle if crypt is not None else None,
        None if dg is None else _ptr(dg), None if sz is None else _ptr(sz), ctypes.c_void_p(out_dev), out_cap,
        offs.ctypes.data, _ptr(kinds), _ptr(status), ctypes.byref(t), ctypes.c_void_p(hip_stream))
    if rc != PBS_OK:
        raise ChunkerError(rc, "pbs_blob_decode_device")
    return offs, kinds, status, t.as_dict()


def blob_decode_host(blob, crypt=None, expect_digest=None, expect_size=None):
    """pbs_blob_decode_host: one blob on the host; (payload bytes, kind, status)."""
    a = _as_u8(blob)
    out = np.zeros(max(a.size, 1), dtype=np.uint8)
    olen = ctypes.c_size_t(0)
    kind, status = ctypes.c_uint8(0), ctypes.c_uint8(0)
    dg = None if expect_digest is None else ctypes.create_string_buffer(bytes(expect_digest), 32)
    if expect_digest is not None and len(bytes(expect_digest)) != 32:
        raise ValueError("the expected digest must be 32 bytes")
    sz = None if expect_size is None else ctypes.byref(ctypes.c_uint64(int(expect_size)))
    rc = lib().pbs_blob_decode_host(_ptr(a), a.size, crypt.handle if crypt is not None else None, dg, sz,
                                    out.ctypes.data, out.size, ctypes.byref(olen), ctypes.byref(kind),
                                    ctypes.byref(status))
    if rc != PBS_OK:
        raise ChunkerError(rc, "pbs_blob_decode_host")
    return out[:olen.value].tobytes(), int(kind.value), int(status.value)


# ---- inflating zstd frames (include/pbs_blob.h) ----
ZST_OK, ZST_BAD_FRAME, ZST_TOO_LARGE, ZST_UNSUPPORTED = range(4)
ZSTD_SIZE_UNKNOWN = (1 << 64) - 1


def zstd_frame_content_size(frame) -> Optional[int]:
    """pbs_zstd_frame_content_size: the header's content size, None when it carries none;
    ValueError when there is no readable frame header."""
    a = _as_u8(frame)
    v = ctypes.c_uint64(0)
    rc = lib().pbs_zstd_frame_content_size(_ptr(a), a.size, ctypes.byref(v))
    if rc != PBS_OK:
        raise ValueError("no zstd frame header")
    return None if v.value == ZSTD_SIZE_UNKNOWN else int(v.value)


def zstd_inflate_host(frame, cap: int):
    """pbs_zstd_inflate_host: the serial mirror of the GPU inflater; (bytes produced into a
    buffer of ``cap`` bytes, status ZST_*)."""
    a = _as_u8(frame)
    out = np.zeros(max(int(cap), 1), dtype=np.uint8)
    olen = ctypes.c_size_t(0)
    status = ctypes.c_uint8(0)
    rc = lib().pbs_zstd_inflate_host(_ptr(a), a.size, out.ctypes.data, int(cap), ctypes.byref(olen),
                                     ctypes.byref(status))
    if rc != PBS_OK:
        raise ChunkerError(rc, "pbs_zstd_inflate_host")
    return out[:olen.value].tobytes(), int(status.value)


def zstd_inflate_device(frames_dev: int, frame_offsets, out_dev: int, out_offsets, hip_stream: int = 0):
    """pbs_zstd_inflate_device: frame i = [frame_offsets[i], frame_offsets[i+1]) at device
    address frames_dev, inflated into the slot [out_offsets[i], out_offsets[i+1]) of out_dev.
    Returns (out_lens (n), status (n, ZST_*), timing dict).  A bad frame is a status."""
    f = np.ascontiguousarray(np.asarray(frame_offsets, dtype=np.uint64))
    o = np.ascontiguousarray(np.asarray(out_offsets, dtype=np.uint64))
    n = max(0, f.size - 1)
    if o.size != n + 1:
        raise ValueError(f"out_offsets holds {o.size} values, {n} frames need {n + 1}")
    lens = np.zeros(n, dtype=np.uint64)
    status = np.zeros(n, dtype=np.uint8)
    t = ZstdInflateTiming()
    rc = lib().pbs_zstd_inflate_device(ctypes.c_void_p(frames_dev), f.ctypes.data, n, ctypes.c_void_p(out_dev),
                                       o.ctypes.data, _ptr(lens), _ptr(status), ctypes.byref(t),
                                       ctypes.c_void_p(hip_stream))
    if rc != PBS_OK:
        raise ChunkerError(rc, "pbs_zstd_inflate_device")
    return lens, status, t.as_dict()


BLOB_ST_BAD_FRAME, BLOB_ST_UNSUPPORTED_FRAME = 8, 9


def blob_decode_inflate_device(blobs_dev: int, blob_offsets, out_dev: int, out_cap: int, chunk_sizes, crypt=None,
                               expect_digests=None, sizes_exact: bool = False, hip_stream: int = 0):
    """pbs_blob_decode_inflate_device: the read path in one call -- load, verify, open, inflate
    and digest the blob images (any mix of the four kinds); chunk i goes to the slot of
    ``chunk_sizes[i]`` bytes at out_offsets[i] of out_dev.  ``expect_digests``: None or (n, 32)
    bytes, checked for all four kinds.  Returns (out_offsets (n + 1), out_lens (n), kinds (n),
    status (n, BLOB_ST_*), timing dict).  A bad blob is a status, never an exception."""
    b = np.ascontiguousarray(np.asarray(blob_offsets, dtype=np.uint64))
    n = max(0, b.size - 1)
    dg, cs = _expect_args(n, expect_digests, chunk_sizes)
    if cs is None:
        raise ValueError("chunk_sizes is required")
    offs = np.zeros(n + 1, dtype=np.uint64)
    lens = np.zeros(n, dtype=np.uint64)
    kinds = np.empty(n, dtype=np.uint8)
    status = np.empty(n, dtype=np.uint8)
    t = BlobDecodeInflateTiming()
    rc = lib().pbs_blob_decode_inflate_device(
        ctypes.c_void_p(blobs_dev), b.ctypes.data, n, crypt.handle if crypt is not None else None,
        None if dg is None else _ptr(dg), _ptr(cs), 1 if sizes_exact else 0, ctypes.c_void_p(out_dev), out_cap,
        offs.ctypes.data, _ptr(lens), _ptr(kinds), _ptr(status), ctypes.byref(t), ctypes.c_void_p(hip_stream))
    if rc != PBS_OK:
        raise ChunkerError(rc, "pbs_blob_decode_inflate_device")
    return offs, lens, kinds, status, t.as_dict()


def debug_arena_allocs() -> int:
    """Device buffers the per-device work areas have allocated so far (tests)."""
    return int(lib().pbs_debug_arena_allocs())


def blob_encode_release() -> None:
    """Free the blob encoder's cached device scratch, the decoder's and the restore calls'."""
    lib().pbs_blob_encode_release()
    if hasattr(lib(), "pbs_restore_release"):  # (absent from an older build in an A/B run)
        lib().pbs_restore_release()


def restore_release() -> None:
    """pbs_restore_release: free the idle work areas of the lookup, copy and restore calls."""
    lib().pbs_restore_release()


def digest_hybrid_release() -> None:
    """Free the hybrid digest's cached pinned host slices."""
    lib().pbs_digest_hybrid_release()


def pipeline_release() -> None:
    """Free the idle pipeline work areas (pipeline_host keeps the stream-sized device
    buffer between calls)."""
    lib().pbs_pipeline_release()


def blob_stream_bound(bounds) -> int:
    b = np.ascontiguousarray(np.asarray(bounds, dtype=np.uint64))
    return int(lib().pbs_blob_stream_bound(b.ctypes.data, max(0, b.size - 1)))


def blob_stream_bound_encrypted(bounds) -> int:
    """44 n + the chunks' bytes: the largest encrypted blob stream of n chunks."""
    b = np.ascontiguousarray(np.asarray(bounds, dtype=np.uint64))
    return int(lib().pbs_blob_stream_bound_encrypted(b.ctypes.data, max(0, b.size - 1)))


def crc32_chunks_async(dev_ptr: int, data_len: int, bounds_dev: int, order_dev: int, n: int, crcs_dev: int,
                       base: int = 0, hip_stream: int = 0):
    """Device-only form (all pointers device memory; order_dev may be 0)."""
    rc = lib().pbs_crc32_chunks_async(ctypes.c_void_p(dev_ptr), data_len, base, ctypes.c_void_p(bounds_dev),
                                      ctypes.c_void_p(order_dev or None), n, ctypes.c_void_p(crcs_dev),
                                      ctypes.c_void_p(hip_stream))
    if rc != PBS_OK:
        raise ChunkerError(rc, "pbs_crc32_chunks_async")


UNCOMPRESSED_BLOB_MAGIC_1_0 = bytes([66, 171, 56, 7, 190, 131, 112, 161])  # file_formats.rs:9


def blob_encode_uncompressed(data, crc: int) -> bytes:
    """DataBlob::encode(data, None, compress=false) (data_blob.rs:159-174) with the CRC
    from crc32_chunks_device: magic || crc LE || data."""
    a = _as_u8(data)
    out = np.empty(a.size + 12, dtype=np.uint8)
    n = lib().pbs_blob_encode_uncompressed(_ptr(a), a.size, crc, out.ctypes.data, out.size)
    if n != a.size + 12:
        raise ValueError(f"data blob too large ({a.size} bytes).")
    return out.tobytes()


def known_chunks_device(digests_dev: int, n: int, known_dev: int, k: int, is_known_dev: int,
                        hip_stream: int = 0) -> int:
    """backup_writer.rs:677-697 on the GPU: is_known[i] = digest i is in the previous
    index (known_dev: k sorted 32-byte digests) or repeats an earlier chunk's digest.
    All pointers device memory; returns the number of known chunks."""
    cnt = ctypes.c_size_t(0)
    rc = lib().pbs_known_chunks_device(ctypes.c_void_p(digests_dev), n, ctypes.c_void_p(known_dev or None),
                                       k, ctypes.c_void_p(is_known_dev), ctypes.byref(cnt),
                                       ctypes.c_void_p(hip_stream))
    if rc != PBS_OK:
        raise ChunkerError(rc, "pbs_known_chunks_device")
    return int(cnt.value)


def didx_build(ends, digests, uuid: bytes = bytes(16), ctime: int = 0):
    """.didx image (bytes) and index_csum of chunks with END offsets ``ends`` and
    32-byte ``digests`` (dynamic_index.rs:28-68 header/entries, :373-391 csum)."""
    e = np.ascontiguousarray(np.asarray(ends, dtype=np.uint64))
    if isinstance(digests, (list, tuple)):
        digests = np.frombuffer(b"".join(bytes(x) for x in digests), dtype=np.uint8)
    d = np.ascontiguousarray(np.asarray(digests, dtype=np.uint8).reshape(-1, 32))
    if d.shape[0] != e.size:
        raise ValueError("ends and digests differ in length")
    if len(uuid) != 16:
        raise ValueError("uuid must be 16 bytes")
    n = e.size
    cap = int(lib().pbs_didx_size(n))
    out = np.empty(cap, dtype=np.uint8)
    csum = (ctypes.c_uint8 * 32)()
    ub = ctypes.create_string_buffer(bytes(uuid), 16)
    rc = lib().pbs_didx_build(e.ctypes.data if n else None, d.ctypes.data if n else None, n, ub,
                              int(ctime), out.ctypes.data, cap, csum)
    if rc != PBS_OK:
        raise ChunkerError(rc, "pbs_didx_build")
    return out.tobytes(), bytes(csum)


class DynamicIndexWriter:
    """dynamic_index.rs:297-391: ``add_chunk(offset, digest)`` per chunk (offset = the
    chunk's END offset, as DynamicChunkWriter passes it), ``close()`` writes the .didx
    file (tmp file + rename) and returns index_csum.  uuid/ctime default to a random
    uuid and the current time (Uuid::generate / epoch_i64 in the reference)."""

    def __init__(self, path: str, uuid: Optional[bytes] = None, ctime: Optional[int] = None):
        import time

        self.path = path
        self.uuid = bytes(uuid) if uuid is not None else os.urandom(16)
        self.ctime = int(time.time()) if ctime is None else int(ctime)
        self.ends = []
        self.digests = []
        self.closed = False

    def add_chunk(self, offset: int, digest: bytes):
        if self.closed:
            raise RuntimeError(f"cannot write to closed dynamic index file {self.path!r}")
        if len(digest) != 32:
            raise ValueError("digest must be 32 bytes")
        self.ends.append(int(offset))
        self.digests.append(bytes(digest))

    def close(self) -> bytes:
        if self.closed:
            raise RuntimeError(f"cannot close already closed archive index file {self.path!r}")
        self.closed = True
        image, csum = didx_build(self.ends, self.digests, self.uuid, self.ctime)
        tmp = os.path.splitext(self.path)[0] + ".tmp_didx"
        with open(tmp, "wb") as f:
            f.write(image)
        os.replace(tmp, self.path)
        return csum


def read_didx(image: bytes):
    """Parse a .didx image: (uuid, ctime, index_csum, ends (u64), digests (n, 32))."""
    if len(image) < DIDX_HEADER or image[:8] != DIDX_MAGIC:
        raise ValueError("not a dynamic index image")
    body = np.frombuffer(image, dtype=np.uint8, offset=DIDX_HEADER)
    if body.size % DIDX_ENTRY:
        raise ValueError("truncated entry")
    ent = body.reshape(-1, DIDX_ENTRY)
    ends = ent[:, :8].copy().view("<u8").reshape(-1)
    ctime = int.from_bytes(image[24:32], "little", signed=True)
    return image[8:24], ctime, image[32:64], ends, ent[:, 8:].copy()


# ---- restoring a .didx stream (include/pbs_restore.h) ----
BLOB_ST_MISSING = 10           # no blob in the store carries the entry's digest
BLOB_ST_NONE_REQUESTED = 255   # the entry lies outside the requested range
LOOKUP_MISSING = 0xFFFFFFFF


def didx_count(image_len: int) -> Optional[int]:
    """pbs_didx_count: entries of an image of that many bytes; None when it is shorter than the
    header or its body is no multiple of 40."""
    n = int(lib().pbs_didx_count(int(image_len)))
    return None if n == ctypes.c_size_t(-1).value else n


def didx_parse(image, cap: Optional[int] = None):
    """pbs_didx_parse: (uuid, ctime, header_csum, computed_csum, ends (u64), digests (n, 32)).
    Raises ChunkerError(PBS_ERR_INVALID) for a short image, a wrong magic, a ragged body or a
    decreasing end, and ChunkerError(PBS_ERR_CAPACITY) when ``cap`` (default: what the image
    holds) is too small."""
    a = _as_u8(image)
    if cap is None:
        cap = didx_count(a.size) or 0
    ends = np.zeros(cap, dtype=np.uint64)
    digests = np.zeros((cap, 32), dtype=np.uint8)
    uuid, hc, cc = (ctypes.c_uint8 * 16)(), (ctypes.c_uint8 * 32)(), (ctypes.c_uint8 * 32)()
    ctime, n = ctypes.c_int64(0), ctypes.c_size_t(0)
    rc = lib().pbs_didx_parse(_ptr(a), a.size, uuid, ctypes.byref(ctime), hc, cc, ends.ctypes.data if cap else None,
                              digests.ctypes.data if cap else None, cap, ctypes.byref(n))
    if rc != PBS_OK:
        raise ChunkerError(rc, "pbs_didx_parse")
    return bytes(uuid), int(ctime.value), bytes(hc), bytes(cc), ends[:n.value], digests[:n.value]


def didx_chunk_from_offset(ends, offset: int):
    """pbs_didx_chunk_from_offset: (entry, offset inside it), or None where the reference's
    chunk_from_offset returns None (offset at or past the end, empty index)."""
    e = np.ascontiguousarray(np.asarray(ends, dtype=np.uint64))
    idx, within = ctypes.c_size_t(0), ctypes.c_uint64(0)
    rc = lib().pbs_didx_chunk_from_offset(e.ctypes.data if e.size else None, e.size, int(offset), ctypes.byref(idx),
                                          ctypes.byref(within))
    if rc == PBS_ERR_INVALID:
        return None
    if rc != PBS_OK:
        raise ChunkerError(rc, "pbs_didx_chunk_from_offset")
    return int(idx.value), int(within.value)


class DynamicIndexReader:
    """dynamic_index.rs:82-275 over the C reader: built from the bytes of a .didx image or from
    a path.  ``index_csum`` is the header's checksum and ``compute_csum()`` the one over the
    entries; as in the reference, opening does not compare them.  ``ctime`` is the header's
    field.  Raises ChunkerError where the reference's ``new`` bails."""

    def __init__(self, source):
        if isinstance(source, (str, os.PathLike)):
            with open(source, "rb") as f:
                source = f.read()
        image = bytes(source)
        self.size = len(image)
        self.uuid, self.ctime, self.index_csum, self._csum, self.ends, self.digests = didx_parse(image)

    def index_count(self) -> int:
        return int(self.ends.size)

    def index_bytes(self) -> int:
        return int(self.ends[-1]) if self.ends.size else 0

    def chunk_end(self, pos: int) -> int:
        if not 0 <= pos < self.ends.size:
            raise IndexError("chunk index out of range")
        return int(self.ends[pos])

    def index_digest(self, pos: int) -> Optional[bytes]:
        return self.digests[pos].tobytes() if 0 <= pos < self.ends.size else None

    def chunk_info(self, pos: int):
        """(start, end, digest) of entry ``pos``, or None past the end."""
        if not 0 <= pos < self.ends.size:
            return None
        return (int(self.ends[pos - 1]) if pos else 0), int(self.ends[pos]), self.digests[pos].tobytes()

    def chunk_from_offset(self, offset: int):
        return didx_chunk_from_offset(self.ends, offset)

    def compute_csum(self):
        """(checksum over the entries, the archive's length)."""
        return self._csum, self.index_bytes()


def _digest_rows(digests) -> np.ndarray:
    if isinstance(digests, (list, tuple)):
        digests = np.frombuffer(b"".join(bytes(x) for x in digests), dtype=np.uint8)
    return np.ascontiguousarray(np.asarray(digests, dtype=np.uint8).reshape(-1, 32))


def digest_lookup_host(digests, store):
    """pbs_digest_lookup_host: (store_pos (n, LOOKUP_MISSING where absent), first (n), n_missing,
    n_unique) of the index digests against the store's digest list, on the host."""
    d, s = _digest_rows(digests), _digest_rows(store)
    pos = np.zeros(d.shape[0], dtype=np.uint32)
    first = np.zeros(d.shape[0], dtype=np.uint32)
    nm, nu = ctypes.c_size_t(0), ctypes.c_size_t(0)
    rc = lib().pbs_digest_lookup_host(d.ctypes.data, d.shape[0], s.ctypes.data if s.shape[0] else None, s.shape[0],
                                      pos.ctypes.data, first.ctypes.data, ctypes.byref(nm), ctypes.byref(nu))
    if rc != PBS_OK:
        raise ChunkerError(rc, "pbs_digest_lookup_host")
    return pos, first, int(nm.value), int(nu.value)


def digest_lookup_device(digests_dev: int, n: int, store_dev: int, m: int, store_pos_dev: int, first_dev: int,
                         hip_stream: int = 0):
    """pbs_digest_lookup_device: all pointers device memory (n and m 32-byte digests, 16-byte
    aligned; n u32 each for the two outputs).  Returns (n_missing, n_unique)."""
    nm, nu = ctypes.c_size_t(0), ctypes.c_size_t(0)
    rc = lib().pbs_digest_lookup_device(ctypes.c_void_p(digests_dev), n, ctypes.c_void_p(store_dev or None), m,
                                        ctypes.c_void_p(store_pos_dev), ctypes.c_void_p(first_dev), ctypes.byref(nm),
                                        ctypes.byref(nu), ctypes.c_void_p(hip_stream))
    if rc != PBS_OK:
        raise ChunkerError(rc, "pbs_digest_lookup_device")
    return int(nm.value), int(nu.value)


def copy_segments_device(src_dev: int, dst_dev: int, src_off, dst_off, lens, hip_stream: int = 0) -> None:
    """pbs_copy_segments_device: segment k moves lens[k] bytes from src_dev + src_off[k] to
    dst_dev + dst_off[k].  An overlapping destination raises ChunkerError(PBS_ERR_INVALID) with
    nothing written."""
    so = np.ascontiguousarray(np.asarray(src_off, dtype=np.uint64))
    do = np.ascontiguousarray(np.asarray(dst_off, dtype=np.uint64))
    ln = np.ascontiguousarray(np.asarray(lens, dtype=np.uint64))
    if not so.size == do.size == ln.size:
        raise ValueError("src_off, dst_off and lens differ in length")
    rc = lib().pbs_copy_segments_device(ctypes.c_void_p(src_dev), ctypes.c_void_p(dst_dev), so.ctypes.data,
                                        do.ctypes.data, ln.ctypes.data, ln.size, ctypes.c_void_p(hip_stream))
    if rc != PBS_OK:
        raise ChunkerError(rc, "pbs_copy_segments_device")


def _index_arrays(index):
    if isinstance(index, DynamicIndexReader):
        return index.ends, index.digests
    ends, digests = index
    return np.ascontiguousarray(np.asarray(ends, dtype=np.uint64)), _digest_rows(digests)


def restore_range_device(index, store_blobs_dev: int, store_offsets, store_digests, out_dev: int, offset: int = 0,
                         length: Optional[int] = None, crypt=None, allow_bad: bool = False, hip_stream: int = 0):
    """pbs_restore_range_device: archive bytes [offset, offset + length) of the stream that
    ``index`` (a DynamicIndexReader, or (ends, digests)) describes, to device address out_dev.
    The store: blob j = [store_offsets[j], store_offsets[j+1]) at device address
    store_blobs_dev, filed under store_digests[j] ((m, 32) bytes, host).  ``length`` None: to the
    end of the archive.  Every distinct chunk of the range is decoded and verified once.
    Returns (status (one BLOB_ST_* per index entry, BLOB_ST_NONE_REQUESTED outside the range),
    timing dict).  The output of an entry that is not OK is zeros; ChunkerError is raised for it
    unless ``allow_bad``."""
    ends, digests = _index_arrays(index)
    n = int(ends.size)
    if digests.shape[0] != n:
        raise ValueError("ends and digests differ in length")
    so = np.ascontiguousarray(np.asarray(store_offsets, dtype=np.uint64))
    sd = _digest_rows(store_digests)
    m = int(sd.shape[0])
    if so.size != m + 1:
        raise ValueError(f"store_offsets holds {so.size} values, {m} blobs need {m + 1}")
    total = int(ends[-1]) if n else 0
    if length is None:
        length = max(0, total - int(offset))
    status = np.full(n, BLOB_ST_NONE_REQUESTED, dtype=np.uint8)
    t = RestoreTiming()
    rc = lib().pbs_restore_range_device(
        ends.ctypes.data if n else None, digests.ctypes.data if n else None, n, ctypes.c_void_p(store_blobs_dev or None),
        so.ctypes.data, sd.ctypes.data if m else None, m, crypt.handle if crypt is not None else None, int(offset),
        int(length), ctypes.c_void_p(out_dev or None), status.ctypes.data if n else None, ctypes.byref(t),
        ctypes.c_void_p(hip_stream))
    if rc != PBS_OK:
        raise ChunkerError(rc, "pbs_restore_range_device")
    if t.failed and not allow_bad:
        bad = [(int(k), int(status[k])) for k in np.flatnonzero((status != BLOB_ST_OK) & (status != BLOB_ST_NONE_REQUESTED))]
        raise ChunkerError(PBS_ERR_INVALID, f"restore: {t.failed} entries failed (entry, status): {bad[:8]}")
    return status, t.as_dict()


def restore_stream_device(index, store_blobs_dev: int, store_offsets, store_digests, out_dev: int, crypt=None,
                          allow_bad: bool = False, window: int = 1 << 30, hip_stream: int = 0):
    """The whole archive to out_dev through restore_range_device, in windows of about
    ``window`` bytes that end on chunk boundaries (a chunk longer than the window is a window
    of its own): this bounds the device scratch to a window's blobs and chunks.  A chunk is
    decoded once per window that names it: dedup holds within a window, not across windows.
    Returns (status per entry, list of the windows' timing dicts).  (A zero-length entry that
    lies exactly on a window boundary belongs to no window and keeps BLOB_ST_NONE_REQUESTED.)"""
    ends, digests = _index_arrays(index)
    n = int(ends.size)
    total = int(ends[-1]) if n else 0
    status = np.full(n, BLOB_ST_NONE_REQUESTED, dtype=np.uint8)
    timings = []
    pos = 0
    while pos < total:
        # the last chunk end within the window, or the end of the chunk that holds `pos`
        k = int(np.searchsorted(ends, pos + max(1, int(window)), side="right"))
        end = int(ends[k - 1]) if k and int(ends[k - 1]) > pos else int(ends[np.searchsorted(ends, pos, side="right")])
        st, t = restore_range_device((ends, digests), store_blobs_dev, store_offsets, store_digests, out_dev + pos,
                                     pos, end - pos, crypt=crypt, allow_bad=allow_bad, hip_stream=hip_stream)
        seen = st != BLOB_ST_NONE_REQUESTED
        status[seen] = st[seen]
        timings.append(t)
        pos = end
    return status, timings


def index_stream_device(chunker: "Chunker", dev_ptr: int, length: int, key=None,
                        hip_stream: int = 0, uuid: bytes = bytes(16), ctime: int = 0):
    """The client's per-stream path on a device-resident stream: chunk boundaries
    (GPU chunker), chunk digests (the hybrid SHA-256: GPU lanes, the longest chunks on
    host cores), then the .didx image and index_csum (host).  Returns (ends, digests,
    csum, didx_bytes)."""
    start = chunker.stream_offset
    ends = chunker.find_cuts_device(dev_ptr, length, is_final=True)
    bounds = np.concatenate([np.array([start], dtype=np.uint64), ends.astype(np.uint64)])
    dig, _ = digest_chunks_hybrid(dev_ptr, length, bounds, base=start, key=key, hip_stream=hip_stream)
    image, csum = didx_build(ends, dig, uuid, ctime)
    return ends, dig, csum, image


def upload_stream_host(data, avg: int, known=None, key=None, piece: int = 1 << 30,
                       uuid: bytes = bytes(16), ctime: int = 0, compress: bool = True,
                       digest_cus: int = 64, blobs_out=None, crypt=None) -> dict:
    """The client's upload of one dynamic-index stream from a host buffer, up to the
    network (pbs-client/src/backup_writer.rs:631-706 upload_chunk_info_stream; the client
    backs up with compress = true, proxmox-backup-client/src/main.rs:1011-1016): chunk
    (ChunkStream), digest every chunk, mark it known when its digest is in ``known`` (the
    previous index's digests, :524-547) or repeats an earlier chunk of this stream (:697),
    build each new chunk's blob -- DataChunkBuilder::new(data).compress(compress).build()
    (:671, :698; zstd frames where shorter, data_blob.rs:139-176) -- and the .didx image.
    Everything up to the blobs runs on the GPU from one HBM copy of the stream
    (pbs_upload_stream_host).  Returns a dict: ends, digests, known (uint8 mask), csum,
    didx (bytes), blobs (uint8 array: the new chunks' blobs back to back; chunk i's is
    blobs[blob_offsets[i]:blob_offsets[i + 1]], empty for a known chunk), blob_offsets
    (n + 1), compressed (n flags), new_chunks = [(start, length), ...], stats (UploadStats,
    backup_writer.rs:56-64) and timing.
    ``blobs_out``: an optional preallocated uint8 array (e.g. pinned) for the blobs.
    ``crypt`` (a CryptConfig): an encrypted backup (pbs_upload_stream_host_crypt) -- the
    digests are SHA-256(chunk || id_key) (``key`` must then be None) and every new chunk is
    an AES-256-GCM blob with a library-drawn IV; timing gains ``encrypt_ms``."""
    a = _as_u8(data)
    cap = a.size // max(int(avg) >> 2, 65) + 4
    ends = np.empty(cap, dtype=np.uint64)
    dig = np.empty((cap, 32), dtype=np.uint8)
    is_known = np.empty(cap, dtype=np.uint8)
    offs = np.zeros(cap + 1, dtype=np.uint64)
    comp = np.empty(cap, dtype=np.uint8)
    if crypt is not None and key is not None:
        raise ValueError("crypt brings its own digest key (id_key)")
    bcap = (BLOB_ENC_HEADER_SIZE if crypt is not None else BLOB_HEADER_SIZE) * cap + a.size
    blobs = blobs_out if blobs_out is not None else np.empty(max(bcap, 1), dtype=np.uint8)
    if blobs.size < bcap:
        raise ValueError(f"blobs_out holds {blobs.size} bytes, the stream needs up to {bcap}")
    kd = np.zeros((0, 32), dtype=np.uint8)
    if known is not None and len(known):
        kd = np.frombuffer(b"".join(sorted(bytes(x) for x in known)), dtype=np.uint8).reshape(-1, 32)
    kb, kl = _key_arg(key)
    n = ctypes.c_size_t(0)
    t = UploadTiming()
    enc_ms = ctypes.c_double(0.0)
    if crypt is not None:
        rc = lib().pbs_upload_stream_host_crypt(avg, _ptr(a), a.size, piece, crypt.handle, digest_cus,
                                                kd.ctypes.data if kd.size else None, kd.shape[0],
                                                1 if compress else 0, ends.ctypes.data, dig.ctypes.data,
                                                is_known.ctypes.data, cap, ctypes.byref(n), blobs.ctypes.data,
                                                blobs.size, offs.ctypes.data, comp.ctypes.data, ctypes.byref(t),
                                                ctypes.byref(enc_ms))
    else:
        rc = lib().pbs_upload_stream_host(avg, _ptr(a), a.size, piece, kb, kl, digest_cus,
                                          kd.ctypes.data if kd.size else None, kd.shape[0], 1 if compress else 0,
                                          ends.ctypes.data, dig.ctypes.data, is_known.ctypes.data, cap,
                                          ctypes.byref(n), blobs.ctypes.data, blobs.size, offs.ctypes.data,
                                          comp.ctypes.data, ctypes.byref(t))
    if rc != PBS_OK:
        raise ChunkerError(rc, "pbs_upload_stream_host_crypt" if crypt is not None else "pbs_upload_stream_host")
    m = n.value
    ends, dig, is_known, offs, comp = ends[:m].copy(), dig[:m].copy(), is_known[:m].copy(), offs[:m + 1].copy(), comp[:m].copy()
    image, csum = didx_build(ends, dig, uuid, ctime)
    starts = np.concatenate([[0], ends[:-1]]).astype(np.uint64) if m else np.zeros(0, np.uint64)
    new = [(int(starts[i]), int(ends[i] - starts[i])) for i in np.flatnonzero(is_known == 0)]
    td = t.as_dict()
    if crypt is not None:
        td["encrypt_ms"] = enc_ms.value
    stats = {k: td[k] for k in ("chunk_count", "chunk_reused", "size", "size_reused", "size_compressed")}
    return {"ends": ends, "digests": dig, "known": is_known, "csum": csum, "didx": image,
            "blobs": blobs[:int(offs[-1])] if m else blobs[:0], "blob_offsets": offs, "compressed": comp,
            "new_chunks": new, "stats": stats, "timing": td}


def pipeline_host(data, avg: int, piece: int = 1 << 30, key=None, digest_cus: int = 64, crc: bool = False):
    """pbs_pipeline_host: chunk END offsets, (n, 32) digests and the timing dict of the
    overlapped copy -> chunk -> digest path over a host buffer; with crc=True also the
    per-chunk blob CRC-32s: (ends, digests, crcs, timing)."""
    a = _as_u8(data)
    # pbs_chunker_cuts_bound without a handle (min_eff = max(avg / 4, 65)); an average
    # that is not a power of two fails in the call below
    cap = a.size // max(int(avg) >> 2, 65) + 4
    ends = np.empty(cap, dtype=np.uint64)
    dig = np.empty((cap, 32), dtype=np.uint8)
    crcs = np.empty(cap, dtype=np.uint32) if crc else None
    n = ctypes.c_size_t(0)
    t = PipelineTiming()
    kb, kl = _key_arg(key)
    rc = lib().pbs_pipeline_host(avg, _ptr(a), a.size, piece, kb, kl, digest_cus, ends.ctypes.data,
                                 dig.ctypes.data, crcs.ctypes.data if crc else None, cap, ctypes.byref(n),
                                 ctypes.byref(t))
    if rc != PBS_OK:
        raise ChunkerError(rc, "pbs_pipeline_host")
    if crc:
        return ends[: n.value].copy(), dig[: n.value].copy(), crcs[: n.value].copy(), t.as_dict()
    return ends[: n.value].copy(), dig[: n.value].copy(), t.as_dict()


# ---- the fixed-size chunk path: .fidx archives, VM images (include/pbs_fixed.h) ----
FIDX_MAGIC = bytes([47, 127, 65, 237, 145, 253, 15, 205])  # file_formats.rs:20-21
FIDX_HEADER = 4096


class FixedChunkStream:
    """chunk_stream.rs:80-134: feed bytes in any pieces; chunks of exactly ``chunk_size`` come
    out and, at the end, one last chunk of any non-zero length (:106-133).  ``feed(data)``
    returns the chunks completed by it, ``finish()`` the last partial chunk in a list (empty
    when the input was a multiple of the chunk size or empty); ``chunks(pieces)`` does both
    over an iterable."""

    def __init__(self, chunk_size: int):
        if chunk_size <= 0:
            raise ValueError("chunk_size must be positive")
        self.chunk_size = int(chunk_size)
        self._buf = bytearray()

    def feed(self, data) -> list:
        self._buf += bytes(data)
        c, out = self.chunk_size, []
        k = len(self._buf) // c
        for j in range(k):
            out.append(bytes(self._buf[j * c:(j + 1) * c]))
        del self._buf[:k * c]
        return out

    def finish(self) -> list:
        out = [bytes(self._buf)] if self._buf else []
        self._buf = bytearray()
        return out

    def chunks(self, pieces: Iterable) -> Iterator[bytes]:
        for piece in pieces:
            yield from self.feed(piece)
        yield from self.finish()


def fidx_count(size: int, chunk_size: int) -> int:
    return int(lib().pbs_fidx_count(int(size), int(chunk_size)))


def fidx_size(n: int) -> int:
    return int(lib().pbs_fidx_size(int(n)))


def fidx_build(digests, size: int, chunk_size: int, uuid: bytes = bytes(16), ctime: int = 0):
    """pbs_fidx_build: the .fidx image (bytes) and index_csum of an archive of ``size`` bytes in
    chunks of ``chunk_size`` with the ceil(size / chunk_size) 32-byte ``digests``
    (fixed_index.rs:20-32 header, :341-362 csum)."""
    d = _digest_rows(digests)
    if chunk_size <= 0:
        raise ChunkerError(PBS_ERR_INVALID, "pbs_fidx_build")
    n = fidx_count(size, chunk_size)
    if d.shape[0] != n:
        raise ValueError(f"{d.shape[0]} digests, the archive has {n} chunks")
    if len(uuid) != 16:
        raise ValueError("uuid must be 16 bytes")
    cap = fidx_size(n)
    out = np.empty(cap, dtype=np.uint8)
    csum = (ctypes.c_uint8 * 32)()
    ub = ctypes.create_string_buffer(bytes(uuid), 16)
    rc = lib().pbs_fidx_build(d.ctypes.data if n else None, int(size), int(chunk_size), ub, int(ctime),
                              out.ctypes.data, cap, csum)
    if rc != PBS_OK:
        raise ChunkerError(rc, "pbs_fidx_build")
    return out.tobytes(), bytes(csum)


def fidx_parse(image, cap: Optional[int] = None):
    """pbs_fidx_parse: (uuid, ctime, header_csum, computed_csum, size, chunk_size, digests (n, 32)).
    Raises ChunkerError with the call's code (``.n`` = the image's entry count where the call
    set it) where FixedIndexReader::new bails, for a chunk size that is no power of two
    (PBS_ERR_NOT_POW2) and when ``cap`` (default: what the image's length holds) is too small."""
    a = _as_u8(image)
    if cap is None:
        cap = max(0, (a.size - FIDX_HEADER) // 32)
    digests = np.zeros((cap, 32), dtype=np.uint8)
    uuid, hc, cc = (ctypes.c_uint8 * 16)(), (ctypes.c_uint8 * 32)(), (ctypes.c_uint8 * 32)()
    ctime, n = ctypes.c_int64(0), ctypes.c_size_t(0)
    size, cs = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = lib().pbs_fidx_parse(_ptr(a), a.size, uuid, ctypes.byref(ctime), hc, cc, ctypes.byref(size), ctypes.byref(cs),
                              digests.ctypes.data if cap else None, cap, ctypes.byref(n))
    if rc != PBS_OK:
        err = ChunkerError(rc, "pbs_fidx_parse")
        err.n = int(n.value)
        raise err
    return bytes(uuid), int(ctime.value), bytes(hc), bytes(cc), int(size.value), int(cs.value), digests[:n.value]


def fidx_chunk_info(size: int, chunk_size: int, pos: int):
    """pbs_fidx_chunk_info: (start, end) of chunk ``pos`` (the last one clipped), None past the end."""
    if pos < 0:
        return None
    s, e = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = lib().pbs_fidx_chunk_info(int(size), int(chunk_size), int(pos), ctypes.byref(s), ctypes.byref(e))
    return (int(s.value), int(e.value)) if rc == PBS_OK else None


def fidx_chunk_from_offset(size: int, chunk_size: int, offset: int):
    """pbs_fidx_chunk_from_offset: (chunk, offset inside it), or None at or past ``size``."""
    idx, within = ctypes.c_size_t(0), ctypes.c_uint64(0)
    rc = lib().pbs_fidx_chunk_from_offset(int(size), int(chunk_size), int(offset), ctypes.byref(idx),
                                          ctypes.byref(within))
    if rc == PBS_ERR_INVALID and chunk_size:
        return None
    if rc != PBS_OK:
        raise ChunkerError(rc, "pbs_fidx_chunk_from_offset")
    return int(idx.value), int(within.value)


def fidx_check_chunk_alignment(size: int, chunk_size: int, end_offset: int, chunk_len: int) -> int:
    """pbs_fidx_check_chunk_alignment (fixed_index.rs:364-392): the chunk's index; ChunkerError
    where the reference bails."""
    idx = ctypes.c_size_t(0)
    rc = lib().pbs_fidx_check_chunk_alignment(int(size), int(chunk_size), int(end_offset), int(chunk_len),
                                              ctypes.byref(idx))
    if rc != PBS_OK:
        raise ChunkerError(rc, "pbs_fidx_check_chunk_alignment")
    return int(idx.value)


class FixedIndexReader:
    """fixed_index.rs:59-215 over the C reader: built from the bytes of a .fidx image or from a
    path.  ``index_csum`` is the header's checksum and ``compute_csum()`` the one over the
    digests; as in the reference, opening does not compare them.  Raises ChunkerError where the
    reference's ``new`` bails, and for a chunk size that is no power of two."""

    def __init__(self, source):
        if isinstance(source, (str, os.PathLike)):
            with open(source, "rb") as f:
                source = f.read()
        (self.uuid, self.ctime, self.index_csum, self._csum, self.size, self.chunk_size,
         self.digests) = fidx_parse(bytes(source))

    def index_count(self) -> int:
        return int(self.digests.shape[0])

    def index_bytes(self) -> int:
        return self.size

    def index_digest(self, pos: int) -> Optional[bytes]:
        return self.digests[pos].tobytes() if 0 <= pos < self.index_count() else None

    def chunk_info(self, pos: int):
        """(start, end, digest) of entry ``pos``, or None past the end."""
        r = fidx_chunk_info(self.size, self.chunk_size, pos)
        return None if r is None else (r[0], r[1], self.digests[pos].tobytes())

    def chunk_from_offset(self, offset: int):
        return fidx_chunk_from_offset(self.size, self.chunk_size, offset)

    def compute_csum(self):
        """(checksum over the digests, the archive's length)."""
        return self._csum, self.size

    def ends(self) -> np.ndarray:
        """The chunk END offsets, the last one clipped to the size."""
        n = self.index_count()
        return np.minimum((np.arange(n, dtype=np.uint64) + 1) * np.uint64(self.chunk_size), np.uint64(self.size))


class FixedIndexWriter:
    """fixed_index.rs:243-461 in memory: digests may come in any order (:394); ``close()``
    returns index_csum and ``image()`` the .fidx bytes (``close(path)`` also writes them: tmp
    file + rename).  A slot never written holds zeros, as the reference's fresh mapping does."""

    def __init__(self, size: int, chunk_size: int, uuid: Optional[bytes] = None, ctime: Optional[int] = None):
        import time

        if chunk_size <= 0 or chunk_size & (chunk_size - 1):
            raise ChunkerError(PBS_ERR_NOT_POW2 if chunk_size > 0 else PBS_ERR_INVALID, "FixedIndexWriter")
        if size <= 0:
            raise ChunkerError(PBS_ERR_INVALID, "FixedIndexWriter: invalid index size")  # :295-296
        self.size, self.chunk_size = int(size), int(chunk_size)
        self.uuid = bytes(uuid) if uuid is not None else os.urandom(16)
        self.ctime = int(time.time()) if ctime is None else int(ctime)
        self.index_length = fidx_count(size, chunk_size)
        self._digests = np.zeros((self.index_length, 32), dtype=np.uint8)
        self._image = None
        self.closed = False

    def check_chunk_alignment(self, end_offset: int, chunk_len: int) -> int:
        return fidx_check_chunk_alignment(self.size, self.chunk_size, end_offset, chunk_len)

    def add_digest(self, index: int, digest: bytes):
        if not 0 <= index < self.index_length:
            raise IndexError(f"add digest failed - index out of range ({index} >= {self.index_length})")
        if self.closed:
            raise RuntimeError("cannot write to closed index file.")
        if len(digest) != 32:
            raise ValueError("digest must be 32 bytes")
        self._digests[index] = np.frombuffer(bytes(digest), dtype=np.uint8)

    def add_chunk(self, end_offset: int, chunk_len: int, digest: bytes) -> int:
        idx = self.check_chunk_alignment(end_offset, chunk_len)
        self.add_digest(idx, digest)
        return idx

    def clone_data_from(self, reader: "FixedIndexReader"):
        if self.index_length != reader.index_count():
            raise ValueError("clone_data_from failed - index sizes not equal")
        for k in range(self.index_length):
            self.add_digest(k, reader.index_digest(k))

    def close(self, path: Optional[str] = None) -> bytes:
        if self.closed:
            raise RuntimeError("cannot close already closed index file.")
        self.closed = True
        self._image, csum = fidx_build(self._digests, self.size, self.chunk_size, self.uuid, self.ctime)
        if path is not None:
            tmp = os.path.splitext(path)[0] + ".tmp_fidx"
            with open(tmp, "wb") as f:
                f.write(self._image)
            os.replace(tmp, path)
        return csum

    def image(self) -> bytes:
        if self._image is None:
            raise RuntimeError("the index is not closed yet")
        return self._image


def fixed_dirty_host(prev, cur, chunk_size: int):
    """pbs_fixed_dirty_host: (flags (n uint8, 1 = some byte of the chunk differs), n_dirty) of two
    host images of equal length, by memcmp per chunk."""
    a, b = _as_u8(prev), _as_u8(cur)
    if a.size != b.size:
        raise ValueError("the images differ in length")
    n = fidx_count(a.size, chunk_size) if chunk_size > 0 else 0
    flags = np.zeros(n, dtype=np.uint8)
    cnt = ctypes.c_size_t(0)
    rc = lib().pbs_fixed_dirty_host(_ptr(a), _ptr(b), a.size, int(chunk_size), _ptr(flags), ctypes.byref(cnt))
    if rc != PBS_OK:
        raise ChunkerError(rc, "pbs_fixed_dirty_host")
    return flags, int(cnt.value)


def fixed_dirty_device(prev_dev: int, cur_dev: int, size: int, chunk_size: int, dirty_dev: int,
                       hip_stream: int = 0) -> int:
    """pbs_fixed_dirty_device: writes the n = ceil(size / chunk_size) flags to device address
    dirty_dev and returns n_dirty.  Both images are device addresses of any alignment."""
    cnt = ctypes.c_size_t(0)
    rc = lib().pbs_fixed_dirty_device(ctypes.c_void_p(prev_dev or None), ctypes.c_void_p(cur_dev or None), int(size),
                                      int(chunk_size), ctypes.c_void_p(dirty_dev or None), ctypes.byref(cnt),
                                      ctypes.c_void_p(hip_stream))
    if rc != PBS_OK:
        raise ChunkerError(rc, "pbs_fixed_dirty_device")
    return int(cnt.value)


def _dirty_args(dirty, prev_digests, n: int):
    if dirty is None:
        return None, None
    d = np.ascontiguousarray(np.asarray(dirty, dtype=np.uint8).reshape(-1))
    if d.size != n:
        raise ValueError(f"the dirty map holds {d.size} flags, the image has {n} chunks")
    if prev_digests is None:
        return d, None
    pd = _digest_rows(prev_digests)
    if pd.shape[0] != n:
        raise ValueError(f"{pd.shape[0]} previous digests, the image has {n} chunks")
    return d, pd


def fixed_digests_device(dev_ptr: int, size: int, chunk_size: int, key=None, dirty=None, prev_digests=None,
                         hip_stream: int = 0):
    """pbs_fixed_digests_device: ((n, 32) digests, index_csum, timing dict) of the image at
    device address dev_ptr.  With ``dirty`` (n flags) the clean chunks take ``prev_digests``
    verbatim and are not read."""
    n = fidx_count(size, chunk_size) if chunk_size > 0 else 0
    d, pd = _dirty_args(dirty, prev_digests, n)
    dig = np.zeros((n, 32), dtype=np.uint8)
    csum = (ctypes.c_uint8 * 32)()
    kb, kl = _key_arg(key)
    t = FixedDigestTiming()
    rc = lib().pbs_fixed_digests_device(ctypes.c_void_p(dev_ptr or None), int(size), int(chunk_size), kb, kl,
                                        d.ctypes.data if d is not None else None,
                                        pd.ctypes.data if pd is not None else None, _ptr(dig), csum, ctypes.byref(t),
                                        ctypes.c_void_p(hip_stream))
    if rc != PBS_OK:
        raise ChunkerError(rc, "pbs_fixed_digests_device")
    return dig, bytes(csum), t.as_dict()


def upload_fixed_host(data, chunk_size: int, known=None, key=None, piece: int = 1 << 30, dirty=None,
                      prev_digests=None, uuid: bytes = bytes(16), ctime: int = 0, compress: bool = True,
                      digest_cus: int = 64, blobs_out=None, crypt=None) -> dict:
    """The client's upload of one fixed-index image (``prefix == "fixed"``,
    backup_writer.rs:272-275) from a host buffer: upload_stream_host over the grid of
    ``chunk_size`` (FixedChunkStream) instead of the chunker's cuts; the same dict, with the
    .fidx image under ``fidx`` and ``csum`` = SHA-256 over the digests alone (:685).
    ``dirty`` (n flags) with ``prev_digests`` (n, 32): a clean chunk takes its previous digest,
    is known, has an empty blob and is neither copied, hashed nor encoded; timing gains
    ``dirty_chunks`` and ``copied_bytes``.  The digests of clean chunks take part in the known
    test only where ``known`` lists them."""
    a = _as_u8(data)
    cap = (fidx_count(a.size, chunk_size) if chunk_size > 0 else 0) + 1
    d, pd = _dirty_args(dirty, prev_digests, cap - 1)
    ends = np.empty(cap, dtype=np.uint64)
    dig = np.empty((cap, 32), dtype=np.uint8)
    is_known = np.empty(cap, dtype=np.uint8)
    offs = np.zeros(cap + 1, dtype=np.uint64)
    comp = np.empty(cap, dtype=np.uint8)
    if crypt is not None and key is not None:
        raise ValueError("crypt brings its own digest key (id_key)")
    bcap = (BLOB_ENC_HEADER_SIZE if crypt is not None else BLOB_HEADER_SIZE) * cap + a.size
    blobs = blobs_out if blobs_out is not None else np.empty(max(bcap, 1), dtype=np.uint8)
    if blobs.size < bcap:
        raise ValueError(f"blobs_out holds {blobs.size} bytes, the image needs up to {bcap}")
    kd = np.zeros((0, 32), dtype=np.uint8)
    if known is not None and len(known):
        kd = np.frombuffer(b"".join(sorted(bytes(x) for x in known)), dtype=np.uint8).reshape(-1, 32)
    kb, kl = _key_arg(key)
    n = ctypes.c_size_t(0)
    t = UploadFixedTiming()
    enc_ms = ctypes.c_double(0.0)
    csum = (ctypes.c_uint8 * 32)()
    dp = d.ctypes.data if d is not None else None
    pp = pd.ctypes.data if pd is not None else None
    tail = (1 if compress else 0, dp, pp, ends.ctypes.data, dig.ctypes.data, is_known.ctypes.data, cap,
            ctypes.byref(n), blobs.ctypes.data, blobs.size, offs.ctypes.data, comp.ctypes.data, csum, ctypes.byref(t))
    if crypt is not None:
        rc = lib().pbs_upload_fixed_host_crypt(int(chunk_size), _ptr(a), a.size, piece, crypt.handle, digest_cus,
                                               kd.ctypes.data if kd.size else None, kd.shape[0], *tail,
                                               ctypes.byref(enc_ms))
    else:
        rc = lib().pbs_upload_fixed_host(int(chunk_size), _ptr(a), a.size, piece, kb, kl, digest_cus,
                                         kd.ctypes.data if kd.size else None, kd.shape[0], *tail)
    if rc != PBS_OK:
        raise ChunkerError(rc, "pbs_upload_fixed_host_crypt" if crypt is not None else "pbs_upload_fixed_host")
    m = n.value
    ends, dig, is_known, offs, comp = ends[:m].copy(), dig[:m].copy(), is_known[:m].copy(), offs[:m + 1].copy(), comp[:m].copy()
    image = fidx_build(dig, a.size, chunk_size, uuid, ctime)[0] if m else b""
    starts = np.concatenate([[0], ends[:-1]]).astype(np.uint64) if m else np.zeros(0, np.uint64)
    new = [(int(starts[k]), int(ends[k] - starts[k])) for k in np.flatnonzero(is_known == 0)]
    td = t.as_dict()
    if crypt is not None:
        td["encrypt_ms"] = enc_ms.value
    stats = {k: td[k] for k in ("chunk_count", "chunk_reused", "size", "size_reused", "size_compressed")}
    return {"ends": ends, "digests": dig, "known": is_known, "csum": bytes(csum), "fidx": image,
            "blobs": blobs[:int(offs[-1])] if m else blobs[:0], "blob_offsets": offs, "compressed": comp,
            "new_chunks": new, "stats": stats, "timing": td}


def restore_fixed_range_device(reader, store_blobs_dev: int, store_offsets, store_digests, out_dev: int,
                               offset: int = 0, length: Optional[int] = None, crypt=None, allow_bad: bool = False,
                               hip_stream: int = 0):
    """pbs_restore_fixed_range_device: image bytes [offset, offset + length) of the archive that
    ``reader`` (a FixedIndexReader, or (digests, size, chunk_size)) describes, to device address
    out_dev; store, result and errors as restore_range_device."""
    if isinstance(reader, FixedIndexReader):
        digests, size, chunk_size = reader.digests, reader.size, reader.chunk_size
    else:
        digests, size, chunk_size = reader
    digests = _digest_rows(digests)
    n = int(digests.shape[0])
    so = np.ascontiguousarray(np.asarray(store_offsets, dtype=np.uint64))
    sd = _digest_rows(store_digests)
    m = int(sd.shape[0])
    if so.size != m + 1:
        raise ValueError(f"store_offsets holds {so.size} values, {m} blobs need {m + 1}")
    if length is None:
        length = max(0, int(size) - int(offset))
    status = np.full(n, BLOB_ST_NONE_REQUESTED, dtype=np.uint8)
    t = RestoreTiming()
    rc = lib().pbs_restore_fixed_range_device(
        digests.ctypes.data if n else None, n, int(size), int(chunk_size), ctypes.c_void_p(store_blobs_dev or None),
        so.ctypes.data, sd.ctypes.data if m else None, m, crypt.handle if crypt is not None else None, int(offset),
        int(length), ctypes.c_void_p(out_dev or None), status.ctypes.data if n else None, ctypes.byref(t),
        ctypes.c_void_p(hip_stream))
    if rc != PBS_OK:
        raise ChunkerError(rc, "pbs_restore_fixed_range_device")
    if t.failed and not allow_bad:
        bad = [(int(k), int(status[k])) for k in np.flatnonzero((status != BLOB_ST_OK) & (status != BLOB_ST_NONE_REQUESTED))]
        raise ChunkerError(PBS_ERR_INVALID, f"restore: {t.failed} entries failed (entry, status): {bad[:8]}")
    return status, t.as_dict()


# ---- garbage collection (include/pbs_gc.h) -------------------------------------------------------

GC_BAD = 1       # PBS_GC_BAD: the name ends in ".bad"
GC_FOREIGN = 2   # PBS_GC_FOREIGN: listed, but at a path phase 1 never touches
GC_KEEP, GC_PENDING, GC_REMOVE = 0, 1, 2
GC_VANISHED = (1 << 64) - 1  # sizes[j] of an entry that could not be stat'ed or is no regular file

_HEX = frozenset(b"0123456789abcdefABCDEF")
_HEX_LOWER = frozenset(b"0123456789abcdef")


def gc_release() -> None:
    """pbs_gc_release: free the idle work areas of the GC calls."""
    lib().pbs_gc_release()


def gc_home_slot(digest, table_log2: int) -> int:
    """pbs_gc_home_slot: the slot at which a digest's probe of a 2^table_log2 table starts."""
    d = _as_u8(digest)
    if d.size != 32:
        raise ValueError("a digest has 32 bytes")
    return int(lib().pbs_gc_home_slot(d.ctypes.data, table_log2))


def list_chunk_store(base):
    """The files ``ChunkStore::get_chunk_iterator`` (pbs-datastore/src/chunk_store.rs:247-343)
    yields under ``base/.chunks/0000 .. ffff`` (missing subdirectories are fine), with its name
    filter (:288-296): 64 or 70 bytes, the first 64 ASCII hex digits of either case; bad = ends
    with ".bad".  Returns (paths, digests (m, 32) uint8, flags (m) uint8).  GC_FOREIGN marks a name
    that ``chunk_path`` never builds -- anything but 64 lower-case hex digits, or those + "." + one
    digit + ".bad", in the subdirectory of its first four digits: phase 1 never touches such a
    path, and it never counts as the chunk being there."""
    root = os.path.join(os.fsencode(base), b".chunks")
    try:
        subs = sorted(s for s in os.listdir(root) if len(s) == 4 and all(c in _HEX_LOWER for c in s))
    except FileNotFoundError:
        subs = []
    paths, digs, flags = [], [], []
    for sub in subs:
        try:
            names = sorted(os.listdir(os.path.join(root, sub)))
        except (FileNotFoundError, NotADirectoryError):
            continue
        for name in names:
            if len(name) not in (64, 70) or not all(c in _HEX for c in name[:64]):
                continue
            f = GC_BAD if name.endswith(b".bad") else 0
            own = all(c in _HEX_LOWER for c in name[:64]) and name[:4] == sub and (
                len(name) == 64 or (name[64:65] == b"." and name[65:66].isdigit() and name[66:] == b".bad"))
            if not own:
                f |= GC_FOREIGN
            paths.append(os.fsdecode(os.path.join(root, sub, name)))
            digs.append(bytes.fromhex(name[:64].decode("ascii")))
            flags.append(f)
    digests = np.frombuffer(b"".join(digs), dtype=np.uint8).reshape(-1, 32).copy()
    return paths, digests, np.asarray(flags, dtype=np.uint8)


def _index_digest_span(image: bytes):
    """(offset, stride, count bound) of the digests of a .didx / .fidx image, by its magic."""
    if image[:8] == DIDX_MAGIC:
        return DIDX_HEADER + 8, DIDX_ENTRY, max(0, (len(image) - DIDX_HEADER) // DIDX_ENTRY)
    return FIDX_HEADER, 32, max(0, (len(image) - FIDX_HEADER) // 32)


class GarbageCollector:
    """One GC run over a chunk store's listing (``list_chunk_store``'s result, or (paths or None,
    digests, flags)): a context manager over a pbs_gc handle (``device=True``: the table lives in
    the memory of ``hip_stream``'s device) or over the host mirror's (``device=False``: no GPU)."""

    def __init__(self, listing, device: bool = True, hip_stream: int = 0):
        paths, digests, flags = listing
        self.paths = list(paths) if paths is not None else None
        self.digests = _digest_rows(digests)
        self.flags = np.ascontiguousarray(np.asarray(flags, dtype=np.uint8).reshape(-1))
        self.m = int(self.digests.shape[0])
        if self.flags.size != self.m:
            raise ValueError(f"{self.m} digests, {self.flags.size} flags")
        self.device = bool(device)
        self._sfx = "" if self.device else "_host"
        h, ms = ctypes.c_void_p(None), ctypes.c_double(0)
        args = [self.digests.ctypes.data if self.m else None, self.flags.ctypes.data if self.m else None, self.m,
                ctypes.byref(h), ctypes.byref(ms)]
        if self.device:
            rc = lib().pbs_gc_begin(*args, ctypes.c_void_p(hip_stream))
        else:
            rc = lib().pbs_gc_begin_host(*args)
        if rc != PBS_OK:
            raise ChunkerError(rc, "pbs_gc_begin" + self._sfx)
        self._h = h
        self.build_ms = float(ms.value)
        self.mark_ms = 0.0   # of the last mark call
        self.sweep_ms = 0.0  # of the last sweep

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def close(self) -> None:
        """pbs_gc_end.  Every later call raises ChunkerError(PBS_ERR_INVALID)."""
        if getattr(self, "_h", None) is not None and not getattr(self, "_closed", False):
            self._closed = True
            (lib().pbs_gc_end if self.device else lib().pbs_gc_end_host)(self._h)

    @property
    def table_log2(self) -> int:
        """L of the device table (2^L slots); None for the host mirror, which keeps a sorted list."""
        return int(lib().pbs_gc_table_log2(self._h)) if self.device else None

    def _fn(self, name: str):
        return getattr(lib(), name + self._sfx)

    def mark(self, base: int, stride: int, n: int, index_bytes: Optional[int] = None, cap: Optional[int] = None):
        """pbs_gc_mark_device (``index_bytes`` given: one index file) or pbs_gc_mark_piece (None: a
        piece, counts no file) over the n digests at address ``base`` + i * ``stride`` -- device
        memory for a device handle, host memory for the mirror.  Returns (the first ``cap``
        positions of missing entries, ascending; n_missing); ``cap`` defaults to n."""
        cap = int(n) if cap is None else int(cap)
        pos = np.zeros(cap, dtype=np.uint32)
        nm, ms = ctypes.c_size_t(0), ctypes.c_double(0)
        tail = [pos.ctypes.data if cap else None, cap, ctypes.byref(nm), ctypes.byref(ms)]
        if index_bytes is None:
            name = "pbs_gc_mark_piece"
            rc = self._fn(name)(self._h, ctypes.c_void_p(base or None), stride, n, *tail)
        else:
            name = "pbs_gc_mark_device" if self.device else "pbs_gc_mark"
            rc = self._fn(name)(self._h, ctypes.c_void_p(base or None), stride, n, int(index_bytes), *tail)
        if rc != PBS_OK:
            raise ChunkerError(rc, name + self._sfx)
        self.mark_ms = float(ms.value)
        return pos[:min(cap, int(nm.value))], int(nm.value)

    def mark_index(self, path_or_bytes, cap: Optional[int] = None) -> np.ndarray:
        """pbs_gc_mark_index_image over a .didx / .fidx file (a path) or image (bytes): the positions
        of its missing entries, ascending (the first ``cap``; default all).  ``n_missing`` keeps
        the count of the last call.  A bad image raises ChunkerError and marks nothing."""
        if isinstance(path_or_bytes, (str, os.PathLike)):
            with open(path_or_bytes, "rb") as f:
                image = f.read()
        else:
            image = bytes(path_or_bytes)
        if cap is None:
            cap = _index_digest_span(image)[2]
        pos = np.zeros(cap, dtype=np.uint32)
        nm, ms = ctypes.c_size_t(0), ctypes.c_double(0)
        rc = self._fn("pbs_gc_mark_index_image")(self._h, image, len(image), pos.ctypes.data if cap else None, cap,
                                                 ctypes.byref(nm), ctypes.byref(ms))
        if rc != PBS_OK:
            raise ChunkerError(rc, "pbs_gc_mark_index_image" + self._sfx)
        self.mark_ms = float(ms.value)
        self.n_missing = int(nm.value)
        return pos[:min(cap, self.n_missing)]

    def touched(self) -> np.ndarray:
        """pbs_gc_touched: touched[j] = 1 for the entries phase 1 would have touched."""
        t = np.zeros(self.m, dtype=np.uint8)
        nt = ctypes.c_size_t(0)
        rc = self._fn("pbs_gc_touched")(self._h, t.ctypes.data if self.m else None, ctypes.byref(nt))
        if rc != PBS_OK:
            raise ChunkerError(rc, "pbs_gc_touched" + self._sfx)
        return t

    def sweep(self, sizes, atimes, phase1_start: int, oldest_writer: int):
        """pbs_gc_sweep: (actions (m) uint8 of GC_KEEP / GC_PENDING / GC_REMOVE, the status as a
        dict with the reference's kebab-case keys)."""
        sz = np.ascontiguousarray(np.asarray(sizes, dtype=np.uint64).reshape(-1))
        at = np.ascontiguousarray(np.asarray(atimes, dtype=np.int64).reshape(-1))
        if sz.size != self.m or at.size != self.m:
            raise ValueError(f"the listing has {self.m} entries: {sz.size} sizes, {at.size} atimes")
        actions = np.zeros(self.m, dtype=np.uint8)
        st, ms = GcStatus(), ctypes.c_double(0)
        rc = self._fn("pbs_gc_sweep")(self._h, sz.ctypes.data if self.m else None, at.ctypes.data if self.m else None,
                                      int(phase1_start), int(oldest_writer), actions.ctypes.data if self.m else None,
                                      ctypes.byref(st), ctypes.byref(ms))
        if rc != PBS_OK:
            raise ChunkerError(rc, "pbs_gc_sweep" + self._sfx)
        self.sweep_ms = float(ms.value)
        return actions, st.as_dict()


def garbage_collection(base, index_paths, phase1_start: Optional[int] = None, oldest_writer: Optional[int] = None,
                       device: bool = True, apply: bool = True):
    """``DataStore::garbage_collection`` (pbs-datastore/src/datastore.rs:1065-1177) over the chunk
    store under ``base`` and the given index files, in the reference's order: list the store and
    mark every index (a vanished index file is skipped, :1029; a file that is neither .fidx nor
    .didx is ignored, :1015); with ``apply`` set the atime of the touched files to now (mtime
    unchanged); THEN lstat every listed file (no regular file, or gone: GC_VANISHED); sweep; with
    ``apply`` unlink the GC_REMOVE entries.  ``phase1_start`` defaults to now (taken before the
    marks), ``oldest_writer`` to it (no writer).  Files created after the listing are outside the
    plan: never removed, not counted.  Returns (status dict with the keys of .gc-status, list of
    (index path, hex digest) warnings: entries whose chunk is absent, every occurrence)."""
    import time

    if phase1_start is None:
        phase1_start = int(time.time())
    if oldest_writer is None:
        oldest_writer = phase1_start
    listing = list_chunk_store(base)
    paths = listing[0]
    warnings = []
    with GarbageCollector(listing, device=device) as gc:
        for ip in index_paths:
            name = os.fspath(ip)
            if not (name.endswith(".fidx") or name.endswith(".didx")):
                continue
            try:
                with open(ip, "rb") as f:
                    image = f.read()
            except FileNotFoundError:
                continue
            off, stride, _ = _index_digest_span(image)
            for pos in gc.mark_index(image):
                at = off + stride * int(pos)
                warnings.append((name, image[at:at + 32].hex()))
        if apply:
            for j in np.flatnonzero(gc.touched()):
                try:
                    st = os.lstat(paths[j])
                    os.utime(paths[j], ns=(time.time_ns(), st.st_mtime_ns), follow_symlinks=False)
                except FileNotFoundError:
                    pass
        import stat as _stat
        sizes = np.full(len(paths), GC_VANISHED, dtype=np.uint64)
        atimes = np.zeros(len(paths), dtype=np.int64)
        for j, p in enumerate(paths):
            try:
                st = os.lstat(p)
            except OSError:
                continue
            if _stat.S_ISREG(st.st_mode):
                sizes[j] = st.st_size
                atimes[j] = st.st_atime_ns // 1_000_000_000
        actions, status = gc.sweep(sizes, atimes, phase1_start, oldest_writer)
    if apply:
        for j in np.flatnonzero(actions == GC_REMOVE):
            os.unlink(paths[j])
    return status, warnings


# ---- the verify job (include/pbs_verify.h) -------------------------------------------------------

VERIFY_UNKNOWN, VERIFY_VERIFIED, VERIFY_CORRUPT = 0, 1, 2
VERIFY_MODE_NONE, VERIFY_MODE_ENCRYPT = 0, 1
VERIFY_ST_LOAD_FAILED = 32   # PBS_VERIFY_ST_LOAD_FAILED: the caller could not open or read the file
VERIFY_INDEX_OK, VERIFY_INDEX_WRONG_SIZE, VERIFY_INDEX_WRONG_CSUM = 0, 1, 2
(VERIFY_BLOB_OK, VERIFY_BLOB_WRONG_SIZE, VERIFY_BLOB_WRONG_CSUM, VERIFY_BLOB_LOAD, VERIFY_BLOB_DECODE) = range(5)
_VERIFY_BLOB_ERRORS = ("", "wrong size", "wrong index checksum", "unable to load blob", "unable to decode blob")


def verify_release() -> None:
    """pbs_verify_release: free the idle work areas of the verify calls."""
    lib().pbs_verify_release()


def verify_crypt_mode(crypt_mode) -> int:
    """``FileInfo::chunk_crypt_mode`` (pbs-datastore/src/manifest.rs:39-44) of a manifest's
    "crypt-mode" string, or a VERIFY_MODE_* value as it is: "encrypt" is ENCRYPT, "none" and
    "sign-only" are NONE."""
    if isinstance(crypt_mode, str):
        try:
            return {"encrypt": VERIFY_MODE_ENCRYPT, "none": VERIFY_MODE_NONE, "sign-only": VERIFY_MODE_NONE}[crypt_mode]
        except KeyError:
            raise ValueError(f"unknown crypt mode {crypt_mode!r}") from None
    return int(crypt_mode)


def verify_blob(raw, info) -> int:
    """pbs_verify_blob_host (verify.rs:48-70): ``info`` is (size, csum) of the manifest's FileInfo,
    ``csum`` 32 bytes.  Returns VERIFY_BLOB_*: the first of raw size, SHA-256 of the raw bytes,
    the load (size, magic, CRC), the decode of an unencrypted blob that fails."""
    a = _as_u8(raw)
    size, csum = info
    csum = bytes(csum)
    if len(csum) != 32:
        raise ValueError("a checksum has 32 bytes")
    res = ctypes.c_int(0)
    rc = lib().pbs_verify_blob_host(_ptr(a), a.size, int(size), ctypes.create_string_buffer(csum, 32), ctypes.byref(res))
    if rc != PBS_OK:
        raise ChunkerError(rc, "pbs_verify_blob_host")
    return int(res.value)


def bad_chunk_path(path: str) -> str:
    """The name ``rename_corrupted_chunk`` (verify.rs:79-88) moves a corrupt chunk to:
    "<path>.N.bad" with the first N in 0..8 that does not exist yet -- and N = 9 whether that
    exists or not: the reference's loop stops counting at 9 and overwrites."""
    counter = 0
    while True:
        new_path = f"{path}.{counter}.bad"
        if os.path.exists(new_path) and counter < 9:
            counter += 1
        else:
            return new_path


class VerifyWorker:
    """``VerifyWorker`` (src/backup/verify.rs:27-46) over a chunk store's listing
    (``list_chunk_store``'s result, or (paths or None, digests[, flags])): a context manager over a
    pbs_verify handle (``device=True``: table and states live in the memory of ``hip_stream``'s
    device) or over the host mirror's (``device=False``: no GPU).  Only chunk files proper belong
    in the listing: entries whose flags are not 0 (.bad files, foreign names) are dropped.  The
    states -- the worker's verified_chunks / corrupt_chunks -- live until ``close``."""

    def __init__(self, listing, device: bool = True, hip_stream: int = 0):
        paths, digests = listing[0], _digest_rows(listing[1])
        if len(listing) > 2 and listing[2] is not None:
            keep = np.flatnonzero(np.asarray(listing[2], dtype=np.uint8).reshape(-1) == 0)
            digests = np.ascontiguousarray(digests[keep])
            paths = [paths[j] for j in keep] if paths is not None else None
        self.paths = list(paths) if paths is not None else None
        self.digests = digests
        self.m = int(digests.shape[0])
        self.device = bool(device)
        self._sfx = "" if self.device else "_host"
        h, ms = ctypes.c_void_p(None), ctypes.c_double(0)
        args = [self.digests.ctypes.data if self.m else None, self.m, ctypes.byref(h), ctypes.byref(ms)]
        if self.device:
            rc = lib().pbs_verify_begin(*args, ctypes.c_void_p(hip_stream))
        else:
            rc = lib().pbs_verify_begin_host(*args)
        if rc != PBS_OK:
            raise ChunkerError(rc, "pbs_verify_begin" + self._sfx)
        self._h = h
        self.build_ms = float(ms.value)
        self.plan_ms = 0.0       # of the last plan
        self.timing = None       # of the last submit

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def close(self) -> None:
        """pbs_verify_end.  Every later call raises ChunkerError(PBS_ERR_INVALID)."""
        if getattr(self, "_h", None) is not None and not getattr(self, "_closed", False):
            self._closed = True
            (lib().pbs_verify_end if self.device else lib().pbs_verify_end_host)(self._h)

    def _fn(self, name: str):
        return getattr(lib(), name + self._sfx)

    def states(self) -> np.ndarray:
        """pbs_verify_states: VERIFY_UNKNOWN / VERIFIED / CORRUPT per listing entry."""
        s = np.zeros(self.m, dtype=np.uint8)
        rc = self._fn("pbs_verify_states")(self._h, s.ctypes.data if self.m else None, self.m)
        if rc != PBS_OK:
            raise ChunkerError(rc, "pbs_verify_states" + self._sfx)
        return s

    def plan(self, digests, sizes, crypt_mode):
        """pbs_verify_plan over an index's digests (n, 32) and chunk sizes (n): (todo_store,
        todo_entry), the store positions to read in ascending order and for each the lowest
        index position naming it."""
        d = _digest_rows(digests)
        sz = np.ascontiguousarray(np.asarray(sizes, dtype=np.uint64).reshape(-1))
        n = int(d.shape[0])
        if sz.size != n:
            raise ValueError(f"{n} digests, {sz.size} sizes")
        cap = min(n, self.m)
        ts, te = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32)
        nt, ms = ctypes.c_size_t(0), ctypes.c_double(0)
        rc = self._fn("pbs_verify_plan")(self._h, d.ctypes.data if n else None, sz.ctypes.data if n else None, n,
                                         verify_crypt_mode(crypt_mode), ts.ctypes.data if cap else None,
                                         te.ctypes.data if cap else None, cap, ctypes.byref(nt), ctypes.byref(ms))
        if rc != PBS_OK:
            raise ChunkerError(rc, "pbs_verify_plan" + self._sfx)
        self.plan_ms = float(ms.value)
        return ts[:nt.value], te[:nt.value]

    def abort_index(self) -> None:
        """pbs_verify_abort_index: drop an unfinished plan; no state changes."""
        rc = self._fn("pbs_verify_abort_index")(self._h)
        if rc != PBS_OK:
            raise ChunkerError(rc, "pbs_verify_abort_index" + self._sfx)

    def submit(self, blobs, blob_offsets, load_failed=None):
        """pbs_verify_submit of the plan's next k items.  ``blobs``: for a device handle the device
        address of the raw blob images, for the mirror bytes or an array; ``blob_offsets``: k + 1
        offsets into it; ``load_failed``: None or k flags.  Returns (kinds (k), status (k))."""
        off = np.ascontiguousarray(np.asarray(blob_offsets, dtype=np.uint64).reshape(-1))
        k = max(0, off.size - 1)
        lf = None
        if load_failed is not None:
            lf = np.ascontiguousarray(np.asarray(load_failed, dtype=np.uint8).reshape(-1))
            if lf.size != k:
                raise ValueError(f"{k} blobs, {lf.size} load_failed flags")
        if self.device:
            ptr = ctypes.c_void_p(int(blobs) or None)
        else:
            keep = _as_u8(blobs)
            ptr = _ptr(keep)
        kinds, status = np.zeros(k, dtype=np.uint8), np.zeros(k, dtype=np.uint8)
        t = VerifyTiming()
        rc = self._fn("pbs_verify_submit")(self._h, ptr, off.ctypes.data if off.size else None,
                                           None if lf is None else _ptr(lf), k, _ptr(kinds), _ptr(status),
                                           ctypes.byref(t))
        if rc != PBS_OK:
            raise ChunkerError(rc, "pbs_verify_submit" + self._sfx)
        self.timing = t.as_dict()
        return kinds, status

    def _lists(self, n_hint: int):
        cs = np.zeros(max(self.m, 1), dtype=np.uint32)
        mp = np.zeros(max(int(n_hint), 1), dtype=np.uint32)
        return cs, mp

    def finish(self, n_hint: Optional[int] = None):
        """pbs_verify_finish: (result dict, corrupt_store -- the store positions that became
        CORRUPT in this index, ascending -- and missing_pos, the index positions whose chunk is
        absent).  ``n_hint``: the index's length (bounds missing_pos; default 2^20 entries, and
        the call is repeated nowhere: pass it for longer indexes)."""
        cs, mp = self._lists((1 << 20) if n_hint is None else n_hint)
        res, nc, nm = VerifyResult(), ctypes.c_size_t(0), ctypes.c_size_t(0)
        rc = self._fn("pbs_verify_finish")(self._h, ctypes.byref(res), cs.ctypes.data, cs.size, ctypes.byref(nc),
                                           mp.ctypes.data, mp.size, ctypes.byref(nm))
        if rc != PBS_OK:
            raise ChunkerError(rc, "pbs_verify_finish" + self._sfx)
        return res.as_dict(), cs[:min(cs.size, nc.value)].copy(), mp[:min(mp.size, nm.value)].copy()

    def verify_index(self, image, crypt_mode, info=None, store=None, budget: int = 0):
        """pbs_verify_index_device / pbs_verify_index_host over a .didx / .fidx image (bytes or a
        path).  ``info``: None or (size, csum) of the manifest's FileInfo, either of which may be
        None; ``store``: (blobs, offsets) -- the chunk files of the listing back to back, for a
        device handle a device address, for the mirror bytes or an array -- with m + 1 offsets;
        ``budget``: the bound of a batch in bytes (0: none).  Returns (result dict, corrupt_store,
        missing_pos).  A bad image raises ChunkerError and changes nothing."""
        if isinstance(image, (str, os.PathLike)):
            with open(image, "rb") as f:
                image = f.read()
        image = bytes(image)
        if store is None:
            raise ValueError("store=(blobs, offsets) is required")
        blobs, offsets = store
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint64).reshape(-1))
        if off.size != self.m + 1:
            raise ValueError(f"the listing has {self.m} entries: {off.size} offsets")
        if self.device:
            ptr = ctypes.c_void_p(int(blobs) or None)
        else:
            keep = _as_u8(blobs)
            ptr = _ptr(keep)
        isz = icsum = None
        if info is not None:
            if info[0] is not None:
                isz = ctypes.byref(ctypes.c_uint64(int(info[0])))
            if info[1] is not None:
                if len(bytes(info[1])) != 32:
                    raise ValueError("a checksum has 32 bytes")
                icsum = ctypes.create_string_buffer(bytes(info[1]), 32)
        cs, mp = self._lists(_index_digest_span(image)[2])
        res, nc, nm = VerifyResult(), ctypes.c_size_t(0), ctypes.c_size_t(0)
        name = "pbs_verify_index_device" if self.device else "pbs_verify_index_host"
        rc = getattr(lib(), name)(self._h, image, len(image), verify_crypt_mode(crypt_mode), isz, icsum, ptr,
                                  off.ctypes.data, int(budget), ctypes.byref(res), cs.ctypes.data, cs.size,
                                  ctypes.byref(nc), mp.ctypes.data, mp.size, ctypes.byref(nm))
        if rc != PBS_OK:
            raise ChunkerError(rc, name)
        return res.as_dict(), cs[:min(cs.size, nc.value)].copy(), mp[:min(mp.size, nm.value)].copy()


def _manifest_of(snapshot_dir):
    """``BackupDir::load_manifest``: index.json.blob through the blob decoder, then JSON."""
    import json

    with open(os.path.join(snapshot_dir, "index.json.blob"), "rb") as f:
        raw = f.read()
    payload, kind, status = blob_decode_host(raw)
    if status != BLOB_ST_OK:
        raise ValueError(f"manifest blob: status {status}")
    if kind == BLOB_KIND_COMPRESSED:
        cap = 1 << 20
        while True:
            data, zst = zstd_inflate_host(payload, cap)
            if zst == ZST_TOO_LARGE and cap < (128 << 20):
                cap *= 4
                continue
            if zst != ZST_OK:
                raise ValueError(f"manifest blob: zstd status {zst}")
            payload = data
            break
    manifest = json.loads(payload.decode("utf-8"))
    if not isinstance(manifest.get("files"), list):
        raise ValueError("manifest without files")
    return manifest


def verify_snapshot(base, snapshot_dir, worker: VerifyWorker, rename: bool = False, batch_bytes: int = 256 << 20):
    """``verify_backup_dir_with_lock`` (src/backup/verify.rs:364-446) for the snapshot directory
    ``snapshot_dir`` of the datastore under ``base``, with ``worker`` (over
    ``list_chunk_store(base)``) carrying the chunk states from snapshot to snapshot.  Walks the
    manifest's files as :404-432 does: a .blob through ``verify_blob``; a .fidx / .didx through
    the size and checksum check, the plan, the todo chunk files read from ``base/.chunks`` in
    batches of about ``batch_bytes`` (a file that cannot be read is a load failure), and the
    finish.  With ``rename`` the chunks found corrupt are moved to ``bad_chunk_path`` (:72-106).
    Returns ("ok" | "failed", [(filename, None | error text, result dict | None)]).  A manifest
    that does not load is ("failed", []).  Not done here: writing verify_state back into the
    manifest, snapshot locks, namespaces and group walking, the filter callback, the task log."""
    if worker.paths is None:
        raise ValueError("the worker's listing has no paths")
    try:
        manifest = _manifest_of(snapshot_dir)
    except (OSError, ValueError, ChunkerError):
        return "failed", []
    results = []
    for info in manifest["files"]:
        name = str(info.get("filename", ""))
        res = None
        try:
            size, csum = int(info["size"]), bytes.fromhex(info["csum"])
            path = os.path.join(snapshot_dir, name)
            if name.endswith(".blob"):
                with open(path, "rb") as f:
                    raw = f.read()
                v = verify_blob(raw, (size, csum))
                err = _VERIFY_BLOB_ERRORS[v] or None
            elif name.endswith(".fidx") or name.endswith(".didx"):
                mode = verify_crypt_mode(info.get("crypt-mode", "none"))
                err, res = _verify_index_files(worker, path, name.endswith(".fidx"), mode, size, csum, rename,
                                               batch_bytes)
            else:
                err = f"unable to parse archive type of {name!r}"
        except (OSError, ValueError, KeyError, ChunkerError) as e:
            try:
                worker.abort_index()
            except ChunkerError:
                pass
            err = str(e) or type(e).__name__
        results.append((name, err, res))
    return ("ok" if all(e is None for _, e, _ in results) else "failed"), results


def _verify_index_files(worker, path, fixed, mode, info_size, info_csum, rename, batch_bytes):
    """verify_fixed_index / verify_dynamic_index (:272-314) + verify_index_chunks with the chunk
    files read from disk: (None | error text, result dict | None)."""
    if fixed:
        r = FixedIndexReader(path)
        n = r.index_count()
        sizes = np.minimum(np.uint64(r.chunk_size), np.uint64(r.size) - np.arange(n, dtype=np.uint64) * np.uint64(r.chunk_size))
    else:
        r = DynamicIndexReader(path)
        n = r.index_count()
        sizes = np.diff(np.concatenate([[0], r.ends]).astype(np.uint64))
    if r.index_bytes() != info_size:
        return f"wrong size ({info_size} != {r.index_bytes()})", None
    if r.compute_csum()[0] != info_csum:
        return "wrong index checksum", None
    todo_store, _ = worker.plan(r.digests, sizes, mode)
    t = 0
    while t < todo_store.size:
        parts, offs, failed = [], [0], []
        while t < todo_store.size and (not parts or offs[-1] < batch_bytes):
            try:
                with open(worker.paths[int(todo_store[t])], "rb") as f:
                    data = f.read()
                failed.append(0)
            except OSError:
                data = b""
                failed.append(1)
            parts.append(data)
            offs.append(offs[-1] + len(data))
            t += 1
        raw = np.frombuffer(b"".join(parts), dtype=np.uint8)
        if worker.device:
            import torch

            dev = torch.from_numpy(raw.copy()).to("cuda") if raw.size else None
            worker.submit(dev.data_ptr() if dev is not None else 0, offs, failed)
        else:
            worker.submit(raw, offs, failed)
    res, corrupt, _ = worker.finish(n)
    if rename:
        for j in corrupt:
            p = worker.paths[int(j)]
            try:
                os.rename(p, bad_chunk_path(p))
            except FileNotFoundError:
                pass  # (:96)
    return (None if res["ok"] else "chunks could not be verified"), res


# ---- the sync job (include/pbs_sync.h) -----------------------------------------------------------

SYNC_DUP, SYNC_EXISTS, SYNC_FETCH = 0, 1, 2
SYNC_ST_LOAD_FAILED = 32          # PBS_SYNC_ST_LOAD_FAILED: the caller could not fetch the blob
SYNC_NONE = (1 << 64) - 1         # PBS_SYNC_NONE: first_failed of a result with no failing item
_ENC_MAGICS = (bytes([123, 103, 133, 190, 34, 45, 76, 240]), bytes([230, 89, 27, 191, 11, 191, 216, 11]))


def sync_release() -> None:
    """pbs_sync_release: free the idle work areas of the sync calls."""
    lib().pbs_sync_release()


def chunk_path(base, digest) -> str:
    """``ChunkStore::chunk_path`` (pbs-datastore/src/chunk_store.rs:557-570):
    base/.chunks/<first four hex digits>/<hex>."""
    h = bytes(digest).hex()
    return os.path.join(base, ".chunks", h[:4], h)


def _index_entries(image: bytes, n: int):
    """(digests (n, 32), chunk_info sizes (n)) of an accepted .didx / .fidx image."""
    off, stride, _ = _index_digest_span(image)
    head = off - (stride - 32)
    rows = np.frombuffer(image, dtype=np.uint8, count=n * stride, offset=head).reshape(n, stride)
    digests = np.ascontiguousarray(rows[:, stride - 32:])
    if stride == 32:
        size, cs = (int.from_bytes(image[o:o + 8], "little") for o in (64, 72))
        sizes = np.minimum(np.uint64(cs), np.uint64(size) - np.arange(n, dtype=np.uint64) * np.uint64(cs))
    else:
        ends = np.ascontiguousarray(rows[:, :8]).view("<u8").reshape(-1)
        sizes = np.diff(np.concatenate([[0], ends]).astype(np.uint64))
    return digests, sizes.astype(np.uint64)


class SyncWorker:
    """The target side of a sync job (``pull_index_chunks``, src/server/pull.rs:605-705) over the
    local chunk store's listing (``list_chunk_store``'s result, or (paths or None, digests[,
    flags]); entries whose flags are not 0 are dropped): a context manager over a pbs_sync handle
    (``device=True``: table, digest list, present and claimed bytes live in the memory of
    ``hip_stream``'s device) or over the host mirror's (``device=False``: no GPU).  ``reserve``:
    the number of chunks the job is expected to add; with enough of it the table is never rebuilt.
    The claimed bytes -- ``downloaded_chunks`` -- live until ``new_group``, everything else until
    ``close``."""

    def __init__(self, listing, reserve: int = 0, device: bool = True, hip_stream: int = 0):
        digests = _digest_rows(listing[1])
        if len(listing) > 2 and listing[2] is not None:
            keep = np.flatnonzero(np.asarray(listing[2], dtype=np.uint8).reshape(-1) == 0)
            digests = np.ascontiguousarray(digests[keep])
        m = int(digests.shape[0])
        self.device = bool(device)
        self.hip_stream = int(hip_stream)
        self._sfx = "" if self.device else "_host"
        h, ms = ctypes.c_void_p(None), ctypes.c_double(0)
        args = [digests.ctypes.data if m else None, m, int(reserve), ctypes.byref(h), ctypes.byref(ms)]
        if self.device:
            rc = lib().pbs_sync_begin(*args, ctypes.c_void_p(hip_stream))
        else:
            rc = lib().pbs_sync_begin_host(*args)
        if rc != PBS_OK:
            raise ChunkerError(rc, "pbs_sync_begin" + self._sfx)
        self._h = h
        self.build_ms = float(ms.value)
        self.plan_ms = 0.0          # of the last plan
        self.timing = None          # of the last submit
        self.index_digests = None   # of the open index: (n, 32)
        self.index_sizes = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def close(self) -> None:
        """pbs_sync_end.  Every later call raises ChunkerError(PBS_ERR_INVALID)."""
        if getattr(self, "_h", None) is not None and not getattr(self, "_closed", False):
            self._closed = True
            (lib().pbs_sync_end if self.device else lib().pbs_sync_end_host)(self._h)

    def _fn(self, name: str):
        return getattr(lib(), name + self._sfx)

    def _check(self, rc: int, name: str) -> None:
        if rc != PBS_OK:
            raise ChunkerError(rc, name + self._sfx)

    @property
    def count(self) -> int:
        """pbs_sync_count: the entries, listed and appended (0 after ``close``)."""
        return int(self._fn("pbs_sync_count")(self._h))

    @property
    def table_log2(self) -> int:
        """pbs_sync_table_log2."""
        return int(self._fn("pbs_sync_table_log2")(self._h))

    def listing(self):
        """pbs_sync_listing: (digests (count, 32), present (count)) as they stand."""
        n = ctypes.c_size_t(0)
        self._check(self._fn("pbs_sync_listing")(self._h, None, None, 0, ctypes.byref(n)), "pbs_sync_listing")
        d, p = np.zeros((n.value, 32), dtype=np.uint8), np.zeros(n.value, dtype=np.uint8)
        self._check(self._fn("pbs_sync_listing")(self._h, _ptr(d), _ptr(p), n.value, ctypes.byref(n)), "pbs_sync_listing")
        return d, p

    def new_group(self) -> None:
        """pbs_sync_new_group: a fresh ``downloaded_chunks`` (pull.rs:1134)."""
        self._check(self._fn("pbs_sync_new_group")(self._h), "pbs_sync_new_group")

    def plan(self, digests, sizes):
        """pbs_sync_plan over an index's digests (n, 32) and chunk sizes (n): (verdict (n) of
        SYNC_DUP / SYNC_EXISTS / SYNC_FETCH, fetch_store, fetch_entry, touch_store)."""
        d = _digest_rows(digests)
        sz = np.ascontiguousarray(np.asarray(sizes, dtype=np.uint64).reshape(-1))
        n = int(d.shape[0])
        if sz.size != n:
            raise ValueError(f"{n} digests, {sz.size} sizes")
        v = np.zeros(n, dtype=np.uint8)
        fs, fe, ts = (np.zeros(n, dtype=np.uint32) for _ in range(3))
        nf, nt, ms = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_double(0)
        rc = self._fn("pbs_sync_plan")(self._h, _ptr(d), _ptr(sz), n, _ptr(v), _ptr(fs), _ptr(fe), n, ctypes.byref(nf),
                                       _ptr(ts), n, ctypes.byref(nt), ctypes.byref(ms))
        self._check(rc, "pbs_sync_plan")
        self.plan_ms = float(ms.value)
        self.index_digests, self.index_sizes = d, sz
        return v, fs[:nf.value], fe[:nf.value], ts[:nt.value]

    def lists(self):
        """pbs_sync_lists: (fetch_store, fetch_entry, touch_store) of the open index again."""
        nf, nt = ctypes.c_size_t(0), ctypes.c_size_t(0)
        self._check(self._fn("pbs_sync_lists")(self._h, None, None, 0, ctypes.byref(nf), None, 0, ctypes.byref(nt)),
                    "pbs_sync_lists")
        fs, fe, ts = np.zeros(nf.value, np.uint32), np.zeros(nf.value, np.uint32), np.zeros(nt.value, np.uint32)
        rc = self._fn("pbs_sync_lists")(self._h, _ptr(fs), _ptr(fe), fs.size, ctypes.byref(nf), _ptr(ts), ts.size,
                                        ctypes.byref(nt))
        self._check(rc, "pbs_sync_lists")
        return fs, fe, ts

    def plan_index(self, image, info=None):
        """pbs_sync_index_image over a .didx / .fidx image (bytes or a path).  ``info``: None or
        (size, csum) of the manifest's FileInfo, either of which may be None.  Returns
        (index_check, verdict, fetch_store, fetch_entry, touch_store); with index_check
        VERIFY_INDEX_WRONG_SIZE / WRONG_CSUM nothing was claimed, no index is open and the lists
        are empty.  A bad image raises ChunkerError and changes nothing."""
        if isinstance(image, (str, os.PathLike)):
            with open(image, "rb") as f:
                image = f.read()
        image = bytes(image)
        isz = icsum = None
        if info is not None:
            if info[0] is not None:
                isz = ctypes.byref(ctypes.c_uint64(int(info[0])))
            if info[1] is not None:
                if len(bytes(info[1])) != 32:
                    raise ValueError("a checksum has 32 bytes")
                icsum = ctypes.create_string_buffer(bytes(info[1]), 32)
        cap = _index_digest_span(image)[2]
        v = np.zeros(cap, dtype=np.uint8)
        fs, fe, ts = (np.zeros(cap, dtype=np.uint32) for _ in range(3))
        chk, n = ctypes.c_uint32(0), ctypes.c_size_t(0)
        nf, nt, ms = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_double(0)
        rc = self._fn("pbs_sync_index_image")(self._h, image, len(image), isz, icsum, ctypes.byref(chk), ctypes.byref(n),
                                              _ptr(v), cap, _ptr(fs), _ptr(fe), cap, ctypes.byref(nf), _ptr(ts), cap,
                                              ctypes.byref(nt), ctypes.byref(ms))
        self._check(rc, "pbs_sync_index_image")
        self.plan_ms = float(ms.value)
        if chk.value != VERIFY_INDEX_OK:
            return int(chk.value), v[:0], fs[:0], fe[:0], ts[:0]
        self.index_digests, self.index_sizes = _index_entries(image, n.value)
        return 0, v[:n.value], fs[:nf.value], fe[:nf.value], ts[:nt.value]

    def submit(self, blobs, blob_offsets, load_failed=None):
        """pbs_sync_submit of the next k fetch items.  ``blobs``: for a device handle the device
        address of the raw blob images, for the mirror bytes or an array; ``blob_offsets``: k + 1
        offsets into it; ``load_failed``: None or k flags.  Returns (kinds (k), status (k))."""
        off = np.ascontiguousarray(np.asarray(blob_offsets, dtype=np.uint64).reshape(-1))
        k = max(0, off.size - 1)
        lf = None
        if load_failed is not None:
            lf = np.ascontiguousarray(np.asarray(load_failed, dtype=np.uint8).reshape(-1))
            if lf.size != k:
                raise ValueError(f"{k} blobs, {lf.size} load_failed flags")
        if self.device:
            ptr = ctypes.c_void_p(int(blobs) or None)
        else:
            keep = _as_u8(blobs)
            ptr = _ptr(keep)
        kinds, status = np.zeros(k, dtype=np.uint8), np.zeros(k, dtype=np.uint8)
        t = VerifyTiming()
        rc = self._fn("pbs_sync_submit")(self._h, ptr, off.ctypes.data if off.size else None,
                                         None if lf is None else _ptr(lf), k, _ptr(kinds), _ptr(status), ctypes.byref(t))
        self._check(rc, "pbs_sync_submit")
        self.timing = t.as_dict()
        return kinds, status

    def finish(self) -> dict:
        """pbs_sync_finish: the result dict (pbs_sync_result; first_failed SYNC_NONE when no item failed)."""
        res = SyncResult()
        self._check(self._fn("pbs_sync_finish")(self._h, ctypes.byref(res)), "pbs_sync_finish")
        return res.as_dict()

    def abort_index(self) -> None:
        """pbs_sync_abort_index: drop the rest of the plan; claims and appended entries stay."""
        self._check(self._fn("pbs_sync_abort_index")(self._h), "pbs_sync_abort_index")

    def pull_index(self, image, info, remote, budget: int = 0):
        """One index from a source store that is resident (a local-to-local sync): ``remote`` is
        (digests (M, 32), blobs, offsets (M + 1)), the source's chunk files back to back -- for a
        device handle a device address, for the mirror bytes or an array.  ``plan_index``, then
        the fetch digests are looked up in the remote listing (``digest_lookup_device`` /
        ``digest_lookup_host``; a digest the source lacks is a load failure), packed in batches
        (``copy_segments_device``) whose blobs plus unencrypted output slots stay at or below
        ``budget`` bytes (0: no bound; one blob always goes) and submitted until the plan is
        drained, then ``finish``.  Returns (index_check, result dict or None, dict(verdict,
        fetch_store, fetch_entry, touch_store, kinds, status))."""
        chk, verdict, fs, fe, ts = self.plan_index(image, info)
        out = dict(verdict=verdict, fetch_store=fs, fetch_entry=fe, touch_store=ts, kinds=np.zeros(0, np.uint8),
                   status=np.zeros(0, np.uint8))
        if chk != VERIFY_INDEX_OK:
            return chk, None, out
        try:
            out["kinds"], out["status"] = self._pull_fetch_list(fe, remote, int(budget))
        except Exception:
            self.abort_index()
            raise
        return 0, self.finish(), out

    def _pull_fetch_list(self, fe, remote, budget):
        rdig, rblobs, roff = _digest_rows(remote[0]), remote[1], np.asarray(remote[2], dtype=np.uint64).reshape(-1)
        M, k = int(rdig.shape[0]), int(fe.size)
        if roff.size != M + 1:
            raise ValueError(f"the remote listing has {M} entries: {roff.size} offsets")
        if k == 0:
            return np.zeros(0, np.uint8), np.zeros(0, np.uint8)
        want = np.ascontiguousarray(self.index_digests[fe])
        sizes = self.index_sizes[fe]
        torch = None
        if self.device:
            import torch

            t_want, t_rem = torch.from_numpy(want).cuda(), torch.from_numpy(np.ascontiguousarray(rdig)).cuda()
            t_pos, t_first = (torch.empty(k, dtype=torch.int32, device="cuda") for _ in range(2))
            torch.cuda.synchronize()
            digest_lookup_device(t_want.data_ptr(), k, t_rem.data_ptr() if M else 0, M, t_pos.data_ptr(),
                                 t_first.data_ptr(), self.hip_stream)
            pos = t_pos.cpu().numpy().view(np.uint32)
        else:
            rblobs = _as_u8(rblobs)
            pos = digest_lookup_host(want, rdig)[0]
        lf = (pos == LOOKUP_MISSING).astype(np.uint8)
        at = np.where(lf, 0, pos).astype(np.int64)
        src = np.where(lf, 0, roff[at] if M else 0).astype(np.uint64)
        lens = np.where(lf, 0, (roff[at + 1] - roff[at]) if M else 0).astype(np.uint64)
        # the magic read of every blob: an encrypted one takes no output slot in its batch
        hl = np.minimum(lens, 8)
        ho = np.arange(k, dtype=np.uint64) * np.uint64(8)
        if self.device:
            t_heads = torch.zeros(8 * k, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            copy_segments_device(int(rblobs), t_heads.data_ptr(), src, ho, hl, self.hip_stream)
            heads = t_heads.cpu().numpy()
        else:
            heads = np.zeros(8 * k, dtype=np.uint8)
            for t in range(k):
                heads[8 * t:8 * t + int(hl[t])] = rblobs[int(src[t]):int(src[t]) + int(hl[t])]
        enc = np.array([lens[t] >= 12 and heads[8 * t:8 * t + 8].tobytes() in _ENC_MAGICS for t in range(k)])
        need = lens + np.where(enc, 0, sizes).astype(np.uint64)
        kinds, status = [], []
        t0 = 0
        while t0 < k:
            t1, used = t0, 0
            while t1 < k:  # (the rule of verify::batch_end)
                nd = int(need[t1])
                if budget and t1 > t0 and used + nd > budget:
                    break
                used += nd
                t1 += 1
            blens = lens[t0:t1]
            offs = np.concatenate([[0], np.cumsum(blens)]).astype(np.uint64)
            total = int(offs[-1])
            if self.device:
                pack = torch.empty(max(total, 1), dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                if total:
                    copy_segments_device(int(rblobs), pack.data_ptr(), src[t0:t1], offs[:-1], blens, self.hip_stream)
                kd, st = self.submit(pack.data_ptr(), offs, lf[t0:t1])
            else:
                parts = [rblobs[int(src[t]):int(src[t]) + int(lens[t])] for t in range(t0, t1)]
                kd, st = self.submit(np.concatenate(parts + [np.zeros(1, np.uint8)]), offs, lf[t0:t1])
            kinds.append(kd)
            status.append(st)
            t0 = t1
        return np.concatenate(kinds), np.concatenate(status)


def _write_atomic(path: str, data: bytes) -> None:
    os.makedirs(os.path.dirname(path), exist_ok=True)
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        f.write(data)
    os.rename(tmp, path)


def pull_snapshot(remote_base, remote_snapshot_dir, local_base, local_snapshot_dir, worker: SyncWorker,
                  batch_bytes: int = 256 << 20):
    """``pull_snapshot`` / ``pull_single_archive`` (src/server/pull.rs:724-940) between two
    datastore directories, with ``worker`` (over ``list_chunk_store(local_base)``) carrying the
    store and ``downloaded_chunks`` from snapshot to snapshot.  The source's manifest goes to
    ``index.json.tmp``; a local manifest with the same raw bytes means "no data changes".  Per
    file of the manifest: a local file that already matches the manifest is skipped; otherwise the
    source's file is copied to ``<stem>.tmp``, a .blob checked by the SHA-256 and size of its raw
    bytes, an index by ``plan_index`` (size and checksum), its fetch list read from
    ``remote_base/.chunks`` in batches of about ``batch_bytes`` (a file that cannot be read is a
    load failure), submitted, and the chunks that verified written under ``local_base/.chunks``;
    the chunks on the touch list get a new atime; the ``.tmp`` is renamed into place.  The walk
    stops at the first file that fails (its ``.tmp`` stays behind, as the reference's does), and
    the manifest is renamed into place only after the last file.  Returns ("ok" | "failed",
    [(filename, None | error text, result dict | None)]).  Not done here: the client log,
    cleanup_unreferenced_files, locks, owners, groups and namespaces, remove_vanished."""
    def tmp_of(path):  # PathBuf::set_extension("tmp")
        return os.path.splitext(path)[0] + ".tmp"

    os.makedirs(local_snapshot_dir, exist_ok=True)
    manifest_name = os.path.join(local_snapshot_dir, "index.json.blob")
    try:
        with open(os.path.join(remote_snapshot_dir, "index.json.blob"), "rb") as f:
            raw_manifest = f.read()
        with open(tmp_of(manifest_name), "wb") as f:
            f.write(raw_manifest)
        if os.path.exists(manifest_name):
            with open(manifest_name, "rb") as f:
                if f.read() == raw_manifest:  # "no data changes"
                    os.unlink(tmp_of(manifest_name))
                    return "ok", []
        manifest = _manifest_of(remote_snapshot_dir)
    except (OSError, ValueError, ChunkerError):
        return "failed", []
    results = []
    for info in manifest["files"]:
        name = str(info.get("filename", ""))
        res, err = None, None
        try:
            size, csum = int(info["size"]), bytes.fromhex(info["csum"])
            path = os.path.join(local_snapshot_dir, name)
            kind = "blob" if name.endswith(".blob") else "fidx" if name.endswith(".fidx") else \
                "didx" if name.endswith(".didx") else None
            if kind is None:
                raise ValueError(f"unable to parse archive type of {name!r}")
            if os.path.exists(path):  # (:876-909)
                if kind == "blob":
                    with open(path, "rb") as f:
                        raw = f.read()
                    have = (sha256(raw), len(raw))
                else:
                    have = (FixedIndexReader if kind == "fidx" else DynamicIndexReader)(path).compute_csum()
                if have == (csum, size):
                    results.append((name, None, None))
                    continue
            with open(os.path.join(remote_snapshot_dir, name), "rb") as f:
                raw = f.read()
            tmp = tmp_of(path)
            with open(tmp, "wb") as f:
                f.write(raw)
            if kind == "blob":
                if len(raw) != size:
                    err = f"wrong size for file '{name}' ({size} != {len(raw)})"
                elif sha256(raw) != csum:
                    err = f"wrong checksum for file '{name}'"
            else:
                err, res = _pull_index_files(worker, raw, name, size, csum, remote_base, local_base, batch_bytes)
            if err is None:
                os.rename(tmp, path)
        except (OSError, ValueError, KeyError, ChunkerError) as e:
            try:
                worker.abort_index()
            except ChunkerError:
                pass
            err = str(e) or type(e).__name__
        results.append((name, err, res))
        if err is not None:
            return "failed", results
    os.rename(tmp_of(manifest_name), manifest_name)
    return "ok", results


def _pull_index_files(worker, image, name, info_size, info_csum, remote_base, local_base, batch_bytes):
    """verify_archive + pull_index_chunks with the chunk files read from and written to disk:
    (None | error text, result dict | None)."""
    import time

    chk, _, fs, fe, ts = worker.plan_index(image, (info_size, info_csum))
    if chk == VERIFY_INDEX_WRONG_SIZE:
        return f"wrong size for file '{name}'", None
    if chk == VERIFY_INDEX_WRONG_CSUM:
        return f"wrong checksum for file '{name}'", None
    digests = worker.index_digests
    t = 0
    while t < fe.size:
        parts, offs, failed, digs = [], [0], [], []
        while t < fe.size and (not parts or offs[-1] < batch_bytes):
            dg = digests[int(fe[t])].tobytes()
            try:
                with open(chunk_path(remote_base, dg), "rb") as f:
                    data = f.read()
                failed.append(0)
            except OSError:
                data = b""
                failed.append(1)
            parts.append(data)
            digs.append(dg)
            offs.append(offs[-1] + len(data))
            t += 1
        raw = np.frombuffer(b"".join(parts), dtype=np.uint8)
        if worker.device:
            import torch

            dev = torch.from_numpy(raw.copy()).to("cuda") if raw.size else None
            _, status = worker.submit(dev.data_ptr() if dev is not None else 0, offs, failed)
        else:
            _, status = worker.submit(raw, offs, failed)
        for dg, data, st in zip(digs, parts, status):
            if st == BLOB_ST_OK:
                _write_atomic(chunk_path(local_base, dg), data)  # insert_chunk
    if ts.size:
        all_digests, _ = worker.listing()
        for c in ts:
            p = chunk_path(local_base, all_digests[int(c)].tobytes())
            try:
                st = os.lstat(p)
                os.utime(p, ns=(time.time_ns(), st.st_mtime_ns), follow_symlinks=False)
            except FileNotFoundError:
                pass
    res = worker.finish()
    if not res["ok"]:
        return f"sync of {name!r} failed at fetch item {res['first_failed']}", res
    return None, res


# ---- the backup session (include/pbs_backup.h) ----------------------------------------------------

BACKUP_KIND_NOT_FILE = 254
BACKUP_ST_BAD_PARAM, BACKUP_ST_WRONG_LENGTH = 33, 34
(BACKUP_INS_NONE, BACKUP_INS_NEW, BACKUP_INS_DUP_SAME, BACKUP_INS_OVERWRITE_EMPTY, BACKUP_INS_DUP_KEEP_FIRST,
 BACKUP_INS_DUP_KEEP_SMALLER, BACKUP_INS_REPLACE_BIGGER) = range(7)
BACKUP_INS_ERR_TYPE, BACKUP_INS_ERR_READ, BACKUP_INS_ERR_UNENC_TO_ENC, BACKUP_INS_ERR_ENC_UNCOMPRESSED = 16, 17, 18, 19
BACKUP_ACT_NONE, BACKUP_ACT_WRITE, BACKUP_ACT_TOUCH = 0, 1, 2
BACKUP_REG_NONE, BACKUP_REG_OK, BACKUP_REG_ERR_LARGE, BACKUP_REG_ERR_MULTI_SMALL = 0, 1, 2, 3
(BACKUP_E_FINISHED, BACKUP_E_NO_WRITER, BACKUP_E_NO_SUCH_CHUNK, BACKUP_E_STRANGE_OFFSET, BACKUP_E_INDEX_RANGE,
 BACKUP_E_CHUNK_COUNT, BACKUP_E_SIZE, BACKUP_E_EXPECTED_COUNT, BACKUP_E_CSUM, BACKUP_E_OPEN_WRITER, BACKUP_E_NO_FILES,
 BACKUP_E_REUSE_NO_IMAGE, BACKUP_E_REUSE_CSUM, BACKUP_E_REUSE_LENGTH, BACKUP_E_TOO_MANY_WRITERS) = range(64, 79)
BACKUP_NONE = (1 << 64) - 1       # PBS_BACKUP_NONE: first_failed of a batch with no failing item


def backup_release() -> None:
    """pbs_backup_release: free the idle work areas of the backup session's calls."""
    lib().pbs_backup_release()


class BackupSession:
    """One backup session on one datastore (``BackupEnvironment``, src/api2/backup/environment.rs,
    with ``UploadChunk`` and ``ChunkStore::insert_chunk``) over the store's listing: ``listing``
    is (digests (m, 32), file lengths (m), magics (m): BLOB_KIND_*, BLOB_KIND_NONE or
    BACKUP_KIND_NOT_FILE).  A context manager over a pbs_backup handle (``device=True``: the
    table, the digest list and the per-entry state live in the memory of ``hip_stream``'s device)
    or over the host mirror's (``device=False``: no GPU).  A call returns 0 or the positive
    BACKUP_E_* code with which the reference's request fails; a negative code raises
    ChunkerError."""

    def __init__(self, listing, reserve: int = 0, device: bool = True, hip_stream: int = 0):
        digests = _digest_rows(listing[0])
        m = int(digests.shape[0])
        sizes = np.ascontiguousarray(np.asarray(listing[1], dtype=np.uint64).reshape(-1))
        kinds = np.ascontiguousarray(np.asarray(listing[2], dtype=np.uint8).reshape(-1))
        if sizes.size != m or kinds.size != m:
            raise ValueError(f"{m} digests, {sizes.size} sizes, {kinds.size} kinds")
        self.device = bool(device)
        self._sfx = "" if self.device else "_host"
        h, ms = ctypes.c_void_p(None), ctypes.c_double(0)
        args = [_ptr(digests), _ptr(sizes), _ptr(kinds), m, int(reserve), ctypes.byref(h), ctypes.byref(ms)]
        if self.device:
            args.append(ctypes.c_void_p(hip_stream))
        rc = self._fn("pbs_backup_begin")(*args)
        if rc != PBS_OK:
            raise ChunkerError(rc, "pbs_backup_begin" + self._sfx)
        self._h = h
        self.build_ms = float(ms.value)
        self.ms = 0.0           # of the last register_previous / append
        self.timing = None      # of the last upload
        self._entries = {}      # wid -> index entries (what the close's image holds)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def close(self) -> None:
        """pbs_backup_end.  Every later call raises ChunkerError(PBS_ERR_INVALID)."""
        if getattr(self, "_h", None) is not None and not getattr(self, "_closed", False):
            self._closed = True
            self._fn("pbs_backup_end")(self._h)

    def _fn(self, name: str):
        return getattr(lib(), name + self._sfx)

    def _code(self, rc: int, name: str) -> int:
        if rc < 0:
            raise ChunkerError(rc, name + self._sfx)
        return int(rc)

    @property
    def count(self) -> int:
        return int(self._fn("pbs_backup_count")(self._h))

    @property
    def table_log2(self) -> int:
        return int(self._fn("pbs_backup_table_log2")(self._h))

    def listing(self) -> dict:
        """pbs_backup_listing: dict(digests (count, 32), present, size, kind, known, known_size)."""
        n = ctypes.c_size_t(0)
        self._code(self._fn("pbs_backup_listing")(self._h, None, None, None, None, None, None, 0, ctypes.byref(n)),
                   "pbs_backup_listing")
        c = n.value
        out = dict(digests=np.zeros((c, 32), np.uint8), present=np.zeros(c, np.uint8), size=np.zeros(c, np.uint64),
                   kind=np.zeros(c, np.uint8), known=np.zeros(c, np.uint8), known_size=np.zeros(c, np.uint32))
        self._code(self._fn("pbs_backup_listing")(self._h, *[_ptr(a) for a in out.values()], c, ctypes.byref(n)),
                   "pbs_backup_listing")
        return out

    def lookup(self, digest):
        """lookup_chunk: the registered length, or None."""
        d = np.frombuffer(bytes(digest), dtype=np.uint8)
        size = ctypes.c_uint32(0)
        rc = self._code(self._fn("pbs_backup_lookup")(self._h, _ptr(d), ctypes.byref(size)), "pbs_backup_lookup")
        return int(size.value) if rc == 0 else None

    def stats(self) -> dict:
        s = BackupStat()
        self._code(self._fn("pbs_backup_stats")(self._h, ctypes.byref(s)), "pbs_backup_stats")
        return s.as_dict()

    def finish(self) -> int:
        """finish_backup's state checks: 0, BACKUP_E_OPEN_WRITER, BACKUP_E_NO_FILES or BACKUP_E_FINISHED."""
        return self._code(self._fn("pbs_backup_finish")(self._h, None), "pbs_backup_finish")

    def register_previous(self, digests, sizes) -> int:
        """register_chunk for every chunk of the previous backup's index (mod.rs:859-863)."""
        d = _digest_rows(digests)
        s = np.ascontiguousarray(np.asarray(sizes, dtype=np.uint32).reshape(-1))
        if s.size != d.shape[0]:
            raise ValueError(f"{d.shape[0]} digests, {s.size} sizes")
        ms = ctypes.c_double(0)
        rc = self._fn("pbs_backup_register_previous")(self._h, _ptr(d), _ptr(s), s.size, ctypes.byref(ms))
        self.ms = float(ms.value)
        return self._code(rc, "pbs_backup_register_previous")

    def register_index_image(self, image):
        """register_previous from a .didx / .fidx image (bytes or a path): (code, entries).  A bad
        image raises ChunkerError and changes nothing."""
        if isinstance(image, (str, os.PathLike)):
            with open(image, "rb") as f:
                image = f.read()
        image = bytes(image)
        n, ms = ctypes.c_size_t(0), ctypes.c_double(0)
        rc = self._fn("pbs_backup_register_index_image")(self._h, image, len(image), ctypes.byref(n), ctypes.byref(ms))
        self.ms = float(ms.value)
        return self._code(rc, "pbs_backup_register_index_image"), int(n.value)

    def upload(self, wid: int, digests, sizes, blobs, blob_offsets, encoded_sizes=None):
        """pbs_backup_upload of k chunks.  ``blobs``: for a device handle the device address of
        the blob images, for the mirror bytes or an array; ``blob_offsets``: k + 1 offsets into
        it.  Returns (code, dict(status, crc, ins, action, is_duplicate, compressed_size, reg,
        first_failed))."""
        d = _digest_rows(digests)
        s = np.ascontiguousarray(np.asarray(sizes, dtype=np.uint32).reshape(-1))
        off = np.ascontiguousarray(np.asarray(blob_offsets, dtype=np.uint64).reshape(-1))
        k = max(0, off.size - 1)
        if s.size != k or d.shape[0] != k:
            raise ValueError(f"{k} blobs, {d.shape[0]} digests, {s.size} sizes")
        es = None
        if encoded_sizes is not None:
            es = np.ascontiguousarray(np.asarray(encoded_sizes, dtype=np.uint32).reshape(-1))
            if es.size != k:
                raise ValueError(f"{k} blobs, {es.size} encoded sizes")
        if self.device:
            ptr = ctypes.c_void_p(int(blobs) or None)
        else:
            keep = _as_u8(blobs)
            ptr = _ptr(keep)
        out = dict(status=np.zeros(k, np.uint8), crc=np.zeros(k, np.uint32), ins=np.zeros(k, np.uint8),
                   action=np.zeros(k, np.uint8), is_duplicate=np.zeros(k, np.uint8),
                   compressed_size=np.zeros(k, np.uint32), reg=np.zeros(k, np.uint8))
        ff, t = ctypes.c_uint64(BACKUP_NONE), BackupTiming()
        rc = self._fn("pbs_backup_upload")(self._h, int(wid), _ptr(d), _ptr(s), None if es is None else _ptr(es), ptr,
                                           off.ctypes.data if off.size else None, k, *[_ptr(a) for a in out.values()],
                                           ctypes.byref(ff), ctypes.byref(t))
        self.timing = t.as_dict()
        out["first_failed"] = int(ff.value)
        return self._code(rc, "pbs_backup_upload"), out

    def create_dynamic(self, uuid: bytes = bytes(16), ctime: int = 0):
        """(code, wid)."""
        wid = ctypes.c_uint32(0)
        rc = self._fn("pbs_backup_create_dynamic")(self._h, bytes(uuid), int(ctime), ctypes.byref(wid))
        self._entries[int(wid.value)] = 0
        return self._code(rc, "pbs_backup_create_dynamic"), int(wid.value)

    def create_fixed(self, size: int, chunk_size: int, uuid: bytes = bytes(16), ctime: int = 0, reuse_image=None,
                     reuse_csum=None):
        """(code, wid).  ``reuse_csum``: the incremental writer (mod.rs:471-507) over the previous
        index image ``reuse_image``."""
        wid = ctypes.c_uint32(0)
        img = None if reuse_image is None else bytes(reuse_image)
        rc = self._fn("pbs_backup_create_fixed")(self._h, int(size), int(chunk_size), bytes(uuid), int(ctime), img,
                                                 len(img) if img is not None else 0,
                                                 None if reuse_csum is None else bytes(reuse_csum), ctypes.byref(wid))
        self._entries[int(wid.value)] = -fidx_count(size, chunk_size) if chunk_size > 0 else 0  # (fixed: negative)
        return self._code(rc, "pbs_backup_create_fixed"), int(wid.value)

    def _append(self, name: str, wid: int, digests, offsets):
        d = _digest_rows(digests)
        o = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint64).reshape(-1))
        if o.size != d.shape[0]:
            raise ValueError(f"{d.shape[0]} digests, {o.size} offsets")
        done, err, ms = ctypes.c_size_t(0), ctypes.c_int(0), ctypes.c_double(0)
        rc = self._fn(name)(self._h, int(wid), _ptr(d), _ptr(o), o.size, ctypes.byref(done), ctypes.byref(err),
                            ctypes.byref(ms))
        self.ms = float(ms.value)
        if self._entries.get(int(wid), -1) >= 0 and name == "pbs_backup_dynamic_append":
            self._entries[int(wid)] += int(done.value)
        return self._code(rc, name), int(done.value), int(err.value)

    def dynamic_append(self, wid: int, digests, offsets):
        """(code, n_done, err)."""
        return self._append("pbs_backup_dynamic_append", wid, digests, offsets)

    def fixed_append(self, wid: int, digests, offsets):
        """(code, n_done, err)."""
        return self._append("pbs_backup_fixed_append", wid, digests, offsets)

    def _close_writer(self, name: str, wid: int, chunk_count: int, size: int, csum: bytes, image_bytes: int):
        img = np.zeros(image_bytes, dtype=np.uint8)
        res, st = ctypes.c_int(0), BackupWriterStat()
        rc = self._fn(name)(self._h, int(wid), int(chunk_count), int(size), bytes(csum), _ptr(img), img.size,
                            ctypes.byref(res), ctypes.byref(st))
        rc = self._code(rc, name)
        if rc == 0 and res.value != BACKUP_E_NO_WRITER:
            self._entries.pop(int(wid), None)  # (the writer is gone, whatever the checks said)
        ok = rc == 0 and res.value == 0
        return rc, int(res.value), (img.tobytes() if ok else None), (st.as_dict() if ok else None)

    def dynamic_close(self, wid: int, chunk_count: int, size: int, csum: bytes):
        """(code, result, .didx image or None, stat dict or None)."""
        return self._close_writer("pbs_backup_dynamic_close", wid, chunk_count, size, csum,
                                  int(lib().pbs_didx_size(max(self._entries.get(int(wid), 0), 0))))

    def fixed_close(self, wid: int, chunk_count: int, size: int, csum: bytes):
        """(code, result, .fidx image or None, stat dict or None)."""
        return self._close_writer("pbs_backup_fixed_close", wid, chunk_count, size, csum,
                                  int(lib().pbs_fidx_size(max(-self._entries.get(int(wid), 0), 0))))

    def add_blob(self, raw):
        """(code, BLOB_ST_* of from_raw + verify_crc)."""
        a = _as_u8(raw)
        st = ctypes.c_uint8(0)
        rc = self._fn("pbs_backup_add_blob")(self._h, _ptr(a), a.size, ctypes.byref(st))
        return self._code(rc, "pbs_backup_add_blob"), int(st.value)


def backup_snapshot(session: "BackupSession", up: dict, upload=None, previous=None, manifest_blob=None) -> dict:
    """What ``upload_stream_host`` produced (``up``) through one session, as the client's requests
    arrive: the previous index's chunks are registered (``previous``: (digests, sizes) or None),
    a dynamic writer is created, the new chunks' blobs are uploaded in one batch (``upload``: for
    a device session a function from the blob bytes (uint8 array) to (device address, keep-alive);
    None for the mirror), every chunk is appended, the writer is closed with the client's checksum
    and, with ``manifest_blob``, the manifest is added and the session finished.  Returns
    dict(upload, append, close, image, stat, finish, written): ``written`` maps each digest whose
    action is WRITE to the blob the store must hold (the CRC the session computed in bytes 8..12).
    Stops at the first failing request; the keys after it are None."""
    out = dict.fromkeys(("upload", "append", "close", "image", "stat", "finish"))
    out["written"] = {}
    if previous is not None and session.register_previous(*previous):
        return out
    rc, wid = session.create_dynamic()
    if rc:
        return out
    ends, digests, off = up["ends"], up["digests"], up["blob_offsets"]
    starts = np.concatenate([[0], ends[:-1]]).astype(np.uint64) if ends.size else np.zeros(0, np.uint64)
    new = np.flatnonzero(up["known"] == 0)
    blobs = _as_u8(up["blobs"])
    boff = np.concatenate([[0], np.cumsum((off[1:] - off[:-1])[new])]).astype(np.uint64)
    # (known chunks have empty blobs, so the new chunks' blobs already follow one another)
    sizes = (ends - starts)[new].astype(np.uint32)
    ptr, keep = upload(blobs) if session.device else (blobs, None)
    rc, res = session.upload(wid, digests[new], sizes, ptr, boff + (off[new[0]] if new.size else 0))
    del keep
    out["upload"] = res
    if rc or res["first_failed"] != BACKUP_NONE:
        return out
    for j, t in enumerate(new):
        if res["action"][j] == BACKUP_ACT_WRITE:
            b = bytearray(blobs[int(off[t]):int(off[t + 1])].tobytes())
            b[8:12] = int(res["crc"][j]).to_bytes(4, "little")
            out["written"][digests[t].tobytes()] = bytes(b)
    out["append"] = session.dynamic_append(wid, digests, starts)
    if out["append"] != (0, ends.size, 0):
        return out
    rc, result, image, stat = session.dynamic_close(wid, ends.size, int(ends[-1]) if ends.size else 0, up["csum"])
    out["close"], out["image"], out["stat"] = (rc, result), image, stat
    if rc or result or manifest_blob is None:
        return out
    if session.add_blob(manifest_blob) != (0, BLOB_ST_OK):
        return out
    out["finish"] = session.finish()
    return out
