// The piecewise copy of the read path: unaligned 16-byte loads from global memory, the work
// item of segment_copy_kernel (pbs_restore.hip, the one translation unit that compiles it) and
// the two host calls that build and launch item lists.  Used by pbs_blob_decode_device,
// pbs_blob_decode_inflate_device, pbs_copy_segments_device and pbs_restore_range_device; the
// dirty map (pbs_fixed.hip) and the GCM kernels (gcm_dev.h) take the load helpers only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

namespace pbs {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
// Addresses travel as integers; pointers made from them are marked as global memory so that
// the loads and stores are global_*, not flat_*, instructions.
#define PBS_GLOBAL __attribute__((address_space(1)))
typedef PBS_GLOBAL uint8_t* gbytes;
typedef const PBS_GLOBAL uint8_t* gcbytes;
// 16 bytes from any address: one global load of four dwords at alignment 1 (gfx950 reads
// global memory at any alignment; DESIGN.md section 10 on why not two aligned loads)
struct __attribute__((packed, aligned(1))) U16Unaligned {
    u32x4 v;
};
__device__ __forceinline__ u32x4 load16(gcbytes p) { return reinterpret_cast<const PBS_GLOBAL U16Unaligned*>(p)->v; }

constexpr uint32_t kPiece = 65536;  // bytes one workgroup moves per item
constexpr int kCopyThreads = 256;

// One work item of segment_copy_kernel (its contract: pbs_restore.hip)
struct CopyItem {
    uint64_t src, dst, len;
};

class DevArena;
// Appends the items of one segment of `len` bytes (none when len == 0); src == 0: zeros.  The
// first item ends on the destination's first 16-byte boundary + 64 KiB, so every later piece
// starts on a boundary and has no head bytes.
void add_items(std::vector<CopyItem>& items, uint64_t src, uint64_t dst, uint64_t len);
// Launches the items on `st` from slot `slot` of `ar` (nothing when there are none).  The
// caller synchronises `st` before `items` or the arena go away.
int copy_items_async(const std::vector<CopyItem>& items, DevArena& ar, unsigned slot, int ncu, hipStream_t st);

}  // namespace pbs
