// sgym_snapshot.hpp -- snapshot_copy_kernel: the rows of the masked scenarios of every state array of a handle, copied into a
// snapshot (sg_snapshot_save) or back (sg_snapshot_restore) by one launch.
//
// The host (h_snapshot.hip) describes every state array once per snapshot as a segment: where it lies on the handle and in the
// snapshot, how its bytes map to scenarios (the kind), and how many 16-byte chunks it has.  The table travels by value.  Every
// workgroup walks the segments one after the other (a uniform loop: the segment's fields are scalar loads of the kernel arguments)
// and inside a segment the grid strides over the chunks, consecutive lanes on consecutive chunks.  A chunk is 16 bytes at a 16-byte
// boundary -- the two copies of an array have the same address modulo 16 -- and its two 8-byte halves are looked at one by one: the
// scenario that owns the half is masked or not.  Both masked: one 16-byte load and store.  One masked: an 8-byte load and store.
// Units narrower than 8 bytes (an int32 per scenario, a byte per driver) never get a narrow access: the half is read on both sides,
// the masked units' bytes are taken from the source, and the 8 bytes are stored whole; no other segment shares such a word (the host
// pads them apart), and no other kernel runs beside this one on the handle's stream, so the bytes written back unchanged are nobody's.
// In block columns (the 64-slot state blocks) two even-aligned adjacent slots belong to one scenario (EP >= 4 and even), so a masked
// scenario's part of a 512-byte row is always whole 16-byte chunks.
// Global loads and stores only (address space 1), no LDS, no atomic, no barrier.  Included through sgym_launch.hpp; the kernel is
// emitted by k_snap.hip alone (SG_UNIT_SNAP), the host units see the table.
#pragma once
#include "sgym_device.hpp"

namespace sg {

// how the bytes of a segment map to scenarios
enum {
    SNAP_SCENARIO = 0, // per-scenario contiguous unit: unit u of a plane belongs to scenario u
    SNAP_ENTITY = 1,   // per-entity contiguous unit: unit u belongs to scenario u / EP
    SNAP_LIST = 2,     // per-list-entry contiguous unit (the drivers): unit u belongs to scenario scen_of[u]
    SNAP_BLOCK = 3     // block columns: [blocks][rows][64] eight-byte lanes, lane l of block b belongs to scenario (b * 64 + l) / EP
};

struct SnapSeg {
    char *live, *snap;       // plane 0 of the array on the handle / in the snapshot (equal modulo 16)
    const int32_t *scen_of;  // SNAP_LIST: [units] the scenario of every unit
    uint64_t plane_bytes;    // bytes of one plane that units cover
    uint64_t plane_stride;   // bytes from one plane to the next (the same on both sides)
    uint64_t chunks;         // 16-byte chunks per plane, an aligned one at either end included
    uint32_t planes;         // planes of the array (the pose record: one per row and coordinate)
    uint32_t unit;           // bytes of a unit: a multiple of 8, or 1, 2 or 4 (SNAP_BLOCK: 8)
    uint32_t kind;
    uint32_t rows;           // SNAP_BLOCK: rows per block
};

constexpr int SNAP_MAX_SEGS = 24;
struct SnapTable {
    SnapSeg seg[SNAP_MAX_SEGS];
    int32_t n, R, EP;
};

#ifdef SG_UNIT_SNAP // (emitted by the one object that launches it: csrc/Makefile, sgym_launch.hpp)
typedef unsigned long long snap_u64x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ bool snap_masked(const SG_GLOBAL uint8_t *mask, uint32_t scen, uint32_t R)
{
    return scen < R && (mask == nullptr || mask[scen] != 0);
}

// the bytes of the 8-byte half at offset o of a plane (0 <= o < plane_bytes) that belong to masked scenarios, as a byte-select word
// (0: none, ~0: all).  I: the type the offsets are divided in -- uint32_t for planes below 2 GiB, where a division costs a fifth
template <typename I>
__device__ __forceinline__ uint64_t snap_select_in(const SnapSeg &s, I o, const SG_GLOBAL uint8_t *mask, uint32_t R, uint32_t EP)
{
    if (s.kind == SNAP_BLOCK) {
        const I blk = o / (I)(s.rows * ROW);
        const uint32_t lane = ((uint32_t)o & (ROW - 1)) >> 3;
        return snap_masked(mask, (uint32_t)(blk * 64 + lane) / EP, R) ? ~0ull : 0ull;
    }
    const SG_GLOBAL int32_t *scen_of = (const SG_GLOBAL int32_t *)s.scen_of;
    const auto owner = [&](I u) -> uint32_t {
        return s.kind == SNAP_SCENARIO ? (uint32_t)u : (s.kind == SNAP_ENTITY ? (uint32_t)u / EP : (uint32_t)scen_of[u]);
    };
    if (s.unit >= 8) return snap_masked(mask, owner(o / (I)s.unit), R) ? ~0ull : 0ull;
    uint64_t sel = 0;
    const uint64_t ones = (1ull << (8 * s.unit)) - 1; // (unit 1, 2 or 4)
    for (uint32_t j = 0; j < 8; j += s.unit)
        if ((uint64_t)o + j < s.plane_bytes && snap_masked(mask, owner((o + (I)j) / (I)s.unit), R)) sel |= ones << (8 * j);
    return sel;
}

__device__ __forceinline__ uint64_t snap_select(const SnapSeg &s, int64_t o, const SG_GLOBAL uint8_t *mask, uint32_t R, uint32_t EP)
{
    if (o < 0 || (uint64_t)o >= s.plane_bytes) return 0;
    return s.plane_bytes <= 0x7fffffffull ? snap_select_in<uint32_t>(s, (uint32_t)o, mask, R, EP) : snap_select_in<uint64_t>(s, (uint64_t)o, mask, R, EP);
}

// restore == 0: handle -> snapshot; else snapshot -> handle.  mask: DEVICE [R] or nullptr (every scenario).
static __global__ __launch_bounds__(256) void snapshot_copy_kernel(const SnapTable t, const uint8_t *mask_, int restore)
{
    const SG_GLOBAL uint8_t *mask = (const SG_GLOBAL uint8_t *)mask_;
    const uint64_t tid = (uint64_t)blockIdx.x * 256 + threadIdx.x, stride = (uint64_t)gridDim.x * 256;
    const uint32_t R = (uint32_t)t.R, EP = (uint32_t)t.EP;
    for (int si = 0; si < t.n; ++si) {
        const SnapSeg &s = t.seg[si];
        const uint64_t n = s.chunks * s.planes;
        for (uint64_t g = tid; g < n; g += stride) {
            uint64_t plane = 0, c = g;
            if (s.planes > 1) { plane = g / s.chunks; c = g - plane * s.chunks; }
            const uint64_t pbase = plane * s.plane_stride;
            const uint32_t mis = (uint32_t)((uintptr_t)(s.live + pbase) & 15);
            const int64_t off = (int64_t)(c * 16) - (int64_t)mis; // of the chunk in its plane: the first chunk may begin before the plane
            const uint64_t m0 = snap_select(s, off, mask, R, EP), m1 = snap_select(s, off + 8, mask, R, EP);
            if ((m0 | m1) == 0) continue;
            const SG_GLOBAL char *src = (const SG_GLOBAL char *)((restore ? s.snap : s.live) + (int64_t)pbase + off);
            SG_GLOBAL char *dst = (SG_GLOBAL char *)((restore ? s.live : s.snap) + (int64_t)pbase + off);
            if ((m0 & m1) == ~0ull) {
                *(SG_GLOBAL snap_u64x2 *)dst = *(const SG_GLOBAL snap_u64x2 *)src;
                continue;
            }
            for (int half = 0; half < 2; ++half) {
                const uint64_t m = half ? m1 : m0;
                if (m == 0) continue;
                uint64_t v = *(const SG_GLOBAL uint64_t *)(src + 8 * half);
                if (m != ~0ull) v = (v & m) | (*(const SG_GLOBAL uint64_t *)(dst + 8 * half) & ~m);
                *(SG_GLOBAL uint64_t *)(dst + 8 * half) = v;
            }
        }
    }
}
#endif // SG_UNIT_SNAP

} // namespace sg
