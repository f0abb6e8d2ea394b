// k_snap.hip -- snapshot_copy_kernel: the masked scenarios' rows of every state array, handle -> snapshot or back, as one launch
// (sgym_snapshot.hpp; sg_snapshot_save / sg_snapshot_restore, h_snapshot.hip).
#define SG_UNIT_SNAP
#include <algorithm>
#include "sgym_launch.hpp"

namespace sgl {
void snapshot_copy(hipStream_t s, const sg::SnapTable &t, const uint8_t *mask, int restore)
{
    uint64_t most = 0, total = 0; // chunks of the largest segment, of all of them
    for (int i = 0; i < t.n; ++i) {
        const uint64_t n = t.seg[i].chunks * t.seg[i].planes;
        most = std::max(most, n);
        total += n;
    }
    if (total == 0) return;
    // enough workgroups to fill the device a few times over (256 compute units x 8), never more than the largest segment has work for
    const unsigned grid = (unsigned)std::min<uint64_t>(2048, (most + 255) / 256);
    sg::snapshot_copy_kernel<<<dim3(grid), dim3(256), 0, s>>>(t, mask, restore);
}
} // namespace sgl
