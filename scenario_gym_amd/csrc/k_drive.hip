// k_drive.hip -- drive_kernel: the VehicleController step of the drivers of sg_set_drivers (sgym_drive.hpp).
#include "sgym_launch.hpp"
#include "sgym_drive.hpp"

namespace sgl {
void drive(hipStream_t s, const sg::Params &p, double timestep, const int32_t *scen, const int32_t *slot, int64_t n, const double *actions,
           double *ext)
{
    if (n <= 0) return;
    sg::drive_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s>>>(p.stat, p.dyn, p.sdyn, p.EP, p.FROWS, timestep, scen, slot, n,
                                                                             actions, ext);
}
} // namespace sgl
