// k_geom.hip -- road_info_kernel: which road geometries contain each entity / each point (sgym_geom.hpp).
#define SG_UNIT_GEOM
#include "sgym_launch.hpp"

namespace sgl {
void road_info(hipStream_t s, const sg::Params &p, const sg::RoadIndex &R, const sg::RoadGeom &G, bool has_road, const int32_t *scen,
               const double *xy, int64_t n, int cap, int32_t *count, int32_t *geoms, uint32_t *layers)
{
    if (n <= 0) return;
    sg::road_info_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s>>>(p.dyn, p.E, p.EP, p.FROWS, R, G, has_road ? 1 : 0, scen, xy, n, cap,
                                                                                 count, geoms, layers);
}
} // namespace sgl
