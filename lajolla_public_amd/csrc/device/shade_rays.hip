// k_shade for a pass over a table of rays or probes (lj_radiance_rays / lj_irradiance, dprobe.h): the RAYS instantiations
// of the shade kernel of kernels.hip — one per feature set and staging, as for a camera pass — and their launcher, launch_shade_rays.
// A translation unit of its own, so that they compile beside kernels.hip, the longest job of a product build, and not after it: of
// kernels.hip this unit keeps the templates and nothing else.
#define LJ_SHADE_RAYS_UNIT 1
#include "kernels.hip"
