// vrt_launch_rays_hdr_sun.hip -- the ray batches' VRT_MODE_FULL kernel over SunPaths<...> (include/vrt.h vrt_set_sun_disc),
// HDR forms, in an object of its own: vrt_launch_rays_paths.hip.h
#include "vrt_launch_rays_paths.hip.h"

template struct vrt::launch::RayPaths<true, vrt::launch::PathFamily::kSun>;
