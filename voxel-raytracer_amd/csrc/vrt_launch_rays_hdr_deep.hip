// vrt_launch_rays_hdr_deep.hip -- the ray batches' VRT_MODE_FULL kernel over DeepPaths<...> (include/vrt.h vrt_set_path_depth),
// HDR forms, in an object of its own: vrt_launch_rays_paths.hip.h
#include "vrt_launch_rays_paths.hip.h"

template struct vrt::launch::RayPaths<true, vrt::launch::PathFamily::kDeep>;
