// vrt_launch_rays_emitm.hip -- the ray batches' VRT_MODE_FULL kernel over EmitMisPaths<...> (include/vrt.h vrt_set_emitter_mis),
// plain forms, in an object of its own: vrt_launch_rays_paths.hip.h
#include "vrt_launch_rays_paths.hip.h"

template struct vrt::launch::RayPaths<false, vrt::launch::PathFamily::kEmitMis>;
