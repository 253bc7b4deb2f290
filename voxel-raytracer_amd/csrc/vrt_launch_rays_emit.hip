// vrt_launch_rays_emit.hip -- the ray batches' VRT_MODE_FULL kernel over EmitPaths<...> (include/vrt.h vrt_set_emitter_sampling),
// plain forms, in an object of its own: vrt_launch_rays_paths.hip.h
#include "vrt_launch_rays_paths.hip.h"

template struct vrt::launch::RayPaths<false, vrt::launch::PathFamily::kEmit>;
