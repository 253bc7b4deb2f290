// vrt_launch_accum_deep.hip -- the accumulation's VRT_MODE_FULL kernels over DeepPaths<...> (include/vrt.h vrt_set_path_depth),
// plain forms, in an object of their own: vrt_launch_accum.hip.h
#include "vrt_launch_accum.hip.h"

template struct vrt::launch::AccumPaths<false, vrt::launch::PathFamily::kDeep>;
