// vrt_launch_accum_sun.hip -- the accumulation's VRT_MODE_FULL kernels over SunPaths<...> (include/vrt.h vrt_set_sun_disc),
// plain forms, in an object of their own: vrt_launch_accum.hip.h
#include "vrt_launch_accum.hip.h"

template struct vrt::launch::AccumPaths<false, vrt::launch::PathFamily::kSun>;
