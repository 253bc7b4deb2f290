// vrt_launch_accum_emit.hip -- the accumulation's VRT_MODE_FULL kernels over EmitPaths<...> (include/vrt.h vrt_set_emitter_sampling),
// plain forms, in an object of their own: vrt_launch_accum.hip.h
#include "vrt_launch_accum.hip.h"

template struct vrt::launch::AccumPaths<false, vrt::launch::PathFamily::kEmit>;
