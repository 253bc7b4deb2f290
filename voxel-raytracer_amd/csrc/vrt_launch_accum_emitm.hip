// vrt_launch_accum_emitm.hip -- the accumulation's VRT_MODE_FULL kernels over EmitMisPaths<...> (include/vrt.h vrt_set_emitter_mis),
// plain forms, in an object of their own: vrt_launch_accum.hip.h
#include "vrt_launch_accum.hip.h"

template struct vrt::launch::AccumPaths<false, vrt::launch::PathFamily::kEmitMis>;
