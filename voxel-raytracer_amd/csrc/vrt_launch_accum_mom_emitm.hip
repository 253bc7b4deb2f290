// vrt_launch_accum_mom_emitm.hip -- the accumulation's VRT_MODE_FULL kernels over EmitMisPaths<...> (include/vrt.h vrt_set_emitter_mis),
// the forms that keep moments (vrt_accum_keep_moments), in an object of their own: vrt_launch_accum.hip.h
#include "vrt_launch_accum.hip.h"

template struct vrt::launch::AccumPaths<true, vrt::launch::PathFamily::kEmitMis, true>;
