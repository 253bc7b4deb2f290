"""The camera paths of the temporal-pass tests (test_temporal.py, test_gpu_temporal.py) -- TEST INFRASTRUCTURE ONLY: the frames of
tests/guide_worlds.py as the first pose of each world, then a yaw of a few degrees, then a translation of a fraction of a voxel; and
the previous camera a pass is handed: prev_view_proj is the float64 inverse of inv_projection times the float64 inverse of inv_view,
rounded once to float32."""
import numpy as np

import guide_worlds as GW
import oracle_temporal as T

YAW, STEP = 3.0, (0.3, 0.1, -0.2)      # degrees; voxels


def poses(name):
    """-> three poses (x, y, z, yaw, pitch): guide_worlds' own, yawed, then moved as well"""
    p = GW.FRAMES[name][0]
    yawed = (p[0], p[1], p[2], p[3] + YAW, p[4])
    moved = (p[0] + STEP[0], p[1] + STEP[1], p[2] + STEP[2], p[3] + YAW, p[4])
    return [p, yawed, moved]


def camera(V, pose, size=(GW.W, GW.H)):
    """-> (inv_projection, inv_view, camera_pos) as Context.set_camera takes them"""
    return V.camera_block(pose[:3], pose[3], pose[4], size[0], size[1])[:3]


def prev_camera(cam):
    """what a pass whose history was written under `cam` is handed: (prev_view_proj[16], prev_camera_pos[4])"""
    return T.view_proj(cam[0], cam[1]), np.ascontiguousarray(cam[2], np.float32)


def temporal_of(cam_prev=None, **kw):
    """an oracle_temporal.Temporal with the previous camera of cam_prev (None: the first frame) and make()'s keywords"""
    if cam_prev is None:
        return T.make(**kw)
    vp, cp = prev_camera(cam_prev)
    return T.make(vp, cp, **kw)
