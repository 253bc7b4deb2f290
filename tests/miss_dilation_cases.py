"""Worlds, views and ray geometry shared by tests/test_miss_dilation.py (host mask against the oracle) and
tests/test_gpu_miss_dilation.py (the device with the mask on against off): cases in which the miss mask's dilation of the occupancy
boxes (vrt_miss.h kDilate, 0.25 voxel: the proof's bound, DESIGN 3 "Miss tiles") decides whether a tile is cleared -- a few stopping
voxels seen by rays that pass 0.25 to 1 voxel beside them, and rays that reach a voxel after several hundred march steps."""
import numpy as np

STOP = (0xa0a0a0ff, 3.0, 0.0, 0.0)   # opaque: refraction byte 255, a cell that stops a ray
AIR = (0x80ff80c0, 1.0, 0.0, 0.0)    # refraction 1.0 = byte 85: the medium of empty space, a unit cell no ray stops in

FEW = {  # worlds of one or a few stopping voxels
    "one": [(10, 20, 30)],
    "negative": [(-5, -7, -3)],
    "three": [(10, 20, 30), (13, 20, 30), (10, 23, 31)],
}


def few_voxel_world(V, name):
    w = V.World()
    for x, y, z in FEW[name]:
        w.insert(x, y, z, *STOP)
    return w


def pixel_rays(ip, iv, W, H):
    """the centre lines of the frame's rays in float64, as the shader makes them (comp:624-641): (H, W, 3) unit vectors"""
    P = np.asarray(ip, np.float64).reshape(4, 4).T   # column-major
    Vm = np.asarray(iv, np.float64).reshape(4, 4).T
    u = np.arange(W) / W * 2.0 - 1.0
    v = np.arange(H) / H * 2.0 - 1.0
    uu, vv = np.meshgrid(u, v)
    clip = np.stack([uu, vv, -np.ones_like(uu), np.ones_like(uu)], -1)
    view = clip @ P.T
    view = view[..., :3] / view[..., 3:4]
    view /= np.linalg.norm(view, axis=-1, keepdims=True)
    d = view @ Vm[:3, :3].T
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def meets_box(eye, d, mn, mx):
    """per ray: does the half-line eye + t d, t >= 0, meet the closed box [mn, mx]? (slabs) -> (bool, t_in, t_out)"""
    eye, mn, mx = (np.asarray(a, np.float64) for a in (eye, mn, mx))
    with np.errstate(divide="ignore", invalid="ignore"):
        ta, tb = (mn - eye) / d, (mx - eye) / d
    lo, hi = np.minimum(ta, tb), np.maximum(ta, tb)
    par = d == 0.0   # parallel to a slab: inside it for every t, or never
    inside = (eye >= mn) & (eye <= mx)
    lo = np.where(par, np.where(inside, -np.inf, np.inf), lo)
    hi = np.where(par, np.where(inside, np.inf, -np.inf), hi)
    t0, t1 = np.maximum(lo.max(-1), 0.0), hi.min(-1)
    return t0 <= t1, t0, t1


def approach_kind(eye, d, t0, t1, voxel):
    """for rays that meet voxel's box dilated by 1 over [t0, t1]: where they come closest to the box itself (summed over the axes), the
    number of axes on which that point lies outside the box -- 1 beside a face, 2 beside an edge, 3 beside a corner, 0: it enters"""
    s = np.linspace(0.0, 1.0, 65)
    p = eye + (t0[:, None] + (t1 - t0)[:, None] * s)[..., None] * d[:, None, :]
    mn = np.asarray(voxel, np.float64)
    out = np.maximum(np.maximum(mn - p, p - (mn + 1.0)), 0.0)   # per axis: how far outside
    best = np.argmin(out.sum(-1), axis=1)   # the summed distance: smallest where the fewest axes are outside
    o = out[np.arange(len(best)), best]
    return (o > 0.02).sum(-1)


def tiles_any(a):
    """(H, W) bool -> per 8 x 8 tile: any pixel set"""
    H, W = a.shape
    th, tw = (H + 7) // 8, (W + 7) // 8
    p = np.zeros((th * 8, tw * 8), bool)
    p[:H, :W] = a
    return p.reshape(th, 8, tw, 8).any(axis=(1, 3))


def look(eye, target):
    d = np.asarray(target, np.float64) - np.asarray(eye, np.float64)
    return (float(np.degrees(np.arctan2(d[2], d[0]))),
            float(np.clip(np.degrees(np.arctan2(d[1], np.hypot(d[0], d[2]))), -89.0, 89.0)))


def grazing_views(seed=20261017, n=36):
    """seeded search poses: a line that passes a voxel at a gap of 0.3 to 0.9 voxel beside a face, an edge or a corner, seen from 4 to
    10 voxels away by a camera aimed near it -> (world name, (x, y, z, yaw, pitch), W, H)"""
    rng = np.random.default_rng(seed)
    names = sorted(FEW)
    out = []
    for i in range(n):
        name = names[i % len(names)]
        vox = np.asarray(FEW[name][int(rng.integers(0, len(FEW[name])))], np.float64)
        k = 1 + i % 3                                   # axes on which the line lies outside the box
        axes = rng.permutation(3)[:k]
        off = np.zeros(3)
        off[axes] = rng.choice([-1.0, 1.0], size=k) * (0.5 + rng.uniform(0.3, 0.9, size=k))
        g = vox + 0.5 + off                             # the point of closest approach
        d = rng.normal(size=3)
        if k < 3:
            d[axes] = 0.0                               # along the face or the edge ...
        else:
            d -= off * (d @ off) / (off @ off)          # ... or across the corner's diagonal
        d = d / np.linalg.norm(d) + rng.normal(size=3) * 0.01
        eye = g - d / np.linalg.norm(d) * float(rng.uniform(4.0, 10.0))
        yaw, pitch = look(eye, g + rng.uniform(-1.0, 1.0, size=3))
        W, H = int(rng.integers(64, 129)), int(rng.integers(48, 97))
        out.append((name, (float(eye[0]), float(eye[1]), float(eye[2]), yaw, pitch), W, H))
    return out


def axis_views():
    """views along each axis in both directions, exactly and a hair off it, whose centre ray passes 0.3 to 0.8 voxel beside the voxel
    of world "one": every ray of the frame goes the negative way on the axis for three of them, and around the centre column and
    row a component of the direction is zero or tiny -- where miss_forward() stops trusting the mask"""
    vox = np.asarray(FEW["one"][0], np.float64) + 0.5
    out = []
    for axis, sign, yaw, pitch in ((0, 1, 0.0, 0.0), (0, -1, 180.0, 0.0), (2, 1, 90.0, 0.0), (2, -1, -90.0, 0.0), (1, 1, 0.0, 89.0),
                                   (1, -1, 0.0, -89.0)):
        for j, (dyaw, dpitch) in enumerate(((0.0, 0.0), (1e-4, 1e-4), (-1e-3, 0.0))):
            side = np.zeros(3)
            others = [k for k in range(3) if k != axis]
            side[others[j % 2]] = 0.5 + (0.3, 0.55, 0.8)[j]
            if j == 2:
                side[others[1]] = -(0.5 + 0.4)
            eye = vox + side
            eye[axis] -= sign * (5.0 + j)
            out.append(("one", (float(eye[0]), float(eye[1]), float(eye[2]), yaw + dyaw, pitch + dpitch), 64 + 16 * j, 48 + 8 * j))
    return out


def zoomed(ip, zoom):
    """the inverse projection narrowed by `zoom` (still separable: it keeps its ray tables)"""
    ip = np.array(ip, np.float32).reshape(-1).copy()
    ip[0] = np.float32(ip[0] / zoom)
    ip[5] = np.float32(ip[5] / zoom)
    return ip


LONG = ("plus_x", "minus_x", "minus_xz")
LONG_CELLS = 900   # unit cells of AIR on the centre ray's way (the march gives up after 1,024 steps)
LONG_W, LONG_H = 128, 96


def long_path_world(V, name):
    """the eye near a corner of the world [-1023, 1024)^3, LONG_CELLS unit cells of AIR along the centre ray and, near their far end,
    one stopping voxel whose box the centre ray passes 0.3 to 0.6 voxel beside -> (world, pose, stopping voxel)"""
    n = LONG_CELLS
    k = np.arange(n)
    if name == "plus_x":        # y, z near -1015, x from -1016 up
        cells = np.stack([-1016 + k, np.full(n, -1015), np.full(n, -1015)], 1)
        pose = (-1018.5, -1014.3, -1014.5, 0.002, 0.002)
        stop = (-1016 + n - 6, -1014, -1015)             # the cell above the row: 0.3 above the ray
    elif name == "minus_x":     # y, z near 1014, x from 1016 down
        cells = np.stack([1016 - k, np.full(n, 1014), np.full(n, 1014)], 1)
        pose = (1019.5, 1014.45, 1014.5, 180.0 - 0.002, -0.002)
        stop = (1016 - n + 6, 1013, 1014)                # the cell below the row: 0.45 below the ray
    else:                       # towards -x and -z at once: the staircase of cells the line x = z + 0.3 crosses
        i = 1012 - np.arange(n // 2)
        cells = np.concatenate([np.stack([i, np.full(len(i), 1000), i], 1), np.stack([i, np.full(len(i), 1000), i - 1], 1)])
        pose = (1015.8, 1000.4, 1015.5, -135.0, -0.002)   # not level: a zero y component sends the shader's ray backwards
        j = int(i[-1]) + 5
        stop = (j, 1001, j)                              # the cell above the staircase: 0.6 above the ray
    w = V.World()
    w.insert_many(cells.astype(np.int32), np.full(len(cells), AIR[0], np.uint32), AIR[1], AIR[2], AIR[3])
    w.insert(int(stop[0]), int(stop[1]), int(stop[2]), *STOP)
    return w, pose, stop


def long_path_camera(V, pose, stop, W=LONG_W, H=LONG_H, px_per_voxel=8.0):
    """the pose's camera narrowed until the stopping voxel spans px_per_voxel pixels -> (inv_proj, inv_view, cam_pos)"""
    ip, iv, cp, _ = V.camera_block(pose[:3], pose[3], pose[4], W, H)
    dist = float(np.linalg.norm(np.asarray(stop, np.float64) + 0.5 - np.asarray(pose[:3])))
    zoom = px_per_voxel * (2.0 * abs(float(ip[5])) / H) * dist
    return zoomed(ip, zoom), iv, cp
