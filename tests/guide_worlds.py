"""The frames and rays of the guide-plane tests (test_guides.py, test_gpu_guides.py) -- TEST INFRASTRUCTURE ONLY: the reference's
room with its glass seen from inside and from outside, and the lamp room of tests/emit_worlds.py seen through its pane, at a frame size of whole
tiles and at one with partial tiles on both edges; and the picking rays both sides of the vrt_cast_rays comparison use."""
import numpy as np

from conftest import room_world
import emit_worlds

W, H = 40, 24              # five by three whole 8 x 8 tiles
RAGGED = (43, 21)          # no multiple of 8 either way: partial tiles on the right, a ragged last tile row
FIRST, N = 5, 8            # the accumulations' first sample index and sample count
FRAMES = {                 # name -> (pose, (aperture, focus distance))
    "room": ((14.5, 30.5, 16.5, 32.0, -10.0), (0.75, 20.0)),
    "lamp": (emit_worlds.POSE, emit_worlds.LENS),
    "outside": ((98.5, 34.5, 52.5, 197.0, -8.0), (1.25, 45.0)),   # the room from outside: sky around it
}
SOURCES = {"corner": (False, False), "jitter": (True, False), "lens": (False, True), "jitter_lens": (True, True)}   # jitter, lens


def world(V, name):
    """-> V.World (the caller closes it)"""
    return emit_worlds.lamp_room(V) if name == "lamp" else room_world(V)


def camera(V, name, size=(W, H)):
    pose = FRAMES[name][0]
    return V.camera_block(pose[:3], pose[3], pose[4], size[0], size[1])[:3]


def lens_of(name, source):
    """(aperture, focus) of a source of SOURCES in frame `name`"""
    return FRAMES[name][1] if SOURCES[source][1] else (0.0, 1.0)


def picking_rays(n=300, seed=3):
    """n directions from the lamp room's eye: every one ends on the closed room's shell, its table, lamps or pane"""
    d = np.random.default_rng(seed).normal(size=(n, 3)).astype(np.float32)
    return np.array(emit_worlds.EYE, np.float32), d
