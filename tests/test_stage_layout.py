"""The staging layouts of csrc/vrt_stage.h on the CPU. Every entry point that takes host buffers declares the planes of its device
block once, and the block's size, each plane's pointer and the copies come from that declaration. tests/stage_layout_main.cpp
declares every block of the library the same way and holds each plane's offset and each total to the arithmetic the entry points
wrote out by hand before: at 1, 2, 63, 64, 65, 1000 and 2^30 rays with both origin strides, at 1 to 7680 x 4320 pixels, for every
subset of the optional outputs. It runs as a program of its own under the host sanitizers; nothing is loaded into Python. What the
entry points then do with the layouts is held bit for bit to fresh contexts on the MI355X (test_gpu_buffer_growth.py)."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "voxel-raytracer_amd", "csrc")
# cases per row: rays (7) x origin strides (2) x output subsets, or pixels (5) x output subsets
ROWS = {"cast_rays": 14, "find_voxels": 7, "shade_rays": 56, "shade_rays_hdr": 112, "guide_rays": 224, "accum_guides": 80,
        "filter_host": 20, "filter_var_host": 80, "filter_accum": 20, "filter_var_accum": 40, "temporal_host": 40, "temporal_accum": 160,
        "temporal_accum_device": 5, "fixed_planes": 1}


def test_every_layout_equals_the_arithmetic_it_replaced(tmp_path):
    exe = str(tmp_path / "stage_layout_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "stage_layout_main.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)   # the sanitizers' runtimes are linked statically: the environment as it is
    assert run.returncode == 0, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr
    got = {r.split()[0]: int(r.split()[1]) for r in run.stdout.splitlines()}
    assert got == ROWS, got


def test_the_layout_part_has_no_hip_in_it():
    """what the program above compiles: the header up to its transfer part names no HIP type and includes nothing of the library"""
    text = open(os.path.join(CSRC, "vrt_stage.h")).read()
    layout = text[:text.index("#ifndef VRT_STAGE_LAYOUT_ONLY")]
    code = "\n".join(line.split("//")[0] for line in layout.splitlines())
    assert "hip" not in code.lower() and "vrt_internal" not in code and '#include "' not in code
