"""The C-ABI libraries load and export every symbol the public headers declare (no compute calls; CPU)."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT


def _declared(header, prefix):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(" + prefix + r"\w+)\s*\(", text)))


def test_hip_library_exports_vrt_h(V):
    lib = C.CDLL(V.HIP_LIB)
    names = _declared("vrt.h", "vrt_")
    assert len(names) >= 18
    for n in names:
        assert hasattr(lib, n), f"libvrt_hip.so does not export {n}"
    assert b"gfx950" in V.hip_lib().vrt_version()
    # ... and nothing else: no test hooks, no internals (csrc/vrt_exports.map)
    exported = sorted(l.split()[-1] for l in os.popen(f"nm -D --defined-only {V.HIP_LIB}").read().splitlines() if " T " in l)
    extra = [n for n in exported if n not in names]
    assert not extra, f"libvrt_hip.so exports symbols include/vrt.h does not declare: {extra}"
    assert not any("debug" in n for n in exported)
    # the kernel variants vrt_set_variant() accepts (vrt_variant_available() needs no device)
    assert V.available_variants() == [0, 1, 4, 20, 22]


def test_test_support_library_is_separate(V):
    """The probes the parity suite uses to look inside the dispatch layer live in libvrt_hip_test.so (csrc/test/vrt_test.hip)."""
    lib = C.CDLL(V.TEST_LIB) if os.path.exists(V.TEST_LIB) else None
    assert lib is not None, "make -C voxel-raytracer_amd/csrc builds it"
    for n in ("vrt_test_math", "vrt_test_build_layout", "vrt_test_patch_check", "vrt_test_ray_table", "vrt_test_root0",
              "vrt_test_view_in_range", "vrt_test_wide_find", "vrt_test_tree_is_opaque", "vrt_test_tile_order"):
        assert hasattr(lib, n), n


def test_host_library_exports_vrt_host_h(V):
    lib = C.CDLL(V.HOST_LIB)
    names = _declared("vrt_host.h", "vrth_")
    assert len(names) >= 18
    for n in names:
        assert hasattr(lib, n), f"libvrt_host.so does not export {n}"
    # the C++ host API of the reference is exported too
    for n in ("octree_create", "octree_new", "octree_insert", "octree_find", "octree_ray_cast", "octree_texture",
              "_octree_texel_size", "octree_remove", "octree_delete", "load_vox_file", "VoxelObjCreate",
              "voxel_compare", "voxel_obj_compare", "make_color_rgba", "get_alpha_rgba", "ivec3_equal_vec"):
        out = os.popen(f"nm -DC {V.HOST_LIB} | grep -c ' T {n}'").read().strip()
        assert int(out) >= 1, n


def test_hip_code_object_targets_gfx950(V):
    blob = open(V.HIP_LIB, "rb").read()
    assert b"gfx950" in blob and b"trace_kernel" in blob


def test_no_gpu_means_loud_failure_not_fallback(V):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(V.VrtError) as e:
        V.Context(0)
    assert "no CPU path" in str(e.value) or "HIP" in str(e.value)


def test_cpp_example_links_against_kept_api_and_fails_loudly_without_gpu(V):
    """examples/frame_main.cpp uses the reference's own names (octree_create, load_vox_file, Camera, ...) and the
    C-ABI; it must build from include/ + the two libraries, and with no GPU exit non-zero with a message."""
    import subprocess
    import torch
    exe = os.path.join(ROOT, "examples", "frame_main")
    assert os.path.exists(exe), "make -C voxel-raytracer_amd/csrc builds it"
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    r = subprocess.run([exe, os.path.join(ROOT, "tests/golden/maps/monu9.vox"), "32", "16"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 2 and r.stderr.strip(), (r.returncode, r.stderr)


def test_argument_validation_without_device(V):
    L = V.hip_lib()
    assert L.vrt_create(0, None) == -1
    assert L.vrt_shard_rows(1080, 8, 0, 8) == 136 and L.vrt_shard_rows(1080, 8, 7, 8) == 128
    assert sum(L.vrt_shard_rows(1080, 8, s, 8) for s in range(8)) == 1080
    assert sum(L.vrt_shard_rows(67, 8, s, 3) for s in range(3)) == 67
    assert L.vrt_shard_rows(10, 0, 0, 1) < 0 and L.vrt_shard_rows(10, 8, 2, 2) < 0
    assert V.shard_row_indices(20, 8, 1, 2) == list(range(8, 16))


def test_product_never_touches_the_oracle():
    """Nothing shipped under voxel-raytracer_amd/ may reference oracle/ (the checker is not the product)."""
    pkg = os.path.join(ROOT, "voxel-raytracer_amd")
    for base, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h", ".hpp", ".c", "Makefile")):
                text = open(os.path.join(base, f), errors="ignore").read().lower()
                # comments may SAY "oracle"; no file may include, import, link, load or path into it
                for needle in ("oracle/", "oracle_py", "liboracle", "oracle.h", "import oracle", "o_render", "o_octree"):
                    assert needle not in text, (base, f, needle)


def test_only_the_allowed_callers_run_the_oracle():
    """Besides tests/, only __graft_entry__.smoke() and bench.py's cpu_baseline leg may import or load anything under oracle/
    (build() compiles it, which is not using it); the scripts under tools/ and examples/ never do."""
    import ast
    for d in ("tools", "examples"):
        for base, _, files in os.walk(os.path.join(ROOT, d)):
            for f in files:
                if f.endswith((".py", ".sh", ".cpp", ".hip", ".h", ".c")):
                    text = open(os.path.join(base, f), errors="ignore").read()
                    for needle in ("oracle_py", "liboracle", "oracle.h", "import oracle", '"oracle"', "'oracle'", "o_render", "o_octree", "o_denoise"):
                        assert needle not in text, (base, f, needle)
    for name, allowed in (("bench.py", {"cpu_baseline"}), ("__graft_entry__.py", {"smoke", "build"})):
        tree = ast.parse(open(os.path.join(ROOT, name)).read())
        for fn in [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)]:
            src_names = {getattr(x, "id", None) for x in ast.walk(fn)} | {a.name for x in ast.walk(fn) if isinstance(x, ast.Import) for a in x.names}
            strings = {x.value for x in ast.walk(fn) if isinstance(x, ast.Constant) and isinstance(x.value, str)}
            touches = "oracle_py" in src_names or "oracle" in strings or any(s.startswith("oracle/") or "liboracle" in s for s in strings if "\n" not in s and len(s) < 80)
            if touches:
                assert fn.name in allowed, (name, fn.name)
        top = [n for n in tree.body if isinstance(n, (ast.Import, ast.ImportFrom))]
        assert not any("oracle" in a.name for n in top for a in n.names), name

