"""The C-ABI libraries load and export every symbol the public headers declare, and the binding's signature tables and struct
mirrors agree with those headers (no compute calls; CPU)."""
import ctypes as C
import os
import re
import subprocess

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


def _plain(header):
    """a header's text without comments and preprocessor lines"""
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    return re.sub(r"^\s*#.*$", "", text, flags=re.M)


_STRUCT = r"typedef\s+struct\s+\w+\s*\{(.*?)\}\s*(\w+)\s*;"


def _prototypes(header, prefix):
    """{name: (return type, [parameter declarations])} of every function the header declares; prototypes span lines"""
    text = re.sub(_STRUCT, "", _plain(header), flags=re.S)
    protos = {}
    for ret, name, params in re.findall(r"([\w\s\*]+?)\b(" + prefix + r"\w+)\s*\(([^)]*)\)\s*;", text):
        params = [" ".join(p.split()) for p in params.split(",")]
        protos[name] = (" ".join(ret.split()), [] if params == ["void"] else params)
    return protos


def _struct_fields(header):
    """{struct name: [field names]} of the header's typedef'd structs, in declaration order"""
    out = {}
    for body, name in re.findall(_STRUCT, _plain(header), flags=re.S):
        decls = [d.strip() for d in body.split(";") if d.strip()]
        out[name] = [re.match(r"\**\s*(\w+)", f.strip()).group(1) for d in decls for f in d.split(None, 1)[1].split(",")]
    return out


_SCALARS = {"int": (C.c_int, C.c_int32), "int32_t": (C.c_int, C.c_int32), "uint32_t": (C.c_uint32,), "size_t": (C.c_size_t,),
            "long": (C.c_long,), "float": (C.c_float,), "uint64_t": (C.c_uint64,)}


def _mirrors(V):
    return {"vrt_params": V.Params, "vrt_view": V.View, "vrt_patch": V.Patch, "vrt_scene_info": V.SceneInfo, "vrt_ray_hit": V.RayHit,
            "vrt_tonemap": V.Tonemap, "vrt_filter": V.Filter, "vrt_filter_var": V.FilterVar, "vrt_temporal": V.Temporal,
            "vrt_temporal_mom": V.TemporalMom}


def _class_error(decl, ctype, mirrors, is_return=False):
    """None where a C declaration (a parameter with its name, or a return type) and a ctypes type fall in the same class"""
    if "*" in decl or "[" in decl:
        if ctype not in (C.c_void_p, C.c_char_p) and not (isinstance(ctype, type) and issubclass(ctype, C._Pointer)):
            return f"'{decl}' is a pointer, the table has {ctype}"
        m = re.search(r"\b(vrt_\w+)\s*\*", decl)
        if m and m.group(1) in mirrors and ctype is not C.c_void_p and getattr(ctype, "_type_", None) is not mirrors[m.group(1)]:
            return f"'{decl}' points at {m.group(1)}, the table's {ctype} does not point at its mirror"
        return None
    words = decl.replace("const", " ").split()
    ctype_of = " ".join(words if is_return else words[:-1])   # a parameter carries its name
    if ctype_of == "void" and is_return:
        return None if ctype is None else f"returns void, the table has {ctype}"
    if ctype_of not in _SCALARS:
        return f"'{decl}': a type this test does not know"
    return None if ctype in _SCALARS[ctype_of] else f"'{decl}' is {ctype_of}, the table has {ctype}"


def _table_errors(protos, table, mirrors):
    errors = []
    for name, (ret, params) in sorted(protos.items()):
        if name not in table:
            errors.append(f"{name}: no row")
            continue
        res, args = table[name]
        if len(args) != len(params):
            errors.append(f"{name}: {len(params)} parameters in the header, {len(args)} in the table")
            continue
        for decl, ctype, is_ret in [(ret, res, True)] + [(p, a, False) for p, a in zip(params, args)]:
            e = _class_error(decl, ctype, mirrors, is_ret)
            if e:
                errors.append(f"{name}: {e}")
    return errors


@pytest.mark.parametrize("header,prefix,table,lib,least", [("vrt.h", "vrt_", "HIP_API", "hip_lib", 120),
                                                           ("vrt_host.h", "vrth_", "HOST_API", "host_lib", 30)])
def test_signature_tables_match_the_headers(V, header, prefix, table, lib, least):
    """Every function a public header declares has a row in the binding's table for that library, with as many parameters and
    each parameter and the return type in the prototype's class (pointer, int, uint32_t, size_t, long, float, uint64_t, void);
    a pointer to a mirrored struct points at the mirror or is a void pointer. The loaded library carries exactly the table."""
    protos, rows, mirrors = _prototypes(header, prefix), getattr(V, table), _mirrors(V)
    assert sorted(protos) == _declared(header, prefix) and len(protos) >= least   # the parser saw every function
    assert _table_errors(protos, rows, mirrors) == []
    L = getattr(V, lib)()
    for name, (res, args) in rows.items():
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    # the checker itself: a pointer declared as an int, a short row, a float for an int, a pointer at the wrong mirror
    name = prefix + "version"
    planted = dict(rows, **{name: (C.c_int, [])})
    assert _table_errors(protos, planted, mirrors) == [f"{name}: 'const char *' is a pointer, the table has {C.c_int}"]
    if header == "vrt.h":
        res, args = rows["vrt_set_lens"]
        assert len(_table_errors(protos, dict(rows, vrt_set_lens=(res, args[:-1])), mirrors)) == 1
        assert len(_table_errors(protos, dict(rows, vrt_set_lens=(res, [args[0], C.c_int, args[2]])), mirrors)) == 1
        assert len(_table_errors(protos, dict(rows, vrt_set_lens=(res, [C.c_int] + args[1:])), mirrors)) == 1
        res, args = rows["vrt_filter_default"]
        assert len(_table_errors(protos, dict(rows, vrt_filter_default=(res, [C.POINTER(V.FilterVar)])), mirrors)) == 1
        assert len(_table_errors(protos, dict(rows, vrt_filter_default=(C.c_int, args)), mirrors)) == 1


def test_struct_mirrors_match_the_header(V, tmp_path):
    """sizeof, and every field's name, offset and size, of the public structs from a C compiler against include/vrt.h, equal to
    the ctypes mirrors (and, for vrt_ray_hit, to RAY_HIT_DTYPE)"""
    fields, mirrors = _struct_fields("vrt.h"), _mirrors(V)
    assert sorted(fields) == sorted(mirrors)   # every struct of the header has a mirror
    lines = []
    for s in sorted(fields):
        lines.append(f'    printf("{s} %zu\\n", sizeof({s}));')
        lines += [f'    printf("{s}.{f} %zu %zu\\n", offsetof({s}, {f}), sizeof((({s} *)0)->{f}));' for f in fields[s]]
    src = tmp_path / "probe.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vrt.h"\nint main(void) {\n' + "\n".join(lines) + "\n    return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        key, *nums = line.split()
        got[key] = [int(v) for v in nums]
    want = {}
    for s, m in mirrors.items():
        want[s] = [C.sizeof(m)]
        assert [k for k, _ in m._fields_] == fields[s], s
        want.update({f"{s}.{k}": [getattr(m, k).offset, getattr(m, k).size] for k, _ in m._fields_})
    assert got == want
    ray = ("hit", "coord", "place", "leaf", "steps")
    assert [got["vrt_ray_hit"][0]] + [got[f"vrt_ray_hit.{f}"][0] for f in ray] == [40, 0, 4, 16, 28, 36]
    assert V.RAY_HIT_DTYPE.itemsize == 40 and V.RAY_HIT_DTYPE.names == ray
    assert [V.RAY_HIT_DTYPE.fields[f][1] for f in ray] == [got[f"vrt_ray_hit.{f}"][0] for f in ray]
    assert [V.RAY_HIT_DTYPE.fields[f][0].itemsize for f in ray] == [got[f"vrt_ray_hit.{f}"][1] for f in ray]


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

