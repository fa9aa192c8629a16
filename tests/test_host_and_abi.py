"""CPU: host-side logic and the C-ABI surface (library loads, exports every declared symbol,
argument validation happens before any kernel launch, product fails loudly without a GPU)."""
import ctypes as C
import os
import re

import pytest
import torch

import abi_check
import gaussianprediction_amd as gpa
from gaussianprediction_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "gp_hip.h")).read()
    declared = set(re.findall(r"\b(gp_[a-z_0-9]+)\s*\(", hdr)) - {"gp_alloc_fn"}
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    l = _lib.lib()
    for name in declared:
        assert hasattr(l, name), name
    assert b"gfx950" in l.gp_version()


def test_struct_sizes_match_header_layout():
    assert C.sizeof(_lib.RasterSettingsC) == 9 * 4 + 4 + 4 * 8 + 8 + 8 + 8 + 4 + 4 + 8 + 4 + 4   # 9 x 4-byte + pad + 4 pointers + capacity + status pointer + event + depth-key bits, base, range pointer + raw_activations + reserved
    assert C.sizeof(_lib.RasterInputsC) == 9 * 8
    assert C.sizeof(_lib.RasterSavedC) == 7 * 8
    assert C.sizeof(_lib.RasterGradsC) == 9 * 8 + 8 + 8     # + accumulate_shs (padded) + adam_shs
    assert C.sizeof(_lib.AdamFuseC) == 4 * 8 + 5 * 4 + 4 + 8 + 8   # 4 pointers, 5 floats + pad, step, skip_flag
    assert C.sizeof(_lib.MlpParamsC) == 4 * 4 + 12 * 8      # 4 dims, w[5], b[5], packed, scratch (round 6)
    assert C.sizeof(_lib.MlpInputC) == 8 + 3 * 4 + 4 + 3 * 8
    assert C.sizeof(_lib.BlendArgsC) == 2 * 8 + 3 * 4 + 4 + 6 * 8


def test_mlp_scratch_size_query():
    """gp_mlp_scratch_bytes (round 6): 8 KB of counters (32 row tiles x 128 B + the error word at byte 4096) + the exchange region of
    four hidden layers; 0 where the feature-split kernels do not run (more than 512 rows)."""
    l = _lib.lib()
    assert int(l.gp_mlp_scratch_bytes(C.c_int64(250))) == 8192 + 4 * 250 * 256 * 4
    assert int(l.gp_mlp_scratch_bytes(C.c_int64(512))) == 8192 + 4 * 512 * 256 * 4
    assert int(l.gp_mlp_scratch_bytes(C.c_int64(513))) == 0 and int(l.gp_mlp_scratch_bytes(C.c_int64(0))) == 0


def test_abi_validation_errors_are_reported_not_thrown():
    l = _lib.lib()
    st = _lib.RasterSettingsC(0, 0, 1.0, 1.0, 1.0, 3, 16, 0, 0, None, None, None, None)
    inp = _lib.RasterInputsC(0, None, None, None, None, None, None, None, None)
    out = _lib.RasterOutputsC(None, None, None, None)
    saved = _lib.RasterSavedC()
    alloc = _lib.TorchAllocator("cpu")
    rc = l.gp_raster_forward(C.byref(st), C.byref(inp), C.byref(out), C.byref(saved), alloc.cb, None, None)
    assert rc != 0 and b"image size" in l.gp_last_error()
    st.image_height, st.image_width = 16, 16
    inp.num_gaussians = 4
    rc = l.gp_raster_forward(C.byref(st), C.byref(inp), C.byref(out), C.byref(saved), alloc.cb, None, None)
    assert rc != 0 and b"exactly one of either SHs" in l.gp_last_error()
    p = _lib.MlpParamsC(104, 128, 4, 7)
    x = _lib.MlpInputC(0, 32, 10, 6, None, None, None)
    rc = l.gp_mlp_forward(C.byref(p), C.byref(x), None, None, None)
    assert rc != 0 and b"d=4, w=256" in l.gp_last_error()
    with pytest.raises(_lib.GpHipError):
        _lib.check(rc, "gp_mlp_forward")


def test_retired_debug_keys_are_refused():
    """A script that still selects a removed kernel variant fails at the call; it does not time the default in silence."""
    l = _lib.lib()
    for k in (2, 3, 7, 10):
        assert l.gp_debug_option(k, 1) != 0 and b"retired" in l.gp_last_error()
    assert l.gp_debug_option(5, 0) == 0


def test_debug_index_entries_validate_their_arguments():
    """gp_debug_sort_pairs / gp_debug_scan_blocks / gp_debug_bin_lists refuse bad arguments before anything touches a device."""
    l = _lib.lib()
    err = l.gp_last_error

    def sort(algo, keys, vals, n, nbits, by_value=None, outs=(8, 8, None, None)):
        return l.gp_debug_sort_pairs(algo, keys, vals, n, nbits, by_value, outs[0], outs[1], outs[2], outs[3], None)

    assert sort(2, 8, None, 4, 32) != 0 and b"algo 2" in err()
    assert sort(0, 8, None, -1, 32) != 0 and b"n out of range" in err()
    assert sort(0, 8, None, 1 << 32, 32) != 0 and b"n out of range" in err()          # (cut to 32 bits this is n == 0: rc 0)
    for nbits in (0, 33):
        assert sort(0, 8, None, 4, nbits) != 0 and b"nbits" in err()
    assert sort(0, 8, 8, 4, 32, by_value=8, outs=(8, 8, 8, 8)) != 0 and b"iota values" in err()   # the epilogue indexes by_value with the values
    assert sort(0, 8, None, 4, 32, by_value=8, outs=(8, 8, None, 8)) != 0 and b"sorted_out" in err()
    assert sort(1, 8, None, 4, 24) != 0 and b"32 key bits" in err()
    assert sort(1, 8, 8, 4, 32) != 0 and b"iota values" in err()
    assert sort(1, 8, None, 512 * 8192 + 1, 32) != 0 and b"n <= 4194304" in err()
    assert sort(0, None, None, 4, 32) != 0 and b"null argument" in err()
    assert sort(0, 8, None, 4, 32, outs=(None, 8, None, None)) != 0 and b"null argument" in err()
    assert sort(0, None, None, 0, 32, outs=(None, None, None, None)) == 0              # nothing to sort

    assert l.gp_debug_scan_blocks(8, -1, 8, 8, None) != 0 and b"n out of range" in err()
    assert l.gp_debug_scan_blocks(8, 4, 8, None, None) != 0 and b"null argument" in err()

    def bins(path, n, gx, gy, capacity=0, ids=8, rects=8, pl=8, ranges=8, status=8, r_out=None):
        r = C.c_uint32(77) if r_out is None else r_out
        return l.gp_debug_bin_lists(path, n, gx, gy, ids, rects, capacity, pl, ranges, status, C.byref(r) if r is not False else None, None)

    assert bins(2, 4, 4, 4) != 0 and b"path 2" in err()
    assert bins(1, -1, 4, 4) != 0 and b"n out of range" in err()
    for gx, gy in ((0, 4), (4, 0), (65536, 1), (4097, 4097)):
        assert bins(1, 4, gx, gy) != 0 and b"bad tile grid" in err()
    assert bins(1, 4, 4, 4, capacity=-1) != 0 and b"capacity out of range" in err()
    assert bins(1, 4, 4, 4, capacity=1 << 31) != 0 and b"capacity out of range" in err()
    assert bins(1, 4, 4, 4, ranges=None) != 0 and b"null argument" in err()
    assert bins(1, 4, 4, 4, status=None) != 0 and b"null argument" in err()
    assert bins(1, 4, 4, 4, r_out=False) != 0 and b"null argument" in err()
    # the counting path is refused where the forward would not take it: no silent switch to the other path
    assert bins(0, 512 * 8192 + 1, 85, 64) != 0 and b"binning by counting does not take" in err()
    assert bins(0, 1000, 8193, 1) != 0 and b"binning by counting does not take" in err()
    assert bins(0, 0, 4, 4) != 0 and b"binning by counting does not take" in err()


def test_rasterizer_argument_contract_and_no_cpu_fallback():
    bg = torch.zeros(3)
    rs = gpa.GaussianRasterizationSettings(image_height=32, image_width=32, tanfovx=0.5, tanfovy=0.5, bg=bg,
                                           scale_modifier=1.0, viewmatrix=torch.eye(4), projmatrix=torch.eye(4),
                                           sh_degree=3, campos=torch.zeros(3), prefiltered=False)
    assert rs.debug is False                      # reference does not pass debug (gaussian_renderer/__init__.py:49)
    r = gpa.GaussianRasterizer(raster_settings=rs)
    m3 = torch.zeros(4, 3)
    with pytest.raises(Exception, match="SHs or precomputed colors"):
        r(means3D=m3, means2D=m3, opacities=torch.ones(4, 1), scales=torch.ones(4, 3), rotations=torch.ones(4, 4))
    with pytest.raises(Exception, match="scale/rotation pair or precomputed 3D covariance"):
        r(means3D=m3, means2D=m3, opacities=torch.ones(4, 1), shs=torch.zeros(4, 16, 3))
    # CPU tensors: the product must fail loudly, never silently fall back
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        r(means3D=m3, means2D=m3, opacities=torch.ones(4, 1), shs=torch.zeros(4, 16, 3), scales=torch.ones(4, 3),
          rotations=torch.ones(4, 4))


def test_deformable_field_state_dict_keys_match_reference():
    net = gpa.Deformable_Field(104, output_dim=7, d=4, w=256, split_xyz=False)
    keys = list(net.state_dict().keys())
    assert keys == ["mlp.0.weight", "mlp.0.bias", "mlp.2.weight", "mlp.2.bias", "mlp.4.weight", "mlp.4.bias",
                    "mlp.6.weight", "mlp.6.bias", "feature_to_deformation.0.weight", "feature_to_deformation.0.bias"]
    assert sum(p.numel() for p in net.parameters()) == 226055
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(torch.zeros(3, 104))


def test_product_does_not_import_the_oracle():
    pkg = os.path.join(ROOT, "gaussianprediction_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in src and "from oracle" not in src and "gp_oracle" not in src.replace("oracle/gp_oracle.c", ""), f


def test_capacity_mode_settings_are_validated_on_the_host():
    """GaussianRasterizationSettings.binning_capacity / binning_status (extension): defaults keep the reference's
    11-kwarg construction working; a capacity without a status word, or a malformed status tensor, is rejected before
    anything is launched."""
    import torch
    from gaussianprediction_amd import rasterizer as R
    dev = torch.device("cpu")
    kw = dict(image_height=8, image_width=8, tanfovx=0.5, tanfovy=0.5, bg=torch.zeros(3), scale_modifier=1.0,
              viewmatrix=torch.eye(4), projmatrix=torch.eye(4), sh_degree=3, campos=torch.zeros(3), prefiltered=False)
    rs = R.GaussianRasterizationSettings(**kw)
    assert rs.debug is False and rs.binning_capacity == 0 and rs.binning_status is None
    st, keep = R._settings_c(rs, dev, 16)
    assert st.binning_capacity == 0 and not st.binning_status
    status = torch.zeros(2, dtype=torch.int32)
    st, keep = R._settings_c(R.GaussianRasterizationSettings(**kw, binning_capacity=1000, binning_status=status), dev, 16)
    assert st.binning_capacity == 1000 and st.binning_status == status.data_ptr() and any(k is status for k in keep)
    with pytest.raises(RuntimeError, match="needs binning_status"):
        R._settings_c(R.GaussianRasterizationSettings(**kw, binning_capacity=1000), dev, 16)
    with pytest.raises(RuntimeError, match="int32"):
        R._settings_c(R.GaussianRasterizationSettings(**kw, binning_capacity=1000, binning_status=torch.zeros(2)), dev, 16)


# ---- one layout, three statements of it: include/gp_hip.h (gcc), gaussianprediction_amd/_lib.py, INTEGRATION.md section 3 ----
_STRUCTS = {"gp_raster_settings": "RasterSettingsC", "gp_raster_inputs": "RasterInputsC", "gp_raster_outputs": "RasterOutputsC",
            "gp_raster_saved": "RasterSavedC", "gp_raster_grads": "RasterGradsC", "gp_adam_fuse": "AdamFuseC",
            "gp_mlp_params": "MlpParamsC", "gp_mlp16_params": "Mlp16ParamsC", "gp_mlp_grads": "MlpGradsC",
            "gp_mlp_input": "MlpInputC", "gp_blend_args": "BlendArgsC", "gp_profile_entry": "ProfileEntryC",
            "gp_step_plan": "StepPlanC", "gp_step_view": "StepViewC", "gp_step_update": "StepUpdateC",
            "gp_hashgrid_config": "HashGridConfigC"}


def _header_layout(tmp_path):
    """{struct: (sizeof, [(field, offset, size)])} of the header, measured by a C program gcc builds from it."""
    hdr = open(os.path.join(ROOT, "include", "gp_hip.h")).read()
    body = []
    for cname in _STRUCTS:
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), hdr, re.S)
        assert m, cname
        text = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        fields = []
        for decl in text.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            for part in decl.split(","):
                name = re.sub(r"\[.*\]", "", part.strip().split()[-1]).lstrip("*")
                fields.append(name)
        body.append('printf("%s %%zu", sizeof(%s));' % (cname, cname))
        for f in fields:
            body.append('printf(" %s:%%zu:%%zu", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (f, cname, f, cname, f))
        body.append('printf("\\n");')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gp_hip.h"\nint main(void){%s return 0;}\n' % "".join(body))
    exe = tmp_path / "layout"
    import subprocess
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = {}
    for line in subprocess.check_output([str(exe)]).decode().splitlines():
        toks = line.split()
        out[toks[0]] = (int(toks[1]), [(t.split(":")[0], int(t.split(":")[1]), int(t.split(":")[2])) for t in toks[2:]])
    return out


def _ctypes_layout(cls):
    return C.sizeof(cls), [(n, getattr(cls, n).offset, getattr(cls, n).size) for n, *_ in cls._fields_]


def test_binding_structs_match_the_header_field_by_field(tmp_path):
    hdr = _header_layout(tmp_path)
    for cname, pyname in _STRUCTS.items():
        cls = getattr(_lib, pyname, None)
        if cls is None:
            continue
        assert _ctypes_layout(cls) == hdr[cname], (cname, _ctypes_layout(cls), hdr[cname])


def test_integration_stub_matches_header_and_binding(tmp_path):
    """INTEGRATION.md section 3 is what an integrator copies: its struct definitions must be the header's (round-2 verdict:
    the stub had fallen two fields behind, so the library would have read past the caller's struct)."""
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = md[md.index("## 3."):md.index("## 4.")]
    code = re.search(r"```python\n(.*?)```", sec, re.S).group(1)
    defs = code[:code.index("# ---- call")]
    assert "gp_raster_forward" in code and "gp_raster_backward" in code
    ns = {}
    exec(defs.replace('lib = C.CDLL("gaussianprediction_amd/libgp_hip.so")', "lib = None"), ns)
    hdr = _header_layout(tmp_path)
    checked = 0
    for cname, pyname in _STRUCTS.items():
        if pyname in ns:
            assert _ctypes_layout(ns[pyname]) == hdr[cname], (cname, _ctypes_layout(ns[pyname]), hdr[cname])
            assert _ctypes_layout(ns[pyname]) == _ctypes_layout(getattr(_lib, pyname))
            checked += 1
    assert checked == 5
    # the call part constructs every struct by keyword, with field names that exist
    import ast
    seen = set()
    for node in ast.walk(ast.parse(code[code.index("# ---- call"):])):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id in ns and hasattr(ns[node.func.id], "_fields_"):
            assert not node.args, f"{node.func.id} constructed positionally"
            assert {k.arg for k in node.keywords} <= {n for n, *_ in ns[node.func.id]._fields_}, node.func.id
            seen.add(node.func.id)
    assert seen == {"RasterSettingsC", "RasterInputsC", "RasterOutputsC", "RasterSavedC", "RasterGradsC"}


# ---- one signature per entry point, two statements of it: include/gp_hip.h and _lib.PROTOTYPES ----
_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "float": C.c_float,
            "size_t": C.c_size_t, "gp_stream_t": _lib.Ptr, "gp_alloc_fn": _lib.Ptr}
_POINTEES = {"float", "double", "void", "int", "int8_t", "int16_t", "int32_t", "int64_t", "uint8_t", "uint16_t", "uint32_t", "uint64_t"}


def _abis():
    """Every binding: the eleven further modules join _lib.ABIS when they are imported."""
    from gaussianprediction_amd import (densify_ops, gcn_ops, jpeg_decode, jpeg_ops, jpeg_sync, kmeans_ops, lpips,  # noqa: F401
                                        png_decode, png_ops, resize_ops, voxel_ops)
    return _lib.ABIS


def test_prototype_table_equals_the_header():
    assert _lib.ABIS[0] is _lib.ABI and _lib.ABI.prototypes is _lib.PROTOTYPES and _lib.ABI.version == _lib.GP_ABI_VERSION
    protos = abi_check.check_table(_lib.ABI, 64, _SCALARS, _POINTEES, {c: getattr(_lib, py) for c, py in _STRUCTS.items()})
    assert set(protos) == set(_lib.EXPORTS) and len(_lib.EXPORTS) == 64
    assert _lib.PROTOTYPES["gp_raster_forward"][1][0]._type_ is _lib.RasterSettingsC           # (POINTER(X) is cached: `is` compares X)
    from gaussianprediction_amd import weights_ops
    assert weights_ops.HashGridConfigC is _lib.HashGridConfigC


def test_prototype_table_is_applied_to_the_library():
    abi_check.check_applied(_lib.ABI)


def test_every_header_has_one_binding_and_no_name_two():
    abis = _abis()
    headers = sorted(a.header for a in abis)
    assert headers == sorted(os.listdir(os.path.join(ROOT, "include"))) and len(headers) == 12, headers       # (twelve .h files, no directory)
    names = [n for a in abis for n in a.prototypes]
    assert len(names) == len(set(names)) == 117, sorted(n for n in set(names) if names.count(n) > 1)


def test_argument_width_survives_without_a_wrapper():
    l = _lib.lib()
    rc = l.gp_raster_mark_visible(1 << 32, None, None, None, None)     # (cut to 32 bits this is n == 0: the early return, rc 0)
    assert rc != 0 and b"n out of range" in l.gp_last_error()
    assert l.gp_mlp_scratch_bytes(250) == 8192 + 4 * 250 * 256 * 4


def test_wrong_argument_kinds_are_refused_before_the_library_runs():
    l = _lib.lib()
    with pytest.raises(C.ArgumentError):
        l.gp_debug_option(0.5, 0)                                      # float for int32_t
    with pytest.raises(C.ArgumentError):
        l.gp_mlp_scratch_bytes(C.c_int32(250))                         # c_int32 for int64_t
    st = _lib.RasterSettingsC(0, 0, 1.0, 1.0, 1.0, 3, 16, 0, 0, None, None, None, None)
    inp = _lib.RasterInputsC(0, None, None, None, None, None, None, None, None)
    out, saved = _lib.RasterOutputsC(None, None, None, None), _lib.RasterSavedC()
    with pytest.raises(C.ArgumentError):
        l.gp_raster_forward(inp, C.byref(inp), C.byref(out), C.byref(saved), None, None, None)    # gp_raster_inputs for the settings
    with pytest.raises(C.ArgumentError):
        l.gp_raster_forward(C.byref(inp), C.byref(inp), C.byref(out), C.byref(saved), None, None, None)
    assert l.gp_raster_forward(st, inp, out, saved, None, None, None) != 0 and b"image size" in l.gp_last_error()   # instance == byref
    # the pointer class: a tensor is its data_ptr(); None, wide ints, ctypes arrays, byref, c_void_p and callbacks as c_void_p takes them
    t = torch.zeros(4)
    assert _lib.Ptr.from_param(t).value == t.data_ptr()
    assert _lib.Ptr.from_param(None) is None
    alloc = _lib.TorchAllocator("cpu")
    for ok in ((1 << 40) + 8, (C.c_uint64 * 4)(), C.byref(C.c_int(0)), C.c_void_p(16), _lib.ptr(t), alloc.cb):
        _lib.Ptr.from_param(ok)
    alloc.release()
    for bad in (0.5, st):
        with pytest.raises(TypeError):
            _lib.Ptr.from_param(bad)


def test_every_call_site_passes_as_many_arguments_as_the_prototype_has():
    """ctypes accepts surplus positional arguments in silence and most call sites only run on a GPU: count them in the source, for
    every table, and find every entry point called somewhere.  A call site is `x.gp_name(...)`, `q(...)` where the file binds `q = x.gp_name`, and
    `_lib.scratch(x.gp_name, ...)`, which calls its first argument with the further positional ones."""
    import ast
    import glob
    table = {name: (abi, len(argtypes)) for abi in _abis() for name, (_, argtypes) in abi.prototypes.items()}
    files = [os.path.join(ROOT, "bench.py"), os.path.join(ROOT, "__graft_entry__.py")]
    for d in ("gaussianprediction_amd", "tools", "tests"):
        files += glob.glob(os.path.join(ROOT, d, "**", "*.py"), recursive=True)
    examined, seen = {abi.header: 0 for abi in _abis()}, set()
    uncalled = {abi.version_fn for abi in _abis()} | {"gp_adam_step"}       # Abi.bind calls version_fn through getattr; nothing in Python calls gp_adam_step
    for path in sorted(files):
        nodes, alias = list(ast.walk(ast.parse(open(path).read(), path))), {}
        for node in nodes:
            if isinstance(node, ast.Assign) and isinstance(node.value, ast.Attribute) and node.value.attr in table:
                for target in node.targets:
                    if isinstance(target, ast.Name):
                        assert alias.setdefault(target.id, node.value.attr) == node.value.attr, (path, node.lineno)
        for node in nodes:
            if not isinstance(node, ast.Call):
                continue
            f, args, keywords = node.func, node.args, node.keywords
            name = f.attr if isinstance(f, ast.Attribute) else alias.get(f.id) if isinstance(f, ast.Name) else None
            if name == "scratch" and args and isinstance(args[0], ast.Attribute):
                name, args, keywords = args[0].attr, args[1:], []
            if name in table:
                abi, want = table[name]
                assert not keywords, (path, node.lineno)
                if any(isinstance(a, ast.Starred) for a in args):
                    continue
                examined[abi.header] += 1
                seen.add(name)
                assert len(args) == want, (os.path.relpath(path, ROOT), node.lineno, name)
    assert sum(examined.values()) >= 300 and all(examined.values()), examined
    print(f"{sum(examined.values())} call sites of {len(seen)} entry points")
    assert seen >= set(table) - uncalled, sorted(set(table) - uncalled - seen)
    assert "gp_adam_step" not in seen                                      # (the exception goes when a call site comes)


def test_allocator_block_releases_on_every_path_and_prefers_the_callback_error():
    l = _lib.lib()
    st = _lib.RasterSettingsC(0, 0, 1.0, 1.0, 1.0, 3, 16, 0, 0, None, None, None, None)       # image size 0: the library refuses
    inp = _lib.RasterInputsC(0, None, None, None, None, None, None, None, None)
    out, saved = _lib.RasterOutputsC(None, None, None, None), _lib.RasterSavedC()

    def failing_call(alloc):
        rc = l.gp_raster_forward(st, inp, out, saved, alloc.cb, None, None)
        assert rc != 0
        return rc

    with _lib.TorchAllocator("cpu") as alloc:                          # success: the buffers are reachable inside the block
        assert alloc.cb(None, _lib.GP_BUF_GEOM, 64) == alloc.first(_lib.GP_BUF_GEOM).data_ptr()
        assert alloc.first(_lib.GP_BUF_IMAGE) is None
    assert alloc.bufs is None and alloc.cb is None

    with pytest.raises(KeyError):                                      # allocator error + library error: the allocator's comes out
        with _lib.TorchAllocator("cpu") as alloc:
            assert not alloc.cb(None, 99, 64)                          # (no such buffer class: the callback catches a KeyError)
            assert isinstance(alloc.error, KeyError)
            _lib.check(failing_call(alloc), "gp_raster_forward")
    assert alloc.bufs is None

    with pytest.raises(KeyError):                                      # allocator error although the call returned 0
        with _lib.TorchAllocator("cpu") as alloc:
            alloc.cb(None, 99, 64)
            _lib.check(0, "nothing")
    assert alloc.bufs is None

    with pytest.raises(_lib.GpHipError, match="image size"):           # library error alone
        with _lib.TorchAllocator("cpu") as alloc:
            _lib.check(failing_call(alloc), "gp_raster_forward")
    assert alloc.bufs is None

    with pytest.raises(ZeroDivisionError):                             # an unrelated exception passes through
        with _lib.TorchAllocator("cpu") as alloc:
            alloc.cb(None, _lib.GP_BUF_TEMP, 16)
            1 / 0
    assert alloc.bufs is None
