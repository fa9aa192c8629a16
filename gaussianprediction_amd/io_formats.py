"""On-disk formats of the reference, so that scenes trained with either code base load
in the other:

* `point_cloud.ply` as written by `GaussianModel.save_ply` [REF scene/gaussian_model.py:493-524]: binary little-endian,
  one `vertex` element, float32 columns
  `x y z nx ny nz f_dc_0..2 f_rest_0..44 opacity scale_0..2 rot_0..3`, where f_dc / f_rest are the [N,1,3] / [N,15,3]
  tensors transposed to channel-major ([N,3,1] / [N,3,15]) and flattened, normals are zero, and every value is the RAW
  parameter (log-scale, logit-opacity, un-normalised quaternion).  (The reference writes it through `plyfile`, which is
  not installed here: the header below is the one plyfile emits for that dtype list.)
* `chkpnt<iteration>.pth` = `torch.save((gaussians.state_dict(), optimizer.state_dict(), iteration))`
  [REF train.py:199-201], restored with `load_state_dict(strict=False)` after sizing the model from `_xyz` /
  `super_gaussians` [REF train.py:48-57].  Parameter names are identical here, so the tuple is interchangeable.
* the point cloud a scene starts from, as Open3D's `write_point_cloud` lays a binary PLY out (`save_point_cloud_ply`: double
  `x y z`, double normals, uchar colours), which the reference's `fetchPly` reads [REF scene/dataset_readers.py:112-118].
"""
from __future__ import annotations

import os

import numpy as np
import torch


def ply_attributes(n_dc=3, n_rest=45, n_scale=3, n_rot=4):
    """[REF scene/gaussian_model.py:493-506 construct_list_of_attributes]"""
    names = ["x", "y", "z", "nx", "ny", "nz"]
    names += [f"f_dc_{i}" for i in range(n_dc)]
    names += [f"f_rest_{i}" for i in range(n_rest)]
    names += ["opacity"]
    names += [f"scale_{i}" for i in range(n_scale)]
    names += [f"rot_{i}" for i in range(n_rot)]
    return names


def save_ply(model, path):
    """Write `model`'s Gaussians exactly as the reference's save_ply does."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    if hasattr(model, "_sync_side_stream"):
        model._sync_side_stream()   # a training harness may still be updating / gathering parameters (second stream, all-gather)
    xyz = model._xyz.detach().cpu().numpy()
    normals = np.zeros_like(xyz)
    f_dc = model._features_dc.detach().transpose(1, 2).flatten(start_dim=1).contiguous().cpu().numpy()
    f_rest = model._features_rest.detach().transpose(1, 2).flatten(start_dim=1).contiguous().cpu().numpy()
    opac = model._opacity.detach().cpu().numpy()
    scale = model._scaling.detach().cpu().numpy()
    rot = model._rotation.detach().cpu().numpy()
    table = np.concatenate((xyz, normals, f_dc, f_rest, opac, scale, rot), axis=1).astype("<f4")
    names = ply_attributes(f_dc.shape[1], f_rest.shape[1], scale.shape[1], rot.shape[1])
    assert table.shape[1] == len(names)
    header = "ply\nformat binary_little_endian 1.0\n" + f"element vertex {table.shape[0]}\n" + \
        "".join(f"property float {n}\n" for n in names) + "end_header\n"
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(np.ascontiguousarray(table).tobytes())


_PLY_TYPES = {"float": "<f4", "float32": "<f4", "double": "<f8", "float64": "<f8", "uchar": "u1", "uint8": "u1", "char": "i1",
              "int8": "i1", "short": "<i2", "int16": "<i2", "ushort": "<u2", "uint16": "<u2", "int": "<i4", "int32": "<i4",
              "uint": "<u4", "uint32": "<u4"}


def read_ply_vertices(path):
    """Structured numpy array of the `vertex` element of a binary-little-endian or ascii PLY (scalar properties only)."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        fmt, count, props, in_vertex = None, 0, [], False
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: unterminated PLY header")
            tok = line.decode("ascii").split()
            if not tok:
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                in_vertex = tok[1] == "vertex"
                if in_vertex:
                    count = int(tok[2])
            elif tok[0] == "property" and in_vertex:
                if tok[1] == "list":
                    raise ValueError(f"{path}: list properties on the vertex element are not supported")
                props.append((tok[2], _PLY_TYPES[tok[1]]))
            elif tok[0] == "end_header":
                break
        dt = np.dtype(props)
        if fmt == "binary_little_endian":
            return np.frombuffer(f.read(count * dt.itemsize), dtype=dt, count=count)
        if fmt == "ascii":
            rows = np.loadtxt(f, max_rows=count, ndmin=2)
            out = np.empty(count, dtype=dt)
            for k, (name, _) in enumerate(props):
                out[name] = rows[:, k]
            return out
        raise ValueError(f"{path}: unsupported PLY format {fmt}")


def color_to_uint8(colors):
    """round(clamp(c, 0, 1) * 255) as uint8: Open3D's ColorToUint8, restated from memory of its source (Open3D is not installed where
    this was written, so the rounding of an exact half is unpinned; np.round sends it to the even byte)."""
    return np.round(np.clip(np.asarray(colors, dtype=np.float64), 0.0, 1.0) * 255.0).astype(np.uint8)


def save_point_cloud_ply(path, points, colors=None, normals=None):
    """A point cloud as Open3D's write_point_cloud lays a binary PLY out: little-endian, one `vertex` element, double x y z, double
    nx ny nz where there are normals, uchar red green blue = color_to_uint8(colors) where there are colours -- the field names the
    reference's fetchPly reads [REF scene/dataset_readers.py:112-118].  points / colors / normals: [N, 3] arrays."""
    cols = [("x", "<f8"), ("y", "<f8"), ("z", "<f8")]
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    parts = [(("x", "y", "z"), points)]
    if normals is not None:
        cols += [("nx", "<f8"), ("ny", "<f8"), ("nz", "<f8")]
        parts.append((("nx", "ny", "nz"), np.asarray(normals, dtype=np.float64).reshape(-1, 3)))
    if colors is not None:
        cols += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        parts.append((("red", "green", "blue"), color_to_uint8(colors).reshape(-1, 3)))
    table = np.empty(points.shape[0], dtype=np.dtype(cols))
    for names, a in parts:
        if a.shape != points.shape:
            raise ValueError(f"save_point_cloud_ply: {names} are {a.shape}, the points {points.shape}")
        for k, name in enumerate(names):
            table[name] = a[:, k]
    kinds = {"<f8": "double", "u1": "uchar"}
    header = "ply\nformat binary_little_endian 1.0\n" + f"element vertex {table.shape[0]}\n" + \
        "".join(f"property {kinds[t]} {n}\n" for n, t in cols) + "end_header\n"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(table.tobytes())


def save_mesh_ply(path, vertices, faces, colors=None):
    """A triangle mesh as a binary little-endian PLY: the `vertex` element with float x y z and, where there are colours, uchar red
    green blue = color_to_uint8(colors); the `face` element with `property list uchar int vertex_indices`, three indices each.
    vertices / colors: [Nv, 3]; faces: [Nf, 3] integers (arrays or tensors anywhere; a device tensor is read once)."""
    _write_mesh_ply(path, vertices, faces, colors, None)


def save_mesh_ply_normals(path, vertices, faces, normals=None, colors=None):
    """save_mesh_ply with float nx ny nz after x y z (normals: [Nv, 3], as mesh_ops.vertex_normals gives them); normals=None writes
    the bytes save_mesh_ply writes."""
    _write_mesh_ply(path, vertices, faces, colors, normals)


def _write_mesh_ply(path, vertices, faces, colors, normals):
    host = lambda a: a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)      # noqa: E731
    vertices, faces = host(vertices).astype("<f4").reshape(-1, 3), host(faces).astype("<i4").reshape(-1, 3)
    cols = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")] + ([("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")] if normals is not None else []) + \
        ([("red", "u1"), ("green", "u1"), ("blue", "u1")] if colors is not None else [])
    table = np.empty(vertices.shape[0], dtype=np.dtype(cols))
    for k, name in enumerate("xyz"):
        table[name] = vertices[:, k]
    if normals is not None:
        normals = host(normals).astype("<f4").reshape(-1, 3)
        if normals.shape != vertices.shape:
            raise ValueError(f"save_mesh_ply: the normals are {normals.shape}, the vertices {vertices.shape}")
        for k, name in enumerate(("nx", "ny", "nz")):
            table[name] = normals[:, k]
    if colors is not None:
        colors = color_to_uint8(host(colors)).reshape(-1, 3)
        if colors.shape != vertices.shape:
            raise ValueError(f"save_mesh_ply: the colours are {colors.shape}, the vertices {vertices.shape}")
        for k, name in enumerate(("red", "green", "blue")):
            table[name] = colors[:, k]
    if faces.size and (faces.min() < 0 or faces.max() >= vertices.shape[0]):
        raise ValueError(f"save_mesh_ply: a face names a vertex outside 0 .. {vertices.shape[0] - 1}")
    rows = np.empty(faces.shape[0], dtype=np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    rows["n"], rows["v"] = 3, faces
    kinds = {"<f4": "float", "u1": "uchar"}
    header = "ply\nformat binary_little_endian 1.0\n" + f"element vertex {table.shape[0]}\n" + \
        "".join(f"property {kinds[t]} {n}\n" for n, t in cols) + f"element face {rows.shape[0]}\nproperty list uchar int vertex_indices\nend_header\n"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(table.tobytes())
        f.write(rows.tobytes())


def read_mesh_ply(path, normals=False):
    """(vertices [Nv, 3] float32, faces [Nf, 3] int32, colors [Nv, 3] uint8 or None) of a file save_mesh_ply wrote: binary
    little-endian, scalar vertex properties, then triangles as `list uchar int`.  Anything else is refused.  normals=True: a fourth
    item, the file's nx ny nz as [Nv, 3] float32, or None where it has none."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        fmt, counts, props, element = None, {}, [], None
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: unterminated PLY header")
            tok = line.decode("ascii").split()
            if not tok:
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                element = tok[1]
                counts[element] = int(tok[2])
            elif tok[0] == "property" and element == "vertex":
                if tok[1] == "list":
                    raise ValueError(f"{path}: list properties on the vertex element are not supported")
                props.append((tok[2], _PLY_TYPES[tok[1]]))
            elif tok[0] == "property" and element == "face":
                if tok[1:] != ["list", "uchar", "int", "vertex_indices"]:
                    raise ValueError(f"{path}: the face property must be `list uchar int vertex_indices`")
            elif tok[0] == "end_header":
                break
        if fmt != "binary_little_endian" or list(counts) != ["vertex", "face"]:
            raise ValueError(f"{path}: not a binary little-endian PLY of a vertex and a face element")
        dt, ft = np.dtype(props), np.dtype([("n", "u1"), ("v", "<i4", (3,))])
        raw = f.read()
    if len(raw) != counts["vertex"] * dt.itemsize + counts["face"] * ft.itemsize:
        raise ValueError(f"{path}: {len(raw)} bytes of data do not hold {counts['vertex']} vertices and {counts['face']} triangles")
    table = np.frombuffer(raw, dtype=dt, count=counts["vertex"])
    rows = np.frombuffer(raw, dtype=ft, count=counts["face"], offset=counts["vertex"] * dt.itemsize)
    if (rows["n"] != 3).any():
        raise ValueError(f"{path}: a face that is not a triangle")
    vertices = np.stack([table["x"], table["y"], table["z"]], axis=1).astype(np.float32).reshape(-1, 3)
    colors = np.stack([table["red"], table["green"], table["blue"]], axis=1).reshape(-1, 3) if "red" in table.dtype.names else None
    faces = np.ascontiguousarray(rows["v"], dtype=np.int32).reshape(-1, 3)
    if not normals:
        return vertices, faces, colors
    held = np.stack([table["nx"], table["ny"], table["nz"]], axis=1).astype(np.float32).reshape(-1, 3) if "nx" in table.dtype.names else None
    return vertices, faces, colors, held


def load_ply(path, sh_degree=3, device="cpu"):
    """Raw parameter tensors from a reference-format point_cloud.ply (inverse of save_ply)."""
    v = read_ply_vertices(path)
    n_rest = 3 * ((sh_degree + 1) ** 2 - 1)
    cols = lambda names: np.stack([np.asarray(v[n], dtype=np.float32) for n in names], axis=1)   # noqa: E731
    xyz = cols(["x", "y", "z"])
    f_dc = cols([f"f_dc_{i}" for i in range(3)]).reshape(-1, 3, 1)
    rest_names = [n for n in v.dtype.names if n.startswith("f_rest_")]
    if len(rest_names) != n_rest:
        raise ValueError(f"{path}: {len(rest_names)} f_rest columns, sh_degree {sh_degree} needs {n_rest}")
    f_rest = cols([f"f_rest_{i}" for i in range(n_rest)]).reshape(-1, 3, n_rest // 3)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)                               # noqa: E731
    return dict(xyz=t(xyz), features_dc=t(f_dc).transpose(1, 2).contiguous(), features_rest=t(f_rest).transpose(1, 2).contiguous(),
                opacity=t(cols(["opacity"])), scaling=t(cols([n for n in v.dtype.names if n.startswith("scale_")])),
                rotation=t(cols([n for n in v.dtype.names if n.startswith("rot_")])))


def save_checkpoint(model, optimizer_state, iteration, path):
    """[REF train.py:199-201]"""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    if hasattr(model, "_sync_side_stream"):
        model._sync_side_stream()
    torch.save((model.state_dict(), optimizer_state, iteration), path)


def load_checkpoint(path, args, sh_degree=3, time_input_dim=None, xyz_input_dim=60, device="cpu"):
    """Rebuild a GaussianModel from a reference-format checkpoint [REF train.py:48-57].  Returns
    (model, optimizer_state, iteration)."""
    from .gaussian_model import GaussianModel
    model_params, opt_state, iteration = torch.load(path, map_location=device, weights_only=False)
    if time_input_dim is None:                       # D_in = feature_dim + xyz_input_dim + time_input_dim
        time_input_dim = model_params["df_model.mlp.0.weight"].shape[1] - args.feature_dim - xyz_input_dim
    m = GaussianModel(sh_degree, args)
    m.set_inputDim(time_input_dim, xyz_input_dim)
    kp = model_params.get("super_gaussians")
    m.create_from_tensors(model_params["_xyz"], model_params["_features_dc"], model_params["_features_rest"],
                          model_params["_scaling"], model_params["_rotation"], model_params["_opacity"],
                          model_params["motion_feature"], kp, model_params.get("super_gaussians_feature"),
                          with_weights_model="weights_model.params" in model_params)
    missing, unexpected = m.load_state_dict(model_params, strict=False)
    m.active_sh_degree = m.max_sh_degree
    return m.to(device), opt_state, iteration
