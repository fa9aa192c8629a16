"""csrc/gp_mesh.h restated in numpy: the components by a plain union of the definition (not the device's hooking rounds), the filter
by boolean masks and cumulative sums, the normals in float32 one operation at a time with the incidences of a vertex added one after
the other in ascending 3 f + corner."""
import numpy as np

F = np.float32


def good_faces(faces, nv):
    """[Nf] bool: every index of the face lies in [0, nv)."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    return ((faces >= 0) & (faces < nv)).all(axis=1)


def components(faces, nv):
    """(status, vertex_label [nv], face_label [nf], labels [C], vertex_counts [C], face_counts [C]), int32: the definition, by union."""
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    good = good_faces(faces, nv)
    root = list(range(nv))

    def find(v):
        while root[v] != v:
            root[v] = root[root[v]]
            v = root[v]
        return v

    for a, b, c in faces[good].tolist():
        for u, v in ((a, b), (b, c)):
            ru, rv = find(u), find(v)
            if ru != rv:
                root[max(ru, rv)] = min(ru, rv)          # the smaller index stays the root: the root is the component's smallest
    vertex_label = np.array([find(v) for v in range(nv)], np.int32).reshape(nv)
    face_label = np.full(len(faces), -1, np.int32)
    face_label[good] = vertex_label[faces[good, 0]]
    labels = np.flatnonzero(vertex_label == np.arange(nv)).astype(np.int32)
    vertex_counts = np.bincount(vertex_label, minlength=max(nv, 1))[labels].astype(np.int32)
    face_counts = np.bincount(face_label[good], minlength=max(nv, 1))[labels].astype(np.int32)
    return int(not good.all()), vertex_label, face_label, labels, vertex_counts, face_counts


def kept_labels(labels, face_counts, min_triangles=None, keep_largest=None):
    """[C] bool, the rule of gp_mesh.h."""
    keep = face_counts >= 1
    if min_triangles is not None:
        keep &= face_counts >= min_triangles
    if keep_largest is not None:
        order = np.lexsort((labels, -face_counts.astype(np.int64)))          # most faces first, ties to the smaller label
        among = np.zeros(len(labels), bool)
        among[order[:keep_largest]] = True
        keep &= among
    return keep


def filter_components(vertices, faces, rows, min_triangles=None, keep_largest=None):
    """(status, vertices', faces', vertex_index, face_index, [rows']): rows is a list of [nv, k] arrays that follow the vertices."""
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    nv = len(vertices)
    status, vertex_label, face_label, labels, _, face_counts = components(faces, nv)
    keep_label = np.zeros(max(nv, 1), bool)
    keep_label[labels] = kept_labels(labels, face_counts, min_triangles, keep_largest)
    keep_vertex = keep_label[vertex_label] if nv else np.zeros(0, bool)
    good = good_faces(faces, nv)
    keep_face = np.zeros(len(faces), bool)
    keep_face[good] = keep_vertex[faces[good]].all(axis=1)
    new_id = np.cumsum(keep_vertex) - 1
    return (status, vertices[keep_vertex], new_id[faces[keep_face]].astype(np.int32).reshape(-1, 3), np.flatnonzero(keep_vertex).astype(np.int32),
            np.flatnonzero(keep_face).astype(np.int32), [np.asarray(r)[keep_vertex] for r in rows])


def face_vectors(vertices, faces):
    """[Nf, 3] float32: (b - a) x (c - a), zeros for a face with an index out of range."""
    vertices, faces = np.asarray(vertices, F).reshape(-1, 3), np.asarray(faces, np.int32).reshape(-1, 3)
    good = good_faces(faces, len(vertices))
    out = np.zeros((len(faces), 3), F)
    a, b, c = (vertices[faces[good, k]] for k in range(3))
    with np.errstate(all="ignore"):
        e1, e2 = b - a, c - a
        out[good, 0] = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        out[good, 1] = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        out[good, 2] = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    return out


def vertex_normals(vertices, faces):
    """[Nv, 3] float32."""
    vertices, faces = np.asarray(vertices, F).reshape(-1, 3), np.asarray(faces, np.int32).reshape(-1, 3)
    nv = len(vertices)
    fv = face_vectors(vertices, faces)
    good = np.repeat(good_faces(faces, nv), 3)
    ids = np.flatnonzero(good)                           # incidences 3 f + corner, ascending
    vertex = faces.reshape(-1)[ids].astype(np.int64)
    order = np.argsort(vertex, kind="stable")
    ids, vertex = ids[order], vertex[order]
    first = np.searchsorted(vertex, vertex, side="left")
    turn = np.arange(len(ids)) - first                   # the how-manieth incidence of its vertex
    total = np.zeros((nv, 3), F)
    by_turn = np.argsort(turn, kind="stable")
    bounds = np.searchsorted(turn[by_turn], np.arange(int(turn.max()) + 2 if len(turn) else 1))
    with np.errstate(all="ignore"):
        for k in range(len(bounds) - 1):                 # one incidence per vertex and turn: every addition is a single float32 one
            sel = by_turn[bounds[k]:bounds[k + 1]]
            total[vertex[sel]] = total[vertex[sel]] + fv[ids[sel] // 3]
        x, y, z = total[:, 0], total[:, 1], total[:, 2]
        length = np.sqrt((x * x + y * y) + z * z)
        ok = np.isfinite(length) & (length > 0)
        out = np.zeros((nv, 3), F)
        out[ok] = total[ok] / length[ok, None]
    return out
