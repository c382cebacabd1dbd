"""numpy mesh containers for Trainer.meshing / vis.marching_cubes (trainer.py:46-103, vis.py:6-22).

The reference returns trimesh.Trimesh and open3d.geometry.PointCloud objects.  Neither package is a dependency of
this project, so these classes carry the part of their interface the reference's meshing path uses:
TriMesh.apply_translation / apply_scale / apply_transform, .vertices, .faces, .vertex_normals,
.visual.vertex_colors and export(); PointCloud.points / .colors.

TriMesh does not process its input (trimesh's default merges duplicate vertices; marching cubes output is already
welded).  Normals are transformed by the inverse transpose of the linear part and renormalised, and the faces are
flipped when that part has a negative determinant, which is trimesh's documented behaviour; trimesh is not
installed where the fixtures were made, so no fixture pins this part.
"""
from __future__ import annotations

import numpy as np


class _Visual:
    """trimesh's ColorVisuals, vertex colours only: stored RGBA uint8 [V, 4], alpha 255 unless given."""

    def __init__(self, n: int):
        self._n = n
        self._colors = None

    @property
    def vertex_colors(self) -> np.ndarray:
        if self._colors is None:
            return np.tile(np.array([102, 102, 102, 255], np.uint8), (self._n, 1))     # trimesh's default grey
        return self._colors

    @vertex_colors.setter
    def vertex_colors(self, c) -> None:
        c = np.asarray(c)
        if c.ndim != 2 or c.shape[0] != self._n or c.shape[1] not in (3, 4):
            raise ValueError(f"vertex_colors: expected [{self._n}, 3 or 4], got {c.shape}")
        if c.dtype != np.uint8:
            c = (c * 255 if np.issubdtype(c.dtype, np.floating) else c).astype(np.uint8)
        if c.shape[1] == 3:
            c = np.concatenate([c, np.full((self._n, 1), 255, np.uint8)], axis=1)
        self._colors = np.ascontiguousarray(c)

    @property
    def has_colors(self) -> bool:
        return self._colors is not None


class TriMesh:
    def __init__(self, vertices, faces, vertex_normals=None):
        self.vertices = np.ascontiguousarray(vertices, np.float64)
        self.faces = np.ascontiguousarray(faces, np.int64).reshape(-1, 3)
        self.vertex_normals = None if vertex_normals is None else np.ascontiguousarray(vertex_normals, np.float64)
        self.visual = _Visual(len(self.vertices))

    def __len__(self) -> int:
        return len(self.vertices)

    def apply_translation(self, t) -> "TriMesh":
        self.vertices = self.vertices + np.asarray(t, np.float64).reshape(3)
        return self

    def apply_scale(self, s) -> "TriMesh":
        """Scalar or per-axis scale about the origin."""
        s = np.asarray(s, np.float64)
        m = np.eye(4)
        m[:3, :3] = np.diag(np.broadcast_to(s, (3,)))
        return self.apply_transform(m)

    def apply_transform(self, m) -> "TriMesh":
        m = np.asarray(m, np.float64).reshape(4, 4)
        lin = m[:3, :3]
        self.vertices = self.vertices @ lin.T + m[:3, 3]
        if self.vertex_normals is not None:
            n = self.vertex_normals @ np.linalg.inv(lin)          # (inverse transpose) applied to row vectors
            norm = np.linalg.norm(n, axis=1, keepdims=True)
            self.vertex_normals = n / np.where(norm > 0, norm, 1.0)
        if np.linalg.det(lin) < 0:
            self.faces = np.ascontiguousarray(self.faces[:, ::-1])
        return self

    def export(self, path: str) -> None:
        """.obj (text: v / vn / f, colours as the common 'v x y z r g b' extension) or binary little-endian .ply
        (float vertices, uchar RGBA colours when set, int32 faces)."""
        if path.endswith(".obj"):
            _write_obj(self, path)
        elif path.endswith(".ply"):
            _write_ply(self, path)
        else:
            raise ValueError(f"export: unsupported extension in {path} (.obj or .ply)")


class PointCloud:
    """open3d.geometry.PointCloud as the save_pcd branch fills it: points [N,3], colors [N,3] in [0, 1]."""

    def __init__(self, points, colors=None):
        self.points = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
        self.colors = None if colors is None else np.ascontiguousarray(colors, np.float64).reshape(-1, 3)

    def __len__(self) -> int:
        return len(self.points)


def _write_obj(m: TriMesh, path: str) -> None:
    with open(path, "w") as f:
        if m.visual.has_colors:
            c = m.visual.vertex_colors[:, :3] / 255.0
            for v, cc in zip(m.vertices, c):
                f.write(f"v {v[0]:.8g} {v[1]:.8g} {v[2]:.8g} {cc[0]:.6g} {cc[1]:.6g} {cc[2]:.6g}\n")
        else:
            for v in m.vertices:
                f.write(f"v {v[0]:.8g} {v[1]:.8g} {v[2]:.8g}\n")
        if m.vertex_normals is not None:
            for n in m.vertex_normals:
                f.write(f"vn {n[0]:.8g} {n[1]:.8g} {n[2]:.8g}\n")
            for a, b, c in m.faces + 1:
                f.write(f"f {a}//{a} {b}//{b} {c}//{c}\n")
        else:
            for a, b, c in m.faces + 1:
                f.write(f"f {a} {b} {c}\n")


def _write_ply(m: TriMesh, path: str) -> None:
    col = m.visual.has_colors
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(m.vertices)}",
            "property float x", "property float y", "property float z"]
    if m.vertex_normals is not None:
        head += ["property float nx", "property float ny", "property float nz"]
    if col:
        head += ["property uchar red", "property uchar green", "property uchar blue", "property uchar alpha"]
    head += [f"element face {len(m.faces)}", "property list uchar int vertex_indices", "end_header"]
    fields = [("xyz", "<f4", (3,))]
    if m.vertex_normals is not None:
        fields.append(("n", "<f4", (3,)))
    if col:
        fields.append(("rgba", "u1", (4,)))
    v = np.zeros(len(m.vertices), dtype=fields)
    v["xyz"] = m.vertices
    if m.vertex_normals is not None:
        v["n"] = m.vertex_normals
    if col:
        v["rgba"] = m.visual.vertex_colors
    f = np.zeros(len(m.faces), dtype=[("k", "u1"), ("i", "<i4", (3,))])
    f["k"] = 3
    f["i"] = m.faces
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        fh.write(v.tobytes())
        fh.write(f.tobytes())


def read_ply(path: str):
    """Reads back what TriMesh.export writes to .ply: (vertices [V,3] f4, normals or None, rgba or None, faces)."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").splitlines()
    nv = int(next(l for l in head if l.startswith("element vertex")).split()[-1])
    nf = int(next(l for l in head if l.startswith("element face")).split()[-1])
    fields = [("xyz", "<f4", (3,))]
    if "property float nx" in head:
        fields.append(("n", "<f4", (3,)))
    if "property uchar red" in head:
        fields.append(("rgba", "u1", (4,)))
    v = np.frombuffer(data, dtype=fields, count=nv, offset=end)
    f = np.frombuffer(data, dtype=[("k", "u1"), ("i", "<i4", (3,))], count=nf, offset=end + v.nbytes)
    assert (f["k"] == 3).all()
    names = v.dtype.names
    return (v["xyz"].copy(), v["n"].copy() if "n" in names else None, v["rgba"].copy() if "rgba" in names else None,
            f["i"].astype(np.int64))


__all__ = ["TriMesh", "PointCloud", "read_ply"]
