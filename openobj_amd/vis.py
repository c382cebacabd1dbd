"""vis.marching_cubes (vis.py:6-22): skimage.measure.marching_cubes(occupancy, level, gradient_direction='ascent') ->
trimesh.Trimesh with the vertices divided by (dim - 1), here on the GPU (ops.marching_cubes, objnerf_mesh.hip) and
returning a mesh.TriMesh."""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .mesh import TriMesh


def marching_cubes(occupancy, level=0.5, device="cuda:0"):
    """occupancy: [d,d,d] device tensor or numpy array.  None exactly where the reference's try/except returns None:
    skimage's ValueError (level outside [min, max] of the volume) and RuntimeError (no vertex)."""
    vol = occupancy if torch.is_tensor(occupancy) else torch.from_numpy(np.ascontiguousarray(occupancy))
    if not vol.is_cuda:
        vol = vol.to(device)
    vol = vol.float()
    lo, hi = (float(x) for x in torch.aminmax(vol))
    if level < lo or level > hi:
        return None
    verts, faces, normals = ops.marching_cubes(vol, level, gradient_direction="ascent")
    if verts.shape[0] == 0:
        return None
    dim = vol.shape[0]
    vertices = verts.cpu().numpy() / (dim - 1)          # float32 / int, as the reference divides skimage's output
    return TriMesh(vertices=vertices, faces=faces.cpu().numpy(), vertex_normals=normals.cpu().numpy())
