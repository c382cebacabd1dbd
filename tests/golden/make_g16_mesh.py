#!/usr/bin/env python3
"""Generate g16_mesh.npz by RUNNING the reference's Trainer.meshing (trainer.py:46-103) and skimage's marching cubes.

Run in the build container only (it needs /root/reference and scikit-image, neither of which travels):

    python tests/golden/make_g16_mesh.py

scikit-image is imported for real; if this interpreter has none, SKIMAGE_PYTHON names another interpreter that has
it, and every marching_cubes call is run there on the same float32 volume (only arrays cross).  open3d is stubbed
with a point-cloud stand-in that keeps its points / colours, trimesh with a recording stand-in that implements the
three apply_* calls and `visual`; the rest of the reference's GUI imports are MagicMock stubs as in make_golden.py.

Cases:
  a   hidden-32 object (obj_id 1), seeded init with the alpha bias shifted, rotated non-cubic box, grid_dim 32,
      save_mesh + if_color + if_part: parameters (on a 2^-10 grid, as int16), occupancy volume, skimage's vertices
      and V / F, the final vertices, colours, the part features of 32 vertices picked by edge key
  b   the same for the hidden-128 background network (obj_id 0), grid_dim 24
  c   the save_pcd branch of (a): the point count, every 4th point and colour
  d   analytic volumes given straight to skimage: sphere (d = 33), torus (genus 1), two touching blobs, 12^3 noise:
      skimage's vertices and normals (fp16), V, F, Euler characteristic, area, signed volume, closedness
"""
import os
import subprocess
import sys
import tempfile
import types
from unittest.mock import MagicMock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference/objnerf"
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

try:                                                       # the real skimage first, before any stub
    import skimage.measure as _skm
    _SK_PY = None
except ImportError:
    _skm = None
    _SK_PY = os.environ.get("SKIMAGE_PYTHON")
    if not _SK_PY:
        raise SystemExit("scikit-image is not importable here: set SKIMAGE_PYTHON to an interpreter that has it")

_SK_SCRIPT = """
import sys, numpy as np, skimage.measure as m
d = np.load(sys.argv[1])
v, f, n, _ = m.marching_cubes(d["vol"], float(d["level"]), gradient_direction=str(d["gd"]))
np.savez(sys.argv[2], v=v, f=f, n=n)
"""


def sk_marching_cubes(vol, level=0.5, gradient_direction="ascent"):
    """skimage.measure.marching_cubes -> (verts, faces, normals, values); raises as skimage does."""
    vol = np.ascontiguousarray(vol, np.float32)
    if _skm is not None:
        return _skm.marching_cubes(vol, level, gradient_direction=gradient_direction)
    if level < vol.min() or level > vol.max():
        raise ValueError("Surface level must be within volume data range.")
    with tempfile.TemporaryDirectory() as tmp:
        a, b = os.path.join(tmp, "in.npz"), os.path.join(tmp, "out.npz")
        np.savez(a, vol=vol, level=np.float64(level), gd=np.array(gradient_direction))
        r = subprocess.run([_SK_PY, "-c", _SK_SCRIPT, a, b], capture_output=True, text=True)
        if r.returncode != 0:
            if "No surface found" in r.stderr:
                raise RuntimeError("No surface found at the given iso value.")
            raise SystemExit(r.stderr)
        o = np.load(b)
        return o["v"], o["f"], o["n"], None


RECORD = {}


class RecMesh:
    """trimesh.Trimesh stand-in: keeps what the reference gives it and applies the three transforms."""

    def __init__(self, vertices, faces, vertex_normals=None):
        self.vertices = np.asarray(vertices, np.float64)
        self.faces = np.asarray(faces)
        self.vertex_normals = vertex_normals
        self.visual = types.SimpleNamespace(vertex_colors=None)

    def apply_translation(self, t):
        self.vertices = self.vertices + np.asarray(t, np.float64)

    def apply_scale(self, s):
        m = np.eye(4)
        m[:3, :3] = np.diag(np.broadcast_to(np.asarray(s, np.float64), (3,)))
        self.apply_transform(m)

    def apply_transform(self, m):
        m = np.asarray(m, np.float64)
        self.vertices = self.vertices @ m[:3, :3].T + m[:3, 3]


def _mc_stub(vol, level=0.5, gradient_direction="ascent", **kw):
    out = sk_marching_cubes(vol, level, gradient_direction)
    RECORD["vol"] = np.asarray(vol, np.float32).copy()
    RECORD["sk"] = out[:3]
    return out


class _PCD:
    def __init__(self):
        self.points = self.colors = None

    def voxel_down_sample(self, voxel_size):
        return self


skm = types.ModuleType("skimage.measure")
skm.marching_cubes = _mc_stub
sk = types.ModuleType("skimage")
sk.measure = skm
tm = types.ModuleType("trimesh")
tm.Trimesh = RecMesh
o3d = MagicMock()
o3d.geometry.PointCloud = _PCD
o3d.utility.Vector3dVector = lambda x: np.asarray(x)
sys.modules.update({"skimage": sk, "skimage.measure": skm, "trimesh": tm, "open3d": o3d})
for name in ["cv2", "imgviz", "bidict", "matplotlib", "matplotlib.pyplot"]:
    sys.modules.setdefault(name, MagicMock())
sys.path.insert(0, REF)

import trainer as ref_trainer          # noqa: E402
import mesh_util as U                  # noqa: E402


QUANT = 1024.0
N_PART = 32


def make_cfg(obj_id, hidden, scale):
    return types.SimpleNamespace(obj_id=obj_id, training_device="cpu", hidden_feature_size=hidden,
                                 clip_point_feature_size=512, obj_scale=scale, n_unidir_funcs=5, W=1200, H=680)


def rot(a, b, c):
    ca, sa, cb, sb, cc, sc = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(c), np.sin(c)
    Rz = np.array([[ca, -sa, 0], [sa, ca, 0], [0, 0, 1]])
    Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    Rx = np.array([[1, 0, 0], [0, cc, -sc], [0, sc, cc]])
    return Rz @ Ry @ Rx


def run_case(out, tag, obj_id, hidden, scale, grid_dim, seed, box, obj_center):
    torch.manual_seed(seed)
    t = ref_trainer.Trainer(make_cfg(obj_id, hidden, scale))
    with torch.no_grad():                   # weights on a 2^-10 grid: stored exactly as int16, compressed small
        for p in list(t.fc_occ_map.parameters()) + [t.pe.B_layer.weight]:
            p.copy_(torch.round(p * QUANT) / QUANT)
    # shift the alpha bias until 5-50 % of the grid is occupied
    chosen = None
    for shift in [0.0, 0.5, -0.5, 1.0, -1.0, 1.5, -1.5, 2.0, -2.0, 3.0, -3.0]:
        with torch.no_grad():
            t.fc_occ_map.out_alpha.bias.add_(shift)
        RECORD.clear()
        r = t.meshing(box, obj_center, grid_dim=grid_dim, save_pcd=False, save_mesh=True, if_color=True, if_part=True)
        frac = float((RECORD["vol"] > 0.5).mean()) if "vol" in RECORD else 0.0
        if r is not None and r[1] is not None and 0.05 <= frac <= 0.5:
            chosen = shift
            break
        with torch.no_grad():
            t.fc_occ_map.out_alpha.bias.add_(-shift)
    assert chosen is not None, tag
    _, mesh, partfeat = r
    print(f"{tag}: alpha bias shift {chosen}, occupied {frac:.3f}, V {len(mesh.vertices)}, F {len(mesh.faces)}")
    for i, p in enumerate(t.fc_occ_map.parameters()):
        out[f"{tag}_q{i}"] = torch.round(p.detach() * QUANT).numpy().astype(np.int16)       # p = q / QUANT exactly
    out[f"{tag}_qB"] = torch.round(t.pe.B_layer.weight.detach() * QUANT).numpy().astype(np.int16)
    out[f"{tag}_occ"] = RECORD["vol"]
    v, f, n = RECORD["sk"]
    out[f"{tag}_sk_verts"] = v.astype(np.float32)
    out[f"{tag}_sk_VF"] = np.array([len(v), len(f)], np.int64)
    out[f"{tag}_verts"] = mesh.vertices.astype(np.float32)
    out[f"{tag}_colors"] = np.asarray(mesh.visual.vertex_colors)
    keys = U.edge_keys(v)
    cand = np.nonzero(keys >= 0)[0]
    pick = cand[np.argsort(keys[cand], kind="stable")][:: max(1, len(cand) // N_PART)][:N_PART]
    out[f"{tag}_part_idx"] = pick.astype(np.int64)
    out[f"{tag}_part_feat"] = partfeat[torch.from_numpy(pick)].numpy().astype(np.float32)
    out[f"{tag}_meta"] = np.array([obj_id, hidden, scale, grid_dim], np.float64)
    out[f"{tag}_box_center"], out[f"{tag}_box_R"], out[f"{tag}_box_extent"] = box.center, box.R, box.extent
    out[f"{tag}_obj_center"] = obj_center.numpy()
    return t


def main():
    out = {}
    box_a = types.SimpleNamespace(center=np.array([0.30, -0.20, 0.50]), R=rot(0.4, -0.3, 0.2),
                                  extent=np.array([1.2, 0.8, 1.0]))
    t = run_case(out, "a", 1, 32, 2.0, 32, 3, box_a, torch.tensor([0.28, -0.18, 0.46]))
    # (c): the save_pcd branch of (a), same network
    pcd, m, pf = t.meshing(box_a, torch.tensor([0.28, -0.18, 0.46]), grid_dim=32, save_pcd=True)
    assert m is None and pf is None
    pts = np.asarray(pcd.points, np.float32)
    out["c_n"] = np.array([len(pts)], np.int64)
    out["c_points"] = pts[::4]                               # every 4th point of the reference's order
    out["c_colors"] = np.asarray(pcd.colors, np.float32)[::4]
    box_b = types.SimpleNamespace(center=np.array([0.1, 0.2, -0.1]), R=rot(-0.2, 0.15, 0.5),
                                  extent=np.array([4.0, 3.0, 2.5]))
    run_case(out, "b", 0, 128, 5.0, 24, 7, box_b, torch.tensor([0.0, 0.0, 0.0]))
    # (d): analytic volumes straight to skimage
    # sphere and torus are regenerated by the tests (sqrt and + - * / are correctly rounded: the same bits on any
    # machine; the tests check the stored checksum); blobs (exp) and noise travel as data
    for name, vol in [("sphere", U.vol_sphere()), ("torus", U.vol_torus()), ("blobs", U.vol_blobs()),
                      ("noise", U.vol_noise())]:
        v, f, n, _ = sk_marching_cubes(vol, 0.5, "ascent")
        if name in ("blobs", "noise"):
            out[f"d_{name}_vol"] = vol
        out[f"d_{name}_sum"] = np.array([vol.astype(np.float64).sum()])
        out[f"d_{name}_verts"], out[f"d_{name}_normals"] = v.astype(np.float32), n.astype(np.float16)
        closed = U.is_closed_oriented(f) if name != "noise" else False
        out[f"d_{name}_stats"] = np.array([len(v), len(f), U.euler(v, f), U.area(v, f), U.signed_volume(v, f),
                                           float(closed)], np.float64)
        fd = sk_marching_cubes(vol, 0.5, "descent")[1]
        assert np.array_equal(fd, f[:, ::-1])
        print(f"d_{name}: V {len(v)} F {len(f)}")
    path = os.path.join(HERE, "g16_mesh.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
