"""GPU: marching cubes (ops.marching_cubes, objnerf_mesh.hip), vis.marching_cubes and Trainer.meshing against the
numpy statement of the extraction (tests/mesh_util.py) and against the reference's own outputs (g16_mesh.npz:
skimage and trainer.py:46-103, made by tests/golden/make_g16_mesh.py)."""
import types

import numpy as np
import pytest
import torch

import mesh_util as U
from openobj_amd import cfg as ocfg
from openobj_amd import ops, render_rays, trainer, vis

pytestmark = pytest.mark.gpu

QUANT = 1024.0


@pytest.fixture(scope="module")
def g16():
    from conftest import load_golden
    return load_golden("g16_mesh")


def mc(vol, level=0.5, gd="ascent"):
    v, f, n = ops.marching_cubes(torch.as_tensor(vol).cuda(), level, gd)
    return v.cpu().numpy(), f.cpu().numpy(), n.cpu().numpy()


def analytic(g, name):
    if f"d_{name}_vol" in g:
        return g[f"d_{name}_vol"]
    return {"sphere": U.vol_sphere, "torus": U.vol_torus}[name]()


def same_as_numpy(vol, level=0.5):
    V, F, N = mc(vol, level)
    v, f, n = U.marching_cubes_np(vol, level)
    assert np.array_equal(F, f)                               # same table, same order
    assert np.array_equal(V, v)                               # same fp32 arithmetic
    assert np.abs(N - n).max() <= 1e-6
    return V, F, N


@pytest.mark.parametrize("name", ["sphere", "torus", "blobs", "noise"])
def test_fixture_volumes_against_skimage(g16, dev, name):
    vol = analytic(g16, name)
    V, F, N = same_as_numpy(vol)
    sv, sn = g16[f"d_{name}_verts"], g16[f"d_{name}_normals"].astype(np.float32)
    nV, nF, chi, area, svol, closed = g16[f"d_{name}_stats"]
    ia, ib = U.match_by_edge(V, sv)
    assert len(ib) == (U.edge_keys(sv) >= 0).sum() == len(V)
    assert np.abs(V[ia] - sv[ib]).max() <= 5e-5
    assert np.sign(U.signed_volume(V, F)) == np.sign(svol)
    if name == "noise":
        d = vol.shape[0]
        be = U.boundary_edges(F)
        on_border = lambda i: ((V[i] <= 1e-6) | (V[i] >= d - 1 - 1e-6)).any(1)
        assert (on_border(be[:, 0]) & on_border(be[:, 1])).all()
        return
    cos = (N[ia] * sn[ib]).sum(1)
    assert cos.min() > 0.99 and cos.mean() > 0.999
    assert U.is_closed_oriented(F) and U.euler(V, F) == chi
    assert abs(U.area(V, F) - area) <= 1e-3 * area
    assert abs(U.signed_volume(V, F) - svol) <= 1e-3 * abs(svol)


@pytest.mark.parametrize("d", [2, 33, 97])
def test_dims_against_numpy(dev, d):
    rng = np.random.default_rng(d)
    vol = rng.random((d, d, d)).astype(np.float32) if d < 97 else U.vol_sphere(d) + 0.02 * rng.random((d, d, d)).astype(np.float32)
    same_as_numpy(vol)


def test_descent_reverses_faces(dev):
    vol = U.vol_sphere(20)
    va, fa, na = mc(vol)
    vd, fd, nd = mc(vol, gd="descent")
    assert np.array_equal(va, vd) and np.array_equal(na, nd) and np.array_equal(fd, fa[:, ::-1])
    with pytest.raises(ValueError):
        ops.marching_cubes(torch.as_tensor(vol).cuda(), 0.5, "sideways")


def test_sphere_512(dev):
    """2^27 points: int64 offsets and a 256 MiB workspace; closed, chi 2, every vertex on the radius."""
    d = 512
    x = torch.arange(d, device=dev, dtype=torch.float32) - (d - 1) / 2.0
    r2 = x[:, None, None] ** 2 + x[None, :, None] ** 2 + x[None, None, :] ** 2
    R = 200.0
    vol = 0.5 + 0.5 * (1.0 - torch.sqrt(r2) / R)
    V, F, N = ops.marching_cubes(vol)
    V, F = V.cpu().numpy().astype(np.float64), F.cpu().numpy()
    assert len(V) > 500000
    assert U.is_closed_oriented(F) and U.euler(V, F) == 2
    rad = np.linalg.norm(V - (d - 1) / 2.0, axis=1)
    assert np.abs(rad - R).max() < 0.01


def test_empty_volumes(dev):
    for vol in (torch.zeros(16, 16, 16), torch.ones(16, 16, 16)):
        V, F, N = ops.marching_cubes(vol.cuda())
        assert V.shape == (0, 3) and F.shape == (0, 3) and N.shape == (0, 3)
        assert vis.marching_cubes(vol) is None
    assert vis.marching_cubes(torch.full((8, 8, 8), 0.7)) is None            # level below the volume's range
    vol = U.vol_sphere(16)
    assert vis.marching_cubes(vol, level=float(vol.max()) + 0.1) is None


def test_values_equal_to_the_level_stay_closed(dev):
    vol = np.round(U.vol_sphere(30) * 8.0) / 8.0                             # many corners exactly at 0.5
    assert (vol == 0.5).sum() > 100
    V, F, N = same_as_numpy(vol.astype(np.float32))
    assert U.is_closed_oriented(F)


def test_bit_reproducible(dev):
    vol = torch.as_tensor(U.vol_noise(40, seed=9)).cuda()
    a = ops.marching_cubes(vol)
    b = ops.marching_cubes(vol)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


def test_vis_marching_cubes_divides_by_dim(dev):
    vol = U.vol_sphere(25)
    m = vis.marching_cubes(vol)
    V, F, N = mc(vol)
    assert np.array_equal(m.vertices, (V / 24).astype(np.float64)) and np.array_equal(m.faces, F)
    m2 = vis.marching_cubes(torch.as_tensor(vol).cuda())
    assert np.array_equal(m2.vertices, m.vertices)


# --- Trainer.meshing ------------------------------------------------------------------------------------------------

def make_trainer(g, tag, dev):
    obj_id, hidden, scale, grid_dim = (int(x) if i != 2 else float(x) for i, x in enumerate(g[f"{tag}_meta"]))
    c = ocfg.Config(ocfg.replica_room0_config(train_device=str(dev)))
    c.obj_id = obj_id
    c.hidden_feature_size = hidden
    c.obj_scale = scale
    t = trainer.Trainer(c)
    with torch.no_grad():
        for i, p in enumerate(t.fc_occ_map.parameters()):
            p.copy_(torch.from_numpy(g[f"{tag}_q{i}"].astype(np.float32) / QUANT))
        t.pe.B_layer.weight.copy_(torch.from_numpy(g[f"{tag}_qB"].astype(np.float32) / QUANT))
    box = types.SimpleNamespace(center=g[f"{tag}_box_center"], R=g[f"{tag}_box_R"], extent=g[f"{tag}_box_extent"])
    return t, box, torch.from_numpy(g[f"{tag}_obj_center"]), grid_dim


def our_grid_occ(t, box, obj_center, grid_dim, dev):
    scene_scale = np.asarray(box.extent) / (2.0 * t.bound_extent)
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = box.center
    T[:3, :3] = box.R
    pc = render_rays.make_3D_grid([-1., 1.], grid_dim, dev, scale=torch.from_numpy(scene_scale).float(),
                                  transform=torch.from_numpy(T)).view(-1, 3)
    pc -= obj_center.to(dev)
    return t._eval_grid(pc)[0]


def directed_dist(a, b):
    a, b = torch.as_tensor(a).cuda().double(), torch.as_tensor(b).cuda().double()
    return torch.cat([torch.cdist(x, b).min(1).values for x in a.split(2048)]).cpu().numpy()


def near_level(V_idx, occ, tol=2e-5):
    """Vertices on a lattice edge with an endpoint within tol of the level (the edges a 1e-5 difference in the volume
    may add or remove), and vertices on no single lattice edge."""
    v = np.asarray(V_idx, np.float64)
    nonint = np.abs(v - np.round(v)) > 1e-6
    a = np.argmax(nonint, axis=1)
    p = np.round(v).astype(np.int64)
    p[np.arange(len(v)), a] = np.floor(v[np.arange(len(v)), a]).astype(np.int64)
    q = p.copy()
    o = np.asarray(occ)
    q[np.arange(len(v)), a] = np.minimum(q[np.arange(len(v)), a] + 1, o.shape[0] - 1)
    at = lambda x: o[x[:, 0], x[:, 1], x[:, 2]]
    off_edge = nonint.sum(1) != 1      # on a lattice point (t rounds to 0 or 1), or one of skimage's cell-interior vertices
    return off_edge | (np.abs(at(p) - 0.5) < tol) | (np.abs(at(q) - 0.5) < tol)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_trainer_meshing_against_reference(g16, dev, tag):
    g = g16
    t, box, oc, grid_dim = make_trainer(g, tag, dev)
    occ = our_grid_occ(t, box, oc, grid_dim, dev)
    ref_occ = g[f"{tag}_occ"]
    assert np.abs(occ.cpu().numpy().reshape(ref_occ.shape) - ref_occ).max() <= 1e-5
    # the fixture volume through vis.marching_cubes and the transforms gives the reference's final vertices
    m = vis.marching_cubes(ref_occ)
    m.apply_translation([-0.5, -0.5, -0.5])
    m.apply_scale(2)
    m.apply_scale(np.asarray(box.extent) / (2.0 * t.bound_extent))
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = box.center
    T[:3, :3] = box.R
    m.apply_transform(T)
    n_ours = m.vertices.shape[0]
    V_idx, _, _ = mc(ref_occ)
    ia, ib = U.match_by_edge(V_idx, g[f"{tag}_sk_verts"])
    # every vertex with an edge key is matched; a vertex within 1e-5 of a lattice point has no key (at most a few)
    keyed = U.edge_keys(V_idx) >= 0
    assert len(ia) == keyed.sum()
    assert n_ours - keyed.sum() <= 3
    ref_v = g[f"{tag}_verts"].astype(np.float64)
    ext = float(np.max(box.extent))
    assert np.abs(m.vertices[ia] - ref_v[ib]).max() <= 1e-5 * ext
    # end to end on our own volume
    pcd, mesh, part = t.meshing(box, oc, grid_dim=grid_dim, save_pcd=False, save_mesh=True, if_color=True, if_part=True)
    assert pcd is None
    nV, nF = (int(x) for x in g[f"{tag}_sk_VF"])
    assert abs(len(mesh.vertices) - nV) <= 0.005 * nV and abs(len(mesh.faces) - nF) <= 0.005 * nF
    # symmetric Hausdorff distance of the vertex sets, leaving out the vertices of edges whose endpoint lies within
    # 2e-5 of the level (there the two volumes, <= 1e-5 apart, may classify a corner differently) and skimage's
    # cell-interior vertices (its MC33 tiling; ours has none)
    V_own, _, _ = mc(occ.view(grid_dim, grid_dim, grid_dim))
    occ_np = occ.cpu().numpy().reshape(ref_occ.shape)
    keep_own = ~near_level(V_own, occ_np)
    keep_ref = ~near_level(g[f"{tag}_sk_verts"], ref_occ)
    assert keep_own.mean() > 0.99 and keep_ref.mean() > 0.99
    assert directed_dist(mesh.vertices[keep_own], ref_v).max() <= 1e-3 * ext
    assert directed_dist(ref_v[keep_ref], mesh.vertices).max() <= 1e-3 * ext
    ja, jb = U.match_by_edge(V_own, g[f"{tag}_sk_verts"])
    col = mesh.visual.vertex_colors
    assert col.dtype == np.uint8 and col.shape == (len(mesh.vertices), 4)
    assert np.abs(col[ja, :3].astype(int) - g[f"{tag}_colors"][jb, :3].astype(int)).max() <= 1
    assert part.shape == (len(mesh.vertices), 512)
    pick = g[f"{tag}_part_idx"]
    pos = {int(k): i for k, i in zip(jb, ja)}
    sel = [(pos[int(p)], n) for n, p in enumerate(pick) if int(p) in pos]
    assert len(sel) >= 0.9 * len(pick)
    ours = part[torch.tensor([s for s, _ in sel])].cpu().numpy()
    ref = g[f"{tag}_part_feat"][[n for _, n in sel]]
    assert np.abs(ours - ref).max() <= 1e-4


def test_trainer_meshing_pcd_branch(g16, dev):
    """The save_pcd branch (trainer.py:69-77) point for point: the occupied grid points (after `grid_pc -=
    obj_center`) and their colours, except at grid points within 1e-5 of the level in either volume."""
    g = g16
    t, box, oc, grid_dim = make_trainer(g, "a", dev)
    pcd, mesh, part = t.meshing(box, oc, grid_dim=grid_dim, save_pcd=True)
    assert mesh is None and part is None
    occ = our_grid_occ(t, box, oc, grid_dim, dev).cpu().numpy()
    ref_occ = g["a_occ"].ravel()
    near = (np.abs(occ - 0.5) < 1e-5) | (np.abs(ref_occ - 0.5) < 1e-5)
    ours_idx = np.nonzero(occ > 0.5)[0]                       # grid index of each row of pcd
    ref_idx = np.nonzero(ref_occ > 0.5)[0]                    # ... of each row of the reference's point cloud
    assert len(ref_idx) == int(g["c_n"][0]) and len(pcd.points) == len(ours_idx)
    assert near[np.setxor1d(ours_idx, ref_idx)].all()          # the occupied sets differ only at near points
    stored = ref_idx[::4]                                     # the rows the fixture keeps (every 4th)
    keep = ~near[stored]
    assert keep.sum() >= len(stored) - 2
    row = np.searchsorted(ours_idx, stored[keep])
    assert np.array_equal(ours_idx[row], stored[keep])
    assert np.abs(pcd.points[row] - g["c_points"][keep]).max() <= 1e-5
    assert np.abs(pcd.colors[row] - g["c_colors"][keep]).max() <= 1e-5


def test_trainer_meshing_return_shapes(g16, dev):
    g = g16
    t, box, oc, grid_dim = make_trainer(g, "a", dev)
    assert t.meshing(box, oc, grid_dim=grid_dim, save_pcd=False, save_mesh=False) == (None, None, None)
    pcd, mesh, part = t.meshing(box, oc, grid_dim=grid_dim, save_pcd=False, save_mesh=True)
    assert pcd is None and part is None and mesh.visual.has_colors is False
    with torch.no_grad():
        t.fc_occ_map.out_alpha.bias.fill_(1e4)          # every grid point occupied: occ == 1, no surface
    assert t.meshing(box, oc, grid_dim=grid_dim, save_pcd=False, save_mesh=True) is None
    with torch.no_grad():
        t.fc_occ_map.out_alpha.bias.fill_(-1e4)         # an all-empty network
    assert t.meshing(box, oc, grid_dim=grid_dim) == (None, None)


def test_map_vis_export(g16, dev, tmp_path):
    """python -m openobj_amd.map_vis over mapper-style checkpoints: two objects with boxes, one without."""
    import gzip
    import pickle
    from openobj_amd import map_vis
    from openobj_amd.mesh import read_ply
    t, box, oc, _ = make_trainer(g16, "a", dev)
    box2 = types.SimpleNamespace(center=box.center + 0.05, R=box.R, extent=box.extent * 1.1)
    for obj_id, b in ((1, box), (2, box2), (3, None)):
        d = tmp_path / "ckpt" / str(obj_id)
        d.mkdir(parents=True)
        torch.save({"epoch": 5, "FC_state_dict": t.fc_occ_map.state_dict(), "PE_state_dict": t.pe.state_dict(),
                    "obj_id": obj_id, "bbox": b, "obj_scale": t.obj_scale, "clip_feat": np.full(4, obj_id, np.float32),
                    "caption_feat": np.zeros(4, np.float32), "semantic_id": 10 + obj_id}, str(d / f"obj_{obj_id}.pth"))
    map_vis.main(["--logdir", str(tmp_path), "--grid-dim", "24", "--device", str(dev)])
    with gzip.open(tmp_path / "map_vis.pkl.gz", "rb") as f:
        objs = pickle.load(f)
    assert sorted(objs) == [1, 2]
    for obj_id, o in objs.items():
        assert sorted(o) == sorted(["clip_feat", "caption_feat", "class_id", "mesh", "color", "part_feat"])
        V = len(o["mesh"].vertices)
        assert V > 100 and o["color"].shape == (V, 4) and o["color"].dtype == np.uint8
        assert o["part_feat"].shape == (V, 512)
        assert np.allclose(np.linalg.norm(o["part_feat"], axis=1), 1.0, atol=1e-5)
        assert o["class_id"] == 10 + obj_id and o["clip_feat"][0] == obj_id
        v, n, c, f = read_ply(str(tmp_path / "map_vis" / f"obj_{obj_id}.ply"))
        assert len(v) == V and np.array_equal(f, o["mesh"].faces)
    assert not (tmp_path / "map_vis" / "obj_3.ply").exists()
