"""CPU: the marching-cubes case table that ships in libobjnerf_hip.so (objnerf_mc_tables), the numpy statement of the
extraction against skimage's fixture meshes (g16_mesh.npz, tests/golden/make_g16_mesh.py), and the host mesh types
(openobj_amd/mesh.py)."""
import importlib.util
import os

import numpy as np
import pytest

import mesh_util as U
from conftest import ROOT, load_golden
from openobj_amd.mesh import PointCloud, TriMesh, read_ply

@pytest.fixture(scope="module")
def tables():
    return U.shipped_tables()


@pytest.fixture(scope="module")
def g16():
    return load_golden("g16_mesh")


def case_tris(tables, c):
    _, _, nt, tri = tables
    return [tuple(int(e) for e in tri[c, 3 * k:3 * k + 3]) for k in range(int(nt[c]))]


def edge_corners(tables, e):
    c0, ax, _, _ = tables
    return int(c0[e]), int(c0[e]) | (1 << int(ax[e]))


def faces_of_cube():
    """(axis, side) -> the 4 corners of that cube face."""
    return {(a, s): [c for c in range(8) if ((c >> a) & 1) == s] for a in range(3) for s in range(2)}


def test_table_matches_generator():
    spec = importlib.util.spec_from_file_location("gen_mc_tables", os.path.join(ROOT, "tools", "gen_mc_tables.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    assert open(g.OUT).read() == g.render(g.build())


def test_edges_are_the_cube_edges(tables):
    seen = set()
    for e in range(12):
        a, b = edge_corners(tables, e)
        assert bin(a ^ b).count("1") == 1 and a < b
        seen.add((a, b))
    assert len(seen) == 12


def test_triangles_use_crossing_edges_only(tables):
    for c in range(256):
        for tri in case_tris(tables, c):
            assert len(set(tri)) == 3
            for e in tri:
                a, b = edge_corners(tables, e)
                assert ((c >> a) & 1) != ((c >> b) & 1), (c, tri)
        crossing = {e for e in range(12) if ((c >> edge_corners(tables, e)[0]) & 1) != ((c >> edge_corners(tables, e)[1]) & 1)}
        used = {e for tri in case_tris(tables, c) for e in tri}
        assert used == crossing, c                     # every crossing edge carries a vertex
    assert case_tris(tables, 0) == [] and case_tris(tables, 255) == []


def directed(tris):
    out = []
    for a, b, c in tris:
        out += [(a, b), (b, c), (c, a)]
    return out


def test_inside_edges_pair_up_and_boundary_lies_on_faces(tables):
    """Inside a cube every triangle edge is shared by exactly two triangles with opposite directions; the others
    (used once) are the surface's boundary and lie in one face of the cube."""
    fc = faces_of_cube()
    for c in range(256):
        d = directed(case_tris(tables, c))
        assert len(set(d)) == len(d), c
        for (a, b) in d:
            if (b, a) in d:
                continue
            on = [f for f, cs in fc.items() if all(x in cs for x in edge_corners(tables, a) + edge_corners(tables, b))]
            assert len(on) == 1, (c, a, b)


def face_segments(tables, c, face):
    """Directed boundary segments case c leaves on `face`, each end named by its lattice edge relative to the face:
    (corner, corner) pairs, so that two cells sharing the face can compare."""
    fc = faces_of_cube()[face]
    d = directed(case_tris(tables, c))
    segs = set()
    for (a, b) in d:
        if (b, a) in d:
            continue
        ca, cb = edge_corners(tables, a), edge_corners(tables, b)
        if all(x in fc for x in ca + cb):
            segs.add((ca, cb))
    return segs


def test_face_cuts_are_face_local_and_agree_across_the_face(tables):
    """For all 256 cases and 6 faces the segments on a face depend only on that face's 4 corner bits, and the cell on
    the other side (the same 4 values at the mirrored corners) draws the same segments in the opposite direction:
    no cracks."""
    fc = faces_of_cube()
    by_bits = {}
    for c in range(256):
        for (a, s), cs in fc.items():
            bits = tuple((c >> x) & 1 for x in cs)
            segs = face_segments(tables, c, (a, s))
            assert by_bits.setdefault(((a, s), bits), segs) == segs, (c, a, s)
    for c in range(256):
        for a in range(3):
            # this cell's face (a, 1) is the neighbour's face (a, 0): corner x there is x ^ (1 << a) here
            mine = face_segments(tables, c, (a, 1))
            nb = 0
            for x in fc[(a, 1)]:
                nb |= ((c >> x) & 1) << (x ^ (1 << a))
            theirs = face_segments(tables, nb, (a, 0))
            m = lambda p: tuple(sorted(y ^ (1 << a) for y in p))
            mapped = {(m(p), m(q)) for (p, q) in theirs}
            assert mapped == {(tuple(sorted(q)), tuple(sorted(p))) for (p, q) in mine}, (c, a)


def analytic(g, name):
    if f"d_{name}_vol" in g:
        return g[f"d_{name}_vol"]
    vol = {"sphere": U.vol_sphere, "torus": U.vol_torus}[name]()
    assert vol.astype(np.float64).sum() == g[f"d_{name}_sum"][0]
    return vol


@pytest.mark.parametrize("name", ["sphere", "torus", "blobs", "noise"])
def test_mesh_checker_on_skimage_fixture(g16, name):
    """Fixture self-consistency: the stored skimage statistics are those of a closed mesh of the expected topology
    (sphere 2, torus 0, two blobs joined by a neck 2), and the edge-key matcher keys skimage's edge vertices."""
    v = g16[f"d_{name}_verts"]
    nV, nF, chi, area, vol, closed = g16[f"d_{name}_stats"]
    assert len(v) == nV
    if name == "noise":
        return
    assert closed == 1.0 and chi == {"sphere": 2, "torus": 0, "blobs": 2}[name]
    assert vol > 0                                          # skimage 'ascent' winds the high side inward
    assert (U.edge_keys(v) >= 0).all()


@pytest.mark.parametrize("name", ["sphere", "torus", "blobs", "noise"])
def test_numpy_statement_against_skimage(g16, name, tables):
    """The extraction objnerf_mesh.hip performs, stated in numpy with the shipped table, against skimage on the fixture
    volumes: the same edge vertices, winding, topology, area and volume (noise: watertight inside the volume)."""
    vol = analytic(g16, name)
    V, F, N = U.marching_cubes_np(vol, 0.5, tables)
    sv, sn = g16[f"d_{name}_verts"], g16[f"d_{name}_normals"].astype(np.float32)
    nV, nF, chi, area, svol, closed = g16[f"d_{name}_stats"]
    ia, ib = U.match_by_edge(V, sv)
    keyed = U.edge_keys(sv) >= 0
    assert len(ib) == keyed.sum() == len(V)                  # skimage's edge vertices == ours (its interior ones aside)
    assert np.abs(V[ia] - sv[ib]).max() <= 5e-5
    cos = (N[ia] * sn[ib]).sum(1)
    if name != "noise":
        # central differences against skimage's own gradient estimate: the same direction, not the same digits
        assert cos.min() > 0.99 and cos.mean() > 0.999, (cos.min(), cos.mean())
        assert U.is_closed_oriented(F)
        assert U.euler(V, F) == chi
        assert abs(U.area(V, F) - area) <= 1e-3 * area
        assert abs(U.signed_volume(V, F) - svol) <= 1e-3 * abs(svol)
    else:
        d = vol.shape[0]
        be = U.boundary_edges(F)
        on_border = lambda i: ((V[i] <= 1e-6) | (V[i] >= d - 1 - 1e-6)).any(1)
        assert (on_border(be[:, 0]) & on_border(be[:, 1])).all()
        assert np.sign(U.signed_volume(V, F)) == np.sign(svol)


def fixture_trimesh(g, tag):
    d = int(g[f"{tag}_meta"][3])
    return TriMesh(g[f"{tag}_sk_verts"] / (d - 1), np.zeros((0, 3), np.int64))


@pytest.mark.parametrize("tag", ["a", "b"])
def test_trimesh_transforms_reproduce_reference_vertices(g16, tag):
    """Trainer.meshing's transforms (trainer.py:85-90) on skimage's fixture vertices give the reference's final
    vertices."""
    g = g16
    obj_id = int(g[f"{tag}_meta"][0])
    bound_extent = 0.995 if obj_id == 0 else 0.9
    scene_scale = g[f"{tag}_box_extent"] / (2.0 * bound_extent)
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = g[f"{tag}_box_center"]
    T[:3, :3] = g[f"{tag}_box_R"]
    m = fixture_trimesh(g, tag)
    m.apply_translation([-0.5, -0.5, -0.5])
    m.apply_scale(2)
    m.apply_scale(scene_scale)
    m.apply_transform(T)
    ref = g[f"{tag}_verts"].astype(np.float64)
    scale = np.abs(ref).max()
    assert np.abs(m.vertices - ref).max() <= 1e-6 * scale


def test_trimesh_normals_and_winding_under_a_reflection():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float64)
    m = TriMesh(v, [[0, 1, 2]], vertex_normals=np.tile([0.0, 0.0, 1.0], (3, 1)))
    m.apply_scale([2.0, 1.0, -1.0])
    assert (m.faces == [[2, 1, 0]]).all()
    assert np.allclose(m.vertex_normals, [[0, 0, -1]] * 3)
    m.apply_scale([4.0, 1.0, 1.0])                          # inverse transpose: a normal in x shrinks
    assert np.allclose(np.linalg.norm(m.vertex_normals, axis=1), 1.0)


def test_vertex_colors_are_rgba_uint8():
    m = TriMesh(np.zeros((2, 3)), np.zeros((0, 3)))
    m.visual.vertex_colors = np.array([[255, 0, 10], [1, 2, 3]], np.uint8)
    assert m.visual.vertex_colors.dtype == np.uint8 and m.visual.vertex_colors.shape == (2, 4)
    assert (m.visual.vertex_colors[:, 3] == 255).all()


def test_export_round_trip(tmp_path):
    vol = U.vol_sphere(12)
    V, F, N = U.marching_cubes_np(vol, 0.5)
    m = TriMesh(V, F, vertex_normals=N)
    rgba = (np.arange(len(V) * 3) % 256).astype(np.uint8).reshape(-1, 3)
    m.visual.vertex_colors = rgba
    m.export(str(tmp_path / "m.ply"))
    v, n, c, f = read_ply(str(tmp_path / "m.ply"))
    assert np.array_equal(v, V) and np.array_equal(n, N) and np.array_equal(c[:, :3], rgba) and np.array_equal(f, F)
    m.export(str(tmp_path / "m.obj"))
    vs, vn, fs = [], [], []
    for line in open(tmp_path / "m.obj"):
        p = line.split()
        if p[0] == "v":
            vs.append([float(x) for x in p[1:]])
        elif p[0] == "vn":
            vn.append([float(x) for x in p[1:]])
        elif p[0] == "f":
            fs.append([int(x.split("//")[0]) - 1 for x in p[1:]])
    vs = np.array(vs)
    assert np.abs(vs[:, :3] - V).max() < 1e-6 and np.abs(vs[:, 3:] - rgba / 255.0).max() < 1e-5
    assert np.abs(np.array(vn) - N).max() < 1e-6 and np.array_equal(np.array(fs), F)
    p = PointCloud(V, rgba / 255.0)
    assert len(p) == len(V) and p.colors.shape == (len(V), 3)
