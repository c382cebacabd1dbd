"""Helpers of the marching-cubes tests (tests/test_mesh.py, tests/test_mesh_gpu.py): a plain numpy statement of the
extraction objnerf_mesh.hip performs (same table, same vertex / face order), the analytic volumes of fixture g16 and
the mesh checks (watertight, orientation, Euler characteristic, area, enclosed volume, edge-keyed vertex matching)."""
import ctypes as C

import numpy as np


def shipped_tables():
    """(edge_c0 [12], edge_axis [12], ntri [256], tri [256][3 * max_tris]) as compiled into the library."""
    from openobj_amd import _lib
    l = _lib.lib()
    maxt = int(l.objnerf_mc_tables(None, None, None, None))
    c0 = np.zeros(12, np.uint8)
    ax = np.zeros(12, np.uint8)
    nt = np.zeros(256, np.uint8)
    tri = np.zeros((256, 3 * maxt), np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert l.objnerf_mc_tables(p(c0), p(ax), p(nt), p(tri)) == maxt
    return c0, ax, nt, tri


def corner_offsets():
    return np.array([(c & 1, (c >> 1) & 1, (c >> 2) & 1) for c in range(8)], np.int64)


def gradient(vol):
    """Central differences, one-sided at the border, per axis: [d][d][d][3] float32."""
    g = np.zeros(vol.shape + (3,), np.float32)
    for a in range(3):
        v = np.moveaxis(vol, a, 0)
        ga = np.empty_like(v)
        ga[1:-1] = (v[2:] - v[:-2]) * np.float32(0.5)
        ga[0] = v[1] - v[0]
        ga[-1] = v[-1] - v[-2]
        g[..., a] = np.moveaxis(ga, 0, a)
    return g


def marching_cubes_np(vol, level, tables=None):
    """numpy statement of objnerf_mc_count / objnerf_mc_emit ('ascent').  -> (verts [V,3], faces [F,3], normals [V,3])."""
    vol = np.ascontiguousarray(vol, np.float32)
    level = np.float32(level)
    d = vol.shape[0]
    c0, ax, nt, tri = shipped_tables() if tables is None else tables
    above = vol > level
    mask = np.zeros(vol.shape, np.int64)
    for a in range(3):
        cr = np.zeros(vol.shape, bool)
        s0 = [slice(None)] * 3
        s1 = [slice(None)] * 3
        s0[a] = slice(0, d - 1)
        s1[a] = slice(1, d)
        cr[tuple(s0)] = above[tuple(s0)] != above[tuple(s1)]
        mask |= cr.astype(np.int64) << a
    flat = mask.reshape(-1)
    nv = ((flat & 1) + ((flat >> 1) & 1) + ((flat >> 2) & 1))
    base = np.concatenate([[0], np.cumsum(nv)[:-1]])
    g = gradient(vol).reshape(-1, 3)
    vf = vol.reshape(-1)
    verts, normals = [], []
    pts = np.argwhere(np.ones(vol.shape, bool))               # lattice points in linear order
    strides = np.array([d * d, d, 1])
    vid_pt, vid_ax = [], []
    for a in range(3):
        sel = np.nonzero((flat >> a) & 1)[0]
        vid_pt.append(sel)
        vid_ax.append(np.full(len(sel), a))
    vp = np.concatenate(vid_pt)
    va = np.concatenate(vid_ax)
    order = np.lexsort((va, vp))
    vp, va = vp[order], va[order]
    q = vp + strides[va]
    v0, v1 = vf[vp], vf[q]
    t = (level - v0) / (v1 - v0)
    verts = pts[vp].astype(np.float32)
    verts[np.arange(len(vp)), va] += t
    n = (np.float32(1) - t)[:, None] * g[vp] + t[:, None] * g[q]
    # skimage's normals point down the gradient, whatever gradient_direction says
    normals = -n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), np.float32(1e-30))
    # faces
    cells = np.argwhere(np.ones((d - 1,) * 3, bool))
    off = corner_offsets()
    case = np.zeros(len(cells), np.int64)
    for c in range(8):
        p = cells + off[c]
        case |= above[p[:, 0], p[:, 1], p[:, 2]].astype(np.int64) << c
    faces = []
    cnt = nt[case].astype(np.int64)
    keep = np.nonzero(cnt)[0]
    for ci in keep:
        cc = case[ci]
        for k in range(int(cnt[ci])):
            f = []
            for e in tri[cc, 3 * k:3 * k + 3]:
                owner = cells[ci] + off[c0[e]]
                o = owner @ strides
                a = int(ax[e])
                f.append(base[o] + bin(int(flat[o]) & ((1 << a) - 1)).count("1"))
            faces.append(f)
    faces = np.array(faces, np.int64).reshape(-1, 3)
    return verts.astype(np.float32), faces.astype(np.int32), normals.astype(np.float32)


# --- analytic volumes (fixture g16 case d) -------------------------------------------------------------------------

def vol_sphere(d=33, r=None):
    r = (d - 1) * 0.37 if r is None else r
    c = (d - 1) / 2.0
    x = np.indices((d, d, d)).astype(np.float64) - c
    return (1.0 - np.sqrt((x ** 2).sum(0)) / r).astype(np.float32) * 0.5 + 0.5      # 0.5 on the sphere, high inside


def vol_torus(d=40, R=None, r=None):
    R = (d - 1) * 0.28 if R is None else R
    r = (d - 1) * 0.11 if r is None else r
    c = (d - 1) / 2.0
    x, y, z = np.indices((d, d, d)).astype(np.float64) - c
    q = np.sqrt(x ** 2 + y ** 2) - R
    return (0.5 + 0.5 * (1.0 - np.sqrt(q ** 2 + z ** 2) / r)).astype(np.float32)


def vol_blobs(d=28):
    """Two spheres whose 0.5 level sets touch along a short neck."""
    c1 = np.array([(d - 1) * 0.33, (d - 1) * 0.5, (d - 1) * 0.5])
    c2 = np.array([(d - 1) * 0.67, (d - 1) * 0.52, (d - 1) * 0.49])
    x = np.indices((d, d, d)).astype(np.float64)
    r = (d - 1) * 0.17
    f = np.zeros((d, d, d))
    for c in (c1, c2):
        f += np.exp(-((x - c[:, None, None, None]) ** 2).sum(0) / (2 * r * r))
    return (f / f.max()).astype(np.float32)


def vol_noise(d=12, seed=5):
    return np.random.default_rng(seed).random((d, d, d), dtype=np.float64).astype(np.float32)


# --- checks ----------------------------------------------------------------------------------------------------------

def directed_edges(faces):
    f = np.asarray(faces, np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def boundary_edges(faces):
    """Directed edges without their reverse (for a closed, consistently oriented mesh: none)."""
    e = directed_edges(faces)
    n = int(e.max()) + 1 if len(e) else 1
    key = e[:, 0] * n + e[:, 1]
    rev = e[:, 1] * n + e[:, 0]
    u, cnt = np.unique(key, return_counts=True)
    assert cnt.max() <= 1, "a directed edge is used twice (inconsistent orientation or non-manifold)"
    return e[~np.isin(key, rev)]


def is_closed_oriented(faces):
    return len(boundary_edges(faces)) == 0


def euler(verts, faces):
    e = directed_edges(faces)
    und = np.unique(np.sort(e, axis=1), axis=0)
    used = np.unique(np.asarray(faces).reshape(-1))
    return len(used) - len(und) + len(faces)


def area(verts, faces):
    v = np.asarray(verts, np.float64)[np.asarray(faces)]
    return 0.5 * np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1).sum()


def signed_volume(verts, faces):
    v = np.asarray(verts, np.float64)[np.asarray(faces)]
    return np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0


def edge_keys(verts, tol=1e-5):
    """Owning lattice edge of each vertex: (floor coords, axis of the non-integral coordinate) packed to one int;
    -1 for a vertex on a lattice point (t == 0) or off every edge (a cell-interior vertex)."""
    v = np.asarray(verts, np.float64)
    fl = np.floor(v)
    frac = v - np.round(v)
    nonint = np.abs(frac) > tol
    ok = nonint.sum(1) == 1
    a = np.argmax(nonint, axis=1)
    base = np.round(v)
    base[np.arange(len(v)), a] = fl[np.arange(len(v)), a]
    b = base.astype(np.int64)
    key = ((b[:, 0] * 2048 + b[:, 1]) * 2048 + b[:, 2]) * 3 + a
    key[~ok] = -1
    return key


def match_by_edge(va, vb, tol=1e-5):
    """-> (ia, ib): indices of the vertices of va and vb on the same lattice edge."""
    ka, kb = edge_keys(va, tol), edge_keys(vb, tol)
    common, ia, ib = np.intersect1d(ka[ka >= 0], kb[kb >= 0], return_indices=True)
    ia = np.nonzero(ka >= 0)[0][ia]
    ib = np.nonzero(kb >= 0)[0][ib]
    return ia, ib
