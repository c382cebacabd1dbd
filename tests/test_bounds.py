"""CPU: the statement of sceneObject.get_bound (vmap.py:287-384) in tests/bound_util.py, and the host half of
openobj_amd/bounds.py (hull candidates, ordering, corners) against it.  The device half is tests/test_bounds_gpu.py."""
import numpy as np
import pytest

from openobj_amd import bounds
try:
    from tests import bound_util as BU
except ImportError:          # plain `pytest tests/` puts tests/ itself, not the repository root, on sys.path
    import bound_util as BU


def _rot(rs):
    q, _ = np.linalg.qr(rs.randn(3, 3))
    return q * np.sign(np.linalg.det(q))


def _cloud(rs, n, scale=(0.6, 0.3, 0.15)):
    return (rs.randn(n, 3) * np.asarray(scale)) @ _rot(rs).T + rs.randn(3)


def _vol(ext):
    return float(np.prod(ext))


def _emulate_search(p):
    """objnerf_obb_search's arithmetic for one problem, in numpy -> (criterion, R, extents, centre)."""
    best = None
    for ni, ei in p["cand"]:
        n = p["normals"][ni]
        a, b = p["edges"][ei]
        e = p["verts"][b] - p["verts"][a]
        u = e - (e @ n) * n
        if np.linalg.norm(u) <= 1e-12 * np.linalg.norm(e):
            continue
        u /= np.linalg.norm(u)
        R = np.stack([u, np.cross(n, u), n], axis=1)
        loc = p["verts"] @ R
        ext = np.ptp(loc, axis=0)
        crit = ext[0] * ext[1] if p["mode"] == 1 else _vol(ext)
        if best is None or crit < best[0]:
            best = (crit, R, ext, R @ ((loc.min(0) + loc.max(0)) / 2) + p["offset"])
    return best


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_box_contains_points_and_beats_aabb_and_pca(seed):
    rs = np.random.RandomState(seed)
    P = _cloud(rs, 400)
    R, ext, c = BU.oriented_bounds(P)
    assert BU.box_contains(R, ext, c, P, 1e-9)
    aabb = _vol(np.ptp(P, axis=0))
    _, _, vt = np.linalg.svd(P - P.mean(0))
    pca = _vol(np.ptp((P - P.mean(0)) @ vt.T, axis=0))
    assert _vol(ext) <= aabb * (1 + 1e-12) and _vol(ext) <= pca * (1 + 1e-12)


def test_extents_invariant_under_rigid_motion_and_ordered():
    rs = np.random.RandomState(3)
    P = _cloud(rs, 300)
    R, ext, c = BU.oriented_bounds(P)
    Q = P @ _rot(rs).T + rs.randn(3) * 5
    R2, ext2, c2 = BU.oriented_bounds(Q)
    np.testing.assert_allclose(ext2, ext, rtol=1e-9)
    for RR, ee in ((R, ext), (R2, ext2)):
        assert np.all(np.diff(ee) >= 0) and abs(np.linalg.det(RR) - 1) < 1e-9
        np.testing.assert_allclose(RR.T @ RR, np.eye(3), atol=1e-9)


def test_corners_follow_the_reference_formula():
    rs = np.random.RandomState(4)
    R, ext, c = BU.oriented_bounds(_cloud(rs, 100))
    b3, b = bounds.finish_box(R, ext, c)
    half = b.extent / 2
    want = np.array([c + R @ (np.array(s) * half) for s in
                     [(-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1), (-1, -1, 1), (1, -1, 1), (1, 1, 1), (-1, 1, 1)]])
    np.testing.assert_allclose(b.points3d, want, atol=1e-12)
    assert b.points3d.shape == (8, 3) and np.all(b.extent >= 0.10) and np.all(b3.extent >= 0.05)
    assert np.array_equal(b3.center, b.center) and np.array_equal(b3.R, b.R)
    import pickle
    b2 = pickle.loads(pickle.dumps(b))                       # goes into checkpoints
    assert np.array_equal(b2.points3d, b.points3d)


def test_coplanar_set_gives_flat_floored_box():
    rs = np.random.RandomState(5)
    xy = rs.rand(200, 2) * [0.8, 0.5]
    P = np.concatenate([xy, np.full((200, 1), 1.5)], axis=1) @ _rot(rs).T
    R, ext, c = BU.oriented_bounds(P)
    assert ext[0] == 0.0 and ext[1] > 0.3
    fb = BU.get_bound(P, voxel=1e-4)
    assert fb is not None and fb[1][0] == pytest.approx(0.10)
    p = bounds.hull_problem(P)
    assert p["mode"] == 1 and len(p["normals"]) == 1
    crit, Rk, extk, ck = _emulate_search(p)
    assert crit == pytest.approx(ext[1] * ext[2], rel=1e-9)


@pytest.mark.parametrize("P", [np.zeros((0, 3)), np.ones((1, 3)), np.array([[0., 0, 0], [1, 1, 1]]),
                               np.outer(np.linspace(0, 1, 50), [0.3, -0.2, 1.0]) + 2.0])
def test_collinear_and_tiny_sets_have_no_box(P):
    assert BU.oriented_bounds(P) is None
    assert bounds.hull_problem(P) is None
    assert bounds.obb_search([None], "cpu") == [None]


def test_backprojection_of_a_2x2_keyframe():
    fx, fy, cx, cy = 2.0, 4.0, 0.5, 0.25
    depth = np.array([[1.0, 2.0], [np.nan, 0.0]], np.float32)      # [W, H]: (x=0, y=0) = 1, (x=0, y=1) = 2, ...
    state = np.array([[1, 1], [1, 1]], np.uint8)
    twc = np.eye(4, dtype=np.float32)
    twc[:3, 3] = [1, 2, 3]
    P = BU.backproject(depth, state, twc, fx, fy, cx, cy)
    # row i = y, column j = x; only (j=0, i=0, z=1) and (j=0, i=1, z=2) survive (NaN and 0 are dropped)
    want = np.array([[(0 - cx) * 1 / fx + 1, (0 - cy) * 1 / fy + 2, 1 + 3],
                     [(0 - cx) * 2 / fx + 1, (1 - cy) * 2 / fy + 2, 2 + 3]])
    np.testing.assert_allclose(P, want, atol=1e-12)
    state[0, 1] = 2
    assert len(BU.backproject(depth, state, twc, fx, fy, cx, cy)) == 1
    np.testing.assert_array_equal(bounds.camera_poses(twc[None])[0], BU.camera_pose(twc))


def test_voxel_down_sums_in_order():
    rs = np.random.RandomState(6)
    P = rs.rand(5000, 3)
    idx, cen = BU.voxel_down(P, 0.1)
    vmin = P.min(0) - 0.05
    key = np.floor((P - vmin) / 0.1).astype(np.int64)
    for t in (0, 7, len(idx) - 1):
        m = (key == idx[t]).all(1)
        s = np.zeros(3)
        for p in P[m]:
            s = s + p
        np.testing.assert_array_equal(cen[t], s / m.sum())


@pytest.mark.parametrize("seed,n", [(7, 60), (8, 400), (9, 700)])
def test_host_candidates_reach_the_exact_minimum(seed, n):
    """bounds.hull_problem's silhouette candidates, evaluated as the kernel does, give the statement's minimum volume
    (which tries every edge of every normal's 2-D hull)."""
    rs = np.random.RandomState(seed)
    P = rs.randn(n, 3) * [0.5, 0.3, 0.2]
    if n > 500:                                                     # every point a hull vertex
        P = P / np.linalg.norm(P, axis=1, keepdims=True) * [0.5, 0.3, 0.2]
    P = P @ _rot(rs).T + rs.randn(3)
    R, ext, c = BU.oriented_bounds(P)
    p = bounds.hull_problem(P)
    assert p["mode"] == 0 and p["cand"].shape[1] == 2
    crit, Rk, extk, ck = _emulate_search(p)
    assert crit == pytest.approx(_vol(ext), rel=1e-9)
    assert BU.box_contains(Rk, extk, ck, P, 1e-9)
