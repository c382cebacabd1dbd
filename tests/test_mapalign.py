"""Field gradients, nearest surface and rigid alignment without a GPU: the specification (tests/mapalign_util.py) against
central differences and a literal reading of its rules, the conditions the GPU tests (tests/test_mapalign_gpu.py) rest on,
asserted on the specification alone, and the host pieces of openobj_amd.map_align."""
import json
import types

import numpy as np
import pytest
import torch

import mapalign_util as A
import mappoints_util as U
from openobj_amd import _lib, map_align, ops

SCENES = [("main", 32), ("bg", 32), ("bg", 128)]


def _scene(scene, bg):
    ref = U.reference(scene, bg)
    return ref["objs"], torch.from_numpy(ref["points"])


@pytest.fixture(scope="module")
def fields():
    cache = {}

    def get(scene, bg):
        if (scene, bg) not in cache:
            objs, pts = _scene(scene, bg)
            cache[(scene, bg)] = A.scene_fields(objs, pts.double())
        return cache[(scene, bg)]

    return get


# ---------------------------------------------------------------------------------------------------------- the field
def test_spec_alpha_is_the_oracle_chain():
    ref = U.reference("bg", 128)
    alpha, _ = A.scene_fields(ref["objs"], torch.from_numpy(ref["points"]), dtype=torch.float32)
    assert (alpha - ref["alpha"]).abs().max() <= 1e-5


@pytest.mark.parametrize("scene,bg", SCENES)
def test_spec_gradient_is_the_central_difference(fields, scene, bg):
    objs, pts = _scene(scene, bg)
    _, grad = fields(scene, bg)
    h = 1e-6
    big = float(grad.norm(dim=-1).max())
    for k, o in enumerate(objs):
        fd = []
        smooth = torch.ones(len(pts), dtype=torch.bool)          # no ReLU changes its branch inside the stencil
        for x in range(3):
            e = torch.zeros(3, dtype=torch.float64)
            e[x] = h
            fd.append((A.field(o, pts.double() + e)[0] - A.field(o, pts.double() - e)[0]) / (2 * h))
            smooth &= (A.relu_pattern(o, pts.double() + e) == A.relu_pattern(o, pts.double() - e)).all(dim=1)
        assert float((~smooth).float().mean()) <= 0.01           # (a kink within 1e-6 of a point: hidden 128 has one)
        err = float((torch.stack(fd, dim=1) - grad[k]).norm(dim=-1)[smooth].max())
        assert err <= 1e-6 * big, (k, err, big)


@pytest.mark.parametrize("ablate,least", [("cat", 1e-2), ("oct3", 1e-2), ("lin", 1e-2)])
def test_every_term_of_the_chain_matters(fields, ablate, least):
    """What the GPU bound (GRAD_CEILING, 1e-3 of the largest |grad|) can tell apart: leaving out any of these terms moves
    the gradient by at least 1e-2 of the scene's largest |grad| -- measured, the smallest of the three scenes: the cat
    layer's direct branch 0.85, octave 3's factor 0.38, the three x / scale entries 1.2e-2."""
    moved = []
    for scene, bg in SCENES:
        objs, pts = _scene(scene, bg)
        _, grad = fields(scene, bg)
        _, cut = A.scene_fields(objs, pts.double(), ablate=ablate)
        moved.append(float((cut - grad).norm(dim=-1).max()) / float(grad.norm(dim=-1).max()))
    print(ablate, moved)
    assert min(moved) >= least
    assert A.GRAD_CEILING * 10 <= least and A.GRAD_TOL <= A.GRAD_CEILING


@pytest.mark.parametrize("scene,bg", SCENES)
def test_an_fp32_oracle_stays_far_inside_the_ceiling(fields, scene, bg):
    objs, pts = _scene(scene, bg)
    _, grad = fields(scene, bg)
    _, g32 = A.scene_fields(objs, pts, dtype=torch.float32)
    err = float((g32.double() - grad).norm(dim=-1).max()) / float(grad.norm(dim=-1).max())
    print(f"fp32 oracle gradient error {err:.2e}")
    assert err <= 1e-5


# ------------------------------------------------------------------------------------------------------ the selection
def _select_by_the_rules(alpha, grad, cand, g_min):
    K, N = alpha.shape
    obj, d = np.full(N, -1, np.int64), np.full(N, np.inf)
    for n in range(N):
        for k in range(K):
            if not cand[k, n]:
                continue
            v = alpha[k, n] / max(np.linalg.norm(grad[k, n]), g_min)
            if obj[n] < 0 or abs(v) < abs(d[n]):
                obj[n], d[n] = k, v
    return obj, d


@pytest.mark.parametrize("scene,bg", SCENES)
def test_select_spec_follows_the_rules_and_is_rarely_ambiguous(fields, scene, bg):
    objs, pts = _scene(scene, bg)
    alpha, grad = fields(scene, bg)
    s = A.select_spec(objs, pts, fields=(alpha, grad))
    obj, d = _select_by_the_rules(alpha.numpy(), grad.numpy(), U.candidate_mask(pts, objs).numpy(), A.G_MIN)
    assert np.array_equal(s["obj"].numpy(), obj) and np.array_equal(s["d"].numpy(), d)
    none = obj < 0
    assert (s["grad"][none] == 0).all() and (s["normal"][none] == 0).all() and torch.isinf(s["d"][none]).all()
    has = ~none
    nrm = s["normal"][has]
    assert ((nrm.norm(dim=-1) - 1).abs() < 1e-12).all()
    assert ((nrm * s["grad"][has]).sum(-1) < 0).all()            # outward: against the gradient
    print(scene, bg, "ambiguous", int(s["ambiguous"].sum()), "of", len(obj), "smallest gap", float(s["gap"].min()))
    assert float(s["ambiguous"].float().mean()) <= A.AMBIGUOUS_CAP


def test_key_round_trip_and_order():
    rs = np.random.RandomState(0)
    d = np.concatenate([[0.0, 1e-30, 1.0, 3.0e38, np.inf], np.abs(rs.randn(200)).astype(np.float32) * 10 ** rs.uniform(-8, 3, 200)])
    d = d.astype(np.float32)
    pair = np.concatenate([[0, 1, 2 ** 31 - 2, 7, 9], rs.randint(0, 2 ** 31 - 1, 200)]).astype(np.int64)
    key = ops.mapalign_key_encode(d, pair)
    assert key.dtype == np.uint64 and (key >> np.uint64(63) == 0).all()
    d2, p2 = ops.mapalign_key_decode(key)
    assert np.array_equal(d2, d) and np.array_equal(p2, pair)
    order = np.lexsort((pair, d))
    assert np.array_equal(np.argsort(key, kind="stable"), order)            # smaller |d| first, then the lower pair
    free = np.array([-1], np.int64).view(np.uint64)
    assert (key < free[0]).all()
    dd, pp = ops.mapalign_key_decode(free)
    assert np.isinf(dd[0]) and pp[0] == -1


# ---------------------------------------------------------------------------------------------- the cloud and the fit
def test_every_object_yields_a_surface_cloud():
    cloud, found = A.surface_cloud(128)
    print("surface points per object", found)
    assert min(found) >= 120 and cloud.shape == (600, 3)
    objs, _ = U.background_scene(128)
    s = A.select_spec(objs, cloud)
    assert float(s["d"].abs().max()) < 1e-9 and float(s["ambiguous"].float().mean()) <= A.AMBIGUOUS_CAP
    cloud32, found32 = A.surface_cloud(32)
    assert min(found32) >= 120


@pytest.mark.parametrize("deg,trans,within", [(2.0, 0.03, 8), (5.0, 0.08, 12)])
def test_fit_spec_converges_quadratically(deg, trans, within):
    cloud, _ = A.surface_cloud(128)
    objs, _ = U.background_scene(128)
    T_true = A.rigid(deg, trans)
    own = (cloud - T_true[:3, 3]) @ T_true[:3, :3]               # T_true^-1: the cloud in its own frame
    r = A.fit_spec(objs, own, iters=within)
    rot, tr = A.pose_error(r["T"], T_true)
    print(deg, [f"{h['rms']:.2e}" for h in r["history"]], rot, tr, r["history"][0]["cond"])
    assert rot < 1e-9 and tr < 1e-9
    assert r["history"][0]["cond"] < 10


def test_fit_spec_under_the_noise_an_fp32_field_may_have():
    cloud, _ = A.surface_cloud(128)
    objs, _ = U.background_scene(128)
    big = float(A.scene_fields(objs, cloud)[1].norm(dim=-1).max())
    T_true = A.rigid(2.0, 0.03)
    own = (cloud - T_true[:3, 3]) @ T_true[:3, :3]
    r = A.fit_spec(objs, own, iters=10, noise=(A.ALPHA_TOL, 1e-3 * big, torch.Generator().manual_seed(1)), fp32_q=True)
    rot, tr = A.pose_error(r["T"], T_true)
    print("noisy fit", rot, tr)
    assert rot < A.POSE_TOL and tr < A.POSE_TOL


def test_normal_eq_spec_by_loops():
    rs = np.random.RandomState(2)
    n = 37
    q, g = rs.randn(n, 3).astype(np.float32), rs.randn(n, 3).astype(np.float32)
    g[3] = 0
    al = (rs.randn(n) * 0.05).astype(np.float32)
    obj = rs.randint(-1, 3, n)
    piv = np.array([0.1, -0.2, 0.3])
    want = np.zeros(29)
    for i in range(n):
        den = max(np.linalg.norm(g[i].astype(np.float64)), A.G_MIN)
        d = float(al[i]) / den
        if obj[i] < 0 or abs(d) > A.TAU:
            continue
        nn = g[i].astype(np.float64) / den
        J = np.concatenate([np.cross(q[i].astype(np.float64) - piv, nn), nn])
        want[:21] += np.outer(J, J)[np.triu_indices(6)]
        want[21:27] += J * d
        want[27] += d * d
        want[28] += 1
    got = A.normal_eq_spec(q, obj, al, g, piv).numpy()
    assert np.allclose(got, want, rtol=1e-12, atol=1e-15)
    Amat, b, ss, cnt = map_align.unpack_sums(got)
    assert np.array_equal(Amat, Amat.T) and cnt == int(want[28]) and ss == got[27] and np.array_equal(b, got[21:27])
    assert np.array_equal(Amat[np.triu_indices(6)], got[:21])


# ---------------------------------------------------------------------------------------------------- the host pieces
@pytest.mark.parametrize("xi", [[0.3, -0.2, 0.5, 1.0, 2.0, -0.5], [1e-6, 2e-6, -1e-6, 0.1, 0.0, 0.2], [0, 0, 0, 1, 2, 3],
                                [2.0, 1.5, -1.0, 0, 0, 0]])
def test_exp_se3_is_the_matrix_exponential(xi):
    got = map_align.exp_se3(xi)
    assert np.abs(got - A.exp_se3(xi).numpy()).max() < 1e-14 * max(1.0, np.abs(got).max())
    c = np.array([0.5, -1.0, 2.0])
    M = map_align.about(got, c)
    x = np.array([0.2, 0.3, -0.4])
    assert np.allclose(M[:3, :3] @ x + M[:3, 3], c + got[:3, :3] @ (x - c) + got[:3, 3], atol=1e-14)


def test_gauss_newton_step_refuses_what_it_cannot_solve():
    sums = np.zeros(29)
    sums[28] = 5
    assert map_align.gauss_newton_step(sums, 1e-6)[0] is None                 # fewer than six inliers
    rs = np.random.RandomState(0)
    n = np.array([0.0, 0.0, 1.0])
    J = np.stack([np.concatenate([np.cross(np.append(rs.randn(2), 0.0), n), n]) for _ in range(50)])     # one plane
    A_ = J.T @ J
    sums = np.concatenate([A_[np.triu_indices(6)], J.T @ rs.randn(50) * 1e-3, [1e-4, 50]])
    xi, info = map_align.gauss_newton_step(sums, 1e-6)
    assert xi is None and info["inliers"] == 50 and not info["cond"] <= 1e12
    J = rs.randn(50, 6)
    d = J @ np.array([1e-3, -2e-3, 5e-4, 1e-2, 0.0, -1e-2])
    A_ = J.T @ J
    xi, info = map_align.gauss_newton_step(np.concatenate([A_[np.triu_indices(6)], J.T @ d, [d @ d, 50]]), 0.0)
    assert np.allclose(xi, -np.array([1e-3, -2e-3, 5e-4, 1e-2, 0.0, -1e-2]), atol=1e-12) and info["cond"] < 1e3


def test_frames_and_pose_files(tmp_path):
    assert map_align.parse_frames(None, 5) == [0, 1, 2, 3, 4]
    assert map_align.parse_frames("1:4", 5) == [1, 2, 3] and map_align.parse_frames("::2", 5) == [0, 2, 4]
    assert map_align.parse_frames("3", 5) == [3] and map_align.parse_frames("2:", 5) == [2, 3, 4]
    for bad in ("1:2:3:4", "::0", "a:b", ""):
        with pytest.raises(ValueError):
            map_align.parse_frames(bad, 5)
    poses = [A.rigid(3.0, 0.1).numpy(), np.eye(4)]
    map_align.write_poses(str(tmp_path / "p.txt"), poses)
    back = np.loadtxt(tmp_path / "p.txt", delimiter=" ").reshape(-1, 4, 4)            # how dataset.py reads traj_w_c.txt
    assert np.array_equal(back, np.stack(poses))
    np.savetxt(tmp_path / "T.txt", poses[0])
    assert np.array_equal(map_align.read_pose(str(tmp_path / "T.txt")), poses[0])
    np.savetxt(tmp_path / "bad.txt", np.eye(3))
    with pytest.raises(ValueError):
        map_align.read_pose(str(tmp_path / "bad.txt"))


class _StubAlign:
    """Stands in for MapAlign in the CLI: records the call, returns a fixed answer."""
    calls = []

    def __init__(self, mp):
        self.mp = mp

    def fit(self, points, T0=None, **kw):
        _StubAlign.calls.append(dict(points=np.asarray(points), T0=T0, kw=kw))
        T = A.rigid(1.0, 0.02).numpy()
        return {"T": T, "converged": True, "history": [{"inliers": 7, "rms": 1e-3, "cond": 2.0, "rot": 0.0, "trans": float("nan")}]}


def test_cli_arguments_and_files_on_a_stub(tmp_path, monkeypatch, capsys):
    from openobj_amd import mesh
    monkeypatch.setattr(map_align, "MapAlign", _StubAlign)
    _StubAlign.calls = []
    pts = np.random.RandomState(0).randn(9, 3).astype(np.float32)
    np.save(tmp_path / "c.npy", pts)
    T0 = A.rigid(2.0, 0.03).numpy()
    np.savetxt(tmp_path / "T.txt", T0)
    out = tmp_path / "out"
    res = map_align.main(["--logdir", "unused", "--points", str(tmp_path / "c.npy"), "--init", str(tmp_path / "T.txt"),
                          "--out", str(out), "--iters", "7", "--tau", "0.2"], _map_factory=lambda: "the map")
    call = _StubAlign.calls[0]
    assert np.array_equal(call["points"], pts) and np.array_equal(call["T0"], T0)
    assert call["kw"] == {"iters": 7, "tau": 0.2, "g_min": 1e-3, "damping": 1e-6}
    rec = json.load(open(out / "align.json"))
    assert np.array_equal(np.array(rec["T"]), res["T"]) and rec["converged"] is True
    assert rec["history"][0]["inliers"] == 7 and rec["history"][0]["trans"] is None          # NaN is not JSON
    v, _, _, f = mesh.read_ply(str(out / "aligned.ply"))
    assert len(f) == 0 and np.allclose(v, pts.astype(np.float64) @ res["T"][:3, :3].T + res["T"][:3, 3], atol=1e-6)
    assert "9 points, converged True" in capsys.readouterr().out
    for argv in (["--logdir", "x", "--out", "y"],                                            # neither source
                 ["--logdir", "x", "--out", "y", "--points", "a.npy", "--config", "c.json"],  # both
                 ["--logdir", "x", "--out", "y", "--config", "c.json", "--init", "T.txt"],
                 ["--logdir", "x", "--out", "y", "--points", "a.npy", "--frames", "0:3"],
                 ["--logdir", "x", "--out", "y", "--config", "c.json", "--stride", "0"]):
        with pytest.raises(SystemExit):
            map_align.main(argv, _map_factory=lambda: "the map")


def test_defaults_are_the_documented_ones():
    from openobj_amd import map_points
    assert map_align.DEFAULT_TAU == 0.1 == A.TAU and map_points.DEFAULT_G_MIN == 1e-3 == A.G_MIN


def test_cpu_tensors_are_rejected():
    cpu_map = types.SimpleNamespace(device=torch.device("cpu"))
    with pytest.raises(_lib.ObjnerfError):
        map_align.MapAlign(cpu_map).fit(torch.zeros(4, 3))
    with pytest.raises(_lib.ObjnerfError):
        map_align.MapAlign(cpu_map).fit(torch.zeros(4, 2))
    z = torch.zeros(4)
    with pytest.raises(_lib.ObjnerfError):
        ops.mapalign_transform(torch.zeros(4, 3), np.eye(4))
    with pytest.raises(_lib.ObjnerfError):
        ops.mapalign_select(4, torch.zeros(4, dtype=torch.int32), z, torch.zeros(4, 3), 1e-3, torch.zeros(4, dtype=torch.int64))
    with pytest.raises(_lib.ObjnerfError):
        ops.mapalign_accumulate(torch.zeros(4, 3), torch.zeros(4, dtype=torch.int32), z, torch.zeros(4, 3), [0, 0, 0], 0.1, 1e-3)
    with pytest.raises(_lib.ObjnerfError):
        ops.embed_backward_pts(types.SimpleNamespace(K=1), torch.zeros(1, 4, 3), torch.zeros(1, 4, 129))
    with pytest.raises(_lib.ObjnerfError):
        ops.mappoints_grad(None, torch.zeros(4, 3), torch.zeros(1, 16), torch.zeros(1, 2, dtype=torch.int32),
                           torch.zeros(2, dtype=torch.int64), torch.zeros(4, dtype=torch.int32), z, torch.zeros(4, 3))


def test_abi_number_does_not_move():
    l = _lib.lib()
    assert l.objnerf_abi_version() == 14                       # additive
    assert l.objnerf_mapalign_workspace_bytes(0) == 0
    assert l.objnerf_mapalign_workspace_bytes(1) == 256 and l.objnerf_mapalign_workspace_bytes(1025) == 512


def test_frames_mode_on_stubs(tmp_path, monkeypatch):
    """--config: the frames named by --frames go through fit_frame from the dataset's own depth and pose; the refined
    poses are written one row-major 4 x 4 per line, as traj_w_c.txt holds them."""
    from openobj_amd import dataset, map_cull
    calls = []

    class Frames:
        def __init__(self, c):
            pass

        def __len__(self):
            return 5

        def depth_and_pose(self, i):
            return np.full((6, 4), 1.0 + i, np.float32), A.rigid(float(i), 0.01 * i).numpy()

    class Align:
        def __init__(self, mp):
            self.mp = mp

        def fit_frame(self, depth, T_WC0, rays_dir, stride=4, **kw):
            calls.append((float(depth[0, 0]), tuple(rays_dir.shape), stride, kw))
            T = np.array(T_WC0)
            T[:3, 3] += 0.5
            return {"T": T, "converged": depth[0, 0] < 4, "history": [{"inliers": 9, "rms": float("inf"), "cond": 3.0}]}

    cfg = types.SimpleNamespace(dataset_format="Replica", fx=10.0, fy=11.0, cx=3.0, cy=2.0)
    monkeypatch.setattr(dataset, "Replica", Frames)
    monkeypatch.setattr(map_cull, "_config", lambda c: cfg)
    monkeypatch.setattr(ops, "rays_dirs", lambda W, H, fx, fy, cx, cy, dev: torch.zeros(W, H, 3))
    monkeypatch.setattr(map_align, "MapAlign", Align)
    out = tmp_path / "out"
    poses, report = map_align.main(["--logdir", "unused", "--config", "scene.json", "--frames", "1:4", "--stride", "2",
                                    "--out", str(out), "--iters", "3"],
                                   _map_factory=lambda: types.SimpleNamespace(device="cpu"))
    assert [c[0] for c in calls] == [2.0, 3.0, 4.0] and all(c[1] == (6, 4, 3) and c[2] == 2 for c in calls)
    assert calls[0][3] == {"iters": 3, "tau": 0.1, "g_min": 1e-3, "damping": 1e-6}
    back = np.loadtxt(out / "poses_refined.txt", delimiter=" ").reshape(-1, 4, 4)
    want = np.stack([A.rigid(float(i), 0.01 * i).numpy() for i in (1, 2, 3)])
    want[:, :3, 3] += 0.5
    assert np.array_equal(back, want) and np.array_equal(np.stack(poses), want)
    rec = json.load(open(out / "align_frames.json"))["frames"]
    assert [r["frame"] for r in rec] == [1, 2, 3] and [r["converged"] for r in rec] == [True, True, False]
    assert rec[0]["history"][0]["rms"] is None                             # infinity is not JSON
    cfg.dataset_format = "TUM"
    with pytest.raises(ValueError):
        map_align.main(["--logdir", "unused", "--config", "scene.json", "--out", str(out)],
                       _map_factory=lambda: types.SimpleNamespace(device="cpu"))
