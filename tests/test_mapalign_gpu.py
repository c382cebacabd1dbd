"""Field gradients, nearest surface and rigid alignment on the GPU against their specification (tests/mapalign_util.py;
tests/test_mapalign.py asserts the conditions on the scenes that these tests rely on).  Bounds: pair alpha <= ALPHA_TOL
(1e-4, the project's), gradients <= GRAD_TOL of the scene's largest |grad| (4 x the measured error, never above 1e-3),
the pose <= POSE_TOL; lists, selections on unambiguous points and everything about order are exact."""
import json
import os

import numpy as np
import pytest
import torch

import mapalign_util as A
import mappoints_util as U
from openobj_amd import cfg as ocfg
from openobj_amd import map_align, map_points, ops, trainer, utils

pytestmark = pytest.mark.gpu


def make_trainer(obj, dev):
    c = ocfg.Config(ocfg.replica_room0_config(train_device=str(dev)))
    c.obj_id = int(obj["obj_id"])
    c.hidden_feature_size = int(obj["hidden"])
    c.clip_point_feature_size = 512
    c.obj_scale = float(obj["scale"])
    t = trainer.Trainer(c)
    with torch.no_grad():
        for q, v in zip(t.fc_occ_map.parameters(), obj["p"]):
            q.copy_(v.to(dev))
        t.pe.B_layer.weight.copy_(obj["B"].to(dev))
    return t


def make_box(obj):
    b = utils.BoundingBox()
    b.center, b.R, b.extent = obj["center"].copy(), obj["R"].copy(), obj["extent"].copy()
    return b


def make_mp(objs, dev, **kw):
    return map_points.MapPoints([map_points.MapObject(make_trainer(o, dev), make_box(o), o["obj_id"], o["class_id"],
                                                      o["obj_center"]) for o in objs], device=dev, bg_ids=(0,), **kw)


def cpu(t):
    return t.detach().cpu()


@pytest.fixture(scope="module")
def surfaced(dev):
    """(scene, bg width) -> (reference, MapPoints, surface(points) with the pair buffers kept, the fp64 fields), once."""
    cache = {}

    def get(scene, bg=32):
        if (scene, bg) not in cache:
            ref = U.reference(scene, bg)
            mp = make_mp(ref["objs"], dev)
            mp._keep_pairs = True
            out = mp.surface(ref["points"])
            pairs, mp._keep_pairs = mp._last_pairs, False
            fields = A.scene_fields(ref["objs"], torch.from_numpy(ref["points"]).double())
            cache[(scene, bg)] = (ref, mp, out, pairs, fields)
        return cache[(scene, bg)]

    return get


def pair_index(ref):
    pt = ref["pair_pt"].long()
    k_of = torch.repeat_interleave(torch.arange(len(ref["objs"])), ref["seg_off"][1:] - ref["seg_off"][:-1])
    return k_of, pt


# ------------------------------------------------------------------------------------------------------ per-pair values
@pytest.mark.parametrize("scene,bg", [("main", 32), ("bg", 32), ("bg", 128), ("bg", 64)])
def test_pair_field_against_the_spec(surfaced, scene, bg):
    """main / bg 32: every pair through objnerf_mappoints_grad; bg 128 / 64: the background's segment through the
    layer-wise chain.  Measured on an MI355X, relative to the scene's largest |grad|: see mapalign_util.GRAD_MEASURED."""
    ref, _, _, pairs, (alpha, grad) = surfaced(scene, bg)
    assert pairs["seg"] == ref["seg_off"].tolist() and torch.equal(cpu(pairs["pair_pt"]), ref["pair_pt"])
    k_of, pt = pair_index(ref)
    a_err = float((cpu(pairs["pair_alpha"]).double() - alpha[k_of, pt]).abs().max())
    big = float(grad.norm(dim=-1).max())
    g_err = A.rel_grad_err(pairs["pair_grad"], grad[k_of, pt], big)
    wide = k_of == 0 if bg != 32 else torch.zeros_like(k_of, dtype=torch.bool)
    for name, sel in (("fused", ~wide), ("layer-wise", wide)):
        if bool(sel.any()):
            print(f"{scene} {bg} {name}: pair_alpha error {float((cpu(pairs['pair_alpha']).double() - alpha[k_of, pt]).abs()[sel].max()):.3e}, "
                  f"pair_grad error {A.rel_grad_err(cpu(pairs['pair_grad'])[sel], grad[k_of, pt][sel], big):.3e} of {big:.1f}")
    assert a_err <= A.ALPHA_TOL
    assert g_err <= A.GRAD_TOL


def test_embed_backward_pts_alone(dev):
    rs = np.random.RandomState(4)
    K, N = 2, 70
    arena = ops.ParamArena(K, ops.NetShape(32, 512, 6), dev)
    B = torch.from_numpy(rs.randn(K, 21, 3).astype(np.float32))
    B = B / B.norm(dim=-1, keepdim=True)
    with torch.no_grad():
        arena.views()[18].copy_(B.to(dev))
        arena.scale.copy_(torch.tensor([2.0, 1.7]))
    arena.version += 1
    pts = torch.from_numpy(rs.uniform(-1.5, 1.5, (K, N, 3)).astype(np.float32))
    d_emb = torch.from_numpy(rs.randn(K, N, 129).astype(np.float32))
    got = cpu(ops.embed_backward_pts(arena, pts.to(dev), d_emb.to(dev)))
    want = []
    bands = 2.0 ** torch.arange(6, dtype=torch.float64)
    for k in range(K):
        x = pts[k].double().requires_grad_(True)
        emb = A._embed(x, B[k].double(), float(np.float32([2.0, 1.7][k])), bands)
        want.append(torch.autograd.grad((emb * d_emb[k].double()).sum(), x)[0])
    err = A.rel_grad_err(got, torch.stack(want))
    print(f"embed_backward_pts error {err:.3e} of the largest |d_pts|")
    assert got.shape == (K, N, 3) and err <= A.EMBED_BWD_TOL


@pytest.mark.parametrize("hidden", [32, 128])
def test_eval_grad(dev, surfaced, hidden):
    ref, _, _, _, _ = surfaced("bg", 128)
    obj = ref["objs"][0 if hidden == 128 else 4]                 # the background; D, at obj_center -0.5
    pts = torch.from_numpy(ref["points"])
    t = make_trainer(obj, dev)
    alpha, grad = t.eval_grad(pts - np.float32(obj["obj_center"]))
    a64, g64 = A.field(obj, pts.double())
    print(f"eval_grad hidden {hidden}: alpha {float((cpu(alpha).double() - a64).abs().max()):.3e}, grad {A.rel_grad_err(grad, g64):.3e}")
    assert float((cpu(alpha).double() - a64).abs().max()) <= A.ALPHA_TOL
    assert A.rel_grad_err(grad, g64) <= A.GRAD_TOL
    if hidden == 32:
        # bit for bit the pair outputs of a one-object map whose box holds every point
        whole = dict(obj, center=np.zeros(3), R=np.eye(3), extent=np.full(3, 8.0))
        mp = make_mp([whole], dev)
        mp._keep_pairs = True
        mp.surface(pts)
        pairs = mp._last_pairs
        assert torch.equal(cpu(pairs["pair_pt"]).long(), torch.arange(len(pts)))
        # (eval_grad takes points already relative to obj_center; the map subtracts it in the kernel: the same fp32 value)
        assert torch.equal(pairs["pair_alpha"], alpha) and torch.equal(pairs["pair_grad"], grad)
    a2, g2 = t.eval_grad(torch.zeros(0, 3))
    assert a2.shape == (0,) and g2.shape == (0, 3)


# ------------------------------------------------------------------------------------------------ position independence
@pytest.mark.parametrize("scene,bg", [("main", 32), ("bg", 128)])
def test_permuted_repeated_and_halved_calls_are_bit_equal(dev, surfaced, scene, bg):
    ref, mp, out, pairs, _ = surfaced(scene, bg)
    pts = ref["points"]
    N = len(pts)
    rs = np.random.RandomState(3)
    perm = rs.permutation(N)
    src = np.concatenate([perm, rs.randint(0, N, 50)])           # every point once, fifty of them again
    mp._keep_pairs = True
    out2 = mp.surface(pts[src])
    pairs2, mp._keep_pairs = mp._last_pairs, False
    # a pair is (object, original point): its values must not depend on where it sat
    k_of, pt = pair_index(ref)
    table_a = {(int(k), int(n)): m for m, (k, n) in enumerate(zip(k_of, pt))}
    seg2 = pairs2["seg"]
    pt2 = cpu(pairs2["pair_pt"]).long().numpy()
    m1 = np.array([table_a[(k, int(src[pt2[m]]))] for k in range(len(seg2) - 1) for m in range(seg2[k], seg2[k + 1])])
    assert len(m1) == seg2[-1] > len(k_of)
    for name in ("pair_alpha", "pair_grad"):
        assert torch.equal(cpu(pairs2[name]), cpu(pairs[name])[m1]), name
    for k in ("obj", "d", "alpha", "grad", "normal", "obj_id"):
        assert torch.equal(out2[k], out[k][torch.from_numpy(src).to(dev)]), k
    # a byte budget the pair buffers exceed: surface() halves the cloud until they fit
    budget = mp._field_bytes(ref["seg_off"].tolist()) // 3
    small = make_mp(ref["objs"], dev, pair_budget_bytes=budget)
    assert small._field_bytes(ref["seg_off"].tolist()) > budget
    st = {}
    out3 = small.surface(pts, stats=st)
    assert st["calls"] > 1
    for k in out:
        assert torch.equal(out3[k], out[k]), k
    for k, v in mp.surface(pts, chunk=100).items():
        assert torch.equal(v, out[k]), k


# ------------------------------------------------------------------------------------------------- select and surface
@pytest.mark.parametrize("scene,bg", [("main", 32), ("bg", 32), ("bg", 128)])
def test_surface_is_the_selection_of_the_spec(surfaced, scene, bg):
    ref, mp, out, _, fields = surfaced(scene, bg)
    s = A.select_spec(ref["objs"], torch.from_numpy(ref["points"]), fields=fields)
    ok = ~s["ambiguous"]
    assert float(s["ambiguous"].float().mean()) <= A.AMBIGUOUS_CAP
    obj = cpu(out["obj"]).long()
    assert out["obj"].dtype == torch.int32 and torch.equal(obj[ok], s["obj"][ok])
    ids = torch.tensor([o["obj_id"] for o in ref["objs"]] + [-1])
    assert torch.equal(cpu(out["obj_id"]), ids[obj])
    none = s["obj"] < 0
    assert torch.isinf(cpu(out["d"])[none]).all() and (cpu(out["d"])[none] > 0).all()
    for k in ("grad", "normal", "alpha"):
        assert (cpu(out[k])[none] == 0).all(), k
    won = ok & ~none
    big = float(fields[1].norm(dim=-1).max())
    assert A.rel_grad_err(cpu(out["grad"])[won], s["grad"][won], big) <= A.GRAD_TOL
    assert float((cpu(out["alpha"]).double() - s["alpha"])[won].abs().max()) <= A.ALPHA_TOL
    # d = alpha / |grad|: both factors within their bounds
    gn = s["grad"][won].norm(dim=-1).clamp(min=A.G_MIN)
    d_tol = A.ALPHA_TOL / gn + s["d"][won].abs() * (A.GRAD_TOL * big / gn) + 1e-6 * s["d"][won].abs()
    assert ((cpu(out["d"]).double()[won] - s["d"][won]).abs() <= d_tol).all()
    g = cpu(out["grad"])
    nrm = cpu(out["normal"])
    want_n = torch.where(g.norm(dim=-1, keepdim=True) > 0, -g / g.norm(dim=-1, keepdim=True).clamp(min=1e-30), torch.zeros_like(g))
    assert float((nrm - want_n).abs().max()) <= 1e-6             # (the same formula, rounded by the host here)


def test_surface_of_one_point_and_of_a_cloud_in_no_box(dev, surfaced):
    ref, mp, out, _, _ = surfaced("main")
    count = ref["cand"].sum(0)
    for n in (int(torch.argmax(count)), int(torch.argmin(count))):          # a point in three boxes, a point in none
        one = mp.surface(ref["points"][n:n + 1])
        for k in out:
            assert torch.equal(one[k], out[k][n:n + 1]), (n, k)
    far = torch.from_numpy(ref["points"]) + 50.0
    st = {}
    res = mp.surface(far, stats=st)
    assert st["pairs"] == 0
    assert (res["obj"] == -1).all() and (res["obj_id"] == -1).all() and torch.isinf(res["d"]).all()
    assert (res["grad"] == 0).all() and (res["normal"] == 0).all() and (res["alpha"] == 0).all()


def test_select_ties_go_to_the_lower_pair(dev):
    pair_pt = torch.tensor([0, 1, 0, 1, 2], dtype=torch.int32, device=dev)
    alpha = torch.tensor([0.5, -0.25, -0.5, 0.25, 3.0], device=dev)
    grad = torch.tensor([[1.0, 0, 0], [0, 2.0, 0], [0, 0, 1.0], [2.0, 0, 0], [0, 0, 0]], device=dev)
    best = torch.full((4,), -1, dtype=torch.int64, device=dev)
    g_min = 2.0 ** -10                                                       # (a power of two: the quotients below are exact)
    ops.mapalign_select(4, pair_pt, alpha, grad, g_min, best)
    seg_off = torch.tensor([0, 2, 5], dtype=torch.int64, device=dev)
    obj, pair, d, a, g = ops.mapalign_resolve(best, seg_off, alpha, grad, g_min, want_pair=True)
    assert cpu(pair).tolist() == [0, 1, 4, -1] and cpu(obj).tolist() == [0, 0, 1, -1]
    assert cpu(d).tolist() == [0.5, -0.125, 3072.0, float("inf")]           # |grad| = 0: the floor g_min
    dk, pk = ops.mapalign_key_decode(cpu(best).numpy().view(np.uint64))
    assert pk.tolist() == [0, 1, 4, -1] and dk.tolist() == [0.5, 0.125, 3072.0, float("inf")]
    assert cpu(a).tolist() == [0.5, -0.25, 3.0, 0.0] and cpu(g).tolist() == [[1.0, 0, 0], [0, 2.0, 0], [0, 0, 0], [0, 0, 0]]


# --------------------------------------------------------------------------------------------------------- accumulate
@pytest.mark.parametrize("N", [1, 256, 257, 2049])
def test_accumulate_against_fp64_sums(dev, N):
    rs = np.random.RandomState(N)
    q = torch.from_numpy(rs.uniform(-2, 2, (N, 3)).astype(np.float32))
    grad = torch.from_numpy((rs.randn(N, 3) * 10).astype(np.float32))
    alpha = torch.from_numpy((rs.randn(N) * 0.8).astype(np.float32))          # |d| around 0.05: both sides of tau
    obj = torch.from_numpy(rs.randint(-1, 4, N).astype(np.int32))
    if N > 4:
        grad[3] = 0                                                           # the floor: d = alpha / g_min, an outlier
        alpha[4] = 0
    obj[0] = 1
    alpha[0], grad[0] = 0.1, torch.tensor([3.0, 0.0, 4.0])                     # |d| = 0.02: at least one inlier
    pivot = [0.25, -0.5, 0.125]
    got = ops.mapalign_accumulate(q.to(dev), obj.to(dev), alpha.to(dev), grad.to(dev), pivot, A.TAU, A.G_MIN)
    again = ops.mapalign_accumulate(q.to(dev), obj.to(dev), alpha.to(dev), grad.to(dev), pivot, A.TAU, A.G_MIN)
    assert got.dtype == torch.float64 and got.shape == (29,) and torch.equal(got, again)
    want = A.normal_eq_spec(q, obj, alpha, grad, pivot)
    assert 1 <= int(want[28]) < max(N, 2) and float(got[28]) == float(want[28])
    err = (cpu(got) - want).abs()
    rel = float((err / want.abs().clamp(min=1e-300)).max())
    print(f"N = {N}: {int(want[28])} inliers, largest relative error of an entry {rel:.2e}")
    assert (err <= 1e-12 * want.abs()).all()


# ------------------------------------------------------------------------------------------------------ label's normal
@pytest.mark.parametrize("scene,bg", [("main", 32), ("bg", 128)])
def test_label_with_normals(surfaced, scene, bg):
    ref, mp, _, _, _ = surfaced(scene, bg)
    pts = ref["points"]
    plain = mp.label(pts, want_color=True)
    mp._keep_pairs = True
    out = mp.label(pts, want_color=True, want_normal=True)
    pairs, mp._keep_pairs = mp._last_pairs, False
    assert set(out) == set(plain) | {"grad", "normal"}
    for k in plain:
        assert out[k].dtype == plain[k].dtype and torch.equal(out[k], plain[k]), k
    win = cpu(pairs["out_pair"]).long()
    lab = cpu(out["obj"]) >= 0
    assert torch.equal(win >= 0, lab) and bool(lab.any())
    g = cpu(pairs["pair_grad"])[win.clamp(min=0)]
    g = torch.where(lab[:, None], g, torch.zeros_like(g))
    assert torch.equal(cpu(out["grad"]), g)
    n = g.norm(dim=-1, keepdim=True)
    assert float((cpu(out["normal"]) - torch.where(n > 0, -g / n.clamp(min=1e-30), torch.zeros_like(g))).abs().max()) <= 1e-6
    assert (cpu(out["normal"])[~lab] == 0).all() and ((cpu(out["normal"])[lab].norm(dim=-1) - 1).abs() < 1e-6).all()
    # the winner's gradient is the spec's for that object
    _, _, _, _, (_, grad) = surfaced(scene, bg)
    obj = cpu(out["obj"]).long()
    want = grad[obj.clamp(min=0), torch.arange(len(pts))]
    assert A.rel_grad_err(cpu(out["grad"])[lab], want[lab], float(grad.norm(dim=-1).max())) <= A.GRAD_TOL


# ------------------------------------------------------------------------------------------------------------ autograd
@pytest.mark.parametrize("hidden", [32, 128])
def test_positions_are_differentiable_through_the_modules(dev, hidden):
    ref = U.reference("bg", 128)
    obj = ref["objs"][0 if hidden == 128 else 2]
    t = make_trainer(obj, dev)
    x = torch.from_numpy(ref["points"][:70]).to(dev)
    w = torch.from_numpy(np.random.RandomState(0).randn(70).astype(np.float32)).to(dev)

    def run(need_pts):
        t.pe.zero_grad()
        p = x.clone().requires_grad_(need_pts)
        alpha, _, _ = t.fc_occ_map(t.pe(p), do_clip=False)
        (alpha.squeeze(-1) * w).sum().backward()
        return p.grad, t.pe.B_layer.weight.grad.clone()

    none, dB0 = run(False)
    g, dB1 = run(True)
    assert none is None and torch.equal(dB0, dB1)                             # d_B: what the backward gave before
    _, g64 = A.field(dict(obj, obj_center=0.0), x.cpu().double())
    want = g64 * w.cpu().double()[:, None]
    err = A.rel_grad_err(g, want)
    print(f"autograd d pts, hidden {hidden}: {err:.3e}")
    assert err <= A.GRAD_TOL


# ----------------------------------------------------------------------------------------------------------- alignment
@pytest.fixture(scope="module")
def clouds():
    def get(bg):
        cloud, _ = A.surface_cloud(bg)
        T_true = A.rigid(2.0, 0.03)
        own = ((cloud - T_true[:3, 3]) @ T_true[:3, :3]).float()              # the cloud in its own frame, fp32 data
        return cloud, T_true, own
    return get


@pytest.mark.parametrize("bg", [128, 32])
def test_fit_recovers_the_pose(dev, clouds, bg):
    objs, _ = U.background_scene(bg)
    cloud, T_true, own = clouds(bg)
    mp = make_mp(objs, dev)
    al = map_align.MapAlign(mp)
    res = al.fit(own.to(dev), iters=10)
    rot, tr = A.pose_error(res["T"], T_true)
    rms = ["%.2e" % h["rms"] for h in res["history"]]
    print(f"bg {bg}: {len(rms)} iterations, rms {rms}, pose error {rot:.2e} rad {tr:.2e} m, "
          f"inliers {res['history'][0]['inliers']}, cond {res['history'][0]['cond']:.2f}")
    assert res["converged"] and len(res["history"]) <= 10
    assert res["T"].dtype == np.float64 and rot <= A.POSE_TOL and tr <= A.POSE_TOL
    spec = A.fit_spec(objs, own, iters=1, fp32_q=True)
    assert abs(res["history"][0]["inliers"] - spec["history"][0]["inliers"]) <= A.AMBIGUOUS_CAP * len(own)
    again = al.fit(own.to(dev), iters=10)
    assert np.array_equal(again["T"], res["T"]) and json.dumps(again["history"]) == json.dumps(res["history"])
    # the same through a budget that halves every call, and from an explicit T0
    seg = ops.mappoints_count(own.to(dev), mp.boxes)[1]
    st = {}
    small = map_align.MapAlign(make_mp(objs, dev, pair_budget_bytes=mp._field_bytes(seg) // 2))
    halved = small.fit(own.to(dev), T0=np.eye(4), iters=10, stats=st)
    assert st["calls"] > len(halved["history"]) and np.array_equal(halved["T"], res["T"])


def test_fit_refuses_what_it_cannot_determine(dev, clouds):
    objs, _ = U.background_scene(32)
    cloud, T_true, own = clouds(32)
    al = map_align.MapAlign(make_mp(objs, dev))
    few = al.fit(cloud[120:124].float().to(dev), iters=5)                     # four points of one object's surface
    assert few["converged"] is False and np.isfinite(few["T"]).all() and np.array_equal(few["T"], np.eye(4))
    assert few["history"][-1]["inliers"] < 6 and len(few["history"]) == 1
    nowhere = al.fit((cloud.float() + 50.0).to(dev), iters=5)                 # no candidate pair at all
    assert nowhere["converged"] is False and nowhere["history"][-1]["inliers"] == 0
    assert np.array_equal(nowhere["T"], np.eye(4))


@pytest.mark.parametrize("distinct", [1, 2])
def test_fit_refuses_a_rank_deficient_cloud(dev, clouds, distinct):
    """Enough inliers, but they cannot determine the pose: one surface point sixteen times over (its normal fixes one
    translation; about the pivot, which is that point, no rotation acts), or two points eight times each (A has rank 2 of
    6).  The sums come from objnerf_mapalign_accumulate; cond(A) > 1e12 ends the run at the first iteration with the T it
    was given."""
    objs, _ = U.background_scene(32)
    cloud, _, _ = clouds(32)
    al = map_align.MapAlign(make_mp(objs, dev))
    pts = cloud[[130, 190][:distinct]].float().repeat(16 // distinct, 1)
    T0 = A.rigid(0.2, 0.005).numpy()
    res = al.fit(pts.to(dev), T0=T0, iters=5)
    last = res["history"][-1]
    print(f"{distinct} distinct point(s): inliers {last['inliers']}, cond {last['cond']:.3e}, rms {last['rms']:.2e}")
    assert res["converged"] is False and len(res["history"]) == 1
    assert last["inliers"] == 16 and not last["cond"] <= map_align.MAX_COND
    assert np.isfinite(res["T"]).all() and np.array_equal(res["T"], T0)


def test_fit_frame_back_projects_valid_depths(dev, clouds):
    objs, _ = U.background_scene(32)
    mp = make_mp(objs, dev)
    W, H = 24, 20
    rays = ops.rays_dirs(W, H, 20.0, 20.0, 12.0, 10.0, dev)
    depth = torch.full((W, H), 1.5, device=dev)
    depth[::8, :] = 0.0                                                       # invalid rows
    seen = []

    class Spy(map_align.MapAlign):
        def fit(self, points, T0=None, **kw):
            seen.append((points, T0, kw))
            return {"T": np.eye(4), "converged": False, "history": []}

    T0 = A.rigid(1.0, 0.01).numpy()
    Spy(mp).fit_frame(depth, T0, rays, stride=4, iters=3)
    pts, T_got, kw = seen[0]
    d, r = depth[::4, ::4], rays[::4, ::4]
    ok = d > 0
    assert torch.equal(pts, (d[..., None] * r)[ok]) and 0 < len(pts) < d.numel()
    assert T_got is T0 and kw == {"iters": 3}
    assert ((pts[:, 2] - 1.5).abs() < 1e-6).all()                            # z-depth: the ray's z component is 1
    empty = Spy(mp).fit_frame(torch.zeros(W, H, device=dev), T0, rays)
    assert empty["converged"] is False and np.array_equal(empty["T"], T0)


def test_cli_from_checkpoints(dev, tmp_path, capsys):
    ref = U.reference("cli")
    logdir, outdir = tmp_path / "log", tmp_path / "out"
    for o in ref["objs"]:
        t = make_trainer(o, dev)
        d = logdir / "ckpt" / str(o["obj_id"])
        os.makedirs(d)
        torch.save({"epoch": 0, "FC_state_dict": t.fc_occ_map.state_dict(), "PE_state_dict": t.pe.state_dict(),
                    "obj_id": o["obj_id"], "bbox": make_box(o), "obj_scale": t.obj_scale, "clip_feat": None,
                    "caption_feat": None, "semantic_id": o["class_id"]}, str(d / f"obj_{o['obj_id']}.pth"))
    cloud = torch.cat([A.surface_points(o, 400, 20 + k)[:100] for k, o in enumerate(ref["objs"])])
    T_true = A.rigid(2.0, 0.03)
    own = ((cloud - T_true[:3, 3]) @ T_true[:3, :3]).float().numpy()
    T0 = A.rigid(0.5, 0.01).numpy()
    np.save(tmp_path / "cloud.npy", own)
    np.savetxt(tmp_path / "T0.txt", T0)
    map_align.main(["--logdir", str(logdir), "--points", str(tmp_path / "cloud.npy"), "--init", str(tmp_path / "T0.txt"),
                    "--out", str(outdir), "--iters", "12", "--device", str(dev)])
    assert f"{len(own)} points, converged True" in capsys.readouterr().out
    rec = json.load(open(outdir / "align.json"))
    api = map_align.MapAlign(make_mp(ref["objs"], dev)).fit(own, T0=T0, iters=12)
    assert np.array_equal(np.array(rec["T"]), api["T"]) and rec["converged"] and len(rec["history"]) == len(api["history"])
    rot, tr = A.pose_error(api["T"], T_true)
    assert rot <= A.POSE_TOL and tr <= A.POSE_TOL
    from openobj_amd import mesh
    v = mesh.read_ply(str(outdir / "aligned.ply"))[0]
    assert np.abs(v - cloud.numpy()).max() < 1e-4
