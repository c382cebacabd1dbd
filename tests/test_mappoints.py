"""openobj_amd.map_points without a GPU: the specification (tests/mappoints_util.py) against the oracle's eval_points
chain and a literal reading of the rules, confusion / miou against hand-worked cases, the host-side validation, and the
conditions the GPU tests (tests/test_mappoints_gpu.py) rely on, asserted on the specification alone."""
import types

import numpy as np
import pytest
import torch

import mappoints_util as U
from oracle import objnerf_oracle as O
from openobj_amd import _lib, map_points, ops


# ---------------------------------------------------------------------------------------------------- specification
def test_spec_scores_are_the_oracle_eval_points_chain():
    """oracle_eval = embed_stacked + mlp_forward_stacked (what tests/test_hip_parity.py holds ops.eval_points to), at
    p - obj_center."""
    ref = U.reference("main")
    objs, pts = ref["objs"], torch.from_numpy(ref["points"])
    K = len(objs)
    fc = [torch.stack([o["p"][i] for o in objs]) for i in range(18)]
    B = torch.stack([o["B"] for o in objs])
    shifted = torch.stack([pts - torch.tensor(np.float32(o["obj_center"])) for o in objs])
    emb = O.embed_stacked(B, torch.full((K,), 2.0), shifted)
    a, c, f = O.mlp_forward_stacked(fc, emb, True)
    assert (ref["alpha"] - a.squeeze(-1)).abs().max() < 1e-5
    assert (ref["color"] - c).abs().max() < 1e-6
    assert (ref["feat"] - f).abs().max() < 1e-5 * max(1.0, float(f.abs().max()))


def _label_by_the_rules(alpha, cand, is_bg):
    K, N = alpha.shape
    obj, out = np.full(N, -1, np.int32), np.full(N, -np.inf, np.float32)
    for n in range(N):
        best = {False: None, True: None}            # per group (foreground, background): (alpha, k)
        for k in range(K):
            if not cand[k, n]:
                continue
            out[n] = max(out[n], alpha[k, n])
            if alpha[k, n] > 0 and (best[is_bg[k]] is None or alpha[k, n] > best[is_bg[k]][0]):
                best[is_bg[k]] = (alpha[k, n], k)
        win = best[False] or best[True]
        if win is not None:
            out[n], obj[n] = win
    return obj, out


@pytest.mark.parametrize("scene,bg", [("main", 32), ("bg", 32), ("bg", 128)])
def test_label_spec_follows_the_rules(scene, bg):
    ref = U.reference(scene, bg)
    obj, alpha = _label_by_the_rules(ref["alpha"].numpy(), ref["cand"].numpy(), ref["is_bg"])
    assert np.array_equal(ref["spec"]["obj"].numpy(), obj)
    assert np.array_equal(ref["spec"]["alpha"].numpy(), alpha)
    lab = obj >= 0
    assert (ref["spec"]["color"][~lab] == 0).all() and (ref["spec"]["part_feat"][~lab] == 0).all()
    n = np.nonzero(lab)[0][0]
    assert torch.equal(ref["spec"]["color"][n], ref["color"][obj[n], n])
    assert torch.equal(ref["spec"]["part_feat"][n], ref["feat"][obj[n], n])


def test_label_spec_tie_and_background_rule():
    """Hand-made alphas: equal alphas go to the lower position; the background never hides an occupied object."""
    alpha = torch.tensor([[5.0, 5.0, -1.0, 9.0, -3.0],       # background
                          [2.0, 0.5, -2.0, -1.0, -4.0],
                          [2.0, 7.0, -0.5, -1.0, -2.0]])
    cand = torch.tensor([[1, 1, 1, 1, 0], [1, 1, 1, 1, 0], [1, 0, 1, 1, 0]], dtype=torch.bool)
    s = U.label_spec(alpha, cand, [True, False, False])
    assert s["obj"].tolist() == [1, 1, -1, 0, -1]
    assert s["alpha"].tolist() == [2.0, 0.5, -0.5, 9.0, -np.inf]
    assert s["ambiguous"].tolist() == [True, False, False, False, False]      # the tie itself is an ambiguous point


# ------------------------------------------------------------------------------------------------ confusion / mIoU
def test_confusion_and_miou_hand_worked():
    gt = torch.tensor([0, 0, 0, 1, 1, 2, -1, 2])
    pred = torch.tensor([0, 0, 1, 1, -1, 0, 1, 7])
    conf = map_points.confusion(pred, gt, 3)
    # ground truth 0: two as 0, one as 1; 1: one as 1, one unlabelled; 2: one as 0, one outside the classes; gt -1 ignored
    assert conf.tolist() == [[2, 1, 0, 0], [0, 1, 0, 1], [1, 0, 0, 1]]
    assert np.array_equal(conf.numpy(), U.confusion_spec(pred, gt, 3))
    r = map_points.miou(conf)
    # IoU 0: tp 2, gt 3, predicted 3 -> 2 / 4;  1: tp 1, gt 2, predicted 2 -> 1 / 3;  2: tp 0, gt 2, predicted 0 -> 0
    assert np.allclose(r["iou"].numpy(), [0.5, 1.0 / 3.0, 0.0])
    assert abs(r["miou"] - (0.5 + 1.0 / 3.0) / 3.0) < 1e-12
    assert abs(r["accuracy"] - 3.0 / 7.0) < 1e-12


def test_miou_skips_absent_classes_and_ignore_value():
    gt = torch.tensor([0, 0, 3, 3, 255])
    pred = torch.tensor([0, 3, 3, 3, 0])
    conf = map_points.confusion(pred, gt, 4, ignore=255)
    assert int(conf.sum()) == 4
    r = map_points.miou(conf)
    assert torch.isnan(r["iou"][1]) and torch.isnan(r["iou"][2])
    assert np.allclose([float(r["iou"][0]), float(r["iou"][3])], [0.5, 2.0 / 3.0])
    assert abs(r["miou"] - (0.5 + 2.0 / 3.0) / 2.0) < 1e-12
    assert abs(r["accuracy"] - 0.75) < 1e-12
    rs = np.random.RandomState(0)
    g, p = rs.randint(-1, 6, 500), rs.randint(-1, 7, 500)
    assert np.array_equal(map_points.confusion(torch.from_numpy(p), torch.from_numpy(g), 6).numpy(), U.confusion_spec(p, g, 6))
    with pytest.raises(ValueError):
        map_points.confusion(torch.zeros(3), torch.zeros(4), 2)


# -------------------------------------------------------------------------------------------------- host validation
def _fake_trainer(hidden=32):
    _, ps = _lib.param_layout(hidden)
    return types.SimpleNamespace(hidden_feature_size=hidden, clip_point_feature_size=512, n_unidir_funcs=5, obj_scale=2.0,
                                 device="cpu", arena=types.SimpleNamespace(params=torch.zeros(1, ps)))


def _box(extent=(1.0, 1.0, 1.0)):
    return types.SimpleNamespace(center=np.zeros(3), R=np.eye(3), extent=np.asarray(extent))


def test_host_validation():
    with pytest.raises(_lib.ObjnerfError, match="no object"):
        map_points.MapPoints([])
    with pytest.raises(_lib.ObjnerfError, match="no box"):
        map_points.MapPoints([map_points.MapObject(_fake_trainer(), _box(), 1), map_points.MapObject(_fake_trainer(), None, 2)])
    with pytest.raises(_lib.ObjnerfError, match="multiple of 32"):
        map_points.MapPoints([map_points.MapObject(_fake_trainer(48), _box(), 1)], device="cpu")
    with pytest.raises(_lib.ObjnerfError, match="center"):
        map_points.box_record(types.SimpleNamespace(center=np.zeros(2), R=np.eye(3), extent=np.ones(3)))
    mp = map_points.MapPoints([map_points.MapObject(_fake_trainer(), _box(), 4, 2),
                               map_points.MapObject(_fake_trainer(128), _box((2, 2, 2)), 0, 0)], device="cpu")
    assert mp.is_bg == [False, True] and mp.wide == [1] and mp.info_host.tolist() == [[0, 0], [-1, 1]]
    rec = mp.boxes[1].numpy()
    assert rec.dtype == np.float32 and rec[12:15].tolist() == [1.0, 1.0, 1.0] and rec[3:12].tolist() == np.eye(3).reshape(-1).tolist()
    for bad in (torch.zeros(5, 2), torch.zeros(5), torch.zeros(2, 5, 3)):
        with pytest.raises(_lib.ObjnerfError, match=r"\[N, 3\]"):
            mp.label(bad)
    with pytest.raises(_lib.ObjnerfError, match="chunk"):
        mp.label(torch.zeros(5, 3), chunk=0)
    with pytest.raises(_lib.ObjnerfError, match="GPU tensor"):       # there is no CPU path
        mp.label(torch.zeros(5, 3))


def test_pair_overflow_is_refused_on_the_host():
    assert ops.mappoints_check_pairs(2 ** 31 - 1) == 2 ** 31 - 1
    with pytest.raises(_lib.ObjnerfError, match="31 bits"):
        ops.mappoints_check_pairs(2 ** 31)


def test_abi_is_14():
    assert _lib.ABI_VERSION == 14 and _lib.lib().objnerf_abi_version() == 14


# --------------------------------------------------------------- what the GPU tests assume, on the specification alone
def test_main_scene_conditions():
    ref = U.reference("main")
    objs, pts, cand = ref["objs"], ref["points"], ref["cand"].numpy()
    assert pts.shape == (3 * 64 + 37, 3) and pts.dtype == np.float32
    assert [o["hidden"] for o in objs] == [32] * 5
    for o in objs:                                   # rotated: no axis of a box lies along a world axis
        assert np.abs(o["R"]).max() < 0.999 and abs(np.linalg.det(o["R"]) - 1.0) < 1e-12
    seg = ref["seg_off"].tolist()
    assert seg[2] - seg[1] == 0                      # an empty segment, in the middle of the list
    assert seg[3] - seg[2] == 64                     # a segment of exactly one tile
    assert seg[1] - seg[0] > 64 and seg[-1] == len(ref["pair_pt"])
    per_point = cand.sum(0)
    assert {0, 1, 2, 3} <= set(per_point.tolist())
    assert U.face_margin(pts, objs) >= U.FACE_MARGIN
    # the fp64 box test agrees with the fp32 one everywhere
    for k, o in enumerate(objs):
        l, half = U.box_locals(pts, o, torch.float64)
        assert np.array_equal((l.abs() <= half).all(dim=1).numpy(), cand[k])
    s = ref["spec"]
    assert int((s["obj"] < 0).sum()) >= 10 and int((s["obj"] >= 0).sum()) >= 40
    assert set(s["obj"][s["obj"] >= 0].tolist()) == {0, 2, 3, 4}       # every object with candidates wins somewhere
    assert s["ambiguous"].float().mean() <= U.AMBIGUOUS_CAP


@pytest.mark.parametrize("bg", [32, 128])
def test_background_scene_conditions(bg):
    ref = U.reference("bg", bg)
    objs, pts, cand, alpha = ref["objs"], ref["points"], ref["cand"], ref["alpha"]
    assert objs[0]["hidden"] == bg and ref["is_bg"] == [True, False, False, False, False]
    assert bool(cand[0].all())                       # the background box contains the whole cloud
    assert U.face_margin(pts, objs) >= U.FACE_MARGIN
    s = ref["spec"]
    assert s["ambiguous"].float().mean() <= U.AMBIGUOUS_CAP
    fg_occ = (cand[1:] & (alpha[1:] > 0)).any(dim=0)
    # the rule is exercised: points with an occupied object whose background alpha is the larger one, points that go to the
    # background, and points nobody claims
    hidden = fg_occ & (alpha[0] > s["alpha"])
    assert int(hidden.sum()) >= 5 and bool((s["obj"][hidden] > 0).all())
    assert int((s["obj"] == 0).sum()) >= 5 and not bool((s["obj"][fg_occ] == 0).any())
    assert int((s["obj"] < 0).sum()) >= 1


@pytest.mark.parametrize("bg", [64, 96])
def test_other_background_widths_conditions(bg):
    """The scenes that drive the head's hidden-64 and any-width instantiations: unambiguous, and the background wins
    somewhere so that its head runs."""
    ref = U.reference("bg", bg)
    assert ref["objs"][0]["hidden"] == bg
    assert ref["spec"]["ambiguous"].float().mean() <= U.AMBIGUOUS_CAP
    assert int((ref["spec"]["obj"] == 0).sum()) >= 5 and int((ref["spec"]["obj"] > 0).sum()) >= 5
