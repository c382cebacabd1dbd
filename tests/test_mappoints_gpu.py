"""openobj_amd.map_points on the GPU against its specification (tests/mappoints_util.py; tests/test_mappoints.py asserts
the conditions on the scenes that these tests rely on).  Bounds: pair alpha <= 1e-4, winners' colour <= 1e-5, winners'
feature <= 1e-4 of the tensor's largest entry -- those of tests/test_hip_parity.py:60-62 for the same chain; lists, labels
and everything about order are exact."""
import json
import os

import numpy as np
import pytest
import torch

import mappoints_util as U
from openobj_amd import cfg as ocfg
from openobj_amd import map_points, mesh, ops, trainer, utils

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


@pytest.fixture(scope="module")
def labelled(dev):
    """(scene, bg width) -> (reference, MapPoints, label(points, colour, feature) with the pair buffers kept), once."""
    cache = {}

    def get(scene, bg=32):
        if (scene, bg) not in cache:
            ref = U.reference(scene, bg)
            mp = make_mp(ref["objs"], dev)
            mp._keep_pairs = True
            out = mp.label(ref["points"], want_color=True, want_feat=True)
            pairs, mp._keep_pairs = mp._last_pairs, False
            cache[(scene, bg)] = (ref, mp, out, pairs)
        return cache[(scene, bg)]

    return get


def cpu(t):
    return t.detach().cpu()


def assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------------ candidate lists
def test_candidate_lists_are_the_specification(dev, labelled):
    ref, mp, _, _ = labelled("main")
    pts = torch.from_numpy(ref["points"]).to(dev)
    seg_off, seg, pair_pt = ops.mappoints_candidates(pts, mp.boxes)
    assert seg_off.dtype == torch.int64 and pair_pt.dtype == torch.int32
    assert torch.equal(cpu(seg_off), ref["seg_off"]) and seg == ref["seg_off"].tolist()
    assert torch.equal(cpu(pair_pt), ref["pair_pt"])
    # the count blocks of 256 points below, at and above a boundary and across several, over [A, EMPTY, B]: the middle
    # segment is empty, so the scan and the emit step over it.  Points drawn from the cloud with repetition (a candidate
    # list does not care), the specification's mask gathered for them.
    rs = np.random.RandomState(5)
    for n in (255, 256, 257, 1025):
        idx = rs.randint(0, len(ref["points"]), n)
        cand = ref["cand"][:3, torch.from_numpy(idx)]
        assert bool(cand[0].any()) and not bool(cand[1].any()) and bool(cand[2].any())
        want_off, want_pt = U.candidate_lists(cand)
        seg_off, seg, pair_pt = ops.mappoints_candidates(torch.from_numpy(ref["points"][idx]).to(dev), mp.boxes[:3].contiguous())
        assert torch.equal(cpu(seg_off), want_off) and seg == want_off.tolist() and torch.equal(cpu(pair_pt), want_pt), n


def test_candidate_lists_of_one_point(dev, labelled):
    ref, mp, _, _ = labelled("main")
    count = ref["cand"].sum(0)
    for n in (int(torch.argmax(count)), int(torch.argmin(count))):          # a point in three boxes, a point in none
        seg_off, seg, pair_pt = ops.mappoints_candidates(torch.from_numpy(ref["points"][n:n + 1]).to(dev), mp.boxes)
        want_off, want_pt = U.candidate_lists(ref["cand"][:, n:n + 1])
        assert torch.equal(cpu(seg_off), want_off) and torch.equal(cpu(pair_pt), want_pt)
        out = mp.label(ref["points"][n:n + 1])
        assert int(out["obj"][0]) == int(ref["spec"]["obj"][n]) or bool(ref["spec"]["ambiguous"][n])


# ------------------------------------------------------------------------------------------------------ per-pair values
@pytest.mark.parametrize("scene,bg", [("main", 32), ("bg", 32), ("bg", 128)])
def test_pair_alpha_against_the_oracle(labelled, scene, bg):
    ref, _, _, pairs = labelled(scene, bg)
    assert pairs["seg"] == ref["seg_off"].tolist()
    pt = ref["pair_pt"].long()
    k_of = torch.repeat_interleave(torch.arange(len(ref["objs"])), ref["seg_off"][1:] - ref["seg_off"][:-1])
    err = (cpu(pairs["pair_alpha"]) - ref["alpha"][k_of, pt]).abs().max().item()
    print(f"pair_alpha max error {err:.3e}")
    assert err <= 1e-4


@pytest.mark.parametrize("scene,bg", [("main", 32), ("bg", 32), ("bg", 128), ("bg", 64), ("bg", 96)])
def test_winners_and_their_values(labelled, scene, bg):
    ref, mp, out, _ = labelled(scene, bg)
    s = ref["spec"]
    ok = ~s["ambiguous"]
    obj = cpu(out["obj"])
    assert obj.dtype == torch.int32 and torch.equal(obj[ok], s["obj"][ok])
    ids = torch.tensor([o["obj_id"] for o in ref["objs"]] + [-1])
    cls = torch.tensor([o["class_id"] for o in ref["objs"]] + [-1])
    assert torch.equal(cpu(out["obj_id"]), ids[obj.long()]) and torch.equal(cpu(out["class_id"]), cls[obj.long()])
    # alpha: the winner's (or the largest candidate's); -inf exactly where the point has no candidate
    none = ~ref["cand"].any(dim=0)
    a = cpu(out["alpha"])
    assert bool((a[none] == -np.inf).all()) and bool(torch.isfinite(a[~none]).all())
    same = ok & ~none & (obj == s["obj"])
    e_a = (a[same] - s["alpha"][same]).abs().max().item()
    lab = same & (obj >= 0)
    assert int(lab.sum()) >= 30
    e_c = (cpu(out["color"])[lab] - s["color"][lab]).abs().max().item()
    f_ref = s["part_feat"][lab]
    e_f = (cpu(out["part_feat"])[lab] - f_ref).abs().max().item() / f_ref.abs().max().item()
    print(f"alpha {e_a:.3e} colour {e_c:.3e} feature {e_f:.3e} (relative to the largest entry)")
    assert e_a <= 1e-4 and e_c <= 1e-5 and e_f <= 1e-4


@pytest.mark.parametrize("scene,bg", [("main", 32), ("bg", 128)])
def test_unlabelled_points_are_exactly_empty(labelled, scene, bg):
    _, _, out, _ = labelled(scene, bg)
    un = out["obj"] < 0
    assert int(un.sum()) >= 1
    assert bool((out["color"][un] == 0).all()) and bool((out["part_feat"][un] == 0).all())
    assert bool((out["obj_id"][un] == -1).all()) and bool((out["class_id"][un] == -1).all())
    assert bool((out["alpha"][un] <= 0).all()) and bool((out["alpha"][~un] > 0).all())
    assert bool((out["part_feat"][~un].abs().sum(dim=1) > 0).all())


def test_normalised_feature(labelled):
    ref, mp, out, _ = labelled("bg", 128)
    o2 = mp.label(ref["points"], want_feat=True, normalise_feat=True)
    lab = out["obj"] >= 0
    f = out["part_feat"][lab]
    assert torch.allclose(o2["part_feat"][lab], f / f.norm(dim=-1, keepdim=True), rtol=0, atol=1e-6)
    assert bool((o2["part_feat"][~lab] == 0).all())


# ------------------------------------------------------------------------------------------------------------ tie-break
def test_equal_alpha_goes_to_the_lower_position(dev, labelled):
    ref, _, _, _ = labelled("main")
    c = ref["objs"][3]                                           # the object that is occupied most often
    twin = dict(c, obj_id=c["obj_id"] + 100)
    one = make_mp([c], dev).label(ref["points"], want_color=True, want_feat=True)
    two = make_mp([c, twin], dev).label(ref["points"], want_color=True, want_feat=True)
    three = make_mp([ref["objs"][1], c, twin], dev).label(ref["points"])      # behind an object with an empty segment
    assert int((one["obj"] == 0).sum()) >= 20
    assert not bool((two["obj"] == 1).any()) and not bool((three["obj"] == 2).any())
    assert_same({k: v for k, v in one.items()}, {k: v for k, v in two.items()})
    assert torch.equal(three["obj"], torch.where(one["obj"] == 0, 1, -1).to(torch.int32)) and torch.equal(three["alpha"], one["alpha"])


# ------------------------------------------------------------------------------------------------------ background rule
@pytest.mark.parametrize("bg", [32, 128])
def test_background_never_hides_an_object(labelled, bg):
    ref, _, out, pairs = labelled("bg", bg)
    K, N = ref["alpha"].shape
    # judged on what the GPU itself computed: its own pair alphas, scattered to [K, N]
    k_of = torch.repeat_interleave(torch.arange(K), ref["seg_off"][1:] - ref["seg_off"][:-1])
    a = torch.full((K, N), -np.inf)
    a[k_of, cpu(pairs["pair_pt"]).long()] = cpu(pairs["pair_alpha"])
    fg_occ = (a[1:] > 0).any(dim=0)
    obj = cpu(out["obj"])
    assert not bool((obj[fg_occ] == 0).any())
    hidden = fg_occ & (a[0] > a[1:].max(dim=0).values)            # the background's alpha is the larger one, and it loses
    assert int(hidden.sum()) >= 5 and bool((obj[hidden] > 0).all())
    assert int((obj == 0).sum()) >= 5
    # and the labels are exactly the rules applied to those alphas
    mine = U.label_spec(a, torch.isfinite(a), ref["is_bg"])
    assert torch.equal(obj, mine["obj"]) and torch.equal(cpu(out["alpha"]), mine["alpha"])


# ----------------------------------------------------------------------------------- position independence, determinism
@pytest.mark.parametrize("scene,bg", [("main", 32), ("bg", 128)])
def test_permutation_repeat_and_chunks_are_bit_equal(dev, labelled, scene, bg):
    ref, mp, out, _ = labelled(scene, bg)
    pts = ref["points"]
    again = mp.label(pts, want_color=True, want_feat=True)
    assert_same(out, again)
    perm = torch.from_numpy(np.random.RandomState(3).permutation(len(pts)))
    shuffled = mp.label(pts[perm.numpy()], want_color=True, want_feat=True)
    assert_same({k: v[perm.to(dev)] for k, v in out.items()}, shuffled)
    assert_same(out, mp.label(pts, want_color=True, want_feat=True, chunk=100))
    # a byte budget the pair buffers exceed: label() halves the cloud until they fit
    small = make_mp(ref["objs"], dev, pair_budget_bytes=20000)
    assert small._pair_bytes(ref["seg_off"].tolist(), True, True) > 20000
    assert_same(out, small.label(pts, want_color=True, want_feat=True))
    plain = mp.label(pts)
    assert set(plain) == {"obj", "obj_id", "class_id", "alpha"}
    assert torch.equal(plain["obj"], out["obj"]) and torch.equal(plain["alpha"], out["alpha"])


# ----------------------------------------------------------------------------------------------------------- end to end
def test_cli_from_checkpoints(dev, tmp_path, capsys):
    ref = U.reference("cli")
    logdir, outdir = tmp_path / "log", tmp_path / "out"
    for o in ref["objs"] + [dict(ref["objs"][1], obj_id=20, no_box=True)]:
        t = make_trainer(o, dev)
        d = logdir / "ckpt" / str(o["obj_id"])
        os.makedirs(d)
        torch.save({"epoch": 0, "FC_state_dict": t.fc_occ_map.state_dict(), "PE_state_dict": t.pe.state_dict(),
                    "obj_id": o["obj_id"], "bbox": None if o.get("no_box") else make_box(o), "obj_scale": t.obj_scale,
                    "clip_feat": None, "caption_feat": None, "semantic_id": o["class_id"]},
                   str(d / f"obj_{o['obj_id']}.pth"))                          # the dict of vmap.py:556-576
    s = ref["spec"]
    cls = np.array([o["class_id"] for o in ref["objs"]] + [-1])
    gt = cls[s["obj"].numpy()].copy()
    gt[::7] = 4                                                  # some disagreement, some ignored points
    gt[::11] = -1
    np.save(tmp_path / "cloud.npy", ref["points"])
    np.save(tmp_path / "gt.npy", gt)
    map_points.main(["--logdir", str(logdir), "--points", str(tmp_path / "cloud.npy"), "--out", str(outdir), "--color",
                     "--feat", "--gt-class", str(tmp_path / "gt.npy"), "--bg-ids", "0", "--device", str(dev)])
    assert "obj 20: the checkpoint carries no box, skipped" in capsys.readouterr().out
    lab = np.load(outdir / "labels.npz")
    assert set(lab.files) == {"obj", "obj_id", "class_id", "alpha", "color", "part_feat"}
    ok = ~s["ambiguous"].numpy()
    assert s["ambiguous"].float().mean() <= U.AMBIGUOUS_CAP
    assert np.array_equal(lab["obj"][ok], s["obj"].numpy()[ok])
    ids = np.array([o["obj_id"] for o in ref["objs"]] + [-1])
    assert np.array_equal(lab["obj_id"], ids[lab["obj"]]) and np.array_equal(lab["class_id"], cls[lab["obj"]])
    won = ok & (lab["obj"] >= 0)
    assert np.abs(lab["color"][won] - s["color"].numpy()[won]).max() <= 1e-5
    norm = np.linalg.norm(lab["part_feat"][won], axis=1)
    assert np.abs(norm - 1).max() < 1e-5                         # the CLI normalises the feature, as map_vis does
    ev = json.load(open(outdir / "eval.json"))
    n_cls = int(max(lab["class_id"].max(), gt.max())) + 1
    want = map_points.miou(map_points.confusion(torch.from_numpy(lab["class_id"]), torch.from_numpy(gt), n_cls))
    assert ev["n_classes"] == n_cls and ev["miou"] == want["miou"] and ev["accuracy"] == want["accuracy"]
    assert np.array_equal(U.confusion_spec(lab["class_id"], gt, n_cls),
                          map_points.confusion(torch.from_numpy(lab["class_id"]), torch.from_numpy(gt), n_cls).numpy())
    for name in ("instances.ply", "classes.ply"):
        v, _, rgba, f = mesh.read_ply(str(outdir / name))
        assert np.array_equal(v, ref["points"]) and rgba.shape == (len(v), 4) and len(f) == 0


# -------------------------------------------------------------------------------------------- calls without a candidate
def _assert_empty(out, sel):
    assert bool((out["obj"][sel] == -1).all()) and bool((out["obj_id"][sel] == -1).all()) and bool((out["class_id"][sel] == -1).all())
    assert bool((out["alpha"][sel] == -np.inf).all())
    assert bool((out["color"][sel] == 0).all()) and bool((out["part_feat"][sel] == 0).all())


def test_a_call_without_any_candidate(labelled):
    """N = 1 outside every box, and a whole cloud outside every box, with colour and feature: label -1, colour 0, feature
    0, alpha -inf (M = 0: there is no pair buffer to read)."""
    ref, mp, _, _ = labelled("bg", 128)
    far = np.full((1, 3), 50.0, np.float32)
    for pts in (far, far + np.arange(70, dtype=np.float32)[:, None]):
        out = mp.label(pts, want_color=True, want_feat=True, normalise_feat=True)
        assert out["color"].shape == (len(pts), 3) and out["part_feat"].shape == (len(pts), 512)
        _assert_empty(out, slice(None))
    n = int(torch.argmin(labelled("main")[0]["cand"].sum(0)))             # a point of the main scene that no box contains
    ref, mp, full, _ = labelled("main")
    assert not bool(ref["cand"][:, n].any())
    one = mp.label(ref["points"][n:n + 1], want_color=True, want_feat=True)
    _assert_empty(one, slice(None))
    assert_same({k: v[n:n + 1] for k, v in full.items()}, one)


@pytest.mark.parametrize("scene,bg", [("main", 32), ("bg", 128)])
def test_a_chunk_without_any_candidate(labelled, scene, bg):
    """100 points outside every box ahead of the scene's points: with chunk = 100 the first call has no pair at all; the
    result equals the unchunked one bit for bit, and the scene's part equals the scene labelled alone."""
    ref, mp, alone, _ = labelled(scene, bg)
    far = (50.0 + np.arange(300, dtype=np.float32)).reshape(100, 3)
    pts = np.concatenate([far, ref["points"]])
    whole = mp.label(pts, want_color=True, want_feat=True)
    assert_same(whole, mp.label(pts, want_color=True, want_feat=True, chunk=100))
    _assert_empty(whole, slice(0, 100))
    assert_same({k: v[100:] for k, v in whole.items()}, alone)


def test_too_many_pairs_for_the_keys_halves_the_call(labelled, monkeypatch):
    """A call whose pairs would not fit the 31 bits of the keys is split like an over-budget one, decided on the counts
    before pair_pt exists; here the limit is lowered so that the scene's 235 pairs exceed it."""
    ref, mp, out, _ = labelled("main")
    monkeypatch.setattr(ops, "MAPPOINTS_MAX_PAIRS", 60)
    st = {}
    got = mp.label(ref["points"], want_color=True, want_feat=True, stats=st)
    assert st["calls"] >= 4
    assert_same(out, got)
    with pytest.raises(ops.ObjnerfError, match="31 bits"):
        ops.mappoints_candidates(torch.from_numpy(ref["points"]).to(out["obj"].device), mp.boxes)
