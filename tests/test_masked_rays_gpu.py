"""GPU: the fp32 fused training kernel leaves out the work of rays the loss masks out -- label 2
(unknown): everything; label 0 (another object): the colour layer -- per wave of 16 samples and per tile of 128.  What it
leaves out has an exact zero factor in the full computation, so nothing here is a new bound:

  1. loss terms and gradients against the fp64-anchored oracle at the 1e-4 of parity_util, without and with the feature loss;
  2. the production launch bit-equal to the test-hook launch (`relu_masks=`), which leaves nothing out;
  3. the inputs of a fully masked ray are irrelevant: other finite pts / z / gt_depth / gt_rgb (/ gt_feat) on every label-2
     ray, other gt_rgb on every label-0 ray -- the same bits;
  4. the same input twice in one workspace, with a step of other labels in between -- the same bits (nothing stale in the
     staging area).

Labels are placed by hand so that every branch occurs, at K = 3 and

  S = 64 (16 + 48), R = 15   two rays per tile, a wave inside one ray: tiles (1,2) (2,1) (2,2) (0,1) (1,0) (0,0) (0,2), ragged (1)
  S = 10 (1 + 9),   R = 29   12 rays per tile: wave 0 inside the label-2 rays 0, 1 beside wave 1 across rays 1 (label 2) and 2 (label 1)
  S = 16 (4 + 12),  R = 19   8 rays per tile, a wave = a ray
  S = 33 (2 + 31),  R = 13   3 rays per tile, 29 slots without a ray

(2 + 31 and not, say, 8 + 25: with few samples towards the surface the untrained networks leave the opacity of these 33-sample
rays saturated, and where only the opacity term is left its gradients are ~1e-6, below the floor parity_util measures
against: the fp32 oracle itself is then 1e-3 from the fp64 anchor.  With the inputs below it is within 3e-6 in every case.)

in three variants: every object has rays of its own; object 1 has none (the cross-object early return zeroes depth and
colour for all); object 2 has only label-2 rays (that and the opacity term's early return: everything is zero).
The hidden-128 background step, whose kernels leave nothing out, is held to 3 and 4 -- and in fp32 to 1 --
at R = 9 on a 14-sample and a 64-sample shape, in fp32 and bf16, in a poisoned workspace, with workgroups whose rays are
all label 2 (the first and the last one among them)."""
import numpy as np
import pytest
import torch

from conftest import T
from openobj_amd import init as obj_init
from openobj_amd import ops, synthetic
from parity_util import assert_grads, assert_terms, check_flips, oracle_step, unpack_masks

pytestmark = pytest.mark.gpu

H = 32
# object 0's labels, tile by tile
PLACED = {
    (16, 48): [1, 2, 2, 1, 2, 2, 0, 1, 1, 0, 0, 0, 0, 2, 1],
    (1, 9): [2, 2, 1, 0, 0, 2, 2, 2, 1, 1, 0, 2] + [2] * 12 + [0, 0, 2, 0, 1],
    (4, 12): [1, 2, 0, 2, 2, 1, 0, 0] + [0, 2, 0, 0, 2, 2, 0, 2] + [2, 1, 0],
    (2, 31): [1, 2, 0, 2, 2, 2, 0, 0, 2, 1, 0, 1, 0],
}
SHAPES = [(n, len(v)) for n, v in PLACED.items()]
VARIANTS = ["own_rays", "object_without_own_rays", "object_all_unknown"]


def _labels(n, variant):
    l0 = np.array(PLACED[n], np.uint8)
    lab = np.stack([l0, l0[::-1], np.roll(l0, 3)])
    if variant == "object_without_own_rays":
        lab[1][lab[1] == 1] = 0
    elif variant == "object_all_unknown":
        lab[2] = 2
    return lab


def _case(dev, n, R, variant, feat):
    K, (n1, n2) = 3, n
    st = obj_init.init_stacked(K, H, 512, seed=11 + n1)
    arena = ops.ParamArena(K, ops.NetShape(H, 512, 6), dev)
    arena.load_stacked(st)
    b = synthetic.random_batch(K, R, n1, n2, seed=310 + n1, feat_dim=512 if feat else 0)
    b["labels"] = _labels(n, variant)
    other = synthetic.random_batch(K, R, n1, n2, seed=900 + n1, feat_dim=512 if feat else 0)
    return arena, st, b, other


def _keys(feat):
    return ["pts", "z", "gt_depth", "gt_rgb", "labels"] + (["gt_feat"] if feat else [])


def _dev(b, feat, dev):
    return {k: T(np.ascontiguousarray(b[k])).to(dev) for k in _keys(feat)}


def _run(arena, ws, batch, feat, **kw):
    ops.train_step(arena, ws, batch, with_feat=feat, **kw)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ws.grads).all()) and bool(torch.isfinite(ws.loss_terms).all())
    return ws.grads.clone(), ws.loss_terms.clone()


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _swapped(b, other, feat):
    """b with the inputs of every label-2 ray, and gt_rgb of every label-0 ray, taken from `other`."""
    u, o = b["labels"] == 2, b["labels"] == 0
    c = {k: np.array(v, copy=True) for k, v in b.items()}
    for k in ["pts", "z", "gt_depth", "gt_rgb"] + (["gt_feat"] if feat else []):
        c[k][u] = other[k][u]
    c["gt_rgb"][o] = other["gt_rgb"][o]
    assert u.any() and o.any() and not np.array_equal(c["pts"], b["pts"]) and not np.array_equal(c["gt_rgb"], b["gt_rgb"])
    return c


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n,R", SHAPES, ids=[f"S{a + b}" for (a, b), _ in SHAPES])
def test_fused_step_with_masked_rays(dev, n, R, variant):
    K, S, feat = 3, n[0] + n[1], False
    arena, st, b, other = _case(dev, n, R, variant, feat)
    batch = _dev(b, feat, dev)
    ws = ops.TrainWorkspace(arena, K, R, S, feat)
    mb = torch.zeros(K, R, S, 6, H // 8, dtype=torch.uint8, device=dev)
    hook = _run(arena, ws, batch, feat, relu_masks=mb)
    prod = _run(arena, ws, batch, feat)
    assert _same(hook, prod)                                                        # 2
    if variant == "object_all_unknown":
        # both early returns (render_rays.py:89-94): the oracle's loss is the constant 0, with no graph to differentiate
        assert float(prod[1].abs().max()) == 0.0 and float(prod[0].abs().max()) == 0.0         # 1
    else:
        masks = unpack_masks(mb.cpu(), H)
        fc, B = list(st[:18]), st[18]
        o32 = oracle_step(fc, B, 2.0, b, feat, masks=masks)
        o64 = oracle_step(fc, B, 2.0, b, feat, dtype=torch.float64, masks=masks)
        check_flips(o64)
        assert_terms(prod[1], o64, o32, feat)                                       # 1
        assert_grads(arena.views(prod[0]), o64, o32, names=ops.TENSOR_NAMES)
        if variant == "own_rays":
            assert float(prod[1][:, :3].min()) > 0.0 and float(prod[0].abs().max()) > 0.0
        else:
            assert float(prod[1][:, :2].abs().max()) == 0.0 and float(prod[1][:, 2].min()) > 0.0
    assert _same(_run(arena, ws, _dev(_swapped(b, other, feat), feat, dev), feat), prod)   # 3
    b2 = dict(b, labels=np.ascontiguousarray(np.roll(b["labels"], 1, axis=1)))               # 4
    b2["labels"][:, 0] = 1
    mid = _run(arena, ws, _dev(b2, feat, dev), feat)
    assert not torch.equal(mid[0], prod[0])
    assert _same(_run(arena, ws, batch, feat), prod)


@pytest.mark.parametrize("variant", VARIANTS[:2])
@pytest.mark.parametrize("n,R", SHAPES, ids=[f"S{a + b}" for (a, b), _ in SHAPES])
def test_fused_step_with_masked_rays_and_the_feature_loss(dev, n, R, variant):
    """The feature instantiations leave nothing out; 1, 3 and 4 hold for them as they did.  (No bit-equality with the
    hook launch here: at S = 64 the production launch spreads the feature term over all eight waves, the hook launch
    runs the any-S form, and the two sum in different orders -- tests/test_fused32_order_gpu.py holds both to the oracle.)"""
    K, S, feat = 3, n[0] + n[1], True
    arena, st, b, other = _case(dev, n, R, variant, feat)
    batch = _dev(b, feat, dev)
    ws = ops.TrainWorkspace(arena, K, R, S, feat)
    mb = torch.zeros(K, R, S, 6, H // 8, dtype=torch.uint8, device=dev)
    _run(arena, ws, batch, feat, relu_masks=mb)           # (for the ReLU branches the oracle is evaluated on)
    prod = _run(arena, ws, batch, feat)
    masks = unpack_masks(mb.cpu(), H)
    fc, B = list(st[:18]), st[18]
    o32 = oracle_step(fc, B, 2.0, b, feat, masks=masks)
    o64 = oracle_step(fc, B, 2.0, b, feat, dtype=torch.float64, masks=masks)
    check_flips(o64)
    assert_terms(prod[1], o64, o32, feat)
    assert_grads(arena.views(prod[0]), o64, o32, names=ops.TENSOR_NAMES)
    assert _same(_run(arena, ws, _dev(_swapped(b, other, feat), feat, dev), feat), prod)
    b2 = dict(b, labels=np.ascontiguousarray(np.roll(b["labels"], 1, axis=1)))
    b2["labels"][:, 0] = 1
    _run(arena, ws, _dev(b2, feat, dev), feat)
    assert _same(_run(arena, ws, batch, feat), prod)


# ---- the hidden-128 background step (objnerf_small_body.h): 1200 x 14-shaped and 64-sample rays at R = 9, fp32 and bf16
# (n1, n2), the workgroups whose rays are all unknown: 5 rays per workgroup at S = 14 (two workgroups), one at S = 64 (nine)
BG_CASES = [((5, 9), (0,)), ((5, 9), (1,)), ((16, 48), (0, 4, 8))]


def _bg_labels(R, rpw, dead):
    lab = np.array([1, 0, 2, 0, 1] * R, np.uint8)[:R]
    for g in dead:
        lab[g * rpw:(g + 1) * rpw] = 2
    assert (lab == 1).any() and (lab == 0).any()
    return lab[None]


@pytest.mark.parametrize("mode", [False, "bf16"], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n,dead", BG_CASES, ids=["S14-first", "S14-last", "S64-first-mid-last"])
def test_background_step_with_masked_rays(dev, n, dead, mode):
    from parity_util import sf_rays_per_wg, small128_route
    K, R, (n1, n2), Hb, feat = 1, 9, n, 128, False
    S = n1 + n2
    route = small128_route(K, R, S, feat, mode="bf16" if mode else "fp32")
    assert route[0] == "A" and route[2] == sf_rays_per_wg(S, feat) and max(dead) < route[3]
    assert route[3] == (2 if S == 14 else 9)
    st = obj_init.init_stacked(K, Hb, 512, seed=21)
    arena = ops.ParamArena(K, ops.NetShape(Hb, 512, 6), dev)
    arena.load_stacked([q.clone() for q in st])
    arena.scale.fill_(5.0)
    b = synthetic.random_batch(K, R, n1, n2, seed=78 + R)
    other = synthetic.random_batch(K, R, n1, n2, seed=978 + R)
    b["labels"] = _bg_labels(R, route[2], dead)
    ws = ops.TrainWorkspace(arena, K, R, S, feat, precision=mode)
    for buf in (ws.buf, getattr(ws, "buf2", None)):
        if buf is not None:
            buf.fill_(0xFF)                                   # a NaN as fp32 and as bf16 pairs
    batch = _dev(b, feat, dev)

    def run(bt, **kw):
        ops.train_step(arena, ws, bt, with_feat=feat, bf16=mode, **kw)
        torch.cuda.synchronize()
        assert int(ws.status.item()) == 0 and bool(torch.isfinite(ws.grads).all())
        return ws.grads.clone(), ws.loss_terms.clone()

    first = run(batch)
    if not mode:                                                                    # 1 (bf16: tests/test_bf16_small_gpu.py)
        mb = torch.zeros(K, R, S, 6, Hb // 8, dtype=torch.uint8, device=dev)
        hook = run(batch, relu_masks=mb)
        masks = unpack_masks(mb.cpu(), Hb)
        fc, B = list(st[:18]), st[18]
        o32 = oracle_step(fc, B, 5.0, b, feat, masks=masks)
        o64 = oracle_step(fc, B, 5.0, b, feat, dtype=torch.float64, masks=masks)
        check_flips(o64)
        assert_terms(hook[1], o64, o32, feat)
        assert_grads(arena.views(hook[0]), o64, o32, names=ops.TENSOR_NAMES)
    assert _same(run(_dev(_swapped(b, other, feat), feat, dev)), first)             # 3
    b2 = dict(b, labels=np.ascontiguousarray(np.roll(b["labels"], 1, axis=1)))      # 4
    assert not torch.equal(run(_dev(b2, feat, dev))[0], first[0])
    assert _same(run(batch), first)
