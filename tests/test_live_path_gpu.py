"""GPU: the fp32 fused training kernel on batches with NOTHING to leave out, and on single-class batches (DESIGN.md
4.1.1).  tests/test_masked_rays_gpu.py places every skip branch by hand inside one batch; here every wave of a launch takes
the same path -- all label 1: the fully live path, the one the benchmark spends 90 % of its waves in; all label 0: every
wave without the colour layer, every tile without the colour tile pairs, and the cross-object early return (no depth or
colour term anywhere).

  K = 3, S = 64 (16 + 48), R = 5     two rays per tile, the last tile ragged        train_fused32_kernel<false, false, 64>
  K = 3, S = 10 (1 + 9),   R = 29    twelve rays per tile, five in the last         train_fused32_kernel<false, false, 0>

Each of the four cases: the production launch bit-equal to the test-hook launch (`relu_masks=`), which leaves nothing out,
in gradients and loss terms; and both against the fp64-anchored oracle with parity_util's 1e-4 assertions, called exactly
as test_fused_step_with_masked_rays calls them (no new bound: the skipped parts have an exact zero factor).

One launch on the FLAT grid (objnerf_train.hip, choose_flat), whose workgroups sweep pieces of two objects and restage
weights, accumulators and lane constants at the segment boundary: K = 50, R = 2048, S = 64 takes it on 256 compute
units.  NT = 1024 tiles per object, T = 51 200 tiles:
    flat     share = ceil(51 200 / 256) = 200 tiles, segments = 1 + ceil(200 / 1024) = 2:   200 + 2 * 4 = 208 tile-equivalents
    strided  G = 5 workgroups per object (250 of 256 CUs, one round), ceil(1024 / 5) = 205:  205 + 4     = 209
    and an object is touched by at most ceil(1024 * 256 / 51 200) + 1 = 7 <= 32 workgroups.
(The rule is not monotonic in R -- ceil(NT / 5) and ceil(T / 256) step at different places -- so the test evaluates it, in
_flat_is_taken, for the device it runs on.)  Hook against
production, bit for bit, for an all-label-1 batch and for synthetic.random_batch's own 55 / 35 / 10 labels; no oracle."""
import numpy as np
import pytest
import torch

from conftest import T
from openobj_amd import init as obj_init
from openobj_amd import ops, synthetic
from parity_util import assert_grads, assert_terms, check_flips, oracle_step, unpack_masks

pytestmark = pytest.mark.gpu

H = 32
KEYS = ["pts", "z", "gt_depth", "gt_rgb", "labels"]
SHAPES = [((16, 48), 5), ((1, 9), 29)]


def _dev(b, dev):
    return {k: T(np.ascontiguousarray(b[k])).to(dev) for k in KEYS}


def _run(arena, ws, batch, **kw):
    ops.train_step(arena, ws, batch, with_feat=False, **kw)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ws.grads).all()) and bool(torch.isfinite(ws.loss_terms).all())
    return ws.grads.clone(), ws.loss_terms.clone()


@pytest.mark.parametrize("label", [1, 0], ids=["all_label_1", "all_label_0"])
@pytest.mark.parametrize("n,R", SHAPES, ids=[f"S{a + b}" for (a, b), _ in SHAPES])
def test_single_class_batch(dev, n, R, label):
    K, (n1, n2) = 3, n
    S = n1 + n2
    st = obj_init.init_stacked(K, H, 512, seed=11 + n1)
    arena = ops.ParamArena(K, ops.NetShape(H, 512, 6), dev)
    arena.load_stacked(st)
    b = synthetic.random_batch(K, R, n1, n2, seed=310 + n1)
    b["labels"] = np.full((K, R), label, np.uint8)
    batch = _dev(b, dev)
    ws = ops.TrainWorkspace(arena, K, R, S, False)
    mb = torch.zeros(K, R, S, 6, H // 8, dtype=torch.uint8, device=dev)
    hook = _run(arena, ws, batch, relu_masks=mb)
    prod = _run(arena, ws, batch)
    assert torch.equal(hook[0], prod[0]) and torch.equal(hook[1], prod[1])
    masks = unpack_masks(mb.cpu(), H)
    fc, B = list(st[:18]), st[18]
    o32 = oracle_step(fc, B, 2.0, b, False, masks=masks)
    o64 = oracle_step(fc, B, 2.0, b, False, dtype=torch.float64, masks=masks)
    check_flips(o64)
    assert_terms(prod[1], o64, o32, False)
    assert_grads(arena.views(prod[0]), o64, o32, names=ops.TENSOR_NAMES)
    if label == 1:
        assert float(prod[1][:, :3].min()) > 0.0 and float(prod[0].abs().max()) > 0.0
    else:       # no ray of any object: the depth and colour terms return early, the opacity term is all there is
        assert float(prod[1][:, :2].abs().max()) == 0.0 and float(prod[1][:, 2].min()) > 0.0


def _flat_is_taken(K, NT, cu, tile_equiv=4):
    """objnerf_train.hip, train_grid + choose_flat, for the fp32 kernel."""
    gmax = max(1, min(max(cu // K, 32), NT))
    strided = min(-(-K * G // cu) * (-(-NT // G) + tile_equiv) for G in range(1, gmax + 1))
    T_ = K * NT
    if T_ < cu:
        return False
    share = -(-T_ // cu)
    flat = share + (1 + -(-share // NT)) * tile_equiv
    return flat < strided and -(-NT * cu // T_) + 1 <= max(cu // K, 32)


def test_flat_grid_hook_equals_production(dev):
    K, R, n1, n2 = 50, 2048, 16, 48
    S = n1 + n2
    cu = torch.cuda.get_device_properties(dev).multi_processor_count
    assert _flat_is_taken(K, R * S // 128, 256)      # the docstring's arithmetic
    assert _flat_is_taken(K, R * S // 128, cu), f"{cu} compute units: this shape does not take the flat grid"
    st = obj_init.init_stacked(K, H, 512, seed=27)
    arena = ops.ParamArena(K, ops.NetShape(H, 512, 6), dev)
    arena.load_stacked(st)
    b = synthetic.random_batch(K, R, n1, n2, seed=4242)
    assert all((b["labels"] == v).any() for v in (0, 1, 2))
    ws = ops.TrainWorkspace(arena, K, R, S, False)
    mb = torch.zeros(K, R, S, 6, H // 8, dtype=torch.uint8, device=dev)
    for labels in (np.ones((K, R), np.uint8), b["labels"]):
        batch = _dev(dict(b, labels=labels), dev)
        hook = _run(arena, ws, batch, relu_masks=mb)
        prod = _run(arena, ws, batch)
        assert torch.equal(hook[0], prod[0]) and torch.equal(hook[1], prod[1])
        assert float(prod[0].abs().max()) > 0.0
