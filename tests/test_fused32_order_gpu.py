"""The fp32 fused training kernel's unit pins the issue order of its MFMAs where two independent accumulator chains are
written alternately (a layer's output pair in mma_f16, a weight-gradient tile pair in wg_pair), which also lets the operand
reads move ahead of their k-step.  No chain's k-order changes, so nothing here is a new bound: loss terms and all gradients
of `ops.train_step` against the oracle at the 1e-4 of parity_util, at the smallest shapes at which a reordered loop can go
wrong, and the test-hook launch (ReLU masks written) bit-equal to the production launch where both exist without the
feature loss.

  K=2, R=6,  S=64   three 2-ray tiles: more than one tile per segment, two objects = two segments
  K=3, R=13, S=10   the any-S instantiation: 12 rays per tile, the last tile is partial
  K=1, R=2,  S=64   with the feature loss: the feature layout with its half and quarter weight-gradient rounds
"""
import pytest
import torch

from conftest import T
from openobj_amd import init as obj_init
from openobj_amd import ops, synthetic
from parity_util import assert_grads, assert_terms, check_flips, oracle_step, unpack_masks

pytestmark = pytest.mark.gpu

H = 32


def _setup(dev, K, R, n1, n2, feat, seed):
    st = obj_init.init_stacked(K, H, 512, seed=seed)
    arena = ops.ParamArena(K, ops.NetShape(H, 512, 6), dev)
    arena.load_stacked(st)
    b = synthetic.random_batch(K, R, n1, n2, seed=seed + 100, feat_dim=512 if feat else 0)
    b["labels"][:, 0] = 1                        # a handful of rays per object: keep the early return out of this test
    keys = ["pts", "z", "gt_depth", "gt_rgb", "labels"] + (["gt_feat"] if feat else [])
    return arena, {k: T(b[k]).to(dev) for k in keys}, st, b


def _both_launches(dev, arena, batch, K, R, S, feat):
    """(grads, loss terms) of the test-hook launch and of the production launch, and the hook's ReLU masks."""
    ws = ops.TrainWorkspace(arena, K, R, S, feat)
    mb = torch.zeros(K, R, S, 6, H // 8, dtype=torch.uint8, device=dev)
    ops.train_step(arena, ws, batch, with_feat=feat, relu_masks=mb)
    torch.cuda.synchronize()
    assert int(ws.status.item()) == 0
    hook = (ws.grads.clone(), ws.loss_terms.clone())
    ops.train_step(arena, ws, batch, with_feat=feat)
    torch.cuda.synchronize()
    assert int(ws.status.item()) == 0
    return hook, (ws.grads.clone(), ws.loss_terms.clone()), mb


def _anchors(st, b, feat, mb):
    masks = unpack_masks(mb.cpu(), H)
    fc, B = list(st[:18]), st[18]
    o32 = oracle_step(fc, B, 2.0, b, feat, masks=masks)
    o64 = oracle_step(fc, B, 2.0, b, feat, dtype=torch.float64, masks=masks)
    check_flips(o64)
    return o32, o64


@pytest.mark.parametrize("K,R,n1,n2", [(2, 6, 16, 48), (3, 13, 1, 9)])
def test_reordered_loops_vs_oracle_and_hook_bit_equality(dev, K, R, n1, n2):
    S = n1 + n2
    arena, batch, st, b = _setup(dev, K, R, n1, n2, False, seed=31 + S)
    hook, prod, mb = _both_launches(dev, arena, batch, K, R, S, False)
    assert torch.equal(hook[0], prod[0]) and torch.equal(hook[1], prod[1])
    o32, o64 = _anchors(st, b, False, mb)
    assert_terms(prod[1], o64, o32, False)
    assert_grads(arena.views(prod[0]), o64, o32, names=ops.TENSOR_NAMES)


def test_feature_layout_rounds_vs_oracle(dev):
    K, R, n1, n2 = 1, 2, 16, 48
    S = n1 + n2
    arena, batch, st, b = _setup(dev, K, R, n1, n2, True, seed=57)
    hook, prod, mb = _both_launches(dev, arena, batch, K, R, S, True)
    o32, o64 = _anchors(st, b, True, mb)
    for grads, terms in (hook, prod):
        assert_terms(terms, o64, o32, True)
        assert_grads(arena.views(grads), o64, o32, names=ops.TENSOR_NAMES)
