"""The S = 64 skipping instantiation of the fp32 fused training kernel runs a weight-gradient round whose other ray is
masked out over one ray alone (wg_pair_ray: the live k-slots four to an MFMA, in the order the full loop takes them in),
and no longer stores zeros for a dead wave.  No sum changes its order, so the test-hook launch (ReLU
masks written: no skips, all 32 steps) is the bit-exact control of the production launch; both are held to the oracle at
parity_util's 1e-4.  The other instantiations are the code they were; their cases stand guard over that.

  K=2, R=19, S=64   every pair of labels as the two rays of a tile, reversed in the second object; one ray in the last tile
  K=3, R=13, S=10   the any-S instantiation: the per-tile rule
  K=1, R=2,  S=64   with the feature loss: the half and quarter rounds
"""
import numpy as np
import pytest
import torch

from conftest import T
from openobj_amd import init as obj_init
from openobj_amd import ops, synthetic
from parity_util import assert_grads, assert_terms, check_flips, oracle_step, unpack_masks

pytestmark = pytest.mark.gpu

H = 32
PAIRS = [(1, 2), (2, 1), (0, 2), (2, 0), (1, 0), (0, 1), (0, 0), (2, 2), (1, 1)]
KEYS = ["pts", "z", "gt_depth", "gt_rgb", "labels"]


def _setup(K, R, n1, n2, feat, seed):
    st = obj_init.init_stacked(K, H, 512, seed=seed)
    b = synthetic.random_batch(K, R, n1, n2, seed=seed + 100, feat_dim=512 if feat else 0)
    b["labels"][:, 0] = 1                        # a handful of rays per object: keep the early return out of this test
    return st, b


def _arena(dev, st, K):
    arena = ops.ParamArena(K, ops.NetShape(H, 512, 6), dev)
    arena.load_stacked(st)
    return arena


def _both_launches(dev, arena, b, K, R, S, feat):
    """(grads, loss terms) of the test-hook launch and of the production launch, and the hook's ReLU masks."""
    batch = {k: T(b[k]).to(dev) for k in KEYS + (["gt_feat"] if feat else [])}
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


def test_label_pairs_hook_bit_equality_oracle_and_dead_ray_inputs(dev):
    K, R, n1, n2 = 2, 19, 16, 48
    S = n1 + n2
    st, b = _setup(K, R, n1, n2, False, seed=71)
    b["labels"][0, :18] = np.array(PAIRS, np.uint8).reshape(-1)
    b["labels"][1, :18] = np.array(PAIRS[::-1], np.uint8).reshape(-1)      # live and dead halves follow each other
    b["labels"][0, 18], b["labels"][1, 18] = 1, 0
    arena = _arena(dev, st, K)
    hook, prod, mb = _both_launches(dev, arena, b, K, R, S, False)
    assert torch.equal(hook[0], prod[0]) and torch.equal(hook[1], prod[1])
    o32, o64 = _anchors(st, b, False, mb)
    for grads, terms in (hook, prod):
        assert_terms(terms, o64, o32, False)
        assert_grads(arena.views(grads), o64, o32, names=ops.TENSOR_NAMES)
    # whatever a label-2 ray carries never reaches a result: other finite inputs there, the same bits out
    other = synthetic.random_batch(K, R, n1, n2, seed=999)
    dead = b["labels"] == 2
    b2 = dict(b)
    for k in ("pts", "z", "gt_depth", "gt_rgb"):
        v = np.array(b[k], copy=True)
        v[dead] = other[k][dead]
        b2[k] = v
    assert dead.sum() == 12 and not np.array_equal(b2["pts"], b["pts"])
    hook2, prod2, _ = _both_launches(dev, arena, b2, K, R, S, False)
    assert torch.equal(prod2[0], prod[0]) and torch.equal(prod2[1], prod[1])
    assert torch.equal(hook2[0], prod[0]) and torch.equal(hook2[1], prod[1])


def test_any_s_instantiation_keeps_the_per_tile_rule(dev):
    K, R, n1, n2 = 3, 13, 1, 9
    S = n1 + n2
    st, b = _setup(K, R, n1, n2, False, seed=83)
    arena = _arena(dev, st, K)
    hook, prod, mb = _both_launches(dev, arena, b, K, R, S, False)
    assert torch.equal(hook[0], prod[0]) and torch.equal(hook[1], prod[1])
    o32, o64 = _anchors(st, b, False, mb)
    assert_terms(prod[1], o64, o32, False)
    assert_grads(arena.views(prod[0]), o64, o32, names=ops.TENSOR_NAMES)


def test_feature_layout_halves_and_quarters(dev):
    K, R, n1, n2 = 1, 2, 16, 48
    S = n1 + n2
    st, b = _setup(K, R, n1, n2, True, seed=97)
    arena = _arena(dev, st, K)
    hook, prod, mb = _both_launches(dev, arena, b, K, R, S, True)
    o32, o64 = _anchors(st, b, True, mb)
    for grads, terms in (hook, prod):
        assert_terms(terms, o64, o32, True)
        assert_grads(arena.views(grads), o64, o32, names=ops.TENSOR_NAMES)
