"""GPU: the bf16 instantiations of the hidden-128 small-batch kernels -- what `--bf16` trains the background network
on -- held to the operand-rounded specification at every row-tile count, ragged tail and feature-branch limit, plus
checks that need no tolerance (workspace contents, input bounds, object order, repeatability) and the statement that the
fp16 mode runs the fp32 kernels on these shapes.  (Only the dispatch-table test at the top runs without a GPU.)

Two routes (objnerf_generic.hip, objgen::train_step; restated in parity_util.small128_route):
  A  train_small_kernel<RT 4 | 5, true, FEAT> (objnerf_small_body.h), then gemm_group16_kernel and reduce_parts_kernel;
  B  mlp_fwd_small_kernel<RT 1..5, true>, the loss launches, heads_bwd_kernel, mlp_bwd_small_kernel<RT, true>, then
     gemm_group16_kernel.

Where the two routes round (the reading behind the specification flags below):
  * mma_f / mma (objnerf_small_body.h:252-266; objnerf_generic.hip, mlp_fwd_small_kernel): BOTH operands -- the fp32 weight image and
    the fp32 activations / embedding in LDS -- are converted by cvt_bf16x8 as the MFMA reads them.  The LDS copies that
    every other consumer reads stay fp32: rounded at the GEMM, not in storage -> act16 = False.
  * the heads (objnerf_small_body.h:397-411; objnerf_generic.hip, the end of mlp_fwd_small_kernel): fp32 dot products of the UNROUNDED h4 / hc
    with fp32 head weights -> round_head_weights = False.  Their weight gradients are fp32 sums over the same LDS rows
    (head_partials, objnerf_small_body.h:481-495) or head_wgrad_kernel on fp32 h4 / hc (objnerf_generic.hip, train_step; act16 = 0
    because acts16_shape needs hidden 256) -> round_head_grads = False.  heads_bwd_kernel (route B, train_step) likewise reads
    fp32 hc / colour and writes fp32 d_hc.
  * mma_b / mma of the backward (objnerf_small_body.h:635-651; objnerf_generic.hip, mlp_bwd_small_kernel): the weight image is rounded
    when staged (put_wb / put_w), the fp32 d_h in LDS by cvt_bf16x8 at the MFMA: the back-propagated gradient is rounded
    as the next GEMM's operand, which is what the specification's activation rounding does on the way back.
  * the weight gradients: route A's `hst` (objnerf_small_body.h:295-297) stores h and d_h rounded for gemm_group16_kernel,
    which on route B rounds the same fp32 values itself (GroupLaunch group(small_bf, ..), objnerf_generic.hip, train_step): operands of the
    weight-gradient GEMMs rounded, as the specification's autograd of a rounded-operand matmul has them.
  * the feature head.  Route A prepares the hoisted head on an fp32 GemmStep (objnerf_generic.hip,
    train_step_small: gemm_step(w, 0, K)): fp32, nothing rounded.  Route B calls feat_prep_enqueue on the step's own
    operand precision (train_step; only the GEMMs BEHIND the small-batch kernels ask for fp32, WgradHow::fp32): the Gram
    matrix and u = W_of^T g are bf16-operand GEMMs, W_of enters rounded while the density / colour heads do not -- a point
    the specification could not express; mlp_forward_stacked_16(round_feat_head=True) states it.
"""
import numpy as np
import pytest
import torch

from conftest import T
from openobj_amd import init as obj_init
from openobj_amd import ops, synthetic
from parity_util import guarded, oracle_step_16, rel_norm, sf_rays_per_wg, small128_route, spec_spread
from test_16bit_spec_gpu import BOUND

gpu = pytest.mark.gpu
H = 128
TRUNK = list(range(14)) + [18]

# (K, R, n1, n2): (rpw, rows of a full workgroup, RT) without / with the feature loss, rays in the last workgroup
ROUTE_A = [
    ((2, 3, 16, 48), (1, 64, 4), (1, 64, 4), (1, 1)),       # full-tile branch of RT 4; the benchmark's ray
    ((2, 3, 16, 47), (1, 63, 4), (1, 63, 4), (1, 1)),       # per-row branch on every workgroup; 63 of 64 compositing lanes
    ((3, 3, 8, 24), (2, 64, 4), (2, 64, 4), (1, 1)),        # last workgroup one ray of two
    ((2, 5, 10, 30), (2, 80, 5), (2, 80, 5), (1, 1)),       # full-tile branch of RT 5; last workgroup half full
    ((2, 5, 8, 25), (2, 66, 5), (2, 66, 5), (1, 1)),        # RT 5, per-row everywhere
    ((2, 7, 4, 12), (5, 80, 5), (5, 80, 5), (2, 2)),        # feature branch at MAXRAY = 5 beside a full 80-row tile
    ((2, 7, 5, 9), (5, 70, 5), (5, 70, 5), (2, 2)),         # the native background ray
    ((2, 9, 4, 7), (7, 77, 5), (5, 55, 4), (2, 4)),         # the feature loss changes RT
    ((2, 23, 1, 3), (20, 80, 5), (16, 64, 4), (3, 7)),      # 16 rays in s_fh[MAXRAY = 20]
]
SELF_COUNTS = (1, 23, 1, 3)                                  # K = 1: the label statistics counted inside the kernel
EARLY_RETURN = (2, 5, 10, 30)
# (K, R, n1, n2): RT, rows in the last workgroup (None: several rounds of workgroups), also with the feature loss
ROUTE_B = [
    ((1, 37, 16, 49), 1, 5, True),
    ((2, 37, 16, 49), 2, 5, True),
    ((8, 17, 16, 49), 3, 1, True),
    ((1, 200, 16, 49), 4, 8, False),
    ((1, 300, 16, 49), 5, 60, False),
    ((1, 400, 16, 49), 5, None, False),
    ((2, 301, 1, 2), 1, 7, True),                            # S = 3, below route A's floor
]
SPEC_CASES = ([(s, f) for s, *_ in ROUTE_A for f in (False, True)] + [(SELF_COUNTS, False)]
              + [(s, f) for s, _, _, ft in ROUTE_B for f in ((False, True) if ft else (False,))])
# the tolerance-free checks: a ragged route-A shape with the feature loss, one without it, a route-B shape
EXACT_CASES = [((2, 9, 4, 7), True), ((2, 5, 8, 25), False), ((2, 37, 16, 49), False)]
FP16_CASES = [((2, 200, 5, 9), False), ((2, 200, 5, 9), True), ((2, 5, 8, 25), False), ((2, 5, 8, 25), True)]


def _id(case):
    (K, R, n1, n2), feat = case
    return f"{K}x{R}x{n1}+{n2}{'-feat' if feat else ''}"


def test_every_case_maps_to_the_kernel_it_names():
    """No GPU: parity_util.small128_route (the dispatch of objnerf_generic.hip restated) puts every case of the tables
    above on the route, row-tile count and tail written beside it."""
    for shape, nofeat, withfeat, last in ROUTE_A:
        K, R, n1, n2 = shape
        S = n1 + n2
        for feat, (rpw, rows, rt), last_rays in ((False, nofeat, last[0]), (True, withfeat, last[1])):
            route, got_rt, got_rpw, nwg = small128_route(K, R, S, feat)
            assert (route, got_rt, got_rpw, got_rpw * S) == ("A", rt, rpw, rows), (shape, feat)
            assert got_rpw == sf_rays_per_wg(S, feat) and R - (nwg - 1) * rpw == last_rays, (shape, feat)
            assert nwg > 1 and 1 <= last_rays <= rpw, (shape, feat)
    assert small128_route(*SELF_COUNTS[:2], 4, False)[:2] == ("A", 5)
    assert small128_route(*EARLY_RETURN[:2], 40, False)[:2] == small128_route(*EARLY_RETURN[:2], 40, True)[:2] == ("A", 5)
    for shape, rt, tail, feat_too in ROUTE_B:
        K, R, n1, n2 = shape
        n = R * (n1 + n2)
        for feat in ((False, True) if feat_too else (False,)):
            route, got_rt, _, wgs = small128_route(K, R, n1 + n2, feat)
            assert (route, got_rt) == ("B", rt), (shape, feat)
            if tail is None:
                assert K * wgs > 256
            else:
                assert K * wgs <= 256 and n - (wgs - 1) * 16 * rt == tail, (shape, n - (wgs - 1) * 16 * rt)
    assert sorted({small128_route(s[0], s[1], s[2] + s[3], f)[1] for s, *_ in ROUTE_B for f in (False,)}) == [1, 2, 3, 4, 5]
    for (K, R, n1, n2), feat in EXACT_CASES:
        want = "A" if n1 + n2 <= 64 else "B"
        assert small128_route(K, R, n1 + n2, feat)[0] == want and small128_route(3, R, n1 + n2, feat)[0] == want
    for (K, R, n1, n2), feat in FP16_CASES:                    # the fp16 mode takes route A too (its fp32 instantiation)
        assert small128_route(K, R, n1 + n2, feat, mode="fp16")[0] == "A"
        assert small128_route(K, R, n1 + n2, feat, mode="fp32", layerwise=True)[0] == "A"


def _setup(dev, K, R, n1, n2, feat, empty_obj=None):
    """Arena (hidden 128, scale 5), its stacked parameters and a batch in which every object has a label-1 ray in its
    first AND in its last workgroup (a tail whose rays carry no depth / colour term would not move the gradient)."""
    st = obj_init.init_stacked(K, H, 512, seed=21)
    arena = ops.ParamArena(K, ops.NetShape(H, 512, 6), dev)
    arena.load_stacked([q.clone() for q in st])
    arena.scale.fill_(5.0)
    b = synthetic.random_batch(K, R, n1, n2, seed=78 + R, feat_dim=512 if feat else 0)
    b["labels"][:, 0] = 1
    b["labels"][:, R - 1] = 1
    if empty_obj is not None:
        b["labels"][empty_obj][b["labels"][empty_obj] == 1] = 0      # render_rays.py:89-94: the early return for ALL objects
    return arena, st, b


def _keys(feat):
    return ["pts", "z", "gt_depth", "gt_rgb", "labels"] + (["gt_feat"] if feat else [])


def _to_dev(b, feat, dev):
    return {k: T(b[k]).to(dev) for k in _keys(feat)}


def _step(arena, batch, K, R, S, feat, mode="bf16", fill=None, ws=None, **kw):
    if ws is None:
        ws = ops.TrainWorkspace(arena, K, R, S, feat, precision=mode)
        for buf in (ws.buf, getattr(ws, "buf2", None)):
            if buf is not None:
                buf.fill_(0 if fill is None else fill)
    ops.train_step(arena, ws, batch, with_feat=feat, bf16=mode, **kw)
    torch.cuda.synchronize()
    assert int(ws.status.item()) == 0 and bool(torch.isfinite(ws.grads).all()) and bool(torch.isfinite(ws.loss_terms).all())
    return ws


def _spec(st, b, feat, route, dev, dtype=None):
    return oracle_step_16(list(st[:18]), st[18], 5.0, b, feat, torch.bfloat16, False, 1.0, device=dev, dtype=dtype,
                          round_feat_head=(route == "B" and feat))


def _against_spec(tag, arena, ws, st, b, feat, route, dev, tensors=None):
    """Loss terms and every gradient tensor of `ws` against the specification; prints kernel distance, the
    specification's own spread (fp32 against fp64 accumulation) and the bound; asserts spread < bound / 10 and distance <
    bound.  Measured on MI355X (profiles/bf16_small_spec.txt): worst distance 3.5e-3, worst spread 7.9e-4."""
    o = _spec(st, b, feat, route, dev)
    o64 = _spec(st, b, feat, route, dev, dtype=torch.float64)
    spread = spec_spread(o, o64)
    cols = 4 if feat else 3
    np.testing.assert_allclose(ws.loss_terms.double().cpu()[:, :cols], o["terms"][:, :cols], rtol=2e-3, atol=1e-5)
    gv = arena.views(ws.grads)
    failed = []
    for i in (range(19) if feat else TRUNK) if tensors is None else tensors:
        bound = BOUND["bf16"] * ((4 if i in ops.FEAT_TENSORS else 2) if feat else 1)
        rel = rel_norm(gv[i], o["grads"][i])
        print(f"{tag} {ops.TENSOR_NAMES[i]:24s} kernel {rel:.2e} spread {spread[i]:.2e} bound {bound:.0e}")
        # a condition on the INPUTS: a case whose specification is this ambiguous says nothing about the kernel
        assert spread[i] < 0.1 * bound, ("reshape this case", tag, ops.TENSOR_NAMES[i], spread[i])
        if not rel < bound:
            failed.append((ops.TENSOR_NAMES[i], rel, bound))
    assert not failed, (tag, failed)
    if not feat:
        for i in ops.FEAT_TENSORS:
            assert float(gv[i].abs().max()) == 0.0
    return o


@gpu
@pytest.mark.parametrize("case", SPEC_CASES, ids=_id)
def test_bf16_small_batch_step_matches_its_specification(dev, case):
    """Every bf16 instantiation of the two routes (module docstring: where they round, hence act16 = False, fp32 heads,
    round_feat_head on route B only) against the operand-rounded specification at the project's own bound -- BOUND["bf16"]
    per tensor, x 2 for the trunk and x 4 for the feature branch's tensors with the feature loss -- with the
    specification's own spread printed beside each distance.  The K = 1 case also runs WITH the label statistics handed
    in: OBJNERF_TRAIN_SELF_COUNTS inside the bf16 kernel must publish what ops.label_counts computes and change no bit."""
    (K, R, n1, n2), feat = case
    route = small128_route(K, R, n1 + n2, feat)[0]
    arena, st, b = _setup(dev, K, R, n1, n2, feat)
    batch = _to_dev(b, feat, dev)
    ws = ops.TrainWorkspace(arena, K, R, n1 + n2, feat, precision="bf16")
    ws.flags.fill_(7)
    ws.counts.fill_(-1)
    _step(arena, batch, K, R, n1 + n2, feat, ws=ws)
    _against_spec(_id(case), arena, ws, st, b, feat, route, dev)
    counts, flags = ops.label_counts(batch["labels"])
    assert torch.equal(ws.counts, counts) and torch.equal(ws.flags, flags) and flags.tolist() == [0, 0]
    if (K, R, n1, n2) == SELF_COUNTS:
        ws1 = _step(arena, batch, K, R, n1 + n2, feat, global_flags=flags, global_counts=counts)
        assert torch.equal(ws1.grads, ws.grads) and torch.equal(ws1.loss_terms, ws.loss_terms)


@gpu
@pytest.mark.parametrize("feat", [False, True])
def test_bf16_small_batch_early_return(dev, feat):
    """render_rays.py:89-94 on a ragged route-A shape: one object without a label-1 ray zeroes the depth, colour (and
    feature) terms and their gradients of EVERY object -- exact zeros -- while the opacity term still trains the trunk,
    which is held against the specification."""
    K, R, n1, n2 = EARLY_RETURN
    arena, st, b = _setup(dev, K, R, n1, n2, feat, empty_obj=K - 1)
    batch = _to_dev(b, feat, dev)
    ws = _step(arena, batch, K, R, n1 + n2, feat)
    assert ws.flags.tolist() == [1, 0]
    t = ws.loss_terms
    assert float(t[:, 0].abs().max()) == 0.0 and float(t[:, 1].abs().max()) == 0.0 and float(t[:, 3].abs().max()) == 0.0
    assert float(t[:, 2].min()) > 0.0
    gv = arena.views(ws.grads)
    for i in (10, 11, 12, 13) + tuple(ops.FEAT_TENSORS):
        assert float(gv[i].abs().max()) == 0.0, ops.TENSOR_NAMES[i]
    o = _against_spec(f"early-return{'-feat' if feat else ''}", arena, ws, st, b, feat, "A", dev,
                      tensors=list(range(10)) + [18])
    assert all(o["none_grad"][i] for i in (10, 11, 12, 13))


def _has(feat):
    return list(range(19)) if feat else TRUNK


def _snap(arena, ws, feat):
    gv = arena.views(ws.grads)
    return torch.cat([gv[i].reshape(-1) for i in _has(feat)] + [ws.loss_terms.reshape(-1)]).clone()


@gpu
@pytest.mark.parametrize("case", EXACT_CASES, ids=_id)
def test_bf16_small_batch_step_ignores_workspace_contents_and_repeats(dev, case):
    """A fresh workspace whose every byte is 0xFF (a NaN both as bf16 pairs and as fp32) against a zero-filled one:
    bit-equal, finite, status 0 -- a weight-gradient contraction that read the rounded copies past row n, an unmasked
    tile tail or a slip in `hst`'s 16-bit index inside the fp32-spaced buffers would read the poison.  A second call in
    the same workspace is bit-equal too."""
    (K, R, n1, n2), feat = case
    arena, _, b = _setup(dev, K, R, n1, n2, feat)
    batch = _to_dev(b, feat, dev)
    wz = _step(arena, batch, K, R, n1 + n2, feat, fill=0)
    wp = _step(arena, batch, K, R, n1 + n2, feat, fill=0xFF)
    ref = _snap(arena, wz, feat)
    assert float(ref.abs().max()) > 0
    assert torch.equal(_snap(arena, wp, feat), ref)
    _step(arena, batch, K, R, n1 + n2, feat, ws=wp)
    assert torch.equal(_snap(arena, wp, feat), ref)


@gpu
@pytest.mark.parametrize("case", EXACT_CASES, ids=_id)
def test_bf16_small_batch_step_reads_no_input_past_its_end(dev, case):
    """Every input as a view into a larger storage with 80 rows of guard behind the data: NaN (255 for the labels) in
    one run, zeros in the other, bit-equal results."""
    (K, R, n1, n2), feat = case
    arena, _, b = _setup(dev, K, R, n1, n2, feat)
    batch = _to_dev(b, feat, dev)
    runs = []
    for nan in (True, False):
        gb = {k: guarded(v, 80, (255 if k == "labels" else float("nan")) if nan else 0, row_dims=3 if k == "pts" else 2)
              for k, v in batch.items()}
        for k in gb:
            assert gb[k].is_contiguous() and torch.equal(gb[k], batch[k])
        runs.append(_snap(arena, _step(arena, gb, K, R, n1 + n2, feat), feat))
    assert torch.equal(runs[0], runs[1])


@gpu
@pytest.mark.parametrize("case", EXACT_CASES, ids=_id)
def test_bf16_small_batch_step_does_not_depend_on_object_order(dev, case):
    """Three objects in order (0, 1, 2) and (2, 0, 1), parameters and batch permuted together: every object's gradients
    and loss terms are bit-equal between the two launches (K is the same, so every reduction is sliced the same way)."""
    (_, R, n1, n2), feat = case
    K = 3
    arena, st, b = _setup(dev, K, R, n1, n2, feat)
    batch = _to_dev(b, feat, dev)
    w1 = _step(arena, batch, K, R, n1 + n2, feat)
    perm = torch.tensor([2, 0, 1])
    arena2 = ops.ParamArena(K, ops.NetShape(H, 512, 6), dev)
    arena2.load_stacked([q[perm].clone() for q in st])
    arena2.scale.fill_(5.0)
    pd = perm.to(dev)
    w2 = _step(arena2, {k: v[pd].contiguous() for k, v in batch.items()}, K, R, n1 + n2, feat)
    g1, g2 = arena.views(w1.grads), arena2.views(w2.grads)
    for i in _has(feat):
        assert torch.equal(g2[i], g1[i][pd]), ops.TENSOR_NAMES[i]
    assert torch.equal(w2.loss_terms, w1.loss_terms[pd])


@gpu
@pytest.mark.parametrize("case", FP16_CASES, ids=_id)
def test_fp16_mode_runs_the_fp32_small_batch_kernels(dev, case):
    """What two skips of test_16bit_spec_gpu.py say: on route A the fp16 mode rounds nothing.  objgen::train_step hands
    train_step_small `operands == 1` (objnerf_generic.hip, train_step) -- false for fp16 -- and train_step_small runs
    its GEMMs on an fp32 GemmStep (gemm_step(w, 0, K)), so the launches are those of an fp32 step: bit-equal gradients and loss
    terms to the fp32-mode step on a layerwise=True workspace (the sizing an fp16 workspace gets)."""
    (K, R, n1, n2), feat = case
    arena, _, b = _setup(dev, K, R, n1, n2, feat)
    batch = _to_dev(b, feat, dev)
    w16 = _step(arena, batch, K, R, n1 + n2, feat, mode="fp16")
    w32 = ops.TrainWorkspace(arena, K, R, n1 + n2, feat, layerwise=True)
    ops.train_step(arena, w32, batch, with_feat=feat)
    torch.cuda.synchronize()
    assert int(w32.status.item()) == 0
    assert torch.equal(_snap(arena, w16, feat), _snap(arena, w32, feat))
    assert float(_snap(arena, w16, feat).abs().max()) > 0
