"""GPU: the training step's two-bit status word (include/objnerf_hip.h: bit 0 = a per-object loss term above 1e5, where the
reference prints "loss explode" and exits, render_rays.py:109-111; bit 1 = a term that is not finite, where it carries
on) on EVERY path that can end a step, and the host merges of such words (object chunks, the forloop strategy, the
iterations of a frame).  The host side without a GPU is tests/test_status_host.py.

The inputs that sit next to the 1e5 threshold are computed from the fp64 oracle alone and cross-checked against the fp32
oracle on the CPU before the GPU is touched; nothing is taken from the code under test."""
import warnings

import numpy as np
import pytest
import torch

from conftest import T
from oracle import objnerf_oracle as O
from openobj_amd import _lib, ops, optim, synthetic
from openobj_amd import init as obj_init
from openobj_amd import loss as oloss
from openobj_amd import render_rays
from openobj_amd import train as otrain
from openobj_amd.render_rays import LossExplode, check_status
from parity_util import assert_terms, oracle_step

pytestmark = pytest.mark.gpu
KEYS = ["pts", "z", "gt_depth", "gt_rgb", "labels"]
THRESH = 1e5
MARGIN = 1e-3               # case b: the colour term sits at 1e5 (1 -+ 1e-3)
SEED_NET, SEED_BATCH = 3, 5

# (hidden, K, R, n1, n2): the smallest shapes that still take each path
SHAPES = {"h32": (32, 3, 32, 16, 48), "h32_s32": (32, 3, 32, 8, 24), "h128_k1": (128, 1, 40, 5, 9),
          "h128_k3": (128, 3, 40, 5, 9), "h256": (256, 2, 64, 16, 48)}

# One list of paths: id -> (shape, feature loss, precision, layerwise, chunking).  chunking: None, "chunks" (k_chunk < K on
# one stream) or "lanes1" / "lanes2" (hidden 256 in a 16-bit mode: chunks on one / alternately on two side streams).
PATHS = {
    "fused32": ("h32", False, False, False, None),                   # train_fused32_kernel + finalize_kernel
    "fused32_feat": ("h32", True, False, False, None),
    "bf16v2": ("h32", False, "bf16", False, None),                   # second generation (64 samples per ray)
    "bf16v2_feat": ("h32", True, "bf16", False, None),
    "bf16v1": ("h32_s32", False, "bf16", False, None),               # first generation: still launched for S != 64
    "bf16v1_feat": ("h32_s32", True, "bf16", False, None),
    "small128_k1": ("h128_k1", False, False, False, None),           # one-launch iteration, reduce_parts_kernel's tail
    "small128_k3": ("h128_k3", False, False, False, None),
    "small128_k1_bf16": ("h128_k1", False, "bf16", False, None),
    "small128_k3_feat": ("h128_k3", True, False, False, None),
    "layerwise32": ("h32", False, False, True, None),                # loss_total_kernel
    "layerwise128": ("h128_k3", False, False, True, None),
    "layerwise128_feat": ("h128_k3", True, False, True, None),
    "chunks128": ("h128_k3", False, False, True, "chunks"),          # ws.status_chunks merged on the host
    "chunks256_fp16_lanes1": ("h256", False, "fp16", False, "lanes1"),
    "chunks256_fp16_lanes2": ("h256", False, "fp16", False, "lanes2"),
    "fused256_fp16": ("h256", False, "fp16", False, None),           # row-split kernel A + finalize256_kernel (atomicOr)
    "fused256_bf16": ("h256", False, "bf16", False, None),
    "fused256_fp16_feat": ("h256", True, "fp16", False, None),       # first form of kernel A (the switch: feature loss)
    "fused256_bf16_feat": ("h256", True, "bf16", False, None),
}
# the 16-bit modes are not the reference's arithmetic: both operands of each of the 6 hidden GEMMs are rounded to the operand
# type (unit roundoff u = 2^-8 bf16, 2^-11 fp16), 12 roundings in a chain -> a first-order bound of 12 u on a term,
# relative to the largest term of its kind (assert_terms' scale); fp32 paths keep assert_terms' own 1e-4
TERM_TOL = {False: 1e-4, "bf16": 12 * 2.0 ** -8, "fp16": 12 * 2.0 ** -11}


def _scale(H):
    return 2.0 if H == 32 else 5.0


def _recompute(terms):
    """The word by its definition: any term above 1e5 sets bit 0, any non-finite term sets bit 1."""
    t = torch.as_tensor(terms).float().cpu()
    return (1 if bool((t > 100000.0).any()) else 0) | (2 if not bool(torch.isfinite(t).all()) else 0)


def _first_counted(labels_k, skip=()):
    idx = [int(i) for i in np.nonzero(labels_k == 1)[0] if int(i) not in skip]
    assert idx, "an object without a label-1 ray"
    return idx[0]


class _Scenario:
    """The cases a-g of one (shape, feature loss) as host batches with what the reference says about each.  Built once per
    process and shared by every path of that shape; never modified afterwards."""

    def __init__(self, shape, feat, kind="train"):
        self.H, self.K, self.R, self.n1, self.n2 = SHAPES[shape]
        self.feat, self.kind = feat, kind
        H, K = self.H, self.K
        self.st = obj_init.init_stacked(K, H, 512, seed=SEED_NET)
        self.b = synthetic.random_batch(K, self.R, self.n1, self.n2, seed=SEED_BATCH, feat_dim=512 if feat else 0)
        if kind == "loss":          # objnerf_step_batch_loss: the network's outputs are INPUTS, formed once in fp32
            with torch.no_grad():
                emb = O.embed_stacked(self.st[18], torch.full((K,), _scale(H)), T(self.b["pts"]))
                a, c, f = O.mlp_forward_stacked(list(self.st[:18]), emb, feat)
            self.alpha, self.color, self.pred_feat = a.contiguous(), c.contiguous(), (f.contiguous() if feat else None)
        self.clean64, self.clean32 = self.oracle(self.b, torch.float64), self.oracle(self.b, None)
        self.var64 = self._var64()
        self.cases = []             # (name, batch, expected status, rows of unpoisoned objects, (o64, o32) for those rows)
        self._build()

    # -- the reference -----------------------------------------------------------------------------------------------
    def oracle(self, b, dtype):
        """dict(terms [K,4] fp64) from the oracle in `dtype` (None: the reference's fp32); raises O.LossExplode where the
        reference exits."""
        if self.kind == "train":
            return oracle_step(list(self.st[:18]), self.st[18], _scale(self.H), b, self.feat, dtype=dtype)
        dt = dtype or torch.float32
        with torch.no_grad():
            _, t = O.step_batch_loss(self.alpha.to(dt), self.color.to(dt), T(b["gt_depth"]).to(dt), T(b["gt_rgb"]).to(dt),
                                     T(b["labels"]), None, T(b["z"]).to(dt),
                                     gt_partfeat=T(b["gt_feat"]).to(dt) if self.feat else None,
                                     pred_partfeat=self.pred_feat.to(dt) if self.feat else None, return_terms=True)
        terms = torch.zeros(self.K, 4, dtype=torch.float64)
        for j, name in enumerate(["depth", "color", "opacity", "feat"]):
            if t[name] is not None:
                terms[:, j] = t[name].double()
        return dict(terms=terms)

    def _var64(self):
        """The fp64 oracle's per-ray depth variance [K,R] (it does not depend on the targets)."""
        b, dt = self.b, torch.float64
        with torch.no_grad():
            if self.kind == "train":
                _, t = O.train_forward_loss(list(self.st[:18]), self.st[18], torch.full((self.K,), _scale(self.H)),
                                            T(b["pts"]), T(b["gt_depth"]), T(b["gt_rgb"]), T(b["labels"]), T(b["z"]),
                                            return_terms=True, mlp_dtype=dt, do_clip=False)
            else:
                _, t = O.step_batch_loss(self.alpha.to(dt), self.color.to(dt), T(b["gt_depth"]).to(dt),
                                         T(b["gt_rgb"]).to(dt), T(b["labels"]), None, T(b["z"]).to(dt), return_terms=True)
        return t["var"].double()

    def _poisoned(self, edits):
        b = {k: v.copy() for k, v in self.b.items()}
        for key, idx, val in edits:
            b[key][idx] = val
        return b

    def _target_for(self, key, idx, j, k, term):
        """The value of target b[key][idx] that puts term j of object k at `term`, from the fp64 oracle alone: for a
        target far above the rendered value, |rendered - target| = target - rendered, so the term is affine in it; two
        probes give slope and intercept."""
        g1, g2 = 50.0, 100.0
        t1 = float(self.oracle(self._poisoned([(key, idx, g1)]), torch.float64)["terms"][k, j])
        t2 = float(self.oracle(self._poisoned([(key, idx, g2)]), torch.float64)["terms"][k, j])
        slope = (t2 - t1) / (g2 - g1)
        assert slope > 0
        return float(np.float32(g1 + (term - t1) / slope))

    def _checked(self, edits, k, j, want_term, explode):
        """Before the GPU is touched: the fp64 oracle puts the term where intended and the fp32 oracle (the reference's
        own arithmetic) falls on the same side of 1e5 -- it exits (LossExplode) exactly when it should."""
        b = self._poisoned(edits)
        for dtype in (torch.float64, None):
            if explode:
                with pytest.raises(O.LossExplode):
                    self.oracle(b, dtype)
            else:
                t = float(self.oracle(b, dtype)["terms"][k, j])
                assert t < THRESH, (dtype, t)
                if dtype is torch.float64:
                    assert abs(t - want_term) < 1e-5 * want_term, (t, want_term)
        return b

    def _build(self):
        K, lab = self.K, self.b["labels"]
        others = lambda *ks: [q for q in range(K) if q not in ks]               # noqa: E731
        clean = (self.clean64, self.clean32)
        self.cases.append(("a_clean", self.b, 0, list(range(K)), clean))
        # b. colour, tight: the last object, then the first
        self.g_hi = {}
        for k in ([K - 1, 0] if K > 1 else [0]):
            r = _first_counted(lab[k])
            for side, sign, word in (("below", -1, 0), ("above", +1, 1)):
                want = THRESH * (1 + sign * MARGIN)
                g = self._target_for("gt_rgb", (k, r, 0), 1, k, want)
                edits = [("gt_rgb", (k, r, 0), g)]
                b = self._checked(edits, k, 1, want, explode=(sign > 0))
                self.cases.append((f"b_colour_{side}_obj{k}", b, word, others(k), clean))
                if sign > 0:
                    self.g_hi[k] = (r, g)
        # c. depth: a ray whose fp64 variance is far from zero; the term at 1e5 / 4 and at 1e5 * 4
        k = K - 1
        counted = np.nonzero(lab[k] == 1)[0]
        r = int(counted[int(torch.argmax(self.var64[k, counted]))])
        assert float(self.var64[k, r]) > 1e-3, float(self.var64[k, r])
        for side, want, word in (("below", THRESH / 4, 0), ("above", THRESH * 4, 1)):
            g = self._target_for("gt_depth", (k, r), 0, k, want)
            b = self._checked([("gt_depth", (k, r), g)], k, 0, want, explode=(word == 1))
            self.cases.append((f"c_depth_{side}_obj{k}", b, word, others(k), clean))
        # d. both bits from different objects (K = 1: from different terms of the one object), then g. a clean step
        k_nan, k_exp = 0, K - 1
        r_exp, g_exp = self.g_hi[k_exp]
        r_nan = _first_counted(lab[k_nan], skip=(r_exp,) if K == 1 else ())
        self.both = self._poisoned([("gt_depth", (k_nan, r_nan), np.nan), ("gt_rgb", (k_exp, r_exp, 0), g_exp)])
        with pytest.raises(O.LossExplode):
            self.oracle(self.both, torch.float64)
        self.cases.append(("d_both", self.both, 3, others(k_nan, k_exp), clean))
        self.cases.append(("g_clean_after_both", self.b, 0, list(range(K)), clean))
        # e. +Inf targets: `inf > 100000` is True, the reference exits
        for name, key, idx in (("colour", "gt_rgb", (k_exp, r_exp, 0)), ("depth", "gt_depth", (k_exp, r_exp))):
            b = self._poisoned([(key, idx, np.inf)])
            for dtype in (torch.float64, None):
                with pytest.raises(O.LossExplode):
                    self.oracle(b, dtype)
            self.cases.append((f"e_inf_{name}", b, 3, others(k_exp), clean))
        # f. the early return shields the test: object K-1 has no label-1 ray, another one (K = 1: the same) has the
        # exploding colour target -- the reference returns zeros before it looks (render_rays.py:89-94)
        k_far = 0
        b = self._poisoned([("gt_rgb", (k_far, self.g_hi[k_far][0], 0), self.g_hi[k_far][1])])
        b["labels"][K - 1][b["labels"][K - 1] == 1] = 0
        o64, o32 = self.oracle(b, torch.float64), self.oracle(b, None)
        assert float(o64["terms"][:, :2].abs().max()) == 0.0 and float(o32["terms"][:, :2].abs().max()) == 0.0
        self.cases.append(("f_early_return", b, 0, list(range(K)), (o64, o32)))
        self.cases.append(("g_clean_at_the_end", self.b, 0, list(range(K)), clean))


_SCENARIOS = {}


def _scenario(shape, feat, kind="train"):
    key = (shape, feat, kind)
    if key not in _SCENARIOS:
        _SCENARIOS[key] = _Scenario(shape, feat, kind)
    return _SCENARIOS[key]


def _host_contract(call, word):
    """bit 0 raises LossExplode, bit 1 alone warns, 0 is silent."""
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        if word & 1:
            with pytest.raises(LossExplode):
                call()
        else:
            call()
    warned = any(issubclass(w.category, RuntimeWarning) for w in rec)
    assert warned == (word == 2), (word, [str(w.message) for w in rec])


def _run_cases(sc, step, tol, label):
    """Every case of the scenario through `step(batch) -> (status tensor, terms [K,4])`; all figures are printed, all
    failures collected, so one run shows the whole picture of a path."""
    fails = []
    for name, b, want, rows, (o64, o32) in sc.cases:
        status_t, terms = step(b)
        word, terms = int(status_t.item()), terms.detach().double().cpu()
        again = _recompute(terms)
        print(f"{label:28s} {name:24s} status {word} want {want} from-terms {again} terms "
              + " ".join("[" + " ".join(f"{v:.6g}" for v in row) + "]" for row in terms.tolist()))
        if word != want:
            fails.append((name, "status", word, "want", want))
        if word != again:
            fails.append((name, "status", word, "but the terms say", again))
        try:
            _host_contract(lambda: check_status(status_t), want)
        except AssertionError as e:          # pragma: no cover
            fails.append((name, "host contract", str(e)))
        if name == "f_early_return" and float(terms[:, :2].abs().max()) != 0.0:
            fails.append((name, "depth / colour terms not zero", terms[:, :2].tolist()))
        if rows:
            try:
                assert_terms(terms[rows], dict(terms=o64["terms"][rows]), dict(terms=o32["terms"][rows]), feat=sc.feat,
                             tol=tol)
            except AssertionError as e:
                fails.append((name, "terms of the unpoisoned objects", rows, str(e)))
    assert not fails, fails


def _dev_batch(b, dev, feat):
    return {k: T(b[k]).to(dev) for k in KEYS + (["gt_feat"] if feat else [])}


@pytest.mark.parametrize("with_optim", [False, True], ids=["grads", "optim"])
@pytest.mark.parametrize("path", list(PATHS))
def test_status_word_of_a_training_step(dev, monkeypatch, path, with_optim):
    """Cases a-h on every path of ops.train_step, without and with the optimiser attached (optim= moves the reduction that
    writes the word into another kernel or instantiation): a. a clean batch gives 0; b. one counted ray's colour target
    puts an object's colour term at 1e5 (1 - 1e-3) -> 0 and at 1e5 (1 + 1e-3) -> 1, for the last and for the first object
    (the rendered colour lies in [0, 1] against a target near 1e7: its error, bf16 included, moves the term by < 1e-7
    relative); c. a depth target on a ray whose fp64 variance exceeds 1e-3 puts the depth TERM at 1e5 / 4 -> 0 and at
    1e5 * 4 -> 1 (the term divides by sqrt(var) + 1e-4 and moves by per cent between precisions, hence the factor);
    d. a NaN depth target in one object and the colour target of b in another -> exactly 3, LossExplode; e. a +Inf colour
    or depth target -> 3 (`inf > 100000`: the reference exits); f. an object without a label-1 ray beside the colour
    target of b -> zero depth / colour terms and 0 (the reference returns before its test); g. a clean step after d, and
    at the end, gives 0 again (the word belongs to the step); h. in every case the word equals the one recomputed from
    ws.loss_terms, check_status keeps the host contract, and the unpoisoned objects' terms pass assert_terms against the
    fp64 oracle (16-bit modes: at TERM_TOL).  With an optimiser the parameters are restored before every step, so each
    step sees the oracle's weights.

    Skipped combinations: a path that the library refuses for its shape or precision (ENOTSUP) is skipped with the
    library's message -- none of the listed paths is at present; `chunks256_fp16_lanes2` is skipped where the device has
    no room for the second lane's buffer (ops.TrainWorkspace then runs one lane, which `chunks256_fp16_lanes1` covers).
    The fp16 mode has no hidden-32 / hidden-128 path of its own (small batches run the fp32 kernels) and is not listed."""
    shape, feat, prec, lw, chunking = PATHS[path]
    sc = _scenario(shape, feat)
    H, K, R, S = sc.H, sc.K, sc.R, sc.n1 + sc.n2
    arena = ops.ParamArena(K, ops.NetShape(H, 512, 6), dev)
    arena.load_stacked([q.clone() for q in sc.st])
    arena.scale.fill_(_scale(H))
    kw = dict(layerwise=lw, precision=prec)
    if chunking:
        kc = 2 if K > 2 else 1
        one = ops.TrainWorkspace(arena, 1, R, S, feat, **kw).nbytes
        if chunking == "lanes1":
            monkeypatch.setenv("OBJNERF_ONE_LANE", "1")
        ws = ops.TrainWorkspace(arena, K, R, S, feat, budget=kc * one + 4096, **kw)
        assert ws.k_chunk == kc and ws.status_chunks.numel() == (K + kc - 1) // kc > 1
        if chunking == "lanes2" and ws.lanes != 2:
            pytest.skip("no room on the device for the second lane's buffer: the workspace runs one lane")
        assert ws.lanes == (2 if chunking == "lanes2" else 1)
    else:
        ws = ops.TrainWorkspace(arena, K, R, S, feat, **kw)
        assert ws.k_chunk == K
    opt = optim.ArenaAdamW(arena, lr=1e-3, weight_decay=0.013) if with_optim else None
    p0 = arena.params.clone()

    def step(b):
        if opt is not None:
            arena.params.copy_(p0)
        try:
            ops.train_step(arena, ws, _dev_batch(b, dev, feat), with_feat=feat, bf16=prec, layerwise=lw, optim=opt)
        except _lib.ObjnerfError as e:
            if "ENOTSUP" in str(e):
                pytest.skip(str(e))
            raise
        torch.cuda.synchronize()
        return ws.status, ws.loss_terms

    _run_cases(sc, step, TERM_TOL[prec], path + ("+optim" if with_optim else ""))


@pytest.mark.parametrize("feat", [False, True], ids=["nofeat", "feat"])
def test_status_word_of_step_batch_loss(dev, feat):
    """The same cases on objnerf_step_batch_loss (loss_total_kernel behind the stand-alone loss): the word and the terms
    from ops.step_batch_loss on the fp32 oracle's network outputs, against the oracle's step_batch_loss in fp64 on those
    outputs; and loss.step_batch_loss, the reference's signature, raises LossExplode / warns / stays silent by the word."""
    sc = _scenario("h32", feat, "loss")
    alpha, color = sc.alpha.squeeze(-1).contiguous().to(dev), sc.color.to(dev)
    pf = sc.pred_feat.to(dev) if feat else None

    def step(b):
        d = _dev_batch(b, dev, feat)
        out = ops.step_batch_loss(alpha, color, d["gt_depth"], d["gt_rgb"], d["labels"], d["z"],
                                  gt_feat=d.get("gt_feat"), pred_feat=pf)
        torch.cuda.synchronize()
        word = int(out["status"].item())
        _host_contract(lambda: oloss.step_batch_loss(alpha[..., None], color, d["gt_depth"], d["gt_rgb"], d["labels"], None,
                                                     d["z"], gt_partfeat=d.get("gt_feat"), pred_partfeat=pf), word)
        return out["status"], out["terms"]

    _run_cases(sc, step, 1e-4, "step_batch_loss" + ("_feat" if feat else ""))


def test_status_word_of_reduce_batch_loss(dev):
    """objnerf_reduce_batch_loss honours the same two bits: its [K] means against the oracle's reduce_batch_loss in fp64
    (which raises where the reference exits).  One masked element of the last, then the first object is chosen -- from the
    fp64 sums alone -- to put that object's mean at 1e5 (1 -+ 1e-3); with the information weight 1 / (sqrt(var) + 1e-4)
    at var = 0.04; a NaN in one object beside an exploding other gives exactly 3; +Inf gives 3; an empty mask zeroes every
    mean and shields the test; a clean call afterwards gives 0."""
    g = torch.Generator().manual_seed(4)
    K, R = 3, 300                                                # (more than one pass of the 256-thread reduction)
    base = torch.rand(K, R, generator=g, dtype=torch.float64)
    var = torch.full((K, R), 0.04, dtype=torch.float64)
    mask = torch.rand(K, R, generator=g) < 0.6
    mask[:, 0] = True

    def run(mat, m, v, want):
        mat = (mat * m).float()
        got, status = ops.reduce_batch_loss(mat.to(dev), None if v is None else v.float().to(dev), m.to(dev), l2=False, avg=True)
        torch.cuda.synchronize()
        word, got = int(status.item()), got.double().cpu()
        print("reduce_batch_loss status", word, "want", want, "means", got.tolist())
        assert word == want == _recompute(got), (word, want, got.tolist())
        _host_contract(lambda: render_rays.reduce_batch_loss(mat.to(dev), var=None if v is None else v.float().to(dev),
                                                             mask=m.to(dev)), want)
        if want & 1:
            for dt in (torch.float64, torch.float32):        # the reference exits, in its own arithmetic too
                with pytest.raises(O.LossExplode):
                    O.reduce_batch_loss(mat.to(dt), var=None if v is None else v.to(dt), mask=m)
        else:
            ref = O.reduce_batch_loss(mat.double(), var=v, mask=m)
            ok = torch.isfinite(ref)
            assert torch.equal(ok, torch.isfinite(got))
            assert float((got[ok] - ref[ok]).abs().max()) < 1e-5 * max(1.0, float(ref[ok].abs().max()))
        return got

    run(base, mask, None, 0)
    run(base, mask, var, 0)
    for v in (None, var):
        info = 1.0 if v is None else 1.0 / (0.04 ** 0.5 + 1e-4)
        for k in (K - 1, 0):
            rest = float((base[k] * mask[k]).sum() - base[k, 0]) * info
            for sign, want in ((-1, 0), (+1, 1)):
                mat = base.clone()
                mat[k, 0] = (THRESH * (1 + sign * MARGIN) * (float(mask[k].sum()) + 1e-10) - rest) / info
                run(mat, mask, v, want)
    mat = base.clone()
    mat[0, 0], mat[K - 1, 0] = float("nan"), 1e9
    run(mat, mask, None, 3)
    run(base, mask, None, 0)                                     # the word belongs to the call
    mat = base.clone()
    mat[1, 0] = float("inf")
    run(mat, mask, var, 3)
    m2 = mask.clone()
    m2[K - 1] = False
    mat = base.clone()
    mat[0, 0] = 1e9
    got = run(mat, m2, None, 0)                                  # early return: zeros for ALL objects, before the test
    assert float(got.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# the merges
# ---------------------------------------------------------------------------------------------------------------------
HUGE = 1e9          # a colour target far beyond the threshold: one counted ray puts the term at >= 1e9 / R


def _two_poisons(b, k_explode, k_nan):
    b = {k: v.copy() for k, v in b.items()}
    b["gt_rgb"][k_explode, _first_counted(b["labels"][k_explode]), 0] = HUGE
    b["gt_depth"][k_nan, _first_counted(b["labels"][k_nan])] = np.nan
    return b


@pytest.mark.parametrize("form", ["h128_fp32", "h256_fp16_lanes1", "h256_fp16_lanes2"])
def test_chunked_step_merges_the_chunks_words_bitwise(dev, monkeypatch, form):
    """K = 4 in chunks of 2: chunk 0 holds the object whose colour explodes (its slot says 1), chunk 1 the object with a
    NaN depth target (2) -- and the other way round.  ws.status is 3 both times (a numeric maximum over the slots gives 2:
    the mapper would warn where the reference exits), and 0 again after a clean step."""
    H, prec = (128, False) if form == "h128_fp32" else (256, "fp16")
    K, R, n1, n2 = (4, 40, 5, 9) if H == 128 else (4, 64, 16, 48)
    arena = ops.ParamArena(K, ops.NetShape(H, 512, 6), dev)
    arena.load_stacked(obj_init.init_stacked(K, H, 512, seed=SEED_NET))
    arena.scale.fill_(5.0)
    kw = dict(layerwise=(H == 128), precision=prec)
    one = ops.TrainWorkspace(arena, 1, R, n1 + n2, False, **kw).nbytes
    if form.endswith("lanes1"):
        monkeypatch.setenv("OBJNERF_ONE_LANE", "1")
    ws = ops.TrainWorkspace(arena, K, R, n1 + n2, False, budget=2 * one + 4096, **kw)
    assert ws.k_chunk == 2 and ws.status_chunks.numel() == 2
    if form.endswith("lanes2") and ws.lanes != 2:
        pytest.skip("no room on the device for the second lane's buffer: the workspace runs one lane")
    assert ws.lanes == (2 if form.endswith("lanes2") else 1)
    b = synthetic.random_batch(K, R, n1, n2, seed=SEED_BATCH)
    for k_explode, k_nan, slots in ((0, 2, [1, 2]), (3, 1, [2, 1])):
        ops.train_step(arena, ws, _dev_batch(_two_poisons(b, k_explode, k_nan), dev, False), bf16=prec, layerwise=(H == 128))
        torch.cuda.synchronize()
        print(form, "slots", ws.status_chunks.tolist(), "merged", int(ws.status.item()))
        assert ws.status_chunks.tolist() == slots
        assert int(ws.status.item()) == 3 == _recompute(ws.loss_terms)
        with pytest.raises(LossExplode):
            check_status(ws.status)
    ops.train_step(arena, ws, _dev_batch(b, dev, False), bf16=prec, layerwise=(H == 128))
    torch.cuda.synchronize()
    assert int(ws.status.item()) == 0 and ws.status_chunks.tolist() == [0, 0]


def test_forloop_strategy_merges_the_objects_words_bitwise(dev):
    """HipTrainLoop(strategy="forloop"): one launch per object, each with a word of its own; object 0 explodes (1), object
    1 has a NaN term (2) and the other way round: loop.status is 3, train_frame raises LossExplode; a clean step gives 0."""
    from openobj_amd import cfg as ocfg
    from openobj_amd import trainer

    def make_cfg():
        c = ocfg.Config(ocfg.replica_room0_config(train_device=str(dev)))
        c.obj_id = 1
        return c

    K, R, n1, n2 = 2, 40, 1, 9
    torch.manual_seed(11)
    ts = [trainer.Trainer(make_cfg()) for _ in range(K)]
    c = make_cfg()
    c.training_strategy = "forloop"
    loop = otrain.HipTrainLoop(c, ts, with_feat=False)
    b = synthetic.random_batch(K, R, n1, n2, seed=SEED_BATCH)
    for k_explode, k_nan in ((0, 1), (1, 0)):
        terms = loop.step(_dev_batch(_two_poisons(b, k_explode, k_nan), dev, False))
        torch.cuda.synchronize()
        words = [int(w.status.item()) for w in loop.wss]
        print("forloop words", words, "merged", int(loop.status.item()))
        assert words[k_explode] == 1 and words[k_nan] == 2
        assert int(loop.status.item()) == 3 == _recompute(terms)
    assert int(loop.ws.status.item()) == 3                       # (the holder train_frame and the mapper read)
    loop.step(_dev_batch(b, dev, False))
    torch.cuda.synchronize()
    assert int(loop.status.item()) == 0


@pytest.mark.parametrize("variant", ["obj_explodes_bg_nan", "bg_explodes_obj_nan", "nan_only"])
def test_frame_reports_the_or_of_its_iterations(dev, tmp_path, monkeypatch, variant):
    """IncrementalMapper.train_frame over 5 iterations of which ONLY iteration 1 is poisoned (the sample pools are edited
    as they leave sample_pools): an exploding colour target in the object chain with a NaN depth target in the background
    chain, the reverse, and NaNs alone.  The reference would have exited in iteration 1, so the frame raises LossExplode
    although its last iteration has no term above 1e5 (each step overwrites the word: read after the loop, bit 0 is gone);
    the NaN-only frame warns and returns its loss terms."""
    from openobj_amd import cfg as ocfg
    from openobj_amd import dataset as ods
    from openobj_amd import mapping
    try:
        from tests import scene_files as SF
    except ImportError:
        import scene_files as SF
    root = tmp_path / "scene"
    SF.write_scene(str(root), "Replica", n_frames=10)
    n_iter = 5
    over = {"dataset.path": str(root), "dataset.format": "Replica", "trainer.part_mode": 0, "camera.w": SF.W,
            "camera.h": SF.H, "camera.fx": SF.FX, "camera.fy": SF.FY, "camera.cx": SF.CX, "camera.cy": SF.CY,
            "render.iters_per_frame": n_iter, "render.n_per_optim_bg": 240, "render.depth_range": [0.0, 8.0]}
    c = ocfg.Config(ocfg.replica_room0_config(train_device=str(dev), **over))
    torch.manual_seed(7)
    m = mapping.IncrementalMapper(c)
    plain = m.sample_pools
    explode = {"obj_explodes_bg_nan": "obj", "bg_explodes_obj_nan": "bg", "nan_only": None}[variant]

    def poisoned_pools():
        pool, bg_pool = plain()
        assert pool is not None and bg_pool is not None
        for name, p in (("obj", pool), ("bg", bg_pool)):
            n = p["labels"].shape[1] // n_iter                   # rays per iteration; iteration 1 trains on [n, 2n)
            p["labels"][:, n] = 1                                # (every object counts that ray: no early return hides it)
            if explode == name:
                p["gt_rgb"][0, n, 0] = HUGE
            else:
                p["gt_depth"][0, n] = float("nan")
        return pool, bg_pool

    monkeypatch.setattr(m, "sample_pools", poisoned_pools)
    hist = []
    run = lambda: m.run(ods.init_loader(c, multi_worker=False), n_frames=1, on_frame=lambda f, l: hist.append(l))  # noqa: E731
    if explode is None:
        with pytest.warns(RuntimeWarning, match="NaN / Inf"):
            run()
        obj, bg = torch.stack(hist[0]["obj"]).cpu(), torch.stack(hist[0]["bg"]).cpu()
        assert obj.shape[0] == bg.shape[0] == n_iter
        for t in (obj, bg):                                      # iteration 0 is clean, iteration 1 carries the NaN terms
            assert bool(torch.isfinite(t[0]).all()) and not bool(torch.isfinite(t[1]).all())
    else:
        with pytest.raises(LossExplode):
            run()
        assert not hist
