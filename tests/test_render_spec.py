"""CPU: what the GPU renderer tests (tests/test_render_gpu.py) rest on, checked on the reference alone -- the bf16
bounds (floor F, ceiling D, 10 F <= D / 4), the ray regimes, and the share of rays / pixels the per-pixel tests leave
out for sitting on a threshold."""
import numpy as np
import pytest
import torch

import render_util as R
from oracle import objnerf_oracle as O

OUTPUTS = ("opacity", "rgb", "depth", "hidden")


@pytest.fixture(scope="module")
def bf16_fd():
    fc, B, scale, r = R.bf16_case(R.BF16_ROWS)
    a = (fc, B, scale, r["origin"], r["dirs"], r["near"], r["far"], r["u"])
    ref = R.render_rays_ref(*a, want_feat=False)
    s64 = R.render_rays_spec_bf16(*a, want_feat=False)
    s32 = R.render_rays_spec_bf16(*a, dtype=torch.float32, want_feat=False)
    F = R.bf16_distances(s32, s64, r["near"], r["far"])
    D = R.bf16_distances(s64, ref, r["near"], r["far"])
    return F, D, ref


def test_bf16_floor_and_ceiling(bf16_fd):
    """F: the fp32 against the fp64 evaluation of the bf16 specification (accumulation of every baddbmm, the
    embedding's sin).  D: the specification against the unrounded fp64 chain.  The GPU bound 10 F must let through at
    most a quarter of what bf16 operands cost, and the committed table must be what this machine computes (2x)."""
    F, D, ref = bf16_fd
    for k in OUTPUTS:
        print(f"bf16 {k:8s} F = {F[k]:.3e}   D = {D[k]:.3e}   10 F / (D / 4) = {40 * F[k] / D[k]:.3f}   "
              f"table F = {R.BF16_TABLE['F'][k]:.3e}  D = {R.BF16_TABLE['D'][k]:.3e}")
    assert float(ref["opacity"].min()) > 0.05 and float(ref["opacity"].max()) < 0.999   # rays that build up slowly
    for k in OUTPUTS:
        assert 10 * F[k] <= D[k] / 4, k
        assert 10 * R.BF16_TABLE["F"][k] <= R.BF16_TABLE["D"][k] / 4, k
        assert 0.5 <= F[k] / R.BF16_TABLE["F"][k] <= 2.0, k
        assert 0.5 <= D[k] / R.BF16_TABLE["D"][k] <= 2.0, k


def test_bias_rounding_flag_changes_only_the_four_embedding_layers():
    """oracle.mlp_forward_stacked_16(round_emb_biases=True) is the default arithmetic with the biases of in_layer,
    cat_layer, color_linear and clip_linear rounded beforehand -- and the default output is unchanged."""
    fc, B = R.make_net("gentle")
    ps = [p[None] for p in fc]
    emb = O.unidirs_embed(torch.randn(1, 64, 3, generator=torch.Generator().manual_seed(1)), B, 2.0)
    a = O.mlp_forward_stacked_16(ps, emb, torch.bfloat16, act16=False, round_emb_biases=True)
    q = list(ps)
    for i in (1, 5, 11, 15):
        q[i] = q[i].bfloat16().float()
    b = O.mlp_forward_stacked_16(q, emb, torch.bfloat16, act16=False)
    c = O.mlp_forward_stacked_16(ps, emb, torch.bfloat16, act16=False)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y)
    assert not torch.equal(a[0], c[0])


def test_reference_helpers_agree_with_the_oracle():
    """render_rays_ref restates oracle.render_forward (fp32) in fp64, and its z is oracle.stratified_bins' bit for bit."""
    fc, B = R.make_net("mixed")
    r = R.make_rays(257, 20, seed=1)
    ref = R.render_rays_ref(fc, B, 2.0, r["origin"], r["dirs"], r["near"], r["far"], r["u"])
    zc = O.stratified_bins(r["near"], r["far"], 20, 257, r["u"])
    z = 0.5 * (zc[..., 1:] + zc[..., :-1])
    assert torch.equal(ref["z"], z)
    pts = r["origin"][None, None, :] + r["dirs"][:, None, :] * z[:, :, None]
    o = O.render_forward([p[None] for p in fc], B[None], torch.tensor([2.0]), pts[None], z[None])
    for k, kk in (("depth", "depth"), ("opacity", "opacity"), ("rgb", "rgb"), ("feat", "feat")):
        assert R.scaled_err(o[kk][0], ref[k]) < 2e-5, k


@pytest.mark.parametrize("hidden", [32, 128])
def test_exclusion_share_render_2d_syn(hidden):
    """The rays the render_2D_syn tests leave out (margin below 1e-4) on the reference alone, and what the scene holds."""
    s = R.syn_scene(hidden)
    r = R.syn_ref(s, render_part=False)
    n_hit, n_keep = int(r["hit"].sum()), int(r["mask"].sum())
    share = float((R.syn_margin(r) < R.MARGIN).double().mean())
    print(f"render_2D_syn hidden {hidden}: {n_hit} hit rays, {n_keep} accepted, excluded share {share:.4%}")
    assert share <= R.EXCLUDE_CAP
    assert 0 < n_hit < int(s["mask"].sum())                 # the box does not cover the mask
    assert 0.1 * n_hit < n_keep < 0.9 * n_hit               # both accepted and rejected rays


def test_exclusion_share_render_2d_syn_bf16():
    """The same for the bf16 case: the margin is the part-C bound, the reference the bf16 specification."""
    o = R.syn_spec_bf16(R.syn_scene_bf16())
    share, kept = float(o["edge"].double().mean()), float(o["keep"].double().mean())
    print(f"render_2D_syn bf16: {int(o['hit'].sum())} hit rays, accepted {kept:.1%}, excluded share {share:.4%}")
    assert share <= R.EXCLUDE_CAP
    assert 0.1 < kept < 0.9


@pytest.mark.parametrize("reverse", [False, True])
def test_exclusion_share_view(reverse):
    v = R.view_scene()
    order = list(v["objects"])[::-1] if reverse else list(v["objects"])
    ref = R.view_ref({k: v["objects"][k] for k in order}, v["T_WC"], v["rays_dir"], v["bg_ids"], v["class_of"],
                     v["draws"])
    share = float((ref["margin"] < R.MARGIN).mean())
    ids = {int(i): int(c) for i, c in zip(*np.unique(ref["maskid"], return_counts=True))}
    print(f"view (reverse={reverse}): ids {ids}, excluded share {share:.4%}")
    assert share <= R.EXCLUDE_CAP
    assert set(ids) == {0, 3, 5, 7, 9}                      # every object and the untouched rest are in the picture
    n3 = int(v["draws"][3].shape[0])
    assert 0 < n3 < 0.1 * v["W"] * v["H"]                   # object 3 is cut by the frustum
    bg = ref["maskid"] == 7
    assert bg.any()
    if not reverse:                                         # painted first, the background leaves no depth behind
        assert (ref["depth"][bg] == 100).all()
    fg = R.view_ref({k: v["objects"][k] for k in order if k != 0}, v["T_WC"], v["rays_dir"], v["bg_ids"], v["class_of"],
                    v["draws"])
    assert np.array_equal(fg["depth"], ref["depth"])        # the background paints colour, never depth


def test_ray_regimes_are_present():
    """The regimes the fp32 GPU cases name, on the reference at the first rays of the same draws."""
    for name, c in R.CONTENT_CASES.items():
        fc, B, r = R.content_case(name, 512)
        ref = R.render_rays_ref(fc, B, c["scale"], r["origin"], r["dirs"], r["near"], r["far"], r["u"], want_feat=False)
        R.check_regime(name, ref, r)
