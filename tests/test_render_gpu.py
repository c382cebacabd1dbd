"""GPU: the novel-view renderers against an fp64 reference and a bf16 specification (tests/render_util.py) --
objnerf_render_fwd in fp32 and bf16 over several grid passes, ragged ray counts and every ray regime, the layer-wise
chunk loop of sceneObject.render_2D_syn, and render_view per pixel.  The bounds of the bf16 cases and the share of
rays left out for sitting on a threshold are derived and checked on the reference alone in tests/test_render_spec.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import render_util as R
from openobj_amd import _lib, ops, render_view, trainer
from openobj_amd import cfg as ocfg
from openobj_amd import vmap as ovmap

pytestmark = pytest.mark.gpu

BAR = 1e-4        # "1e-4 parity" of include/objnerf_hip.h, mode 0: maxerr < 1e-4 * max(1, |ref|max)
H32 = 32


def cu_count(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def make_arena(dev, fc, B, scale):
    arena = ops.ParamArena(1, ops.NetShape(), dev)
    R.load_arena(arena, fc, B)
    arena.scale.fill_(float(scale))
    return arena


def render_fwd_guarded(arena, r, dev, n_bins, seeded=None, want_hfeat=True, bf16=False):
    """ops.render_fwd through the C entry with every output inside a larger tensor: one row of NaN before and after
    the n rows the kernel may write.  Lanes with ray >= n exist in every launch; the guards prove they wrote nothing."""
    origin, dirs, near, far = (r[k].to(dev).contiguous() for k in ("origin", "dirs", "near", "far"))
    u = None if seeded else r["u"].to(dev).contiguous()
    n, S = near.shape[0], n_bins - 1
    width = dict(depth=1, opacity=1, rgb=3, vals=H32, z=S)
    keys = [k for k in width if want_hfeat or k != "vals"]
    big = {k: torch.full((n + 2, width[k]), float("nan"), device=dev) for k in keys}
    ptr = lambda k: big[k][1:].data_ptr() if k in big else None
    net = arena.net.c()
    seed, draw = seeded if seeded else (None, 0)
    ops.check(ops.lib().objnerf_render_fwd(C.byref(net), n, n_bins, arena.params.data_ptr(), arena.scale.data_ptr(),
                                           origin.data_ptr(), dirs.data_ptr(), near.data_ptr(), far.data_ptr(),
                                           None if u is None else u.data_ptr(), ops._seed_of(seed), int(draw) & 0x1FFFFFFF,
                                           ptr("depth"), ptr("opacity"), ptr("rgb"), ptr("vals"), ptr("z"),
                                           _lib.TRAIN_BF16 if bf16 else 0, ops._stream()), "objnerf_render_fwd")
    torch.cuda.synchronize()
    out = {}
    for k in keys:
        assert bool(torch.isnan(big[k][0]).all()) and bool(torch.isnan(big[k][-1]).all()), f"guard row of {k} written"
        body = big[k][1:-1]
        assert not bool(torch.isnan(body).any()), f"{k}: a ray was not written"
        out[k] = body[:, 0] if k in ("depth", "opacity") else body
    return out


def kernel_feat(arena, o):
    """The 512-d feature as render_2D_syn forms it: the linear head on the kernel's composited hidden and opacity."""
    n = o["vals"].shape[0]
    return ops.feature_head(arena, o["vals"].contiguous().reshape(1, n, -1), o["opacity"].contiguous().reshape(1, n))[0]


# ---------------------------------------------------------------------------------------------------------------------
# B. objnerf_render_fwd fp32 against fp64
# ---------------------------------------------------------------------------------------------------------------------
def fp32_cases():
    c = {}
    # at least three trips round the grid-stride loop (2 CUs workgroups x 4 waves x 16 rays a pass) and a ragged tail
    c["multipass_injected"] = dict(n=lambda cu: 3 * 128 * cu + 5, n_bins=20, setting="mixed", rays=dict(seed=3))
    c["multipass_seeded"] = dict(n=lambda cu: 3 * 128 * cu + 5, n_bins=20, setting="mixed", rays=dict(seed=3),
                                 seeded=(1234, 77))
    # the smallest n that puts exactly one wave on a second pass
    c["one_wave_second_pass"] = dict(n=lambda cu: 128 * cu + 16 * 4 + 1, n_bins=150, setting="mixed", rays=dict(seed=4))
    for n in (1, 15, 16, 17, 63, 64, 65):
        c[f"n{n}"] = dict(n=n, n_bins=20, setting="mixed", rays=dict(seed=5))
    for nb in (2, 5, 20, 60, 149, 150):
        c[f"bins{nb}"] = dict(n=1003, n_bins=nb, setting="mixed", rays=dict(seed=6))
        c[f"bins{nb}_seeded"] = dict(n=1003, n_bins=nb, setting="mixed", rays=dict(seed=6), seeded=(99, 5))
    for name, cc in R.CONTENT_CASES.items():
        c[name] = dict(n=2051, n_bins=150, setting=cc["setting"], rays=cc["rays"], scale=cc["scale"], regime=name)
    return c


FP32_CASES = fp32_cases()


@pytest.mark.parametrize("name", list(FP32_CASES))
def test_render_fwd_fp32_against_fp64(dev, name):
    """Depth, opacity, rgb, the composited feature hidden and the 512-d feature (ops.feature_head on the kernel's
    hidden and opacity) within 1e-4 * max(1, |ref|max) of the fp64 chain; z bit-equal to objnerf_box_points (also for
    draws made inside the kernel under the same (seed, draw)); guard rows untouched; want_hfeat=False
    (render_fwd_kernel<false>: another LDS image, the same arithmetic) bit-equal in depth / opacity / rgb; a second
    call bit-equal to the first."""
    c = FP32_CASES[name]
    n = c["n"](cu_count(dev)) if callable(c["n"]) else c["n"]
    n_bins, scale, seeded = c["n_bins"], c.get("scale", 2.0), c.get("seeded")
    fc, B = R.make_net(c["setting"])
    r = R.make_rays(n, n_bins, **c["rays"])
    arena = make_arena(dev, fc, B, scale)
    o = render_fwd_guarded(arena, r, dev, n_bins, seeded=seeded)
    kw = dict(seed=seeded[0], draw=seeded[1]) if seeded else {}
    z, _ = ops.box_points(r["origin"], r["dirs"].to(dev), r["near"].to(dev), r["far"].to(dev),
                          None if seeded else r["u"].to(dev), n_bins, **kw)
    assert torch.equal(o["z"], z)
    ref = R.render_rays_ref(fc, B, scale, r["origin"], r["dirs"], r["near"], r["far"], r["u"], device=dev,
                            z=z if seeded else None)
    if not seeded:
        assert R.scaled_err(z, ref["z"]) < 2e-6
    if "regime" in c or n_bins >= 20 and n >= 1000:         # the case holds what it is there for (on the reference)
        R.check_regime(c.get("regime", "mixed"), ref, r)
    got = dict(depth=o["depth"], opacity=o["opacity"], rgb=o["rgb"], hidden=o["vals"], feat=kernel_feat(arena, o))
    errs = {k: R.scaled_err(got[k], ref[k]) for k in got}
    print(f"\nfp32 {name} n={n} n_bins={n_bins}: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    # the error of every grid pass on its own, so that a failure names the pass
    per_pass = 128 * cu_count(dev)
    for p0 in range(0, n, per_pass):
        for k in got:
            e = R.scaled_err(got[k][p0:p0 + per_pass], ref[k][p0:p0 + per_pass])
            assert e < BAR, f"{k}: {e:.3e} in grid pass {p0 // per_pass}"
    nf = render_fwd_guarded(arena, r, dev, n_bins, seeded=seeded, want_hfeat=False)
    again = render_fwd_guarded(arena, r, dev, n_bins, seeded=seeded)
    for k in ("depth", "opacity", "rgb", "z"):
        assert torch.equal(nf[k], o[k]), f"want_hfeat=False changes {k}"
    for k in o:
        assert torch.equal(again[k], o[k]), f"{k} differs between two calls"


# ---------------------------------------------------------------------------------------------------------------------
# C. objnerf_render_fwd bf16 against its specification
# ---------------------------------------------------------------------------------------------------------------------
BF16_N = {"multipass": lambda cu: 3 * 128 * cu + 5, "one_wave_second_pass": lambda cu: 128 * cu + 16 * 4 + 1}
BF16_N.update({f"n{n}": n for n in (1, 15, 16, 17, 63, 64, 65)})


@pytest.mark.parametrize("name", list(BF16_N))
def test_render_fwd_bf16_against_specification(dev, name):
    """The bf16-operand renderer against render_util.render_rays_spec_bf16 (flags read off the kernel), per output no
    further than 10 F (render_util.BF16_TABLE; tests/test_render_spec.py derives F and D on the reference alone and
    shows 10 F <= D / 4), with and without the feature hidden; guard rows; two calls bit-equal.  Every case renders
    150 bins of the slowly accumulating network: fewer samples per ray cannot meet the ratio (render_util.BF16_CASE).

    Measured on MI355X (profiles/render_bf16_spec.txt)."""
    n = BF16_N[name](cu_count(dev)) if callable(BF16_N[name]) else BF16_N[name]
    fc, B, scale, r = R.bf16_case(n)
    n_bins = R.BF16_CASE["n_bins"]
    arena = make_arena(dev, fc, B, scale)
    a = (fc, B, scale, r["origin"], r["dirs"], r["near"], r["far"], r["u"])
    spec = R.render_rays_spec_bf16(*a, device=dev, want_feat=False)
    bound = R.bf16_bounds()
    o = render_fwd_guarded(arena, r, dev, n_bins, bf16=True)
    assert R.scaled_err(o["z"], spec["z"]) < 2e-6
    got = dict(depth=o["depth"], opacity=o["opacity"], rgb=o["rgb"], hidden=o["vals"])
    d = R.bf16_distances(got, spec, r["near"], r["far"])
    print(f"\nbf16 {name} n={n}: " + "  ".join(f"{k} {d[k]:.2e} (bound {bound[k]:.2e}, D {R.BF16_TABLE['D'][k]:.1e})"
                                              for k in d))
    nf = render_fwd_guarded(arena, r, dev, n_bins, bf16=True, want_hfeat=False)
    again = render_fwd_guarded(arena, r, dev, n_bins, bf16=True)
    for k in o:
        assert torch.equal(again[k], o[k]), f"{k} differs between two calls"
    got_nf = dict(depth=nf["depth"], opacity=nf["opacity"], rgb=nf["rgb"], hidden=spec["hidden"])
    d_nf = R.bf16_distances(got_nf, spec, r["near"], r["far"])
    print("   want_hfeat=False: " + "  ".join(f"{k} {d_nf[k]:.2e}" for k in ("depth", "opacity", "rgb")))
    for k in d:
        assert d[k] <= bound[k], f"{k}: {d[k]:.3e} > {bound[k]:.3e}"
    for k in ("depth", "opacity", "rgb"):
        assert d_nf[k] <= bound[k], f"want_hfeat=False {k}: {d_nf[k]:.3e} > {bound[k]:.3e}"


# ---------------------------------------------------------------------------------------------------------------------
# D. render_2D_syn and render_view per pixel
# ---------------------------------------------------------------------------------------------------------------------
class SceneObj:
    """What render_2D_syn needs of a sceneObject: a trainer, a device and a box."""
    render_2D_syn = ovmap.sceneObject.render_2D_syn

    def __init__(self, dev, fc, B, scale, box, hidden, W, H, obj_id):
        c = ocfg.Config(ocfg.replica_room0_config(train_device=str(dev)))
        c.obj_id, c.W, c.H, c.hidden_feature_size, c.obj_scale = obj_id, W, H, hidden, float(scale)
        self.trainer = trainer.Trainer(c)
        with torch.no_grad():
            for p, q in zip(self.trainer.fc_occ_map.parameters(), fc):
                p.copy_(q)
            self.trainer.pe.B_layer.weight.copy_(B)
        self.training_device = dev
        self.box = box

    def get_bound(self, *a, **k):
        return None, self.box


def syn_object(dev, s, hidden):
    return SceneObj(dev, s["fc"], s["B"], s["scale"], s["box"], hidden, s["W"], s["H"], 1 if hidden == 32 else 0)


def run_syn(obj, s):
    return obj.render_2D_syn(s["T_WC"], None, s["rays_dir"], obj_mask=s["mask"].copy(), render_part=True, draws=s["u"])


def check_syn(res, s, r):
    """mask equal except on rays within 1e-4 of a threshold (at most 0.5 % of the hit rays), depth and feature to the
    1e-4 bar, colour (uint8 truncation of rgb * 255) within 1 -- on the rays both sides keep."""
    mask, depth, color, feat = res
    ref_mask = r["mask"].numpy()
    on_edge = (R.syn_margin(r) < R.MARGIN).numpy()
    assert on_edge.mean() <= R.EXCLUDE_CAP
    edge_img = np.zeros_like(ref_mask)
    hit_img = np.zeros_like(ref_mask)
    hit_img[s["mask"]] = r["hit"].numpy()
    edge_img[hit_img] = on_edge
    assert np.array_equal(mask[~edge_img], ref_mask[~edge_img])
    both = (mask & ref_mask)
    ours, theirs = both[mask], both[ref_mask]               # rows of each side's compact arrays
    assert theirs.sum() >= (1 - R.EXCLUDE_CAP) * ref_mask.sum()
    errs = dict(depth=R.scaled_err(depth[ours], r["depth"].numpy()[theirs]),
                feat=R.scaled_err(feat[ours], r["feat"].numpy()[theirs]))
    dc = int(np.abs(color[ours].astype(int) - r["color"].numpy()[theirs].astype(int)).max())
    print(f"\nrender_2D_syn: {int(r['hit'].sum())} hit, {int(ref_mask.sum())} kept, depth {errs['depth']:.2e} "
          f"feat {errs['feat']:.2e} colour {dc}")
    assert errs["depth"] < BAR and errs["feat"] < BAR and dc <= 1
    assert feat.shape == (int(mask.sum()), 512)


@pytest.mark.parametrize("hidden", [32, 128])
def test_render_2d_syn_per_pixel(dev, hidden):
    """A 160 x 120 camera, an oriented box, a caller-supplied pixel mask, render_part=True against
    oracle.render_2d_syn on the same injected draws: ~2400 hit rays (the fused kernel, or the layer-wise chain)."""
    s = R.syn_scene(hidden)
    r = R.syn_ref(s)
    check_syn(run_syn(syn_object(dev, s, hidden), s), s, r)


def spy(monkeypatch, name):
    """Record what ops.<name> returns to render_2D_syn (the per-ray tensors its public return only shows in part)."""
    calls, real = [], getattr(ops, name)

    def wrapped(*a, **k):
        calls.append(real(*a, **k))
        return calls[-1]

    monkeypatch.setattr(ops, name, wrapped)
    return calls


PER_RAY = ("depth", "opacity", "rgb", "vals")


def test_render_2d_syn_bf16_per_pixel(dev, monkeypatch):
    """trainer.render_bf16 = True (vmap.py's bf16 route into objnerf_render_fwd) on the scene of the fp32 case with
    the network of part C, against render_util.syn_spec_bf16: the per-ray depth / opacity / rgb / feature hidden the
    kernel hands back within the part-C bounds of the specification over every hit ray; the mask equal except on rays
    within that bound of a threshold (at most 0.5 %; share asserted on the CPU); colour within 1; the returned depth
    IS the kernel's, and the returned 512-d feature the linear head on the kernel's hidden and opacity (1e-4 bar)."""
    s = R.syn_scene_bf16()
    spec = R.syn_spec_bf16(s, device=dev)
    obj = syn_object(dev, s, 32)
    obj.trainer.render_bf16 = True
    calls = spy(monkeypatch, "render_fwd")
    mask, depth, color, feat = run_syn(obj, s)
    assert len(calls) == 1
    o = {k: calls[0][k].cpu() for k in PER_RAY}
    got = dict(depth=o["depth"], opacity=o["opacity"], rgb=o["rgb"], hidden=o["vals"])
    d = R.bf16_distances(got, spec, spec["near"], spec["far"])
    bound = R.bf16_bounds()
    print("\nrender_2D_syn bf16: " + "  ".join(f"{k} {d[k]:.2e} (bound {bound[k]:.2e})" for k in d))
    for k in d:
        assert d[k] <= bound[k], f"{k}: {d[k]:.3e} > {bound[k]:.3e}"
    edge = spec["edge"].numpy()
    assert edge.mean() <= R.EXCLUDE_CAP
    hit_img = np.zeros_like(s["mask"])
    hit_img[s["mask"]] = spec["hit"].numpy()
    keep_img, edge_img = np.zeros_like(hit_img), np.zeros_like(hit_img)
    keep_img[hit_img], edge_img[hit_img] = spec["keep"].numpy(), edge
    assert np.array_equal(mask[~edge_img], keep_img[~edge_img])
    keep = mask[hit_img]                                    # the kernel's own decision, per hit ray
    assert np.array_equal(depth, o["depth"].numpy()[keep])
    both = keep & spec["keep"].numpy()
    c_spec = (spec["rgb"].numpy() * 255).astype(np.uint8)
    assert int(np.abs(color[both[keep]].astype(int) - c_spec[both].astype(int)).max()) <= 1
    fc = [p.double() for p in s["fc"]]
    head = o["vals"].double()[keep] @ fc[16].T + o["opacity"].double()[keep][:, None] * fc[17][None, :]
    assert R.scaled_err(feat, head) < BAR
    fp32 = run_syn(syn_object(dev, s, 32), s)
    assert not np.array_equal(fp32[1], depth)


def test_render_2d_syn_chunk_boundaries_do_not_show(dev, monkeypatch):
    """The hidden-128 chain in chunks of 101 rays (several chunks, a ragged last one) against the one-chunk run: the
    per-ray depth, opacity, rgb and feature hidden that objnerf_composite hands back (every hit ray, before any
    threshold or truncation) and the public return (mask, depth, colour, feature) bit-equal."""
    s = R.syn_scene(128)
    obj = syn_object(dev, s, 128)
    calls = spy(monkeypatch, "composite")
    one = run_syn(obj, s)
    assert len(calls) == 1
    per_ray_one = {k: calls[0][k].clone() for k in PER_RAY}
    calls.clear()
    monkeypatch.setattr(ovmap, "RENDER_SAMPLES_PER_CHUNK", 149 * 101)
    n_hit = int(s["u"].shape[0])
    assert n_hit > 3 * 101 and n_hit % 101 != 0
    many = run_syn(obj, s)
    assert len(calls) == -(-n_hit // 101) and calls[-1]["depth"].shape[0] == n_hit % 101
    for k in PER_RAY:
        assert torch.equal(torch.cat([c[k] for c in calls]), per_ray_one[k]), k
    for a, b in zip(one, many):
        assert a.shape == b.shape and np.array_equal(a, b)
    check_syn(many, s, R.syn_ref(s))


def test_render_2d_syn_degenerate_returns(dev):
    s = R.syn_scene(32)
    # the box behind the camera
    behind = dict(s, box=R.box((0.3, 0.1, -3.0), (1.3, 0.9, 0.8)))
    assert syn_object(dev, behind, 32).render_2D_syn(s["T_WC"], None, s["rays_dir"], obj_mask=s["mask"].copy(),
                                                     render_part=True) == (None, None, None)
    # exactly one hit ray: "too few hits" (trainer.py:164-165)
    one = np.zeros_like(s["mask"])
    hit_img = np.zeros_like(s["mask"])
    hit_img[s["mask"]] = R.syn_ref(s, render_part=False)["hit"].numpy()
    w, h = np.argwhere(hit_img)[0]
    one[w, h] = True
    assert one.sum() == 1 and hit_img[one].all()
    assert syn_object(dev, s, 32).render_2D_syn(s["T_WC"], None, s["rays_dir"], obj_mask=one,
                                                render_part=True) == (None, None, None)
    # every hit ray rejected by the masks: empty arrays, a [0, C] feature
    fc, B = R.make_net("empty")
    empty = dict(s, fc=fc, B=B)
    mask, depth, color, feat = run_syn(syn_object(dev, empty, 32), empty)
    assert not mask.any() and mask.shape == (s["W"], s["H"])
    assert depth.shape == (0,) and color.shape == (0, 3) and feat.shape == (0, 512)


@pytest.mark.parametrize("reverse", [False, True])
def test_render_view_per_pixel(dev, reverse):
    """A hidden-128 background (in bg_ids) and three hidden-32 objects -- two overlapping at different depths, one cut
    by the frustum -- with a class_of map and per-object draws, against render_util.view_ref (the reference's merge in
    numpy) in the same dict order: maskid equal, rgb within 1, depth to the 1e-4 bar on every pixel whose margin is at
    least 1e-4 (at most 0.5 % are not); the background paints colour, never depth (tests/test_render_spec.py shows on
    the reference that the depth image is the one without the background)."""
    v = R.view_scene()
    order = list(v["objects"])[::-1] if reverse else list(v["objects"])
    objs = {k: v["objects"][k] for k in order}
    ref = R.view_ref(objs, v["T_WC"], v["rays_dir"], v["bg_ids"], v["class_of"], v["draws"])
    vis = {k: SceneObj(dev, o["fc"], o["B"], o["scale"], o["box"], o["hidden"], v["W"], v["H"], k) for k, o in objs.items()}
    buf = render_view.render_view(vis, v["T_WC"], v["rays_dir"], bg_ids=v["bg_ids"], class_of=v["class_of"],
                                  draws=v["draws"])
    ok = ref["margin"] >= R.MARGIN
    assert (~ok).mean() <= R.EXCLUDE_CAP
    assert np.array_equal(buf.maskid[ok], ref["maskid"][ok])
    dc = int(np.abs(buf.rgb[ok].astype(int) - ref["rgb"][ok].astype(int)).max())
    de = R.scaled_err(buf.depth[ok], ref["depth"][ok])
    print(f"\nrender_view reverse={reverse}: {int((~ok).sum())} pixels left out, colour {dc}, depth {de:.2e}")
    assert dc <= 1 and de < BAR
    bg = buf.maskid == v["class_of"][0]
    assert bg.any()
    if not reverse:                                         # painted first, the background leaves no depth behind
        assert (buf.depth[bg] == 100).all()
