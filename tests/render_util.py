"""Helpers of the renderer tests (test infrastructure only; openobj_amd never imports it): an fp64 reference and a
bf16-operand specification of the per-ray chain objnerf_render_fwd runs, the z-buffer merge of a whole view in numpy,
seeded networks / rays, and the table of bf16 bounds.

What is compared with what
--------------------------
* `render_rays_ref`: stratified bins -> mid-points -> embedding -> network -> compositing, built from the oracle's own
  functions and evaluated in fp64 from the fp32 inputs.  Only the bin edges are fp32, formed exactly as
  oracle.stratified_bins forms them: z is an OUTPUT the kernels are held to bit for bit (against objnerf_box_points,
  which fixture G11 pins), so the reference composites the same kind of numbers.
* `render_rays_spec_bf16`: the same chain with the network replaced by oracle.mlp_forward_stacked_16(bfloat16).  The
  flags are read off objnerf_render_bf16.hip / objnerf_bf16_common.h:
    - hidden layers take packed bf16 operands, `pack32(relu32(av))`, the activations themselves stay fp32 -> act16=False;
    - the density and colour heads read the unrounded fp32 h4 / hc against fp32 rows of sm[] -> round_head_weights=False;
    - the composited feature hidden is the unrounded hf;
    - embedding operands are rounded (pack8 of the x1 / x2 tiles);
    - stage_forward_bf16 stores the biases of the four layers that take the embedding (in_layer, cat_layer,
      color_linear, clip_linear) INSIDE the bf16 weight image, on the constant-1 entry of the embedding tile (w_emb,
      BIAS_COL), so those four biases are bf16 numbers; mid1 / mid2 and the head biases are fp32 (S_BM1, S_BM2, S_HB)
      -> round_emb_biases=True.
  `dtype` is the precision the specification is EVALUATED in (embedding, sin, every accumulation): float64, or float32
  for the second legitimate evaluation the floor F below is made of.  Compositing is fp64 in both.
* `view_ref`: oracle.render_2d_syn per object in dict order and the z-buffer merge of the reference's train.py:581-598
  written out in numpy, with a per-pixel margin image.

The bf16 bounds
---------------
BF16_TABLE holds, per output, F (the distance between the fp32 and the fp64 evaluation of the SAME specification: what
two correct implementations may disagree on) and D (the distance between the specification and the unrounded fp64
chain: what bf16 operands cost).  The GPU tests assert 10 F; tests/test_render_spec.py recomputes both on the CPU,
fails if they drift by more than 2x and asserts 10 F <= D / 4.  Printed by

    python -m pytest tests/test_render_spec.py -q -s -k floor_and_ceiling
"""
import functools
import types

import numpy as np
import torch

from oracle import objnerf_oracle as O

# ---------------------------------------------------------------------------------------------------------------------
# networks and rays
# ---------------------------------------------------------------------------------------------------------------------
# shift of out_alpha.bias (alpha = 10 (w . h4 + b), model.py:88), as fixture G11's ALPHA_BIAS, and a gain on
# out_alpha.weight so that the occupancy really varies along a ray.  mixed: opacities spread over (0, 1); saturate:
# occupancy ~ 1 from the first samples on; empty: occupancy ~ 1e-7 everywhere; gentle: see BF16_CASE.
NET_SETTINGS = {
    "mixed": dict(alpha_bias=-0.45, alpha_gain=3.0),
    "saturate": dict(alpha_bias=2.0, alpha_gain=1.0),
    "empty": dict(alpha_bias=-2.5, alpha_gain=1.0),
    "gentle": dict(alpha_bias=-0.4, alpha_gain=0.1),     # occupancy ~ 0.01 per sample: opacity builds up over ~ 100 samples
}


def make_net(setting="mixed", hidden=32, seed=0, alpha_bias=None):
    """-> (fc: the 18 fp32 tensors of one network in parameters() order, B [21,3]), all from `seed`."""
    g = torch.Generator().manual_seed(1000 + seed)
    fc = O.init_object_params(hidden, generator=g)
    s = NET_SETTINGS[setting]
    fc[8] = fc[8] * s["alpha_gain"]
    fc[9] = fc[9] + (s["alpha_bias"] if alpha_bias is None else alpha_bias)
    B = O.icosa_dirs() + 0.02 * torch.randn(21, 3, generator=g)
    return fc, B


def make_rays(n, n_bins, seed=0, origin=(0.1, -0.2, 0.3), near=(0.2, 1.0), length=(0.5, 2.0), with_u=True):
    """n rays from one origin.  Every quantity has a stream of its own, so the first m rays of a larger draw ARE the
    m-ray draw: the CPU bounds are computed on a prefix of exactly the rays the GPU tests render."""
    rs = [np.random.RandomState(7919 * seed + k) for k in range(4)]
    dirs = rs[0].standard_normal((n, 3)).astype(np.float32)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    lo = rs[1].uniform(near[0], near[1], n).astype(np.float32)
    hi = lo + rs[2].uniform(length[0], length[1], n).astype(np.float32)
    u = rs[3].uniform(0, 1, (n, n_bins)).astype(np.float32) if with_u else None
    t = torch.from_numpy
    return dict(origin=torch.tensor(origin, dtype=torch.float32), dirs=t(dirs), near=t(lo), far=t(hi),
                u=t(u) if with_u else None, n_bins=n_bins)


def load_arena(arena, fc, B):
    arena.load_stacked([p[None] for p in fc] + [B[None]])


# ---------------------------------------------------------------------------------------------------------------------
# the per-ray chain
# ---------------------------------------------------------------------------------------------------------------------
def box_z(near, far, u):
    """Mid-points of the stratified bins, fp32, the arithmetic of oracle.stratified_bins (utils.py:342-379) and
    trainer.py:175 on whatever device the inputs live on (the linspace is formed on the host as the oracle's is)."""
    n, n_bins = u.shape
    lim = torch.linspace(0, 1, n_bins + 1, dtype=torch.float32).to(u.device)
    rng = far - near
    lower = (rng[..., None] * lim + near[..., None])[:, :-1]
    z_cat = lower + u * (rng / n_bins)[..., None]
    return 0.5 * (z_cat[..., 1:] + z_cat[..., :-1])


def _net_fp64(p, emb):
    pres = []
    alpha, color, clip = O.mlp_forward(p, emb, do_clip=True, pres=pres)
    return alpha, color, clip, torch.relu(pres[5])


def _net_bf16(p, emb):
    # the 512-d head is linear and fp32 in the kernel's scheme (applied to the composited hidden afterwards): one row
    # of it is enough to make the oracle return the feature hidden's pre-activation
    ps = [q[None] for q in p]
    ps[16], ps[17] = ps[16][:, :1], ps[17][:, :1]
    shp = emb.shape
    a, c, _, pres = O.mlp_forward_stacked_16(ps, emb.reshape(1, -1, shp[-1]), torch.bfloat16, do_clip=True, act16=False,
                                             round_head_weights=False, want_pre=True, round_emb_biases=True)
    return a.reshape(*shp[:-1], 1), c.reshape(*shp[:-1], 3), None, torch.relu(pres[5]).reshape(*shp[:-1], -1)


def _chain(net, fc, B, scale, origin, dirs, near, far, u, dtype, device, z, chunk, want_feat):
    dev = torch.device(device)
    f32 = lambda t: torch.as_tensor(t).to(dev, torch.float32)
    origin, dirs, near, far = f32(origin), f32(dirs), f32(near), f32(far)
    z = box_z(near, far, f32(u)) if z is None else f32(z)
    n, S = z.shape
    p = [q.to(dev, dtype) for q in fc]
    p64 = [q.to(dev, torch.float64) for q in fc]
    Bd = B.to(dev, dtype)
    chunk = chunk or max(1, ((1 << 18) if dev.type == "cuda" else (1 << 16)) // max(S, 1))
    out = dict(depth=[], opacity=[], opacity10=[], rgb=[], hidden=[], feat=[])
    for r0 in range(0, n, chunk):
        zc = z[r0:r0 + chunk].to(dtype)
        pts = origin.to(dtype)[None, None, :] + dirs[r0:r0 + chunk].to(dtype)[:, None, :] * zc[:, :, None]
        emb = O.unidirs_embed(pts, Bd, float(scale))
        alpha, color, clip, hf = net(p, emb)
        z64 = zc.double()
        term = O.occupancy_to_termination(O.occupancy_activation(alpha.squeeze(-1).double()))
        out["depth"].append(O.render(term, z64))
        out["opacity"].append(term.sum(-1))
        out["opacity10"].append(term[..., :10].sum(-1))            # (reached within the first ten samples)
        out["rgb"].append(O.render(term[..., None], color.double(), dim=-2))
        hid = O.render(term[..., None], hf.double(), dim=-2)
        out["hidden"].append(hid)
        if want_feat:
            if clip is not None:
                out["feat"].append(O.render(term[..., None], clip.double(), dim=-2))
            else:       # out_clip applied after compositing: W hid + b opacity (exact, the head is linear; fp32 weights)
                out["feat"].append(hid @ p64[16].T + out["opacity"][-1][:, None] * p64[17][None, :])
    res = {k: torch.cat(v) for k, v in out.items() if v}
    res["z"] = z
    return res


def render_rays_ref(fc, B, scale, origin, dirs, near, far, u, dtype=torch.float64, device="cpu", z=None, chunk=None,
                    want_feat=True):
    """The unrounded chain.  -> dict(depth [n], opacity [n], opacity10 [n], rgb [n,3], hidden [n,H], feat [n,512], z [n,S]); fp64 on
    `device` except z (fp32).  z: the mid-points to use instead of forming them from u (the seeded kernels draw inside
    the launch; their z is pinned bit for bit to objnerf_box_points and handed in here)."""
    return _chain(_net_fp64, fc, B, scale, origin, dirs, near, far, u, dtype, device, z, chunk, want_feat)


def render_rays_spec_bf16(fc, B, scale, origin, dirs, near, far, u, dtype=torch.float64, device="cpu", z=None,
                          chunk=None, want_feat=True):
    """The bf16-operand specification (banner above), evaluated in `dtype`."""
    return _chain(_net_bf16, fc, B, scale, origin, dirs, near, far, u, dtype, device, z, chunk, want_feat)


def scaled_err(a, ref):
    """max |a - ref| / max(1, max |ref|): the measure of the 1e-4 parity bar (include/objnerf_hip.h, mode 0)."""
    a, ref = torch.as_tensor(a).double().cpu(), torch.as_tensor(ref).double().cpu()
    if ref.numel() == 0:
        return 0.0
    return float((a - ref).abs().max()) / max(1.0, float(ref.abs().max()))


def bf16_distances(a, b, near, far):
    """Per-output distance of two results of the chain: opacity / rgb max abs, depth max |.| / (far - near), the
    composited hidden in relative Frobenius norm."""
    d = lambda k: torch.as_tensor(a[k]).double().cpu() - torch.as_tensor(b[k]).double().cpu()
    span = (torch.as_tensor(far).double().cpu() - torch.as_tensor(near).double().cpu())
    return dict(opacity=float(d("opacity").abs().max()), rgb=float(d("rgb").abs().max()),
                depth=float((d("depth").abs() / span).max()),
                hidden=float(d("hidden").norm() / torch.as_tensor(b["hidden"]).double().norm()))


# The ray content of the fp32 cases (n_bins 150 unless stated): what each case must contain is asserted on the
# REFERENCE by check_regime, in the GPU test and -- on the first rays of the same draws -- in tests/test_render_spec.py.
CONTENT_CASES = {
    "saturate": dict(setting="saturate", scale=2.0, rays=dict(seed=11)),
    "empty": dict(setting="empty", scale=2.0, rays=dict(seed=12)),
    "zero_width": dict(setting="mixed", scale=2.0, rays=dict(seed=13, length=(0.0, 0.0))),
    "near_zero": dict(setting="mixed", scale=2.0, rays=dict(seed=14, near=(0.0, 0.0))),
    "scale_origin": dict(setting="mixed", scale=3.5, rays=dict(seed=15, origin=(12.0, -11.0, 12.0))),
}


def content_case(name, n, n_bins=150):
    c = CONTENT_CASES[name]
    fc, B = make_net(c["setting"])
    return fc, B, make_rays(n, n_bins, **c["rays"])


def check_regime(name, ref, r):
    op = ref["opacity"]
    if name == "saturate":        # exercises T *= (1 - occ) + 1e-10 with occ -> 1
        assert float(ref["opacity10"].min()) >= 0.999
    elif name == "empty":
        assert float(op.max()) < 1e-3
    elif name == "zero_width":
        assert bool((r["near"] == r["far"]).all()) and float(op.max()) > 0.5
    elif name == "near_zero":
        assert bool((r["near"] == 0).all()) and float(op.max()) > 0.5
    elif name == "scale_origin":
        assert float(r["origin"].norm()) > 20 and float(op.max()) > 0.9 and float(op.min()) < 0.1
    else:                          # mixed rays: some terminate, some do not
        assert float(op.max()) > 0.9 and float(op.min()) < 0.1


# The case the bf16 bounds belong to.  The issue's ratio, 10 F <= D / 4, is not reachable with 20 or 60 bins: F is made
# of single events (one operand of one sample rounding the other way), whose weight in a ray is ~ 1 / samples, while D
# is systematic.  Measured on the reference alone (same command), D / (40 F) is 0.3 .. 0.6 for opacity, colour and
# depth at 20 bins, 0.5 .. 1.4 at 60 and 2 .. 3.5 at 150 bins with a network whose occupancy builds up slowly ("gentle").
# So every bf16 case renders 150 bins of the gentle network.
BF16_ROWS = 4096
BF16_CASE = dict(n_bins=150, seed=4, setting="gentle", scale=2.0)
BF16_TABLE = dict(
    F=dict(opacity=1.309e-05, rgb=1.387e-05, depth=1.919e-05, hidden=1.279e-05),
    D=dict(opacity=1.120e-03, rgb=1.040e-03, depth=1.812e-03, hidden=1.644e-03),
)


def bf16_bounds():
    return {k: 10.0 * v for k, v in BF16_TABLE["F"].items()}


def bf16_case(n):
    """-> (fc, B, scale, rays) of the bf16 case at n rays."""
    c = BF16_CASE
    fc, B = make_net(c["setting"])
    return fc, B, c["scale"], make_rays(n, c["n_bins"], seed=c["seed"])


# ---------------------------------------------------------------------------------------------------------------------
# one object in its box, a whole view
# ---------------------------------------------------------------------------------------------------------------------
def camera(W, H, f):
    """-> rays_dir [W,H,3] of a pinhole camera with the principal point in the middle (vmap.py:701-720)."""
    return O.rays_dirs(W, H, f, f, W / 2.0 - 0.5, H / 2.0 - 0.5)


def rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    t = np.deg2rad(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def box(center, extent, axis=(0, 0, 1), deg=0.0):
    return types.SimpleNamespace(center=np.asarray(center, np.float64), R=rot(axis, deg),
                                 extent=np.asarray(extent, np.float64))


def syn_margin(r):
    """Per hit ray of an oracle.render_2d_syn result: how far the accept / reject decision is from flipping."""
    return torch.minimum((r["opacity"] - 0.9).abs(),
                         torch.minimum((r["depth_all"] - r["near"]).abs(), (r["depth_all"] - r["far"]).abs()))


def view_ref(objects, T_WC, rays_dir, bg_ids, class_of, draws):
    """objects: obj_id -> dict(fc, B, scale, box) in the order to render.  -> dict(rgb [W,H,3] uint8,
    maskid [W,H], depth [W,H], margin [W,H]): every object through oracle.render_2d_syn, merged as the reference's
    train.py:581-598 does (a z-buffer test against what is already there; background objects paint colour and id but
    never write depth).  margin: the smallest of |opacity - 0.9|, the distance of depth to near and to far (over the
    objects whose box the pixel's ray hits), the distance of rgb * 255 to the next integer (over the objects that
    accept the ray and so may paint it) and the smallest gap between the depths any two objects offer at the pixel."""
    W, H = rays_dir.shape[:2]
    rgb = np.zeros((W, H, 3), np.uint8)
    maskid = np.zeros((W, H), np.int32)
    depth = np.ones((W, H), np.float32) * 100
    margin = np.full((W, H), np.inf)
    offered = []
    full = torch.ones(W, H, dtype=torch.bool)
    T = torch.as_tensor(np.asarray(T_WC, np.float32))
    for oid, o in objects.items():
        r = O.render_2d_syn(o["fc"], o["B"], o["scale"], T, rays_dir, o["box"].center, o["box"].R, o["box"].extent,
                            full, draws[oid], obj_id=oid, render_part=False)
        if r is None:
            continue
        hit = np.zeros((W, H), bool)
        hit[full.numpy()] = r["hit"].numpy()
        c255 = r["rgb_all"].double().numpy() * 255
        kept = r["mask"].numpy()[hit]                    # (a rejected ray paints nothing: its colour decides nothing)
        m = np.minimum(syn_margin(r).double().numpy(), np.where(kept, np.abs(c255 - np.round(c255)).min(axis=1), np.inf))
        margin[hit] = np.minimum(margin[hit], m)
        obj_mask = r["mask"].numpy()
        this_depth = np.ones((W, H), np.float32) * 100
        this_rgb = np.zeros((W, H, 3), np.uint8)
        this_depth[obj_mask] = r["depth"].numpy()
        this_rgb[obj_mask] = r["color"].numpy()
        offered.append(this_depth.astype(np.float64))
        ok = depth > this_depth
        rgb[ok] = this_rgb[ok]
        maskid[ok] = class_of.get(oid, oid)
        if oid not in bg_ids:
            depth[ok] = this_depth[ok]
    if len(offered) > 1:
        st = np.sort(np.stack(offered), axis=0)
        gap = np.diff(st, axis=0)
        gap[st[1:] >= 100] = np.inf                      # (an object that does not cover the pixel competes with nobody)
        margin = np.minimum(margin, gap.min(axis=0))
    return dict(rgb=rgb, maskid=maskid, depth=depth, margin=margin)


# ---------------------------------------------------------------------------------------------------------------------
# the scenes of the per-pixel tests (shared by the GPU tests and the CPU check of their exclusion share)
# ---------------------------------------------------------------------------------------------------------------------
N_EVAL_BINS = 150        # trainer.py:145-146
EXCLUDE_CAP = 0.005      # at most this share of a compared set may sit on a threshold
MARGIN = 1e-4


def n_hits(T_WC, dirs_C, bx):
    sp = O.sample_points_bbox(torch.as_tensor(np.asarray(T_WC, np.float32)), dirs_C, bx.center, bx.R, bx.extent,
                              torch.zeros(1, 1))
    return 0 if sp is None else int(sp["hit"].sum())


def draws_for(T_WC, rays_dir, mask, bx, seed):
    n = n_hits(T_WC, rays_dir[mask], bx)
    return torch.from_numpy(np.random.RandomState(seed).uniform(0, 1, (n, N_EVAL_BINS)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def syn_scene(hidden):
    """One object in an oriented box seen by a 160 x 120 camera through a caller-supplied pixel mask."""
    W, H = 160, 120
    rays_dir = camera(W, H, 140.0)
    T_WC = np.eye(4, dtype=np.float32)
    T_WC[:3, :3] = rot((0.2, 1.0, 0.1), 8.0).astype(np.float32)
    T_WC[:3, 3] = [0.05, 0.02, -0.1]
    bx = box((0.3, 0.1, 2.0), (1.3, 0.9, 0.8), axis=(1.0, 2.0, 3.0), deg=25.0)
    w, h = np.meshgrid(np.arange(W), np.arange(H), indexing="ij")
    mask = ((3 * w + 5 * h) % 7 < 2) | ((w > 70) & (w < 90) & (h > 50) & (h < 64))
    fc, B = make_net("mixed", hidden=hidden, seed=5, alpha_bias=-0.2)
    return dict(W=W, H=H, rays_dir=rays_dir, T_WC=T_WC, box=bx, mask=mask, fc=fc, B=B, scale=2.0,
                u=draws_for(T_WC, rays_dir, torch.from_numpy(mask), bx, 31))


def syn_ref(s, render_part=True):
    key = f"_ref{int(render_part)}"                           # (kept with the scene: several tests ask for the same one)
    if key not in s:
        s[key] = O.render_2d_syn(s["fc"], s["B"], s["scale"], torch.from_numpy(s["T_WC"]), s["rays_dir"],
                                 s["box"].center, s["box"].R, s["box"].extent, torch.from_numpy(s["mask"]), s["u"],
                                 render_part=render_part)
    return s[key]


def syn_scene_bf16():
    """The scene of syn_scene(32) with the slowly accumulating network the bf16 bounds belong to (BF16_CASE); the bias
    puts the opacities of the box's rays on both sides of the 0.9 threshold."""
    fc, B = make_net(BF16_CASE["setting"], alpha_bias=-0.28)
    return dict(syn_scene(32), fc=fc, B=B, scale=BF16_CASE["scale"])


def syn_spec_bf16(s, device="cpu"):
    """render_2D_syn of the bf16 renderer as its specification has it: the box sampler of the oracle (hit, near, far,
    rays), then render_rays_spec_bf16 and the reject masks of vmap.py:665,672.  -> the per-ray dict of the chain plus
    hit [P], near, far, keep [n_hit] and edge [n_hit]: the rays whose accept / reject decision lies within the part-C
    bound of a threshold (|opacity - 0.9| within the opacity bound, depth within the depth bound -- a share of
    far - near -- of near or far)."""
    mask = torch.from_numpy(s["mask"])
    sp = O.sample_points_bbox(torch.from_numpy(s["T_WC"]), s["rays_dir"][mask], s["box"].center, s["box"].R,
                              s["box"].extent, s["u"])
    o = render_rays_spec_bf16(s["fc"], s["B"], s["scale"], sp["origins"][0], sp["dirs_W"], sp["near"], sp["far"], s["u"],
                              device=device)
    o = {k: v.cpu() for k, v in o.items()}
    near, far = sp["near"].double(), sp["far"].double()
    b = bf16_bounds()
    o["keep"] = ~((o["depth"] < near) | (o["depth"] > far) | (o["opacity"] < 0.9))
    gap = torch.minimum((o["depth"] - near).abs(), (o["depth"] - far).abs()) / (far - near)
    o["edge"] = ((o["opacity"] - 0.9).abs() < b["opacity"]) | (gap < b["depth"])
    o.update(hit=sp["hit"], near=sp["near"], far=sp["far"])
    return o


@functools.lru_cache(maxsize=None)
def view_scene():
    """A hidden-128 background (id 0) and three hidden-32 objects with hand-set boxes: 1 and 2 overlap in the image at
    different depths, 3 is partly outside the frustum."""
    W, H = 80, 60
    rays_dir = camera(W, H, 70.0)
    T_WC = np.eye(4, dtype=np.float32)
    T_WC[:3, 3] = [0.0, 0.05, -0.2]
    boxes = {0: box((0.0, 0.0, 2.6), (5.0, 4.0, 1.5)),
             1: box((-0.2, 0.0, 1.6), (0.9, 0.8, 0.6), axis=(0.0, 1.0, 0.0), deg=20.0),
             2: box((0.2, 0.1, 2.4), (1.2, 1.0, 0.6), axis=(1.0, 1.0, 0.0), deg=-15.0),
             3: box((1.5, -0.7, 1.8), (0.9, 0.7, 0.5), axis=(0.0, 0.0, 1.0), deg=30.0)}
    objects, draws = {}, {}
    full = torch.ones(W, H, dtype=torch.bool)
    for oid, bx in boxes.items():
        hidden = 128 if oid == 0 else 32
        fc, B = make_net("mixed", hidden=hidden, seed=10 + oid, alpha_bias=0.1 if oid == 0 else -0.1)
        objects[oid] = dict(fc=fc, B=B, scale=2.0, box=bx, hidden=hidden)
        draws[oid] = draws_for(T_WC, rays_dir, full, bx, 40 + oid)
    return dict(W=W, H=H, rays_dir=rays_dir, T_WC=T_WC, objects=objects, draws=draws, bg_ids=(0,),
                class_of={0: 7, 1: 3, 2: 5, 3: 9})
