"""Thin tensor-level wrappers over the C ABI (include/objnerf_hip.h).

PyTorch is plumbing here: it owns device memory and the stream; all arithmetic of the path runs in
libobjnerf_hip.so.  Every function requires CUDA(HIP) tensors and raises on anything else.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import AdamWArgs, LossArgs, Net, ObjnerfError, SampleArgs, TRAIN_SELF_COUNTS, TrainArgs, check, lib

EMB1, EMB2, N_DIRS = 87, 42, 21
TENSOR_NAMES = [
    "in_layer.0.weight", "in_layer.0.bias", "mid1.0.0.weight", "mid1.0.0.bias",
    "cat_layer.0.weight", "cat_layer.0.bias", "mid2.0.0.weight", "mid2.0.0.bias",
    "out_alpha.weight", "out_alpha.bias", "color_linear.0.weight", "color_linear.0.bias",
    "out_color.weight", "out_color.bias", "clip_linear.0.weight", "clip_linear.0.bias",
    "out_clip.weight", "out_clip.bias", "B_layer.weight",
]
FEAT_TENSORS = (14, 15, 16, 17)


def tensor_shapes(hidden: int, feat_dim: int = 512) -> List[Tuple[int, ...]]:
    H, Cc = hidden, feat_dim
    return [(H, EMB1), (H,), (H, H), (H,), (H, H + EMB1), (H,), (H, H), (H,), (1, H), (1,),
            (H, EMB2 + H), (H,), (3, H), (3,), (H, EMB2 + H), (H,), (Cc, H), (Cc,), (N_DIRS, 3)]


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    return t.data_ptr()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _req(t: torch.Tensor, dtype, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise _lib.ObjnerfError(f"{name}: expected a GPU tensor (there is no CPU path)")
    if t.dtype != dtype:
        raise _lib.ObjnerfError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        t = t.contiguous()
    return t


@dataclass
class NetShape:
    hidden: int = 32
    feat_dim: int = 512
    n_freqs: int = 6

    def c(self) -> Net:
        return Net(self.hidden, self.feat_dim, self.n_freqs, 0)


class ParamArena:
    """K networks in one object-major fp32 arena [K, p_stride] (+ same-layout grad / Adam buffers).

    `views(buf)` returns the 19 stacked tensors the reference exposes after
    functorch.combine_state_for_ensemble (utils.py:55-62) as strided views of the arena.
    """

    def __init__(self, K: int, net: NetShape, device):
        self.K, self.net = K, net
        self.offsets, self.p_stride = _lib.param_layout(net.hidden, net.feat_dim, net.n_freqs)
        self.P = self.offsets[-1]
        self.shapes = tensor_shapes(net.hidden, net.feat_dim)
        self.params = torch.zeros(K, self.p_stride, dtype=torch.float32, device=device)
        self.scale = torch.full((K,), 2.0, dtype=torch.float32, device=device)
        self.version = 0            # bumped by every writer that goes around torch (the kernels write raw pointers)

    def set_scale(self, value: float) -> None:
        """scale[:] = value, skipped when that is what the last set_scale wrote and nobody has touched the tensor since
        (a module's forward calls this every time; an unconditional fill_ would count as a modification between the
        forward and the backward of an earlier call)."""
        key = (float(value), self.scale._version)
        if getattr(self, "_scale_set", None) == key:
            return
        self.scale.fill_(float(value))
        self._scale_set = (float(value), self.scale._version)

    def state_version(self):
        """What an autograd node compares between its forward and its backward (autograd.py): the kernels' own write
        counter plus torch's in-place counters of the two tensors the kernels read."""
        return (self.version, self.params._version, self.scale._version)

    def owns(self, t: torch.Tensor) -> bool:
        """t is a view into this arena's parameter block."""
        lo = self.params.data_ptr()
        return t.device == self.params.device and lo <= t.data_ptr() < lo + self.params.numel() * 4

    def views(self, buf: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
        buf = self.params if buf is None else buf
        out = []
        for i, shp in enumerate(self.shapes):
            n = 1
            for s in shp:
                n *= s
            out.append(buf[:, self.offsets[i]:self.offsets[i] + n].view(self.K, *shp))
        return out

    def load_stacked(self, tensors: Sequence[torch.Tensor]) -> None:
        """tensors: 19 stacked [K,...] tensors (18 FC in parameters() order + B)."""
        for v, t in zip(self.views(), tensors):
            v.copy_(t.to(v.device))
        self.version += 1

    def has_grad_mask(self, with_feat: bool) -> torch.Tensor:
        m = torch.ones(self.P, dtype=torch.uint8, device=self.params.device)
        if not with_feat:
            m[self.offsets[14]:self.offsets[18]] = 0
        return m


# ---------------------------------------------------------------------------------------------------
def eval_points(arena: ParamArena, pts: torch.Tensor, want_hfeat: bool = False, want_clip: bool = False):
    """pts [K,N,3] -> alpha [K,N], color [K,N,3], hfeat [K,N,H] | None, clip [K,N,C] | None."""
    pts = _req(pts, torch.float32, "pts")
    K, N = pts.shape[0], pts.shape[1]
    dev = pts.device
    alpha = torch.empty(K, N, device=dev)
    color = torch.empty(K, N, 3, device=dev)
    hfeat = torch.empty(K, N, arena.net.hidden, device=dev) if (want_hfeat or want_clip) else None
    clip = torch.empty(K, N, arena.net.feat_dim, device=dev) if want_clip else None
    net = arena.net.c()
    nbytes = int(lib().objnerf_eval_workspace_bytes(C.byref(net), K, N))      # 0 for hidden 32 (fused kernel)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
    check(lib().objnerf_eval_points_ws(C.byref(net), K, N, _ptr(arena.params), arena.p_stride, _ptr(arena.scale),
                                       _ptr(pts), _ptr(alpha), _ptr(color), _ptr(hfeat), _ptr(clip), _ptr(ws), nbytes,
                                       _stream()),
          "objnerf_eval_points_ws")
    return alpha, color, hfeat, clip


def box_rays(T_WC: torch.Tensor, T_OC: torch.Tensor, half_extent: torch.Tensor, dirs_C: torch.Tensor):
    """Camera rays of one view against an oriented box (trainer.py:136-167): dirs_C [P,3] ->
    dirs_W [P,3], near [P] (>= 0), far [P] (+0.2), hit [P] bool."""
    dirs_C = _req(dirs_C, torch.float32, "dirs_C")
    dev = dirs_C.device
    P = dirs_C.shape[0]
    T_WC = T_WC.to(dev, torch.float32).contiguous()
    T_OC = T_OC.to(dev, torch.float32).contiguous()
    half_extent = half_extent.to(dev, torch.float32).contiguous()
    dirs_W = torch.empty(P, 3, device=dev)
    near = torch.empty(P, device=dev)
    far = torch.empty(P, device=dev)
    hit = torch.empty(P, dtype=torch.uint8, device=dev)
    check(lib().objnerf_box_rays(P, _ptr(T_WC), _ptr(T_OC), _ptr(half_extent), _ptr(dirs_C), _ptr(dirs_W), _ptr(near),
                                 _ptr(far), _ptr(hit), _stream()), "objnerf_box_rays")
    return dirs_W, near, far, hit.bool()


def box_points(origin: torch.Tensor, dirs_W: torch.Tensor, near: torch.Tensor, far: torch.Tensor,
               u: Optional[torch.Tensor] = None, n_bins: Optional[int] = None, seed: Optional[int] = None,
               draw: Optional[int] = None):
    """Mid-points of the stratified bins of [near, far] (trainer.py:171-176): u [n, n_bins] (injected draws; None:
    generated in the kernel under `seed` and a per-call counter, n_bins required) -> z_vals [n, n_bins-1],
    pts [n, n_bins-1, 3]."""
    dirs_W = _req(dirs_W, torch.float32, "dirs_W")
    near = _req(near, torch.float32, "near")
    far = _req(far, torch.float32, "far")
    dev = dirs_W.device
    if u is not None:
        u = _req(u, torch.float32, "u")
        n, n_bins = u.shape
    else:
        n, n_bins = near.shape[0], int(n_bins)
    origin = origin.to(dev, torch.float32).contiguous()
    z = torch.empty(n, n_bins - 1, device=dev)
    pts = torch.empty(n, n_bins - 1, 3, device=dev)
    check(lib().objnerf_box_points(n, n_bins, _ptr(origin), _ptr(dirs_W), _ptr(near), _ptr(far), _ptr(u), _seed_of(seed),
                                   0 if u is not None else (_next_offset() if draw is None else int(draw)) & 0x1FFFFFFF,
                                   _ptr(z), _ptr(pts), _stream()),
          "objnerf_box_points")
    return z, pts


def render_fwd(arena: ParamArena, origin: torch.Tensor, dirs_W: torch.Tensor, near: torch.Tensor, far: torch.Tensor,
               u: Optional[torch.Tensor] = None, n_bins: Optional[int] = None, seed: Optional[int] = None,
               draw: Optional[int] = None, want_hfeat: bool = True, want_z: bool = False, bf16: bool = False):
    """The per-object chain of sceneObject.render_2D_syn (vmap.py:644-676) in ONE launch (objnerf_render_fwd, hidden 32):
    mid-points of the stratified bins of [near, far] -> embedding -> network -> compositing, a lane per ray, nothing per
    sample in HBM.  arena: ONE object (K = 1).  u [n, n_bins]: injected draws; None: the Philox draws of box_points under
    (seed, draw).  bf16: opt-in OBJNERF_TRAIN_BF16 arithmetic (bf16 MFMA operands, hardware sin / cos / sigmoid; not the
    reference's fp32).  -> dict(depth [n], opacity [n], rgb [n,3], vals [n,H] | None (composited feature hidden), z | None)."""
    if arena.K != 1 or arena.net.hidden != 32:
        raise ObjnerfError("render_fwd: one hidden-32 object per call")
    dirs_W = _req(dirs_W, torch.float32, "dirs_W")
    near, far = _req(near, torch.float32, "near"), _req(far, torch.float32, "far")
    dev = dirs_W.device
    if u is not None:
        u = _req(u, torch.float32, "u")
        n, n_bins = u.shape
    else:
        n, n_bins = near.shape[0], int(n_bins)
    origin = origin.to(dev, torch.float32).contiguous()
    depth, opacity = torch.empty(n, device=dev), torch.empty(n, device=dev)
    rgb = torch.empty(n, 3, device=dev)
    hf = torch.empty(n, arena.net.hidden, device=dev) if want_hfeat else None
    z = torch.empty(n, n_bins - 1, device=dev) if want_z else None
    net = arena.net.c()
    check(lib().objnerf_render_fwd(C.byref(net), n, n_bins, _ptr(arena.params), _ptr(arena.scale), _ptr(origin), _ptr(dirs_W),
                                   _ptr(near), _ptr(far), _ptr(u), _seed_of(seed),
                                   0 if u is not None else (_next_offset() if draw is None else int(draw)) & 0x1FFFFFFF,
                                   _ptr(depth), _ptr(opacity), _ptr(rgb), _ptr(hf), _ptr(z), _lib.TRAIN_BF16 if bf16 else 0,
                                   _stream()),
          "objnerf_render_fwd")
    return {"depth": depth, "opacity": opacity, "rgb": rgb, "vals": hf, "z": z}


def mlp_forward(arena: ParamArena, emb: torch.Tensor, want_hfeat: bool = False, want_clip: bool = False):
    """emb [K,N,129] -> alpha [K,N], color [K,N,3], hfeat | None, clip | None (OccupancyMap.forward)."""
    emb = _req(emb, torch.float32, "emb")
    K, N = emb.shape[0], emb.shape[1]
    dev = emb.device
    alpha = torch.empty(K, N, device=dev)
    color = torch.empty(K, N, 3, device=dev)
    hfeat = torch.empty(K, N, arena.net.hidden, device=dev) if (want_hfeat or want_clip) else None
    clip = torch.empty(K, N, arena.net.feat_dim, device=dev) if want_clip else None
    net = arena.net.c()
    nbytes = int(lib().objnerf_eval_workspace_bytes(C.byref(net), K, N))      # 0 for hidden 32 (fused kernel)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
    check(lib().objnerf_mlp_forward_ws(C.byref(net), K, N, _ptr(arena.params), arena.p_stride, _ptr(emb), _ptr(alpha),
                                       _ptr(color), _ptr(hfeat), _ptr(clip), _ptr(ws), nbytes, _stream()),
          "objnerf_mlp_forward_ws")
    return alpha, color, hfeat, clip


def embed(arena: ParamArena, pts: torch.Tensor) -> torch.Tensor:
    pts = _req(pts, torch.float32, "pts")
    K, N = pts.shape[0], pts.shape[1]
    E = 3 + N_DIRS * arena.net.n_freqs
    out = torch.empty(K, N, E, device=pts.device)
    net = arena.net.c()
    check(lib().objnerf_embed(C.byref(net), K, N, _ptr(arena.params), arena.p_stride, _ptr(arena.scale),
                              _ptr(pts), _ptr(out), _stream()), "objnerf_embed")
    return out


def mlp_backward(arena: ParamArena, emb: torch.Tensor, d_alpha: torch.Tensor, d_color: torch.Tensor,
                 d_clip: Optional[torch.Tensor] = None):
    """Backward of OccupancyMap.forward (model.py:61-103) for the K stacked networks: -> (grads [K,p_stride] in arena
    layout -- tensors 0..13, 0..17 with d_clip, the rest zero --, d_emb [K,N,129])."""
    emb = _req(emb, torch.float32, "emb")
    K, N = emb.shape[0], emb.shape[1]
    d_alpha = _req(d_alpha.reshape(K, N), torch.float32, "d_alpha")
    d_color = _req(d_color.reshape(K, N, 3), torch.float32, "d_color")
    if d_clip is not None:
        d_clip = _req(d_clip.reshape(K, N, arena.net.feat_dim), torch.float32, "d_clip")
    dev = emb.device
    grads = torch.zeros(K, arena.p_stride, device=dev)
    d_emb = torch.empty_like(emb)
    net = arena.net.c()
    nbytes = int(lib().objnerf_mlp_backward_workspace_bytes(C.byref(net), K, N, 1 if d_clip is not None else 0))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    check(lib().objnerf_mlp_backward_ws(C.byref(net), K, N, _ptr(arena.params), arena.p_stride, _ptr(emb), _ptr(d_alpha),
                                        _ptr(d_color), _ptr(d_clip), _ptr(grads), _ptr(d_emb), _ptr(ws), nbytes, _stream()),
          "objnerf_mlp_backward_ws")
    return grads, d_emb


def embed_backward(arena: ParamArena, pts: torch.Tensor, d_emb: torch.Tensor) -> torch.Tensor:
    """Backward of UniDirsEmbed.forward (embedding.py:46-55) w.r.t. B_layer.weight: -> d B [K,21,3]."""
    pts = _req(pts, torch.float32, "pts")
    K, N = pts.shape[0], pts.shape[1]
    d_emb = _req(d_emb.reshape(K, N, -1), torch.float32, "d_emb")
    d_B = torch.empty(K, N_DIRS, 3, device=pts.device)
    scratch = torch.empty(K * 64, device=pts.device)
    net = arena.net.c()
    check(lib().objnerf_embed_bwd(C.byref(net), K, N, _ptr(arena.params), arena.p_stride, _ptr(arena.scale), _ptr(pts),
                                  _ptr(d_emb), _ptr(d_B), _ptr(scratch), _stream()), "objnerf_embed_bwd")
    return d_B


def occupancy(alpha: torch.Tensor) -> torch.Tensor:
    alpha = _req(alpha, torch.float32, "alpha")
    out = torch.empty_like(alpha)
    check(lib().objnerf_occupancy(alpha.numel(), _ptr(alpha), _ptr(out), _stream()), "objnerf_occupancy")
    return out


def composite(alpha: torch.Tensor, color: Optional[torch.Tensor], z: Optional[torch.Tensor],
              vals: Optional[torch.Tensor] = None, want_term: bool = False,
              input_is_occupancy: bool = False) -> Dict[str, torch.Tensor]:
    """alpha [n,S], color [n,S,3], z [n,S], vals [n,S,V] -> term/depth/var/rgb/opacity/vals."""
    alpha = _req(alpha, torch.float32, "alpha")
    if z is not None:
        z = _req(z, torch.float32, "z")
    n, S = alpha.shape
    dev = alpha.device
    if color is not None:
        color = _req(color, torch.float32, "color")
    V = 0
    out_vals = None
    if vals is not None:
        vals = _req(vals, torch.float32, "vals")
        V = vals.shape[-1]
        out_vals = torch.empty(n, V, device=dev)
    term = torch.empty(n, S, device=dev) if want_term else None
    depth = torch.empty(n, device=dev) if z is not None else None
    var = torch.empty(n, device=dev) if z is not None else None
    rgb = torch.empty(n, 3, device=dev) if color is not None else None
    opacity = torch.empty(n, device=dev)
    check(lib().objnerf_composite(n, S, int(input_is_occupancy), _ptr(alpha), _ptr(color), _ptr(z), _ptr(vals), V, _ptr(term), _ptr(depth),
                                  _ptr(var), _ptr(rgb), _ptr(opacity), _ptr(out_vals), _stream()),
          "objnerf_composite")
    return dict(term=term, depth=depth, var=var, rgb=rgb, opacity=opacity, vals=out_vals)


def feature_head(arena: ParamArena, hfeat: torch.Tensor, weight: Optional[torch.Tensor] = None) -> torch.Tensor:
    """hfeat [K,n,H] (+ weight [K,n]) -> [K,n,C] = out_clip(.) applied after compositing."""
    hfeat = _req(hfeat, torch.float32, "hfeat")
    K, n = hfeat.shape[0], hfeat.shape[1]
    if weight is not None:
        weight = _req(weight, torch.float32, "weight")
    out = torch.empty(K, n, arena.net.feat_dim, device=hfeat.device)
    net = arena.net.c()
    check(lib().objnerf_feature_head(C.byref(net), K, n, _ptr(arena.params), arena.p_stride, _ptr(hfeat),
                                     _ptr(weight), _ptr(out), _stream()), "objnerf_feature_head")
    return out


def label_counts(labels: torch.Tensor):
    labels = _req(labels, torch.uint8, "labels")
    K, R = labels.shape
    counts = torch.empty(K, 2, dtype=torch.int32, device=labels.device)
    flags = torch.empty(2, dtype=torch.int32, device=labels.device)
    check(lib().objnerf_label_counts(K, R, _ptr(labels), _ptr(counts), _ptr(flags), _stream()),
          "objnerf_label_counts")
    return counts, flags


def step_batch_loss(alpha, color, gt_depth, gt_rgb, labels, z, color_scaling=5.0, opacity_scaling=10.0,
                    gt_feat=None, pred_feat=None, feat_scaling=5.0, want_grads=True, flags_in=None, counts_in=None):
    """loss.step_batch_loss on materialised tensors.  Returns dict(total, terms [K,4], d_alpha, d_color,
    d_pred_feat, status)."""
    alpha = _req(alpha, torch.float32, "alpha")
    K, R, S = alpha.shape[0], alpha.shape[1], alpha.shape[2]
    color = _req(color, torch.float32, "color")
    z = _req(z, torch.float32, "z")
    gt_depth = _req(gt_depth, torch.float32, "gt_depth")
    gt_rgb = _req(gt_rgb, torch.float32, "gt_rgb")
    labels = _req(labels, torch.uint8, "labels")
    dev = alpha.device
    Cc = 0
    if gt_feat is not None:
        gt_feat = _req(gt_feat, torch.float32, "gt_feat")
        pred_feat = _req(pred_feat, torch.float32, "pred_feat")
        Cc = gt_feat.shape[-1]
    terms = torch.empty(K, 4, device=dev)
    total = torch.empty(1, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    counts = torch.empty(2 * K + 2, dtype=torch.int32, device=dev)
    d_alpha = torch.empty(K, R, S, device=dev) if want_grads else None
    d_color = torch.empty(K, R, S, 3, device=dev) if want_grads else None
    d_pf = torch.empty_like(pred_feat) if (want_grads and pred_feat is not None) else None
    a = LossArgs(K, R, S, Cc, color_scaling, opacity_scaling, feat_scaling, 0.0, _ptr(alpha), _ptr(color), _ptr(z),
                 _ptr(gt_depth), _ptr(gt_rgb), _ptr(labels), _ptr(pred_feat), _ptr(gt_feat), _ptr(flags_in), _ptr(counts_in),
                 _ptr(terms), _ptr(total), _ptr(d_alpha), _ptr(d_color), _ptr(d_pf), _ptr(counts), _ptr(status))
    check(lib().objnerf_step_batch_loss(C.byref(a), _stream()), "objnerf_step_batch_loss")
    return dict(total=total, terms=terms, d_alpha=d_alpha, d_color=d_color, d_pred_feat=d_pf, status=status,
                counts=counts)


STATUS_BITS = (1, 2)     # bit 0: a loss term above 1e5; bit 1: a term that is not finite (include/objnerf_hip.h)


def merge_status(*words: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The ONE way to merge status words: bitwise OR (they are bit fields -- a numeric maximum of 1 and 2 loses bit 0).
    words: int32 tensors of any length, every element a word (a workspace's per-chunk slots, the words of several loops).
    Returns int32[1] (`out` when given); stays on the words' device, no host synchronisation."""
    flat = words[0].reshape(-1) if len(words) == 1 else torch.cat([w.reshape(-1) for w in words])
    merged = None
    for bit in STATUS_BITS:          # (torch has no OR reduction: per bit, "any element has it")
        has = (flat & bit).amax(dim=0, keepdim=True)
        merged = has if merged is None else merged | has
    if out is None:
        return merged
    out.copy_(merged)
    return out


def status_of_terms(terms: torch.Tensor) -> torch.Tensor:
    """The status word of a set of loss terms by its definition: any term above 1e5 sets bit 0 (render_rays.py:109-111),
    any term that is not finite sets bit 1.  int32[1] on the terms' device, no host synchronisation."""
    t = terms.reshape(-1)
    if t.numel() == 0:
        return torch.zeros(1, dtype=torch.int32, device=t.device)
    explode = (t > 100000.0).any().to(torch.int32)
    nonfinite = (~torch.isfinite(t)).any().to(torch.int32)
    return (explode | (nonfinite << 1)).reshape(1)


# bytes; the layer-wise / hidden-256 paths materialise activations per object chunk (OBJNERF_WORKSPACE_BUDGET_GIB: override)
LAYERWISE_WORKSPACE_BUDGET = int(float(os.environ.get("OBJNERF_WORKSPACE_BUDGET_GIB", "64")) * (1 << 30))


def precision_bits(p) -> int:
    """The opt-in operand precision of a training step -> objnerf_train_args.mode bits.  False / None / "fp32": the
    reference's arithmetic; True / "bf16": OBJNERF_TRAIN_BF16; "fp16": OBJNERF_TRAIN_FP16 (layer-wise path)."""
    if p in (False, None, "fp32"):
        return 0
    if p in (True, "bf16"):
        return 1
    if p == "fp16":
        return 4
    raise ValueError("precision must be fp32 / bf16 / fp16, not {!r}".format(p))


class StreamContext:
    """objnerf_context: the helper stream + events the layer-wise path forks onto.  Created on the current device;
    freed with the object (after a device synchronisation, so no step using it is in flight)."""

    def __init__(self, device):
        self.device = torch.device(device)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(lib().objnerf_context_create(C.byref(h)), "objnerf_context_create")
        self.handle = h

    def __del__(self):
        h, self.handle = getattr(self, "handle", None), None
        if h:
            try:
                torch.cuda.synchronize(self.device)
                lib().objnerf_context_destroy(h)
            except Exception:      # interpreter shutdown
                pass


class TrainWorkspace:
    """Caller-owned buffers of the fused training step, allocated once per (K,R,S).

    The layer-wise path (hidden != 32, S > 64 or layerwise=True) keeps every activation of the objects it works on
    in the workspace; when K objects would need more than `budget` bytes (BASELINE configs[4]: 64 objects x 8192
    rays x 128 samples x hidden 256 is ~0.7 TB), the workspace is sized for `k_chunk` objects and train_step runs
    the objects chunk by chunk -- they are independent networks, only the early-return flags span the batch."""

    def __init__(self, arena: ParamArena, K: int, R: int, S: int, with_feat: bool, layerwise: bool = False,
                 budget: Optional[int] = None, precision=None, context: Optional["StreamContext"] = None):
        """context: a StreamContext to share (the K one-object workspaces of the forloop strategy run one after the other
        on one stream, so one set of helper streams serves them all); None = this workspace owns one when its path uses it."""
        layerwise = layerwise or precision_bits(precision) == 4          # the fp16 mode lives on the layer-wise path
        dev = arena.params.device
        net = arena.net.c()
        wf = int(with_feat) | (2 if layerwise else 0) | (4 if precision_bits(precision) in (1, 4) else 0)   # bit 2: 16-bit modes only
        budget = LAYERWISE_WORKSPACE_BUDGET if budget is None else budget
        self.k_chunk = K
        nbytes = lib().objnerf_train_workspace_bytes(C.byref(net), K, R, S, wf)
        if (arena.net.hidden != 32 or S > 64 or layerwise) and nbytes > budget and K > 1:
            per_obj = lib().objnerf_train_workspace_bytes(C.byref(net), 1, R, S, wf)
            self.k_chunk = max(1, min(K, int(budget // max(1, per_obj))))
            # (measured, round 6: EQUAL chunks -- 8 x 8 objects instead of 7 x 9 + 1 for configs[4]'s 64 -- are slower, 191.6
            # against 187.4 ms per step: the fused hidden-256 kernels gain more from a ninth object per launch than the
            # one-object tail costs)
            nbytes = lib().objnerf_train_workspace_bytes(C.byref(net), self.k_chunk, R, S, wf)
        if nbytes == 0:
            raise _lib.ObjnerfError("objnerf_train_workspace_bytes returned 0")
        self.nbytes = int(nbytes)
        # the layer-wise path runs independent GEMMs side by side on the context's streams
        uses_context = (arena.net.hidden != 32 or S > 64 or layerwise) and dev.type == "cuda"
        self.context = (context if context is not None else StreamContext(dev)) if uses_context else None
        self.buf = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
        # Chunked hidden-256 steps in a 16-bit mode (configs[4]: the two fused kernels of objnerf_train256.hip) run their
        # chunks ALTERNATELY on two streams, each with its own buffer: a chunk's HBM-bound weight-gradient kernel then fills the
        # CUs that the next chunk's kernel A leaves idle at its tail (both hold ~150 KB of LDS per workgroup, so they never
        # share a CU; tools/c5_overlap.py: 3 - 5 % of the step).  Only where a second buffer fits beside the first.
        self.lanes = 1
        self.buf2 = None
        if (self.k_chunk < K and dev.type == "cuda" and arena.net.hidden == 256 and precision_bits(precision) in (1, 4)
                and not (layerwise and precision_bits(precision) != 4) and S in (32, 64, 128)
                and os.environ.get("OBJNERF_ONE_LANE", "0") != "1"):
            # k_chunk was sized for ONE buffer of up to `budget` bytes: the second one is taken only where it leaves a quarter
            # of the device (and at least 16 GiB) free for what comes after this workspace -- sample pools, render buffers,
            # keyframe stores -- instead of "8 GiB above the buffer" (round 5: ~128 GiB of workspace with 8 GiB of slack)
            free, total = torch.cuda.mem_get_info(dev)
            if free - self.nbytes > max(total // 4, 16 << 30):
                self.buf2 = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
                # TWO side streams created back to back (the caller's stream only hands over and collects): streams are dealt
                # to a few hardware queues round-robin in creation order, and two streams that share a queue run their kernels
                # back to back -- a single side stream overlapped with the caller's stream in a fresh process and not in one
                # that had created a dozen streams before; a high-priority side stream the other way round (tools/lanes_ab.sh)
                with torch.cuda.device(dev):        # (events belong to the device current at their creation)
                    self.sides = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
                    self.ev_in, self.ev_out = torch.cuda.Event(), [torch.cuda.Event(), torch.cuda.Event()]
                self.lanes = 2
        self.grads = torch.zeros_like(arena.params)
        self.loss_terms = torch.zeros(K, 4, device=dev)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.status_chunks = torch.zeros((K + self.k_chunk - 1) // self.k_chunk, dtype=torch.int32, device=dev)
        self.counts = torch.zeros(K, 2, dtype=torch.int32, device=dev)
        self.flags = torch.zeros(2, dtype=torch.int32, device=dev)
        # (the workspace size depends on the operand precision: a loop whose precision is toggled must re-allocate)
        self.key = self.make_key(K, R, S, with_feat, precision)

    @staticmethod
    def make_key(K, R, S, with_feat, precision=None):
        return (K, R, S, bool(with_feat), precision_bits(precision))


def train_step(arena: ParamArena, ws: TrainWorkspace, batch: Dict[str, torch.Tensor], color_scaling=5.0,
               opacity_scaling=10.0, feat_scaling=5.0, with_feat=False, obj_center=0.0,
               global_flags: Optional[torch.Tensor] = None, global_counts: Optional[torch.Tensor] = None,
               bf16: bool = False, layerwise: bool = False, relu_masks: Optional[torch.Tensor] = None,
               emb_debug: Optional[torch.Tensor] = None, optim=None) -> None:
    """One fused iteration (train.py:424-472): fills ws.grads, ws.loss_terms, ws.status.

    optim: an optim.ArenaAdamW over `arena` -- the iteration's optimiser.step() (train.py:472-473) runs INSIDE the call
    (objnerf_train_args.optim: the launch that reduces the partial gradients applies AdamW to each element it has just
    summed, with the iteration's early-return flags deciding which tensor groups are stepped); ws.grads is still
    written.  None: gradients only.

    Without global_flags AND global_counts the step derives the label statistics itself (OBJNERF_TRAIN_SELF_COUNTS;
    ws.counts / ws.flags receive them) -- no separate objnerf_label_counts call.

    layerwise: OBJNERF_TRAIN_LAYERWISE -- run the layer-wise (any width) implementation even where the fused
    kernel applies (cross-check of two independent implementations; ws must be built with layerwise=True).

    bf16: operand precision (precision_bits): True / "bf16" = OBJNERF_TRAIN_BF16 (bf16 MFMA operands, fp32 accumulate /
    master weights), "fp16" = OBJNERF_TRAIN_FP16 (layer-wise path; ws built with precision="fp16"); the default is
    the reference's fp32 arithmetic.

    relu_masks: test hook -- uint8 [K,R,S,6,hidden/8] receiving the ReLU branch bits of the iteration
    (objnerf_train_args.relu_masks); None in production.
    emb_debug: test hook -- float32 [K,R,S,129] receiving the embedding rows the fused fp32 kernel formed in registers
    (objnerf_train_args.emb_debug; hidden 32, S <= 64, fp32 only); None in production.

    batch: pts [K,R,S,3] (or origins+dirs), z, gt_depth, gt_rgb, labels u8 (+ gt_feat when with_feat).
    global_flags: optional [2] int32 tensor already max-reduced over all ranks (object sharding)."""
    z = _req(batch["z"], torch.float32, "z")
    K, R, S = z.shape
    labels = _req(batch["labels"], torch.uint8, "labels")
    pts = batch.get("pts")
    pts = _req(pts, torch.float32, "pts") if pts is not None else None
    origins = _req(batch["origins"], torch.float32, "origins") if pts is None else None
    dirs = _req(batch["dirs"], torch.float32, "dirs") if pts is None else None
    gt_depth = _req(batch["gt_depth"], torch.float32, "gt_depth")
    gt_rgb = _req(batch["gt_rgb"], torch.float32, "gt_rgb")
    gt_feat = _req(batch["gt_feat"], torch.float32, "gt_feat") if with_feat else None
    st = _stream()
    self_counts = global_flags is None and global_counts is None
    if not self_counts and (global_flags is None or global_counts is None):
        check(lib().objnerf_label_counts(K, R, _ptr(labels), _ptr(ws.counts), _ptr(ws.flags), st),
              "objnerf_label_counts")
    flags = ws.flags
    if global_flags is not None:
        flags = _req(global_flags, torch.int32, "global_flags")
    counts = ws.counts
    if global_counts is not None:       # one object's rays split over ranks (background): global mask counts
        counts = _req(global_counts, torch.int32, "global_counts")
    net = arena.net.c()
    mode = precision_bits(bf16) | (2 if layerwise else 0)
    if relu_masks is not None:
        relu_masks = _req(relu_masks, torch.uint8, "relu_masks")
        if tuple(relu_masks.shape) != (K, R, S, 6, arena.net.hidden // 8):
            raise ObjnerfError("relu_masks must be uint8 [K,R,S,6,hidden/8]")
    if emb_debug is not None:
        emb_debug = _req(emb_debug, torch.float32, "emb_debug")
        if tuple(emb_debug.shape) != (K, R, S, EMB1 + EMB2):
            raise ObjnerfError("emb_debug must be float32 [K,R,S,129]")
    kc = getattr(ws, "k_chunk", K)
    ctx = ws.context.handle if getattr(ws, "context", None) is not None else None
    if kc >= K:
        oa = None
        if optim is not None:
            if optim.arena is not arena:
                raise ObjnerfError("train_step: optim must be the optimiser of `arena`")
            oa = AdamWArgs(_ptr(optim.exp_avg), _ptr(optim.exp_avg_sq), _ptr(optim._banks), int(optim._bank), 0,
                           optim.lr, optim.betas[0], optim.betas[1], optim.eps, optim.weight_decay, 0.0)
        a = TrainArgs(K, R, S, mode | (TRAIN_SELF_COUNTS if self_counts else 0), color_scaling, opacity_scaling,
                      feat_scaling, obj_center, _ptr(arena.params),
                      arena.p_stride, _ptr(arena.scale), _ptr(pts), _ptr(origins), _ptr(dirs), _ptr(z), _ptr(gt_depth),
                      _ptr(gt_rgb), _ptr(labels), _ptr(gt_feat), _ptr(counts), _ptr(flags), _ptr(ws.grads),
                      _ptr(ws.loss_terms), _ptr(ws.status), _ptr(ws.buf), ws.nbytes, _ptr(relu_masks), ctx, _ptr(emb_debug),
                      C.addressof(oa) if oa is not None else None)
        check(lib().objnerf_train_step(C.byref(net), C.byref(a), st), "objnerf_train_step")
        if optim is not None:
            optim._bank ^= 1
            arena.version += 1          # (the call wrote the arena through raw pointers: torch's counter misses it)
        return
    if self_counts:                     # (the flags span the whole batch, not a chunk of it)
        check(lib().objnerf_label_counts(K, R, _ptr(labels), _ptr(ws.counts), _ptr(ws.flags), st),
              "objnerf_label_counts")
    # layer-wise path, chunk of objects at a time (leading-dimension slices are contiguous views)
    sl = lambda t, k0, k1: None if t is None else t[k0:k1]           # noqa: E731
    two = getattr(ws, "lanes", 1) == 2 and relu_masks is None and emb_debug is None
    if two:                             # (even / odd chunks on the two side streams, each with its buffer, behind this stream)
        main = torch.cuda.current_stream(z.device)
        ws.ev_in.record(main)
        for sd in ws.sides:
            sd.wait_event(ws.ev_in)
    for ci, k0 in enumerate(range(0, K, kc)):
        k1 = min(K, k0 + kc)
        buf = ws.buf2 if (two and (ci & 1)) else ws.buf
        sth = ws.sides[ci & 1].cuda_stream if two else st
        a = TrainArgs(k1 - k0, R, S, mode, color_scaling, opacity_scaling, feat_scaling, obj_center,
                      _ptr(arena.params[k0:k1]), arena.p_stride, _ptr(arena.scale[k0:k1]), _ptr(sl(pts, k0, k1)),
                      _ptr(sl(origins, k0, k1)), _ptr(sl(dirs, k0, k1)), _ptr(z[k0:k1]), _ptr(gt_depth[k0:k1]),
                      _ptr(gt_rgb[k0:k1]), _ptr(labels[k0:k1]), _ptr(sl(gt_feat, k0, k1)), _ptr(counts[k0:k1]),
                      _ptr(flags), _ptr(ws.grads[k0:k1]), _ptr(ws.loss_terms[k0:k1]), _ptr(ws.status_chunks[ci:ci + 1]),
                      _ptr(buf), ws.nbytes, _ptr(sl(relu_masks, k0, k1)), ctx, _ptr(sl(emb_debug, k0, k1)), None)
        check(lib().objnerf_train_step(C.byref(net), C.byref(a), sth), "objnerf_train_step")
    if two:
        for sd, ev in zip(ws.sides, ws.ev_out):
            ev.record(sd)
            main.wait_event(ev)
    merge_status(ws.status_chunks, out=ws.status)
    if optim is not None:              # (chunked: one optimiser launch over the whole arena after the last chunk)
        optim.step(ws.grads, arena.has_grad_mask(with_feat), flags=flags)


def adamw_step(arena: ParamArena, grads: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor,
               has_grad: Optional[torch.Tensor], step: int, lr: float, weight_decay: float, beta1=0.9, beta2=0.999,
               eps=1e-8, params: Optional[torch.Tensor] = None) -> None:
    p = arena.params if params is None else params
    if params is None:
        arena.version += 1              # (raw-pointer write: torch's version counter misses it; autograd.py checks this one)
    check(lib().objnerf_adamw_step(arena.K, arena.P, arena.p_stride, _ptr(p), _ptr(grads), _ptr(exp_avg),
                                   _ptr(exp_avg_sq), _ptr(has_grad), step, lr, beta1, beta2, eps, weight_decay,
                                   _stream()), "objnerf_adamw_step")


def adamw_step_flags(arena: ParamArena, grads: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor,
                     has_grad: Optional[torch.Tensor], flags: torch.Tensor, group_steps: torch.Tensor, bank: int,
                     lr: float, weight_decay: float, beta1=0.9, beta2=0.999, eps=1e-8,
                     params: Optional[torch.Tensor] = None) -> None:
    """AdamW with the iteration's early-return flags deciding on the device which tensor groups received a gradient
    (objnerf_adamw_step_flags); group_steps: int32[2, 3] device counters owned by the caller, `bank` the bank to read
    (the other one receives the advanced counters: alternate it from call to call)."""
    p = arena.params if params is None else params
    if params is None:
        arena.version += 1
    flags = _req(flags, torch.int32, "flags")
    group_steps = _req(group_steps, torch.int32, "group_steps")
    if group_steps.numel() != 6 or bank not in (0, 1):
        raise ObjnerfError("adamw_step_flags: group_steps must be int32[2, 3], bank 0 or 1")
    o = arena.offsets
    check(lib().objnerf_adamw_step_flags(arena.K, arena.P, arena.p_stride, _ptr(p), _ptr(grads), _ptr(exp_avg),
                                         _ptr(exp_avg_sq), _ptr(has_grad), _ptr(flags), _ptr(group_steps), int(bank),
                                         int(o[10]), int(o[14]), int(o[18]), lr, beta1, beta2, eps, weight_decay, _stream()),
          "objnerf_adamw_step_flags")


def ingest_frame(rgb, depth, inst, t_wc, items) -> None:
    """One frame into a keyframe slot of every visible object, one launch (train.py:196-256).
    rgb u8 [W,H,3], depth f32 [W,H], inst int32 [W,H], t_wc f32 [4,4] on the device;
    items = [(store tensors (rgbs_batch, depth_batch, t_wc_batch, bbox), slot, obj_id, box[4])]."""
    import numpy as np
    from ._lib import IngestItem
    rgb = _req(rgb, torch.uint8, "rgb")
    depth = _req(depth, torch.float32, "depth")
    inst = _req(inst, torch.int32, "inst")
    t_wc = _req(t_wc, torch.float32, "t_wc")
    W, H = depth.shape
    arr = (IngestItem * len(items))()
    for i, ((rgbs_b, depth_b, twc_b, bbox_b), slot, obj_id, box) in enumerate(items):
        if rgbs_b.shape[1:] != (W, H, 4) or depth_b.shape[1:] != (W, H) or not 0 <= slot < rgbs_b.shape[0]:
            raise ObjnerfError("ingest_frame: store / frame shapes do not match")
        arr[i] = IngestItem(rgbs_b.data_ptr(), depth_b.data_ptr(), twc_b.data_ptr(), bbox_b.data_ptr(), int(slot),
                            int(obj_id), (C.c_float * 4)(*[float(v) for v in box]))
    host = torch.from_numpy(np.frombuffer(arr, dtype=np.uint8).copy())
    dev_items = host.to(rgb.device)
    check(lib().objnerf_ingest_frame(W, H, _ptr(rgb), _ptr(depth), _ptr(inst), _ptr(t_wc), len(items), _ptr(dev_items),
                                     _stream()), "objnerf_ingest_frame")


def ingest_frame_crops(rgb, depth, inst, t_wc, items, outside) -> None:
    """ingest_frame for cropped stores (objnerf_ingest_frame_crops): items = [(kf_store.KeyframeCropStore, slot,
    obj_id, box[4])]; every store gets room for the box's crop first (it may grow: its arena then moves).  outside:
    device int32 [>= len(items)], entry k receives += the number of "this object" pixels of item k outside its crop."""
    import numpy as np
    from ._lib import IngestCropItem, KfCrops
    from .kf_store import crop_rect
    rgb = _req(rgb, torch.uint8, "rgb")
    depth = _req(depth, torch.float32, "depth")
    inst = _req(inst, torch.int32, "inst")
    t_wc = _req(t_wc, torch.float32, "t_wc")
    outside = _req(outside, torch.int32, "outside")
    W, H = depth.shape
    if outside.numel() < len(items):
        raise ObjnerfError("ingest_frame_crops: one `outside` counter per item expected")
    if len({(id(st), int(slot)) for st, slot, _, _ in items}) != len(items):
        raise ObjnerfError("ingest_frame_crops: a slot is written twice")
    for st, slot, _, box in items:                             # every item is checked before any store is touched
        if (st.W, st.H) != (W, H) or not 0 <= slot < st.F or len(box) != 4:
            raise ObjnerfError("ingest_frame_crops: store / frame shapes do not match")
    rects = [crop_rect(box, W, H) for _, _, _, box in items]
    for (st, slot, _, _), rect in zip(items, rects):
        st.reserve(int(slot), rect)
    arr = (IngestCropItem * len(items))()
    for i, (st, slot, obj_id, box) in enumerate(items):        # (after every reserve: a store may be listed twice)
        _req(st.arena, torch.uint8, "arena"); _req(st.rect, torch.int32, "rect")
        _req(st.t_wc, torch.float32, "t_wc_batch"); _req(st.bbox, torch.float32, "bbox")
        if rects[i][2] * rects[i][3] > st.cap or st.arena.numel() != st.F * st.cap * 8:
            raise ObjnerfError("ingest_frame_crops: the crop does not fit its store")
        arr[i] = IngestCropItem(KfCrops(*st.descriptor()), int(slot), int(obj_id),
                                (C.c_float * 4)(*[float(v) for v in box]), (C.c_int32 * 4)(*rects[i]))
    dev_items = torch.from_numpy(np.frombuffer(arr, dtype=np.uint8).copy()).to(rgb.device)
    check(lib().objnerf_ingest_frame_crops(W, H, _ptr(rgb), _ptr(depth), _ptr(inst), _ptr(t_wc), len(items),
                                           _ptr(dev_items), _ptr(outside), _stream()), "objnerf_ingest_frame_crops")


def keyframe_table(stores) -> torch.Tensor:
    """Device descriptor table of objnerf_sample_rays_stacked: stores = [(rgbs_batch, depth_batch, t_wc_batch, bbox)]
    per object (the tensors must stay alive and in place while the table is used).  int64 [K, 4] of device pointers.
    stores = [kf_store.KeyframeCropStore]: the table of objnerf_sample_rays_crops, int64 [K, 5] (objnerf_kf_crops:
    arena, cap, rect, t_wc, bbox), valid until a store grows (its `version`).  The samplers and object_bounds tell the
    two apart by the row length."""
    from .kf_store import KeyframeCropStore
    if isinstance(stores[0], KeyframeCropStore):
        for st in stores:
            if not isinstance(st, KeyframeCropStore):
                raise ObjnerfError("keyframe_table: dense and cropped stores in one table")
            _req(st.rect, torch.int32, "rect"); _req(st.t_wc, torch.float32, "t_wc_batch")
            _req(st.bbox, torch.float32, "bbox")
            if st.cap <= 0 or st.arena.numel() != st.F * st.cap * 8:
                raise ObjnerfError("keyframe_table: a cropped store without keyframes")
            _req(st.arena, torch.uint8, "arena")
        return torch.tensor([list(st.descriptor()) for st in stores], dtype=torch.int64).to(stores[0].arena.device)
    rows = []
    for rgbs, depth, t_wc, bbox in stores:
        _req(rgbs, torch.uint8, "rgbs_batch"); _req(depth, torch.float32, "depth_batch")
        _req(t_wc, torch.float32, "t_wc_batch"); _req(bbox, torch.float32, "bbox")
        rows.append([rgbs.data_ptr(), depth.data_ptr(), t_wc.data_ptr(), bbox.data_ptr()])
    return torch.tensor(rows, dtype=torch.int64).to(stores[0][0].device)


def _sample_common(K, n_frames, n_px, n_cam2surf, n_bins, dev, want_pts, record, stacked):
    n, S = n_frames * n_px, n_cam2surf + n_bins
    lead = (K,) if stacked else ()
    o = {"rgb": torch.empty(*lead, n, 3, dtype=torch.uint8, device=dev), "depth": torch.empty(*lead, n, device=dev),
         "valid": torch.empty(*lead, n, dtype=torch.uint8, device=dev),
         "labels": torch.empty(*lead, n, dtype=torch.uint8, device=dev), "z": torch.empty(*lead, n, S, device=dev),
         "pts": torch.empty(*lead, n, S, 3, device=dev) if want_pts else None,
         "origins": None if want_pts else torch.empty(*lead, n, 3, device=dev),
         "dirs": None if want_pts else torch.empty(*lead, n, 3, device=dev),
         "kf": torch.empty(*lead, n_frames, dtype=torch.int64, device=dev) if record else None,
         "px": torch.empty(*lead, n, 2, dtype=torch.int32, device=dev) if record else None,
         "ws": torch.empty(*lead, 1 + 6 * n, device=dev)}
    return o


def _partfeat_fields(a: SampleArgs, partfeat, K, F, n, dev, stacked):
    """ABI 6 fields of the part-feature gather (vmap.py:437-452).  partfeat = (global_partfeat [Fn, Wp, Hp, C] fp32,
    use_frame [F] | [K, F] (dataset frame id of every keyframe slot), stride, part_down) or None.  Returns the output
    tensor ([n, C] | [K, n, C]) the launch fills; the frame range is checked here (the reference would raise an
    IndexError from its advanced indexing, the kernel clamps).
    ABI 12: a part_maps.PartStore in place of the dense tensor gathers through its index image (index int32
    [Fn, Wp, Hp] of global row numbers, table fp32 [rows, C] with row 0 zero); the dense map never exists."""
    if partfeat is None:
        return None
    from .part_maps import PartStore               # (part_maps imports this module)
    gpf, use_frame, stride, part_down = partfeat
    index = None
    if isinstance(gpf, PartStore):
        if gpf.index is None or gpf.table is None:
            raise IndexError("use_frame / stride outside the part store (it holds no frame)")
        index = _req(gpf.index, torch.int32, "part_index")
        gpf = _req(gpf.table, torch.float32, "part_table")
        if index.dim() != 3 or gpf.dim() != 2 or gpf.shape[0] < 1 or gpf.shape[1] < 1 or index.device != gpf.device:
            raise ObjnerfError("part store: index [frames, W / part_down, H / part_down] and table [rows, C] expected")
        shape = tuple(index.shape) + (gpf.shape[1],)
    else:
        gpf = _req(gpf, torch.float32, "global_partfeat")
        if gpf.dim() != 4:
            raise ObjnerfError("global_partfeat must be [frames, W / part_down, H / part_down, C]")
        shape = tuple(gpf.shape)
    uf = torch.as_tensor(np.asarray(use_frame.cpu() if torch.is_tensor(use_frame) else use_frame))   # host bookkeeping
    if int(stride) != stride or int(stride) <= 0 or bool((uf != uf.round()).any()):
        raise ObjnerfError("part features: integer frame ids and stride expected")
    if uf.numel() != K * F:
        raise ObjnerfError("use_frame must hold one frame id per keyframe slot")
    if int(uf.min()) < 0 or int(uf.max()) // int(stride) >= shape[0]:
        raise IndexError("use_frame / stride outside global_partfeat")
    uf = uf.to(torch.int32).contiguous().to(dev)
    out = torch.empty(*((K,) if stacked else ()), n, shape[3], device=dev)
    a.global_partfeat, a.use_frame, a.out_partfeat = _ptr(gpf), _ptr(uf), _ptr(out)
    a.pf_frames, a.pf_w, a.pf_h, a.pf_c = shape
    a.pf_stride, a.part_down = int(stride), float(part_down)
    if index is not None:
        a.part_index, a.pf_rows = _ptr(index), int(gpf.shape[0])
    a._keep = (gpf, uf, index)
    return out


def part_index(masks: torch.Tensor) -> torch.Tensor:
    """objnerf_part_index: masks [M, Hp, Wp] uint8 on the device (already taken on the stride) -> int32 [Hp, Wp], the
    number of the last mask that covers each pixel, -1 where none does (sam_clip_dir.py:118-125).  M may be 0."""
    masks = _req(masks, torch.uint8, "masks")
    if masks.dim() != 3 or masks.shape[1] < 1 or masks.shape[2] < 1:
        raise ObjnerfError("part_index: masks must be [M, Hp, Wp]")
    M, Hp, Wp = masks.shape
    out = torch.empty(Hp, Wp, dtype=torch.int32, device=masks.device)
    check(lib().objnerf_part_index(M, Hp, Wp, _ptr(masks) if M else None, _ptr(out), _stream()), "objnerf_part_index")
    return out


def part_dense(index: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    """objnerf_part_dense: index int32 [...] (0 = the zero row), table fp32 [rows, C] -> fp32 [..., C] = table[index]
    (values outside the table are clamped into it)."""
    index = _req(index, torch.int32, "index")
    table = _req(table, torch.float32, "table")
    if table.dim() != 2 or table.shape[0] < 1 or table.shape[1] < 1 or index.numel() < 1 or index.device != table.device:
        raise ObjnerfError("part_dense: index [...] and table [rows, C] on one device expected")
    out = torch.empty(*index.shape, table.shape[1], device=table.device)
    check(lib().objnerf_part_dense(index.numel(), table.shape[1], table.shape[0], _ptr(index), _ptr(table), _ptr(out),
                                   _stream()), "objnerf_part_dense")
    return out


# ------------------------------------------------------------------------------- the mask front end (objnerf_maskprep.hip)
CC_ROW = 8          # ints per row of the component / final-id tables: first pixel, id, area, x0, y0, x1, y1, frame
CC_MAX_SIDE = 32767
CLIP_SIDE = 224


def _id_images(ids: torch.Tensor, what: str) -> Tuple[int, int, int]:
    if ids.dim() != 3 or not 1 <= ids.shape[0] <= 65535 or not (1 <= ids.shape[1] <= CC_MAX_SIDE and
                                                                1 <= ids.shape[2] <= CC_MAX_SIDE):
        raise ObjnerfError(f"{what}: [F, H, W] with F <= 65535 and H, W <= {CC_MAX_SIDE} expected")
    return int(ids.shape[0]), int(ids.shape[1]), int(ids.shape[2])


def cc_label(ids: torch.Tensor) -> torch.Tensor:
    """objnerf_cc_label: ids int32 [F, H, W] -> int32 [F, H, W], per pixel the flat index (in its frame) of the first pixel
    of its 8-connected component of equal non-zero id, -1 where the id is 0."""
    ids = _req(ids, torch.int32, "ids")
    F, H, W = _id_images(ids, "cc_label")
    label = torch.empty_like(ids)
    check(lib().objnerf_cc_label(F, H, W, _ptr(ids), _ptr(label), _stream()), "objnerf_cc_label")
    return label


def cc_table(ids: torch.Tensor, label: torch.Tensor, cap: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """objnerf_cc_table -> (packed int64 [F + 1 + 4 * cap]: comp_off [F + 1], then the table's [cap, 8] int32 rows, so
    that one copy brings both to the host; slot int32 [F, H, W])."""
    ids, label = _req(ids, torch.int32, "ids"), _req(label, torch.int32, "label")
    F, H, W = _id_images(ids, "cc_table")
    if label.shape != ids.shape or label.device != ids.device or cap < 1:
        raise ObjnerfError("cc_table: label must match ids; cap >= 1")
    dev = ids.device
    nbytes = int(lib().objnerf_cc_table_workspace_bytes(F, H, W))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    packed = torch.zeros(F + 1 + (CC_ROW // 2) * cap, dtype=torch.int64, device=dev)
    slot = torch.empty_like(ids)
    check(lib().objnerf_cc_table(F, H, W, _ptr(ids), _ptr(label), _ptr(ws), nbytes, int(cap), _ptr(packed),
                                 packed.data_ptr() + 8 * (F + 1), _ptr(slot), _stream()), "objnerf_cc_table")
    return packed, slot


def cc_boundary(label: torch.Tensor, slot: torch.Tensor, sel: torch.Tensor, S: int, bcap: int):
    """objnerf_cc_boundary: sel int32 [rows] (component row -> list in [0, S) or -1) -> (boff int32 [S + 1], bpix int32
    [bcap] holding (y << 16) | x; unordered inside a list)."""
    label, slot, sel = _req(label, torch.int32, "label"), _req(slot, torch.int32, "slot"), _req(sel, torch.int32, "sel")
    F, H, W = _id_images(label, "cc_boundary")
    if slot.shape != label.shape or sel.dim() != 1 or sel.numel() < 1 or S < 1 or bcap < 1:
        raise ObjnerfError("cc_boundary: slot must match label; sel [rows], S >= 1, bcap >= 1")
    dev = label.device
    boff = torch.empty(S + 1, dtype=torch.int32, device=dev)
    cursor = torch.empty(S, dtype=torch.int32, device=dev)
    bpix = torch.empty(int(bcap), dtype=torch.int32, device=dev)
    check(lib().objnerf_cc_boundary(F, H, W, _ptr(label), _ptr(slot), _ptr(sel), sel.numel(), int(S), _ptr(boff),
                                    _ptr(cursor), _ptr(bpix), int(bcap), _stream()), "objnerf_cc_boundary")
    return boff, bpix


def cc_gaps(pairs: torch.Tensor, boff: torch.Tensor, bpix: torch.Tensor) -> torch.Tensor:
    """objnerf_cc_gaps: pairs int32 [P, 2] of boundary lists -> int32 [P], the exact minimum squared distance."""
    pairs, boff, bpix = _req(pairs, torch.int32, "pairs"), _req(boff, torch.int32, "boff"), _req(bpix, torch.int32, "bpix")
    if pairs.dim() != 2 or pairs.shape[1] != 2 or pairs.shape[0] < 1 or boff.numel() < 2:
        raise ObjnerfError("cc_gaps: pairs [P, 2] with P >= 1 expected")
    d2 = torch.empty(pairs.shape[0], dtype=torch.int32, device=pairs.device)
    check(lib().objnerf_cc_gaps(pairs.shape[0], _ptr(pairs), boff.numel() - 1, _ptr(boff), _ptr(bpix), bpix.numel(),
                                _ptr(d2), _stream()), "objnerf_cc_gaps")
    return d2


def cc_relabel(label: torch.Tensor, slot: torch.Tensor, final_id: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """objnerf_cc_relabel: final_id int32 [rows] per component -> (ids int32 [F, H, W], stats int32 [F, 256, 8])."""
    label, slot = _req(label, torch.int32, "label"), _req(slot, torch.int32, "slot")
    final_id = _req(final_id, torch.int32, "final_id")
    F, H, W = _id_images(label, "cc_relabel")
    if slot.shape != label.shape or final_id.dim() != 1 or final_id.numel() < 1:
        raise ObjnerfError("cc_relabel: slot must match label; final_id [rows]")
    out = torch.empty_like(label)
    stats = torch.empty(F, 256, CC_ROW, dtype=torch.int32, device=label.device)
    check(lib().objnerf_cc_relabel(F, H, W, _ptr(label), _ptr(slot), _ptr(final_id), final_id.numel(), _ptr(out),
                                   _ptr(stats), _stream()), "objnerf_cc_relabel")
    return out, stats


def clip_crops(image: torch.Tensor, desc: torch.Tensor, hb: torch.Tensor, hk: torch.Tensor, vb: torch.Tensor,
               vk: torch.Tensor, tmp_rows: int) -> torch.Tensor:
    """objnerf_clip_crops: image uint8 [H, W, 3]; desc int32 [n, 8]; hb / vb int32 [n, 224, 2]; hk / vk int32
    [n, 224, k] (include/objnerf_hip.h) -> fp32 [n, 3, 224, 224]."""
    image = _req(image, torch.uint8, "image")
    desc, hb, hk, vb, vk = (_req(t, torch.int32, nm) for t, nm in ((desc, "desc"), (hb, "hb"), (hk, "hk"), (vb, "vb"),
                                                                    (vk, "vk")))
    n = int(desc.shape[0])
    if image.dim() != 3 or image.shape[2] != 3 or desc.shape != (n, 8) or n < 1 or hb.shape != (n, CLIP_SIDE, 2) or \
            vb.shape != (n, CLIP_SIDE, 2) or hk.shape[:2] != (n, CLIP_SIDE) or vk.shape[:2] != (n, CLIP_SIDE) or \
            hk.dim() != 3 or vk.dim() != 3 or tmp_rows < 1:
        raise ObjnerfError("clip_crops: image [H, W, 3], desc [n, 8], bounds [n, 224, 2], coefficients [n, 224, k]")
    dev = image.device
    tmp = torch.empty(n, int(tmp_rows), CLIP_SIDE, 3, dtype=torch.uint8, device=dev)
    out = torch.empty(n, 3, CLIP_SIDE, CLIP_SIDE, dtype=torch.float32, device=dev)
    check(lib().objnerf_clip_crops(n, image.shape[0], image.shape[1], _ptr(image), _ptr(desc), hk.shape[2], _ptr(hb),
                                   _ptr(hk), vk.shape[2], _ptr(vb), _ptr(vk), int(tmp_rows), _ptr(tmp), _ptr(out),
                                   _stream()), "objnerf_clip_crops")
    return out


def _seed_of(seed):
    return (torch.initial_seed() if seed is None else int(seed)) & (2 ** 64 - 1)


def _sample_stacked_call(a: SampleArgs, K: int, table: torch.Tensor) -> None:
    """The stacked sampler launch for either table kind (keyframe_table): [K, 4] dense stores, [K, 5] cropped ones."""
    if table.shape[1] == 5:
        check(lib().objnerf_sample_rays_crops(C.byref(a), K, _ptr(table), _stream()), "objnerf_sample_rays_crops")
    else:
        check(lib().objnerf_sample_rays_stacked(C.byref(a), K, _ptr(table), _stream()), "objnerf_sample_rays_stacked")


def sample_rays_stacked(table: torch.Tensor, F: int, W: int, H: int, rays_dir_cache, kf_ids, u_w, u_h, u, g,
                        n_cam2surf: int, n_bins: int, surface_eps: float, stop_eps: float, min_bound: float = 0.0,
                        obj_center: float = 0.0, partfeat=None):
    """sample_rays for K objects in one launch chain, INJECTED draws: kf_ids [K, n_frames], u_w / u_h
    [K, n_frames, n_px], u [K, n, N+M], g [K, n, M].  Returns the STACKED batch tensors (rgb u8 [K,n,3], depth [K,n],
    valid [K,n] bool, labels u8 [K,n], pts [K,n,S,3], z [K,n,S])."""
    table = _req(table, torch.int64, "table")
    rays_dir_cache = _req(rays_dir_cache, torch.float32, "rays_dir_cache")
    kf_ids = _req(kf_ids, torch.int64, "kf_ids")
    u_w, u_h = _req(u_w, torch.float32, "u_w"), _req(u_h, torch.float32, "u_h")
    u, g = _req(u, torch.float32, "u"), _req(g, torch.float32, "g")
    K, n_frames, n_px = u_w.shape
    if table.shape not in ((K, 4), (K, 5)) or kf_ids.shape != (K, n_frames):
        raise ObjnerfError("sample_rays_stacked: table / kf_ids do not match the draws")
    n = n_frames * n_px
    S = n_cam2surf + n_bins
    if u.shape != (K, n, S) or g.shape != (K, n, n_bins):
        raise ObjnerfError("sample_rays_stacked: u / g shapes")
    o = _sample_common(K, n_frames, n_px, n_cam2surf, n_bins, table.device, True, False, True)
    a = SampleArgs(F, W, H, n_frames, n_px, n_cam2surf, n_bins, 0, surface_eps, stop_eps, min_bound, obj_center,
                   None, None, None, None, _ptr(rays_dir_cache), _ptr(kf_ids), _ptr(u_w), _ptr(u_h), _ptr(u), _ptr(g),
                   _ptr(o["rgb"]), _ptr(o["depth"]), _ptr(o["valid"]), _ptr(o["labels"]), _ptr(o["z"]), _ptr(o["pts"]),
                   _ptr(o["ws"]), 0, 0, 0, None, None, None, None, None)
    pf = _partfeat_fields(a, partfeat, K, F, n, table.device, True)
    _sample_stacked_call(a, K, table)
    r = (o["rgb"], o["depth"], o["valid"].bool(), o["labels"], o["pts"], o["z"])
    return r if partfeat is None else r + (pf,)


def sample_rays_seeded(stores, F: int, W: int, H: int, rays_dir_cache, kf_meta: torch.Tensor, n_frames: int, n_px: int,
                       n_cam2surf: int, n_bins: int, surface_eps: float, stop_eps: float, min_bound: float = 0.0,
                       obj_center: float = 0.0, seed: Optional[int] = None, draw: Optional[int] = None,
                       obj_index: int = 0, want_pts: bool = False, record: bool = False,
                       kf_ids: Optional[torch.Tensor] = None, partfeat=None) -> Dict[str, Optional[torch.Tensor]]:
    """The sampler with its random numbers generated in the kernels (Philox keyed on seed / draw / object / ray / bin;
    nothing random is stored).  stores: a keyframe table [K, 4] (ops.keyframe_table -> stacked call, tensors
    [K, ...]) or the four store tensors of ONE object (tensors without the leading K).  kf_meta int32 [K, 4] | [4]:
    n_keyframes, the slots of the latest two keyframes (-1 while n_keyframes <= 2), the object's random-stream id
    (without kf_meta: obj_index (+ k)); kf_ids overrides the seeded
    keyframe choice.  want_pts = False returns origins / dirs / z -- the pts == NULL form of ops.train_step, the
    [.., n, S, 3] point tensor is never written; record = True adds the drawn keyframes `kf` and pixels `px`.
    partfeat = (global_partfeat, use_frame, stride, part_down): the part-level feature of every ray (vmap.py:437-452)
    is gathered by the same launch -> key "partfeat" [.., n, C].
    Returns a dict: rgb u8, depth, valid (bool), labels u8, z, pts | origins + dirs, kf, px."""
    from .kf_store import KeyframeCropStore
    stacked = torch.is_tensor(stores)
    rays_dir_cache = _req(rays_dir_cache, torch.float32, "rays_dir_cache")
    kf_meta = _req(kf_meta, torch.int32, "kf_meta") if kf_meta is not None else None
    kf_ids = _req(kf_ids, torch.int64, "kf_ids") if kf_ids is not None else None
    table = None
    if stacked:
        table = _req(stores, torch.int64, "table")
        K, dev = table.shape[0], table.device
        if (kf_meta is not None and kf_meta.shape != (K, 4)) or (kf_ids is not None and kf_ids.shape != (K, n_frames)):
            raise ObjnerfError("sample_rays_seeded: kf_meta / kf_ids do not match the table")
        ptrs = [None] * 4
    elif isinstance(stores, KeyframeCropStore):
        # ONE object's cropped store: the crops entry point with K = 1, whose [1][...] layouts are the single call's
        table = keyframe_table([stores])
        K, dev = 1, table.device
        if (kf_meta is not None and kf_meta.shape != (4,)) or (kf_ids is not None and kf_ids.shape != (n_frames,)):
            raise ObjnerfError("sample_rays_seeded: kf_meta / kf_ids do not match the store")
        ptrs = [None] * 4
    else:
        rgbs, depth, t_wc, bbox = stores
        ptrs = [_ptr(_req(rgbs, torch.uint8, "rgbs_batch")), _ptr(_req(depth, torch.float32, "depth_batch")),
                _ptr(_req(t_wc, torch.float32, "t_wc_batch")), _ptr(_req(bbox, torch.float32, "bbox"))]
        K, dev = 1, rgbs.device
    if kf_meta is None and kf_ids is None:
        raise ObjnerfError("sample_rays_seeded: kf_meta or kf_ids")
    o = _sample_common(K, n_frames, n_px, n_cam2surf, n_bins, dev, want_pts, record, stacked)
    a = SampleArgs(F, W, H, n_frames, n_px, n_cam2surf, n_bins, int(obj_index), surface_eps, stop_eps, min_bound,
                   obj_center, *ptrs, _ptr(rays_dir_cache), _ptr(kf_ids), None, None, None, None,
                   _ptr(o["rgb"]), _ptr(o["depth"]), _ptr(o["valid"]), _ptr(o["labels"]), _ptr(o["z"]), _ptr(o["pts"]),
                   _ptr(o["ws"]), _seed_of(seed), (_next_offset() if draw is None else int(draw)) & 0x1FFFFFFF, 0,
                   _ptr(kf_meta), _ptr(o["kf"]), _ptr(o["px"]), _ptr(o["origins"]), _ptr(o["dirs"]))
    o["partfeat"] = _partfeat_fields(a, partfeat, K, F, n_frames * n_px, dev, stacked)
    if table is not None:
        _sample_stacked_call(a, K, table)
    else:
        check(lib().objnerf_sample_rays(C.byref(a), _stream()), "objnerf_sample_rays")
    if kf_ids is not None and record:
        o["kf"] = kf_ids
    o["valid"] = o["valid"].bool()
    del o["ws"]
    return o


def rays_dirs(W: int, H: int, fx: float, fy: float, cx: float, cy: float, device) -> torch.Tensor:
    out = torch.empty(W, H, 3, device=device)
    check(lib().objnerf_rays_dirs(W, H, fx, fy, cx, cy, _ptr(out), _stream()), "objnerf_rays_dirs")
    return out


def sample_rays(rgbs_batch, depth_batch, t_wc_batch, bbox, rays_dir_cache, kf_ids, u_w, u_h, u, g,
                n_cam2surf: int, n_bins: int, surface_eps: float, stop_eps: float, min_bound: float = 0.0,
                obj_center: float = 0.0, partfeat=None):
    """sceneObject.get_training_samples + sample_3d_points with injected draws (vmap.py:386-554).
    partfeat = (global_partfeat, use_frame, stride, part_down): also returns sampled_partfeat [n_frames, n_px, C]
    (vmap.py:437-452), gathered by the same launch."""
    rgbs_batch = _req(rgbs_batch, torch.uint8, "rgbs_batch")
    depth_batch = _req(depth_batch, torch.float32, "depth_batch")
    t_wc_batch = _req(t_wc_batch, torch.float32, "t_wc_batch")
    bbox = _req(bbox, torch.float32, "bbox")
    rays_dir_cache = _req(rays_dir_cache, torch.float32, "rays_dir_cache")
    kf_ids = _req(kf_ids, torch.int64, "kf_ids")
    u_w = _req(u_w, torch.float32, "u_w")
    u_h = _req(u_h, torch.float32, "u_h")
    u = _req(u, torch.float32, "u")
    g = _req(g, torch.float32, "g")
    F, W, H = rgbs_batch.shape[0], rgbs_batch.shape[1], rgbs_batch.shape[2]
    n_frames, n_px = u_w.shape
    n = n_frames * n_px
    S = n_cam2surf + n_bins
    dev = rgbs_batch.device
    out_rgb = torch.empty(n_frames, n_px, 3, dtype=torch.uint8, device=dev)
    out_depth = torch.empty(n_frames, n_px, device=dev)
    out_valid = torch.empty(n, dtype=torch.uint8, device=dev)
    out_labels = torch.empty(n, dtype=torch.uint8, device=dev)
    out_z = torch.empty(n_frames, n_px, S, device=dev)
    out_pts = torch.empty(n_frames, n_px, S, 3, device=dev)
    ws = torch.empty(1 + 6 * n, device=dev)
    a = SampleArgs(F, W, H, n_frames, n_px, n_cam2surf, n_bins, 0, surface_eps, stop_eps, min_bound, obj_center,
                   _ptr(rgbs_batch), _ptr(depth_batch), _ptr(t_wc_batch), _ptr(bbox), _ptr(rays_dir_cache),
                   _ptr(kf_ids), _ptr(u_w), _ptr(u_h), _ptr(u), _ptr(g), _ptr(out_rgb), _ptr(out_depth),
                   _ptr(out_valid), _ptr(out_labels), _ptr(out_z), _ptr(out_pts), _ptr(ws), 0, 0, 0, None, None, None,
                   None, None)
    pf = _partfeat_fields(a, partfeat, 1, F, n, dev, False)
    check(lib().objnerf_sample_rays(C.byref(a), _stream()), "objnerf_sample_rays")
    r = (out_rgb, out_depth, out_valid.bool(), out_labels, out_pts, out_z)
    return r if partfeat is None else r + (pf.reshape(n_frames, n_px, -1),)


def sample_points(sampled_rgbs, sampled_depth, origins, dirs_w, n_cam2surf: int, n_bins: int, surface_eps: float,
                  stop_eps: float, min_bound: float = 0.0, obj_center: float = 0.0, u=None, g=None, seed=None,
                  obj_index: int = 0):
    """sceneObject.sample_3d_points alone (vmap.py:456-554, objnerf_sample_points): the pixels are already gathered.
    sampled_rgbs u8 [n_frames, n_px, 4] (rgb + state), sampled_depth [n_frames, n_px], origins [n_frames, 3], dirs_w
    [n_frames, n_px, 3].  u [n, N + M] / g [n, M]: the reference's draws injected (both or neither; neither = Philox
    draws under `seed` and a per-call counter).  -> (rgb u8, depth, valid bool [n], labels u8 [n], pts, z)."""
    sampled_rgbs = _req(sampled_rgbs, torch.uint8, "sampled_rgbs")
    sampled_depth = _req(sampled_depth, torch.float32, "sampled_depth")
    origins = _req(origins, torch.float32, "origins")
    dirs_w = _req(dirs_w, torch.float32, "dirs_w")
    n_frames, n_px = sampled_depth.shape
    if tuple(sampled_rgbs.shape) != (n_frames, n_px, 4) or tuple(origins.shape) != (n_frames, 3) or \
            tuple(dirs_w.shape) != (n_frames, n_px, 3):
        raise ObjnerfError("sample_points: sampled_rgbs [F,P,4], sampled_depth [F,P], origins [F,3], dirs_w [F,P,3]")
    if (u is None) != (g is None):
        raise ObjnerfError("sample_points: inject both u and g or neither")
    n, S = n_frames * n_px, n_cam2surf + n_bins
    dev = sampled_rgbs.device
    if u is not None:
        u = _req(u, torch.float32, "u")
        g = _req(g, torch.float32, "g")
        draw = 0
    else:
        draw = _next_offset() & 0x1FFFFFFF
    out_rgb = torch.empty(n_frames, n_px, 3, dtype=torch.uint8, device=dev)
    out_depth = torch.empty(n_frames, n_px, device=dev)
    out_valid = torch.empty(n, dtype=torch.uint8, device=dev)
    out_labels = torch.empty(n, dtype=torch.uint8, device=dev)
    out_z = torch.empty(n_frames, n_px, S, device=dev)
    out_pts = torch.empty(n_frames, n_px, S, 3, device=dev)
    ws = torch.empty(1 + 6 * n, device=dev)
    a = SampleArgs(0, 0, 0, n_frames, n_px, n_cam2surf, n_bins, int(obj_index), surface_eps, stop_eps, min_bound,
                   obj_center, None, None, None, None, None, None, None, None, _ptr(u), _ptr(g), _ptr(out_rgb),
                   _ptr(out_depth), _ptr(out_valid), _ptr(out_labels), _ptr(out_z), _ptr(out_pts), _ptr(ws),
                   _seed_of(seed), draw, 0, None, None, None, None, None)
    check(lib().objnerf_sample_points(C.byref(a), _ptr(sampled_rgbs), _ptr(sampled_depth), _ptr(origins), _ptr(dirs_w),
                                      _stream()), "objnerf_sample_points")
    return out_rgb, out_depth, out_valid.bool(), out_labels, out_pts, out_z


# ------------------------------------------------------------------------------------------------
# helper functions of the reference's call surface (objnerf_helpers.hip)
# ------------------------------------------------------------------------------------------------
def render(termination: torch.Tensor, vals: torch.Tensor) -> torch.Tensor:
    """render_rays.render over the last axis of termination [..., S] with vals [..., S] or [..., S, C] (objnerf_render)."""
    termination = _req(termination, torch.float32, "termination")
    S = termination.shape[-1]
    scalar = vals.dim() == termination.dim()
    Cdim = 1 if scalar else vals.shape[-1]
    vals = _req(vals, torch.float32, "vals")
    if tuple(vals.shape[:termination.dim()]) != tuple(termination.shape):
        raise ObjnerfError("render: vals must be termination's shape (+ a channel axis)")
    n = termination.numel() // S
    out = torch.empty(termination.shape[:-1] + (() if scalar else (Cdim,)), device=termination.device)
    if n:
        check(lib().objnerf_render(n, S, Cdim, _ptr(termination), _ptr(vals), _ptr(out), _stream()), "objnerf_render")
    return out


def render_loss(render: torch.Tensor, gt: torch.Tensor, mode: int, normalise: bool = False) -> torch.Tensor:
    """render_rays.render_loss: mode 0 L1, 1 L2 (elementwise, any shape); 2 cos (over the last axis)."""
    render = _req(render, torch.float32, "render")
    gt = _req(gt.expand_as(render) if gt.shape != render.shape else gt, torch.float32, "gt")
    if mode == 2:
        Cdim = render.shape[-1]
        out = torch.empty(render.shape[:-1], device=render.device)
        n = out.numel()
    else:
        Cdim, out = 1, torch.empty_like(render)
        n = out.numel()
    if n:
        check(lib().objnerf_render_loss(n, Cdim, mode, int(normalise), _ptr(render), _ptr(gt), _ptr(out), _stream()),
              "objnerf_render_loss")
    return out


def reduce_batch_loss(loss_mat: torch.Tensor, var, mask: torch.Tensor, l2: bool, avg: bool):
    """render_rays.reduce_batch_loss on [K,R] tensors -> (out [K] or [K,R], status int32[1])."""
    loss_mat = _req(loss_mat, torch.float32, "loss_mat")
    K, R = loss_mat.shape
    var = _req(var, torch.float32, "var") if var is not None else None
    mask = _req(mask.to(torch.uint8), torch.uint8, "mask")
    dev = loss_mat.device
    out = torch.empty(K if avg else (K, R), device=dev) if avg else torch.empty(K, R, device=dev)
    ws = torch.empty(K + 1, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    check(lib().objnerf_reduce_batch_loss(K, R, _ptr(loss_mat), _ptr(var), _ptr(mask), int(l2), int(avg), _ptr(ws), _ptr(out),
                                          _ptr(status), _stream()), "objnerf_reduce_batch_loss")
    return out, status


def make_grid(dim: int, lo: float, hi: float, scale, transform, device) -> torch.Tensor:
    out = torch.empty(dim, dim, dim, 3, device=device)
    scale = _req(scale.to(device).float().reshape(3), torch.float32, "scale") if scale is not None else None
    transform = _req(transform.to(device).float().reshape(4, 4), torch.float32, "transform") if transform is not None else None
    check(lib().objnerf_make_grid(dim, float(lo), float(hi), _ptr(scale), _ptr(transform), _ptr(out), _stream()),
          "objnerf_make_grid")
    return out


def ray_box(origins, directions, bounds_min, bounds_max):
    origins = _req(origins, torch.float32, "origins")
    directions = _req(directions, torch.float32, "directions")
    n, dev = origins.shape[0], origins.device
    bmin = _req(torch.as_tensor(bounds_min, dtype=torch.float32, device=dev).reshape(3), torch.float32, "bounds_min")
    bmax = _req(torch.as_tensor(bounds_max, dtype=torch.float32, device=dev).reshape(3), torch.float32, "bounds_max")
    near, far = torch.empty(n, device=dev), torch.empty(n, device=dev)
    hit = torch.empty(n, dtype=torch.uint8, device=dev)
    check(lib().objnerf_ray_box(n, _ptr(origins), _ptr(directions), _ptr(bmin), _ptr(bmax), _ptr(near), _ptr(far), _ptr(hit),
                                _stream()), "objnerf_ray_box")
    return near, far, hit.bool()


def dirs_w(T_WC: torch.Tensor, dirs_C: torch.Tensor) -> torch.Tensor:
    T_WC = _req(T_WC, torch.float32, "T_WC")
    dirs_C = _req(dirs_C, torch.float32, "dirs_C")
    F = T_WC.shape[0]
    P = dirs_C.numel() // (3 * F)
    out = torch.empty_like(dirs_C)
    check(lib().objnerf_dirs_w(F, P, _ptr(T_WC), _ptr(dirs_C), _ptr(out), _stream()), "objnerf_dirs_w")
    return out


_draw_offset = [0]


def _next_offset() -> int:
    _draw_offset[0] += 1
    return _draw_offset[0]


def stratified_bins(lo, hi, n_bins: int, n_rays: int, device, u: Optional[torch.Tensor] = None,
                    seed: Optional[int] = None, draw: Optional[int] = None) -> torch.Tensor:
    """lo / hi: python scalars or [n_rays] tensors.  u: injected uniforms [n_rays, n_bins]; otherwise the counter-based
    generator under `seed` (default: torch's initial seed) and the call counter `draw` (default: advances per call)."""
    lo_t = _req(lo.to(device), torch.float32, "min_depth") if torch.is_tensor(lo) else None
    hi_t = _req(hi.to(device), torch.float32, "max_depth") if torch.is_tensor(hi) else None
    u = _req(u, torch.float32, "u") if u is not None else None
    out = torch.empty(n_rays, n_bins, device=device)
    sd = torch.initial_seed() if seed is None else seed
    check(lib().objnerf_stratified_bins(n_rays, n_bins, _ptr(lo_t), 0.0 if lo_t is not None else float(lo), _ptr(hi_t),
                                        0.0 if hi_t is not None else float(hi), _ptr(u), sd & (2 ** 64 - 1),
                                        _next_offset() if draw is None else int(draw),
                                        _ptr(out), _stream()), "objnerf_stratified_bins")
    return out


def normal_bins(depth: torch.Tensor, n_bins: int, delta: float, g: Optional[torch.Tensor] = None,
                seed: Optional[int] = None, draw: Optional[int] = None) -> torch.Tensor:
    depth = _req(depth, torch.float32, "depth")
    n_rays = depth.shape[0]
    g = _req(g, torch.float32, "g") if g is not None else None
    out = torch.empty(n_rays, n_bins, device=depth.device)
    sd = torch.initial_seed() if seed is None else seed
    check(lib().objnerf_normal_bins(n_rays, n_bins, _ptr(depth), float(delta), _ptr(g), sd & (2 ** 64 - 1),
                                    _next_offset() if draw is None else int(draw), _ptr(out), _stream()),
          "objnerf_normal_bins")
    return out


def marching_cubes(volume: torch.Tensor, level: float = 0.5, gradient_direction: str = "ascent"):
    """skimage.measure.marching_cubes(volume, level, gradient_direction=...) (vis.py:11-12) on the GPU:
    volume [d,d,d] (2 <= d <= 1024; cast to fp32 like skimage) -> device (verts [V,3] fp32 in index units,
    faces [F,3] int32, normals [V,3] fp32 unit, down the gradient).  One vertex per crossing lattice edge, ordered by
    (owning lattice point, axis); faces by (cell, table order); bit-reproducible (objnerf_mesh.hip).
    Synchronises the stream once: objnerf_mc_count's V and F are read back (.item()) to size the outputs before
    objnerf_mc_emit.  skimage raises where this returns V = F = 0 (no crossing edge) and where `level` lies outside
    [min, max]; vis.marching_cubes maps both to None as the reference does.
    Normals are the central-difference gradient (one-sided at the border) interpolated along the edge.  skimage's
    Lewiner implementation takes forward differences inside the cell instead, so its normals agree with these in sign
    and direction (cos > 0.99, mean > 0.999 on smooth volumes) but not in digits; vertices, faces and winding match."""
    if gradient_direction not in ("ascent", "descent"):
        raise ValueError(f"Incorrect input {gradient_direction} in `gradient_direction`")
    if volume.dim() != 3 or len(set(volume.shape)) != 1:
        raise _lib.ObjnerfError(f"marching_cubes: expected a cubic [d,d,d] volume, got {tuple(volume.shape)}")
    vol = _req(volume if volume.dtype == torch.float32 else volume.float(), torch.float32, "volume")
    d, dev = int(vol.shape[0]), vol.device
    nbytes = int(lib().objnerf_mc_workspace_bytes(d))
    if nbytes == 0:
        raise _lib.ObjnerfError(f"marching_cubes: dim {d} outside 2..1024")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    check(lib().objnerf_mc_count(d, float(level), _ptr(vol), _ptr(ws), nbytes, _ptr(counts), _stream()),
          "objnerf_mc_count")
    V, F = (int(x) for x in counts.tolist())                  # the one host sync
    if V > 2 ** 31 - 1:
        raise _lib.ObjnerfError(f"marching_cubes: {V} vertices do not fit int32 face indices")
    verts = torch.empty(V, 3, device=dev)
    normals = torch.empty(V, 3, device=dev)
    faces = torch.empty(F, 3, dtype=torch.int32, device=dev)
    flags = 1 if gradient_direction == "descent" else 0        # OBJNERF_MC_DESCENT
    check(lib().objnerf_mc_emit(d, float(level), flags, _ptr(vol), _ptr(ws), nbytes, V, F, _ptr(verts) if V else None,
                                _ptr(normals) if V else None, _ptr(faces) if F else None, _stream()), "objnerf_mc_emit")
    return verts, faces, normals


def run_centroids(skeys: torch.Tensor, perm: torch.Tensor, pts: torch.Tensor, n_groups: int):
    """Centroids of the runs of equal keys in skeys (int64 [n], stable-sorted; perm the sort's permutation of the rows
    of pts fp64 [n, 3]): objnerf_voxel_heads, one read-back of the run count V, objnerf_voxel_centroids
    -> (centroids fp64 [V, 3] = the in-order fp64 sum of a run's points / their count, keys int64 [V] without the
    group bits (key >> 42), first int64 [n_groups] = the first run of every group, -1 for a group without points)."""
    n, dev = int(skeys.numel()), skeys.device
    pts = _req(pts, torch.float64, "pts")
    hws = torch.empty(int(lib().objnerf_voxel_heads_workspace_bytes(n)) // 8, dtype=torch.int64, device=dev)
    check(lib().objnerf_voxel_heads(n, _ptr(skeys), _ptr(hws), _stream()), "objnerf_voxel_heads")
    V = int(hws[-1].item())
    cen = torch.empty(V, 3, dtype=torch.float64, device=dev)
    vkeys = torch.empty(V, dtype=torch.int64, device=dev)
    first = torch.full((n_groups,), -1, dtype=torch.int64, device=dev)
    check(lib().objnerf_voxel_centroids(n, _ptr(skeys), _ptr(perm), _ptr(pts), _ptr(hws), V, _ptr(cen), _ptr(vkeys),
                                        _ptr(first), _stream()), "objnerf_voxel_centroids")
    return cen, vkeys, first


def objects_voxels(objects, intrinsics=None, voxel: float = 0.05, **kw):
    """Voxel-down-sampled keyframe point clouds of sceneObjects (vmap.py:303-320) -> per object (voxel indices int64
    [n,3], centroids fp64 [n,3]); objnerf_voxel_scan / _emit / _heads / _centroids (openobj_amd/bounds.py)."""
    from . import bounds
    return bounds.objects_voxels(objects, intrinsics, voxel, **kw)


def object_bounds(objects, intrinsics=None, voxel: float = 0.05, min_extent: float = 0.10, **kw):
    """sceneObject.get_bound (vmap.py:287-384) for a list of objects: the voxel chain above, the hull of each object's
    centroids on the host, objnerf_obb_search for all of them in one launch -> [(bbox3d, bbox) | (None, None)]
    (openobj_amd/bounds.py states the algorithm and its one deviation from trimesh)."""
    from . import bounds
    return bounds.object_bounds(objects, intrinsics, voxel, min_extent, **kw)


# ------------------------------------------------------------------------------------------------ ABI 10: map queries
def _rows(feat: torch.Tensor, name: str):
    """feat [V, D] fp32 on the device, unit stride along D (any row stride) -> (V, D, row stride)."""
    if feat.dtype != torch.float32 or not feat.is_cuda or feat.dim() != 2:
        raise _lib.ObjnerfError(f"{name}: expected a device fp32 [V, D] tensor, got {feat.dtype} {tuple(feat.shape)}")
    if feat.shape[1] > 1 and feat.stride(1) != 1:
        raise _lib.ObjnerfError(f"{name}: the feature dimension must be contiguous")
    V, D = int(feat.shape[0]), int(feat.shape[1])
    return V, D, max(int(feat.stride(0)), D) if V > 1 else D


def _seg(seg_off: torch.Tensor, dev) -> torch.Tensor:
    s = torch.as_tensor(seg_off, dtype=torch.int64).to(dev).contiguous()
    if s.dim() != 1 or s.numel() < 2:
        raise _lib.ObjnerfError("seg_off: expected [S + 1] row offsets")
    return s


def segment_project(feat: torch.Tensor, seg_off, W: torch.Tensor, bias: Optional[torch.Tensor] = None,
                    cosine: bool = False, out: Optional[torch.Tensor] = None):
    """out [V, Q] = feat . W + bias per segment (objnerf_project), W [D, Q] shared or [S, D, Q] per segment (bias [Q] /
    [S, Q]); cosine=True: F.cosine_similarity of every row against every column of W (vis_interaction.py:372, :388).
    -> (out [V, Q] fp32, minmax [S, Q, 2] fp32: the min / max of each segment's rows of out, +inf / -inf if empty)."""
    V, D, rs = _rows(feat, "segment_project")
    dev = feat.device
    seg = _seg(seg_off, dev)
    S = seg.numel() - 1
    Wt = _req(torch.as_tensor(W).to(device=dev, dtype=torch.float32), torch.float32, "W")
    per = Wt.dim() == 3
    if Wt.shape[-2] != D or Wt.dim() not in (2, 3) or (per and Wt.shape[0] != S):
        raise _lib.ObjnerfError(f"segment_project: W {tuple(Wt.shape)} does not match D = {D}, S = {S}")
    Q = int(Wt.shape[-1])
    b = None if bias is None else _req(torch.as_tensor(bias).to(device=dev, dtype=torch.float32), torch.float32, "bias")
    if b is not None and tuple(b.shape) != ((S, Q) if per else (Q,)):
        raise _lib.ObjnerfError(f"segment_project: bias {tuple(b.shape)} does not match W")
    if out is None:
        out = torch.empty(V, Q, device=dev)
    minmax = torch.empty(S, Q, 2, device=dev)
    nbytes = int(lib().objnerf_project_workspace_bytes(S, Q, V))
    if nbytes == 0:
        raise _lib.ObjnerfError(f"segment_project: unsupported S = {S}, Q = {Q}")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    a = _lib.ProjectArgs(S, D, Q, (_lib.PROJ_COSINE if cosine else 0) | (_lib.PROJ_PER_SEGMENT if per else 0), V, rs,
                         _ptr(feat) if V else None, _ptr(seg), _ptr(Wt), _ptr(b), _ptr(out), _ptr(minmax))
    check(lib().objnerf_project(C.byref(a), _ptr(ws), nbytes, _stream()), "objnerf_project")
    return out, minmax


def segment_moments(feat: torch.Tensor, seg_off):
    """objnerf_moments -> (mean [S, D] fp64, scatter [S, D, D] fp64 = sum of (f - m)(f - m)^T over each segment)."""
    V, D, rs = _rows(feat, "segment_moments")
    dev = feat.device
    seg = _seg(seg_off, dev)
    S = seg.numel() - 1
    mean = torch.empty(S, D, dtype=torch.float64, device=dev)
    scatter = torch.empty(S, D, D, dtype=torch.float64, device=dev)
    nbytes = int(lib().objnerf_moments_workspace_bytes(S, D))
    if nbytes == 0:
        raise _lib.ObjnerfError(f"segment_moments: unsupported S = {S}, D = {D}")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    a = _lib.MomentsArgs(S, D, V, rs, _ptr(feat) if V else None, _ptr(seg), _ptr(mean), _ptr(scatter))
    check(lib().objnerf_moments(C.byref(a), _ptr(ws), nbytes, _stream()), "objnerf_moments")
    return mean, scatter


def vertex_colors(seg_off, mode, V: int, rgb: Optional[torch.Tensor] = None, factor=None, constant=None, column=None,
                  proj: Optional[torch.Tensor] = None, minmax: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """objnerf_vertex_colors: [V, 3] fp32 colours, per segment mode[s] in _lib.COLOR_* (RGB: rgb [V, >=3] uint8 x
    factor[s]; CONSTANT: constant[s]; RAINBOW: "rainbow" of proj[:, column[s]] over minmax[s]; PCA: columns 0..2)."""
    dev = torch.device("cuda", torch.cuda.current_device()) if out is None else out.device
    seg = _seg(seg_off, dev)
    S = seg.numel() - 1
    md = torch.as_tensor(mode, dtype=torch.int32).to(dev).contiguous()
    if md.numel() != S:
        raise _lib.ObjnerfError("vertex_colors: one mode per segment")
    fac = None if factor is None else torch.as_tensor(factor, dtype=torch.float64).to(dev).contiguous()
    cst = None if constant is None else torch.as_tensor(constant, dtype=torch.float32).to(dev).reshape(S, 3).contiguous()
    colm = None if column is None else torch.as_tensor(column, dtype=torch.int32).to(dev).contiguous()
    Q, rs = 0, 0
    if rgb is not None:
        if rgb.dtype != torch.uint8 or rgb.dim() != 2 or rgb.shape[1] < 3 or rgb.stride(1) != 1:
            raise _lib.ObjnerfError("vertex_colors: rgb must be uint8 [V, 3 or 4] with unit channel stride")
        rs = int(rgb.stride(0))
    if proj is not None:
        proj = _req(proj, torch.float32, "proj")
        Q = int(proj.shape[1])
    # every array a mode reads must be there and large enough: the kernel trusts these shapes
    mh = md.cpu().numpy()
    if ((mh < _lib.COLOR_RGB) | (mh > _lib.COLOR_PCA)).any():
        raise _lib.ObjnerfError("vertex_colors: unknown mode")
    if (mh == _lib.COLOR_RGB).any() and (rgb is None or fac is None or fac.numel() != S or rgb.shape[0] < V):
        raise _lib.ObjnerfError("vertex_colors: RGB needs rgb [V, 3+] and factor [S]")
    if (mh == _lib.COLOR_CONSTANT).any() and cst is None:
        raise _lib.ObjnerfError("vertex_colors: CONSTANT needs constant [S, 3]")
    if ((mh == _lib.COLOR_RAINBOW) | (mh == _lib.COLOR_PCA)).any():
        if proj is None or minmax is None or proj.shape[0] < V or tuple(minmax.shape) != (S, Q, 2):
            raise _lib.ObjnerfError("vertex_colors: RAINBOW / PCA need proj [V, Q] and minmax [S, Q, 2]")
        if (mh == _lib.COLOR_PCA).any() and Q < 3:
            raise _lib.ObjnerfError("vertex_colors: PCA needs three columns")
        if (mh == _lib.COLOR_RAINBOW).any():
            ch = None if colm is None else colm.cpu().numpy()
            if ch is None or ch.size != S or ((ch[mh == _lib.COLOR_RAINBOW] < 0) | (ch[mh == _lib.COLOR_RAINBOW] >= Q)).any():
                raise _lib.ObjnerfError("vertex_colors: RAINBOW needs column [S] within proj's Q columns")
    if out is None:
        out = torch.empty(V, 3, device=dev)
    a = _lib.ColorArgs(S, Q, int(V), rs, _ptr(seg), _ptr(md), _ptr(rgb), _ptr(fac), _ptr(cst), _ptr(colm), _ptr(proj),
                       _ptr(None if minmax is None else _req(minmax, torch.float32, "minmax")), _ptr(out))
    check(lib().objnerf_vertex_colors(C.byref(a), _stream()), "objnerf_vertex_colors")
    return out


PART_ROW_PAD = 4                        # row stride of part_rows' buffer = H + 4: rows stay 16-byte aligned


def part_rows(hfeat: torch.Tensor, of_w: torch.Tensor, of_b: torch.Tensor, out: Optional[torch.Tensor] = None):
    """The compact rows of a vertex set (objnerf_part_rows): hfeat [V, H] fp32 (any row stride), of_w [C, H], of_b [C]
    -> rows [V, H + 1] = [h s, s], s = 1 / max(|of_w h + of_b|, 1e-8): the unit part feature is [of_w | of_b] . row.
    The result is a view of a [V, H + 4] buffer (`out`, if given, is that buffer): rows stay 16-byte aligned for
    objnerf_project's float4 path; columns H + 1 .. H + 3 of the buffer are zero."""
    V, H, rs = _rows(hfeat, "part_rows")
    dev = hfeat.device
    of_w, of_b = _req(of_w, torch.float32, "part_rows: of_w"), _req(of_b, torch.float32, "part_rows: of_b")
    if of_w.dim() != 2 or int(of_w.shape[1]) != H or tuple(of_b.shape) != (int(of_w.shape[0]),):
        raise ObjnerfError(f"part_rows: of_w [C, {H}], of_b [C], got {tuple(of_w.shape)}, {tuple(of_b.shape)}")
    if of_w.device != dev or of_b.device != dev:
        raise ObjnerfError(f"part_rows: the head is not on {dev}")
    C_ = int(of_w.shape[0])
    if out is None:
        out = torch.empty(V, H + PART_ROW_PAD, device=dev)
    elif (out.dtype != torch.float32 or out.device != dev or tuple(out.shape) != (V, H + PART_ROW_PAD)
          or not out.is_contiguous()):
        raise ObjnerfError(f"part_rows: out must be a contiguous fp32 [{V}, {H + PART_ROW_PAD}] buffer on {dev}")
    check(lib().objnerf_part_rows(V, H, C_, _ptr(hfeat) if V else None, rs, _ptr(of_w), _ptr(of_b),
                                  _ptr(out) if V else None, H + PART_ROW_PAD, _stream()), "objnerf_part_rows")
    return out[:, :H + 1]


def part_expand(rows: torch.Tensor, head: torch.Tensor, index: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out [n, C] = head . rows[index] (objnerf_part_expand): rows [V, H + 1] fp32 (any row stride), head [C, H + 1],
    index int64 [n] on the device (None: every row in order); an index outside [0, V) gives a zero row."""
    V, H1, rs = _rows(rows, "part_expand")
    dev = rows.device
    head = _req(head, torch.float32, "part_expand: head")
    if head.dim() != 2 or int(head.shape[1]) != H1 or head.device != dev:
        raise ObjnerfError(f"part_expand: head [C, {H1}] on {dev}, got {tuple(head.shape)} on {head.device}")
    C_ = int(head.shape[0])
    n = V
    if index is not None:
        if not index.is_cuda or index.device != dev or index.dim() != 1 or index.dtype != torch.int64:
            raise ObjnerfError("part_expand: index: a flat int64 tensor on the rows' device")
        index = index.contiguous()
        n = int(index.shape[0])
    out = torch.empty(n, C_, device=dev)
    check(lib().objnerf_part_expand(V, H1 - 1, C_, _ptr(rows) if V else None, max(rs, H1), _ptr(head), n,
                                    _ptr(index) if index is not None and n else None, _ptr(out) if n else None,
                                    _stream()), "objnerf_part_expand")
    return out


def rainbow_lut() -> np.ndarray:
    """The colour kernel's "rainbow" table [256, 3] fp32 (objnerf_rainbow_lut, host only)."""
    out = np.empty((256, 3), np.float32)
    n = lib().objnerf_rainbow_lut(out.ctypes.data)
    if n != 256:
        raise _lib.ObjnerfError("objnerf_rainbow_lut failed")
    return out


# ------------------------------------------------------------------ cross-frame mask association (objnerf_maskgraph.hip)
_CELL_SLACK = 1.0 + 2.0 ** -20      # cell side = radius x this (include/objnerf_hip.h, objnerf_cell_keys)


def _point_sets(pts: torch.Tensor, seg_off, name: str):
    pts = _req(pts, torch.float64, name)
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise _lib.ObjnerfError(f"{name}: expected [n, 3] fp64 points")
    off = torch.as_tensor(seg_off, dtype=torch.int64).cpu()
    n = int(pts.shape[0])
    if off.dim() != 1 or off.numel() < 2 or int(off[0]) != 0 or int(off[-1]) != n or bool((off[1:] < off[:-1]).any()):
        raise _lib.ObjnerfError(f"{name}: seg_off must rise from 0 to the number of points")
    if n >= 2 ** 31:
        raise _lib.ObjnerfError(f"{name}: at most 2^31 - 1 points")
    return pts, off, n


def cell_keys(pts: torch.Tensor, seg_off, cell: float, shift: float = 0.0, name: str = "cell_keys"):
    """objnerf_cell_keys -> (keys int64 [n] = ix << 42 | iy << 21 | iz, the sets' minimum corners fp64 [S, 3])."""
    pts, off, n = _point_sets(pts, seg_off, name)
    dev = pts.device
    S = off.numel() - 1
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    mins = torch.empty(S, 3, dtype=torch.float64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    check(lib().objnerf_cell_keys(n, S, _ptr(pts) if n else None, _ptr(off.to(dev)), float(cell), float(shift), _ptr(mins),
                                  _ptr(keys) if n else None, _ptr(status), _stream()), "objnerf_cell_keys")
    if int(status.item()) != 0:
        raise _lib.ObjnerfError(f"{name}: a point is not finite or lies more than 2^21 cells from its set's corner")
    return keys, mins


def _sorted_cells(pts: torch.Tensor, key_off: torch.Tensor, sort_off: torch.Tensor, radius: float, name: str):
    """Cell keys on one grid per segment of key_off, sorted (stable) inside every segment of sort_off
    -> (sorted keys, permutation), both int64 [n]."""
    keys, _ = cell_keys(pts, key_off, float(radius) * _CELL_SLACK, 0.0, name)
    return _sort_in_segments(keys, sort_off, pts.device)


def _sort_in_segments(keys: torch.Tensor, off: torch.Tensor, dev):
    """keys sorted (stable) inside every segment of off -> (sorted keys, permutation), both int64 [n]."""
    sk, perm = torch.sort(keys, stable=True)
    seg = torch.repeat_interleave(torch.arange(off.numel() - 1, device=dev), (off[1:] - off[:-1]).to(dev))
    _, order = torch.sort(seg[perm], stable=True)
    return sk[order].contiguous(), perm[order].contiguous()


class DbscanPlan:
    """The sorted cell keys of S point sets for one eps: dbscan() with several min_points reuses them."""

    def __init__(self, pts: torch.Tensor, seg_off, eps: float):
        self.pts, self.off, self.n = _point_sets(pts, seg_off, "dbscan")
        self.eps = float(eps)
        if not self.eps > 0.0:
            raise _lib.ObjnerfError("dbscan: eps must be positive")
        self.S = self.off.numel() - 1
        self.dev = self.pts.device
        self.off_dev = self.off.to(self.dev)
        self.labels = torch.full((self.n,), -1, dtype=torch.int32, device=self.dev)
        if self.n:
            self.keys, self.perm = _sorted_cells(self.pts, self.off, self.off, self.eps, "dbscan")
            self.ws = torch.empty(int(lib().objnerf_dbscan_workspace_bytes(self.n)), dtype=torch.uint8, device=self.dev)

    def run(self, min_points) -> torch.Tensor:
        """objnerf_dbscan: labels int32 [n] (per set, from 0; -1 noise); min_points: one int, or one per set, <= 0
        leaving that set's labels as the previous run wrote them."""
        mp = torch.as_tensor(min_points, dtype=torch.int32).reshape(-1)
        if mp.numel() == 1:
            mp = mp.expand(self.S)
        if mp.numel() != self.S:
            raise _lib.ObjnerfError("dbscan: one min_points per point set")
        mp = mp.contiguous().to(self.dev)
        if self.n:
            check(lib().objnerf_dbscan(self.n, self.S, _ptr(self.pts), _ptr(self.off_dev), _ptr(self.keys), _ptr(self.perm),
                                       _ptr(mp), self.eps, _ptr(self.ws), self.ws.numel(), _ptr(self.labels), _stream()),
                  "objnerf_dbscan")
        return self.labels


def dbscan(pts: torch.Tensor, seg_off, eps: float, min_points) -> torch.Tensor:
    """Segmented DBSCAN of the point sets pts[seg_off[s] : seg_off[s+1]] -> labels int32 [n], scikit-learn's."""
    return DbscanPlan(pts, seg_off, eps).run(min_points).clone()


def cloud_overlap(pts: torch.Tensor, cloud_off, dis_thre: float) -> torch.Tensor:
    """objnerf_cloud_overlap -> count int64 [C, C]: points of cloud a with a point of cloud b nearer than dis_thre."""
    pts, off, n = _point_sets(pts, cloud_off, "cloud_overlap")
    if not float(dis_thre) > 0.0:
        raise _lib.ObjnerfError("cloud_overlap: dis_thre must be positive")
    Cn = off.numel() - 1
    dev = pts.device
    out = torch.empty(Cn, Cn, dtype=torch.int64, device=dev)
    keys = perm = None
    if n:
        keys, perm = _sorted_cells(pts, torch.tensor([0, n]), off, float(dis_thre), "cloud_overlap")
    check(lib().objnerf_cloud_overlap(n, Cn, _ptr(pts) if n else None, _ptr(off.to(dev)), _ptr(keys), _ptr(perm),
                                      float(dis_thre), _ptr(out), _stream()), "objnerf_cloud_overlap")
    return out


def mask_ray_boxes(depth_raw: torch.Tensor, twc: torch.Tensor, boxes: torch.Tensor, fx: float, fy: float, cx: float,
                   cy: float) -> torch.Tensor:
    """objnerf_mask_ray_boxes: depth_raw [F, H, W] int16 holding the uint16 image's bits, twc [F, 4, 4] fp64,
    boxes [N, 6] fp64 -> [F, N, 4] int32 (row_min, col_min, row_max + 1, col_max + 1) in the every-10th-pixel grid."""
    depth_raw = _req(depth_raw, torch.int16, "depth_raw")
    twc = _req(twc, torch.float64, "twc")
    boxes = _req(boxes, torch.float64, "boxes")
    if depth_raw.dim() != 3 or tuple(twc.shape) != (depth_raw.shape[0], 4, 4) or boxes.dim() != 2 or boxes.shape[1] != 6:
        raise _lib.ObjnerfError("mask_ray_boxes: depth_raw [F, H, W], twc [F, 4, 4], boxes [N, 6]")
    F, H, W = (int(v) for v in depth_raw.shape)
    N = int(boxes.shape[0])
    out = torch.empty(F, N, 4, dtype=torch.int32, device=boxes.device)
    a = _lib.RayBoxesArgs(F, N, W, H, float(fx), float(fy), float(cx), float(cy), _ptr(depth_raw), _ptr(twc), _ptr(boxes),
                          _ptr(out))
    check(lib().objnerf_mask_ray_boxes(C.byref(a), _stream()), "objnerf_mask_ray_boxes")
    return out


def mask_points(pix: torch.Tensor, depth: torch.Tensor, pose: torch.Tensor, fx: float, fy: float, cx: float,
                cy: float) -> torch.Tensor:
    """objnerf_mask_points: pix int32 [n] (v * W + u), depth fp32 [H, W], pose fp64 [4, 4] -> world points fp64 [n, 3]."""
    pix = _req(pix, torch.int32, "pix")
    depth = _req(depth, torch.float32, "depth")
    pose = _req(pose, torch.float64, "pose")
    if depth.dim() != 2 or tuple(pose.shape) != (4, 4) or pix.dim() != 1:
        raise _lib.ObjnerfError("mask_points: pix [n], depth [H, W], pose [4, 4]")
    n = int(pix.numel())
    out = torch.empty(n, 3, dtype=torch.float64, device=depth.device)
    a = _lib.MaskPointsArgs(n, int(depth.shape[1]), int(depth.shape[0]), float(fx), float(fy), float(cx), float(cy),
                            _ptr(pix) if n else None, _ptr(depth), _ptr(pose), _ptr(out) if n else None)
    check(lib().objnerf_mask_points(C.byref(a), _stream()), "objnerf_mask_points")
    return out


def mask_hist(pix: torch.Tensor, mask_off, img: torch.Tensor) -> torch.Tensor:
    """objnerf_mask_hist: per mask the 3 x 32-bin histogram of img uint8 [H, W, 3] over pix[mask_off[m] : mask_off[m+1]]
    -> fp32 [M, 96]."""
    pix = _req(pix, torch.int32, "pix")
    img = _req(img, torch.uint8, "img")
    off = torch.as_tensor(mask_off, dtype=torch.int64).cpu()
    n = int(pix.numel())
    if img.dim() != 3 or img.shape[2] != 3 or off.numel() < 2 or int(off[0]) != 0 or int(off[-1]) != n or \
            bool((off[1:] < off[:-1]).any()):
        raise _lib.ObjnerfError("mask_hist: img [H, W, 3] and mask_off rising from 0 to the number of pixels")
    M = off.numel() - 1
    out = torch.empty(M, 96, dtype=torch.float32, device=img.device)
    check(lib().objnerf_mask_hist(n, M, _ptr(pix) if n else None, _ptr(off.to(img.device)), _ptr(img), int(img.shape[1]),
                                  int(img.shape[0]), _ptr(out), _stream()), "objnerf_mask_hist")
    return out


def point_bounds(pts: torch.Tensor, seg_off) -> torch.Tensor:
    """objnerf_point_bounds -> fp64 [S, 6]: (min, max) of every point set (exact)."""
    pts, off, n = _point_sets(pts, seg_off, "point_bounds")
    S = off.numel() - 1
    out = torch.empty(S, 6, dtype=torch.float64, device=pts.device)
    check(lib().objnerf_point_bounds(n, S, _ptr(pts) if n else None, _ptr(off.to(pts.device)), _ptr(out), _stream()),
          "objnerf_point_bounds")
    return out


def mask_affinity(boxes: torch.Tensor, cap: torch.Tensor, clip: torch.Tensor, color: torch.Tensor,
                  boxes2d: Optional[torch.Tensor], weights: Sequence[float], want_terms: bool = False):
    """objnerf_mask_affinity + objnerf_mask_edges: weights = (w_geo, w_cap, w_clip, w_color, w_geo2d)
    -> (W fp32 [N, N], edges int32 [E, 2] with i < j in row-major order, their weights fp32 [E], terms [5, N, N] or None)."""
    boxes = _req(boxes, torch.float64, "boxes")
    cap, clip, color = (_req(t, torch.float32, n) for t, n in ((cap, "cap"), (clip, "clip"), (color, "color")))
    N = int(boxes.shape[0])
    if N < 1 or tuple(boxes.shape) != (N, 6) or cap.dim() != 2 or clip.dim() != 2 or cap.shape[0] != N or \
            clip.shape[0] != N or tuple(color.shape) != (N, 96):
        raise _lib.ObjnerfError("mask_affinity: boxes [N, 6], cap [N, Dc], clip [N, Dl], color [N, 96]")
    wg, wc, wl, wo, w2 = (float(w) for w in weights)
    F = 0
    if w2 != 0.0:
        if boxes2d is None:
            raise _lib.ObjnerfError("mask_affinity: a 2-D weight needs the 2-D boxes")
        boxes2d = _req(boxes2d, torch.int32, "boxes2d")
        if boxes2d.dim() != 3 or boxes2d.shape[1] != N or boxes2d.shape[2] != 4 or boxes2d.shape[0] < 1:
            raise _lib.ObjnerfError("mask_affinity: boxes2d [F, N, 4]")
        F = int(boxes2d.shape[0])
    dev = boxes.device
    W = torch.empty(N, N, dtype=torch.float32, device=dev)
    terms = torch.empty(5, N, N, dtype=torch.float32, device=dev) if want_terms else None
    row_off = torch.empty(N + 1, dtype=torch.int64, device=dev)
    nbytes = int(lib().objnerf_affinity_workspace_bytes(N))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    a = _lib.AffinityArgs(N, F, int(cap.shape[1]), int(clip.shape[1]), wg, wc, wl, wo, w2, _ptr(boxes), _ptr(cap), _ptr(clip),
                          _ptr(color), _ptr(boxes2d) if w2 != 0.0 else None, _ptr(W), _ptr(terms))
    check(lib().objnerf_mask_affinity(C.byref(a), _ptr(ws), nbytes, _ptr(row_off), _stream()), "objnerf_mask_affinity")
    E = int(row_off[-1].item())
    ij = torch.empty(E, 2, dtype=torch.int32, device=dev)
    ew = torch.empty(E, dtype=torch.float32, device=dev)
    if E:
        check(lib().objnerf_mask_edges(N, _ptr(W), _ptr(row_off), E, _ptr(ij), _ptr(ew), _stream()), "objnerf_mask_edges")
    return W, ij, ew, terms


# ---------------------------------------------------------------------------------------------------
# ABI 14: labelling arbitrary points against the whole map (objnerf_mappoints.hip; map_points.MapPoints drives these)
MAPPOINTS_MAX_PAIRS = 2 ** 31 - 1


def mappoints_check_pairs(M: int) -> int:
    """The keys hold a pair in 31 bits (objnerf_mappoints_emit returns EINVAL past that): raise before allocating."""
    if M > MAPPOINTS_MAX_PAIRS:
        raise _lib.ObjnerfError(f"map points: {M} (point, object) pairs do not fit 31 bits; label the cloud in chunks")
    return int(M)


def _csr_count(unit: str, what: str, n: int, K: int, *inputs):
    """objnerf_<unit>_workspace_bytes / _count over n items and K boxes (objnerf_segments.h) -> (seg_off int64 [K + 1] on
    the device, the same as a list, the workspace objnerf_<unit>_emit needs).  The one host sync: seg_off is read back."""
    nbytes = int(getattr(lib(), f"objnerf_{unit}_workspace_bytes")(n, K))
    if nbytes == 0:
        raise _lib.ObjnerfError(f"{unit}_count: {what} = {n}, K = {K} outside the supported range")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=inputs[0].device)
    seg_off = torch.empty(K + 1, dtype=torch.int64, device=inputs[0].device)
    check(getattr(lib(), f"objnerf_{unit}_count")(n, K, *[_ptr(t) for t in inputs], _ptr(ws), nbytes, _ptr(seg_off),
                                                   _stream()), f"objnerf_{unit}_count")
    return seg_off, [int(x) for x in seg_off.tolist()], ws


def _csr_emit(unit: str, n: int, K: int, inputs, ws: torch.Tensor, M: int, outs):
    """objnerf_<unit>_emit into outs (M entries each; no pointer is passed for an empty one)."""
    check(getattr(lib(), f"objnerf_{unit}_emit")(n, K, *[_ptr(t) for t in inputs], _ptr(ws), int(ws.numel()), M,
                                                  *[_ptr(o) if M else None for o in outs], _stream()), f"objnerf_{unit}_emit")
    return outs


def mappoints_count(pts: torch.Tensor, boxes: torch.Tensor):
    """pts [N, 3], boxes [K, 16] (centre | R row-major | extent / 2 | obj_center) -> (seg_off int64 [K + 1] on the device,
    the same as a list, the workspace mappoints_emit needs).  Synchronises once: seg_off is read back, so that the caller
    can decide on M = seg[-1] (allocate, or split the cloud) before anything of that size exists."""
    pts, boxes = _req(pts, torch.float32, "pts"), _req(boxes, torch.float32, "boxes")
    if pts.dim() != 2 or pts.shape[1] != 3 or pts.shape[0] < 1 or boxes.dim() != 2 or boxes.shape[1] != 16 or boxes.shape[0] < 1:
        raise _lib.ObjnerfError("mappoints_count: pts [N >= 1, 3], boxes [K >= 1, 16]")
    return _csr_count("mappoints", "N", int(pts.shape[0]), int(boxes.shape[0]), pts, boxes)


def mappoints_emit(pts: torch.Tensor, boxes: torch.Tensor, ws: torch.Tensor, M: int) -> torch.Tensor:
    """After mappoints_count on the same pts and boxes -> pair_pt int32 [M]: object-major, ascending in the point index
    inside an object."""
    pts, boxes = _req(pts, torch.float32, "pts"), _req(boxes, torch.float32, "boxes")
    M = mappoints_check_pairs(M)
    return _csr_emit("mappoints", int(pts.shape[0]), int(boxes.shape[0]), (pts, boxes), ws, M,
                     (torch.empty(M, dtype=torch.int32, device=pts.device),))[0]


def mappoints_candidates(pts: torch.Tensor, boxes: torch.Tensor):
    """mappoints_count + mappoints_emit -> (seg_off on the device, the same as a list, pair_pt int32 [M])."""
    seg_off, seg, ws = mappoints_count(pts, boxes)
    return seg_off, seg, mappoints_emit(pts, boxes, ws, seg[-1])


def mappoints_eval(arena: ParamArena, pts, boxes, info, seg_off, pair_pt, pair_alpha, pair_color, pair_hfeat, best) -> None:
    """The ragged fused evaluation of the hidden-32 objects (info [K, 2] int32: arena row or -1, background flag); one
    atomicMax per pair into best [N] (int64 storage of the unsigned keys, zeroed by the caller)."""
    net = arena.net.c()
    check(lib().objnerf_mappoints_eval(C.byref(net), int(boxes.shape[0]), int(pts.shape[0]), int(pair_pt.shape[0]),
                                       _ptr(arena.params), arena.p_stride, _ptr(arena.scale), _ptr(pts), _ptr(boxes),
                                       _ptr(info), _ptr(seg_off), _ptr(pair_pt), _ptr(pair_alpha), _ptr(pair_color),
                                       _ptr(pair_hfeat), _ptr(best), _stream()), "objnerf_mappoints_eval")


def mappoints_wide_bytes(arena: ParamArena, n: int, want_feat: bool) -> int:
    """Device bytes mappoints_wide takes for a segment of n pairs of a wide object, beside the pair buffers."""
    if n <= 0:
        return 0
    net = arena.net.c()
    return int(lib().objnerf_eval_workspace_bytes(C.byref(net), 1, n)) + n * (24 + (arena.net.hidden * 4 if want_feat else 0))


def mappoints_wide(arena: ParamArena, pts, pair_pt, pair0: int, n: int, obj_center: float, background: bool, pair_alpha,
                   pair_color, want_feat: bool, best):
    """A wider network (the hidden-128 background) over its contiguous segment [pair0, pair0 + n): gather,
    objnerf_eval_points_ws, merge -- three launch groups whatever n is.  -> its hidden rows [n, H] or None."""
    if n <= 0:
        return None
    dev = pts.device
    gpts = torch.empty(n, 3, device=dev)
    seg_pt = pair_pt[pair0:pair0 + n]
    check(lib().objnerf_mappoints_gather(n, _ptr(seg_pt), _ptr(pts), float(obj_center), _ptr(gpts), _stream()),
          "objnerf_mappoints_gather")
    color = pair_color[pair0:pair0 + n] if pair_color is not None else torch.empty(n, 3, device=dev)
    hfeat = torch.empty(n, arena.net.hidden, device=dev) if want_feat else None
    net = arena.net.c()
    nbytes = int(lib().objnerf_eval_workspace_bytes(C.byref(net), 1, n))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
    check(lib().objnerf_eval_points_ws(C.byref(net), 1, n, _ptr(arena.params), arena.p_stride, _ptr(arena.scale), _ptr(gpts),
                                       _ptr(pair_alpha[pair0:pair0 + n]), _ptr(color), _ptr(hfeat), None, _ptr(ws), nbytes,
                                       _stream()), "objnerf_eval_points_ws")
    check(lib().objnerf_mappoints_merge(n, pair0, _ptr(pair_pt), _ptr(pair_alpha), 1 if background else 0, _ptr(best),
                                        _stream()), "objnerf_mappoints_merge")
    return hfeat


def mappoints_resolve(best, seg_off, pair_color, M: int, want_pair: bool = False):
    """best [N] -> (obj int32 [N] (-1: unlabelled), alpha [N], winning pair int32 [N] | None, colour [N, 3] | None).
    pair_color [M, 3] or None (no colour wanted); M = 0 -- no pair, an empty pair_color -- gives -1, -inf and colour 0."""
    N, K, dev = int(best.shape[0]), int(seg_off.shape[0]) - 1, best.device
    obj = torch.empty(N, dtype=torch.int32, device=dev)
    alpha = torch.empty(N, device=dev)
    pair = torch.empty(N, dtype=torch.int32, device=dev) if want_pair else None
    color = torch.empty(N, 3, device=dev) if pair_color is not None else None
    check(lib().objnerf_mappoints_resolve(N, K, int(M), _ptr(best), _ptr(seg_off), _ptr(pair_color), _ptr(obj), _ptr(alpha),
                                          _ptr(pair), _ptr(color), _stream()), "objnerf_mappoints_resolve")
    return obj, alpha, pair, color


def mappoints_head(best, seg_off, pair_pt, heads, feat_dim: int, out_feat) -> None:
    """out_clip for the winners only, rows written straight to out_feat [N, C] (zeroed by the caller).  heads: per object
    (of_w [C, H], of_b [C], hfeat rows or None, row0, H) -- hfeat None for an object with an empty segment."""
    N, K, M, dev = int(best.shape[0]), int(seg_off.shape[0]) - 1, int(pair_pt.shape[0]), best.device
    if M == 0:
        return
    arr = (_lib.MapPointsHead * K)()
    widths = 0
    for h in heads:
        widths |= {32: 1, 64: 2, 128: 4}.get(int(h[4]), 8)        # OBJNERF_MAPPOINTS_W*
    for k, (of_w, of_b, hfeat, row0, H) in enumerate(heads):
        if H % 32 != 0:
            raise _lib.ObjnerfError(f"mappoints_head: hidden width {H} is not a multiple of 32")
        arr[k] = _lib.MapPointsHead(_ptr(of_w), _ptr(of_b), _ptr(hfeat), int(row0), int(H), 0)
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
    nbytes = int(lib().objnerf_mappoints_head_workspace_bytes(M))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    win_pair = torch.empty(3 * min(N, M), dtype=torch.int32, device=dev)
    check(lib().objnerf_mappoints_head(K, int(feat_dim), N, M, _ptr(best), _ptr(seg_off), _ptr(pair_pt), _ptr(table),
                                       widths, _ptr(ws), nbytes, _ptr(win_pair), _ptr(out_feat), _stream()),
          "objnerf_mappoints_head")


# --------------------------------------------------- field gradients, nearest surface, alignment (objnerf_mapalign.hip)
MAPALIGN_SUMS = 29            # 21 upper entries of J J^T | 6 of J d | sum d^2 | inliers


def _pair_shapes(what: str, pair_pt, pair_alpha, pair_grad) -> int:
    M = int(pair_pt.shape[0])
    if pair_pt.dim() != 1 or tuple(pair_alpha.shape) != (M,) or tuple(pair_grad.shape) != (M, 3):
        raise _lib.ObjnerfError(f"{what}: pair_pt [M], pair_alpha [M], pair_grad [M, 3]; got {tuple(pair_pt.shape)}, "
                                f"{tuple(pair_alpha.shape)}, {tuple(pair_grad.shape)}")
    return M


def mappoints_grad(arena: ParamArena, pts, boxes, info, seg_off, pair_pt, pair_alpha, pair_grad) -> None:
    """The ragged fused field gradient of the hidden-32 objects: pair_alpha [M] = 10 * raw and pair_grad [M, 3] =
    d alpha / d p (world units) for every pair of an object with info [k, 0] >= 0; other pairs are left alone."""
    pts, boxes = _req(pts, torch.float32, "pts"), _req(boxes, torch.float32, "boxes")
    info, seg_off = _req(info, torch.int32, "info"), _req(seg_off, torch.int64, "seg_off")
    pair_pt = _req(pair_pt, torch.int32, "pair_pt")
    for name, t in (("pair_alpha", pair_alpha), ("pair_grad", pair_grad)):
        if _req(t, torch.float32, name) is not t:
            raise _lib.ObjnerfError(f"mappoints_grad: {name} must be contiguous (it is written in place)")
    K = int(boxes.shape[0])
    if pts.dim() != 2 or pts.shape[1] != 3 or pts.shape[0] < 1 or tuple(boxes.shape) != (K, 16) or K < 1 or \
            tuple(info.shape) != (K, 2) or tuple(seg_off.shape) != (K + 1,):
        raise _lib.ObjnerfError("mappoints_grad: pts [N >= 1, 3], boxes [K >= 1, 16], info [K, 2], seg_off [K + 1]")
    M = _pair_shapes("mappoints_grad", pair_pt, pair_alpha, pair_grad)
    net = arena.net.c()
    check(lib().objnerf_mappoints_grad(C.byref(net), K, int(pts.shape[0]), M, _ptr(arena.params), arena.p_stride,
                                       _ptr(arena.scale), _ptr(pts), _ptr(boxes), _ptr(info), _ptr(seg_off),
                                       _ptr(pair_pt) if M else None, _ptr(pair_alpha) if M else None,
                                       _ptr(pair_grad) if M else None, _stream()), "objnerf_mappoints_grad")


def embed_backward_pts(arena: ParamArena, pts: torch.Tensor, d_emb: torch.Tensor) -> torch.Tensor:
    """Backward of UniDirsEmbed.forward (embedding.py:46-55) w.r.t. the positions: pts [K, N, 3], d_emb [K, N, 129] ->
    d_pts [K, N, 3]."""
    pts = _req(pts, torch.float32, "pts")
    if pts.dim() != 3 or pts.shape[2] != 3 or pts.shape[0] != arena.K or pts.shape[1] < 1:
        raise _lib.ObjnerfError(f"embed_backward_pts: pts [{arena.K}, N >= 1, 3], got {tuple(pts.shape)}")
    K, N = int(pts.shape[0]), int(pts.shape[1])
    E = 3 + N_DIRS * arena.net.n_freqs
    if d_emb.numel() != K * N * E:
        raise _lib.ObjnerfError(f"embed_backward_pts: d_emb [{K}, {N}, {E}], got {tuple(d_emb.shape)}")
    d_emb = _req(d_emb.reshape(K, N, E), torch.float32, "d_emb")
    d_pts = torch.empty(K, N, 3, device=pts.device)
    net = arena.net.c()
    check(lib().objnerf_embed_bwd_pts(C.byref(net), K, N, _ptr(arena.params), arena.p_stride, _ptr(arena.scale), _ptr(pts),
                                      _ptr(d_emb), _ptr(d_pts), _stream()), "objnerf_embed_bwd_pts")
    return d_pts


def field_grad_layerwise(arena: ParamArena, pts: torch.Tensor, chunk: int = 1 << 18):
    """alpha [N], d alpha / d p [N, 3] of ONE network of any width at pts [N, 3] (already relative to obj_center) through
    the layer-wise chain objnerf_embed -> objnerf_mlp_forward_ws / objnerf_mlp_backward_ws (d_alpha = 1, d_color = 0) ->
    objnerf_embed_bwd_pts, in chunks of `chunk` points.  The slow path: the hidden-32 objects of a map
    go through mappoints_grad."""
    pts = _req(pts, torch.float32, "pts")
    if arena.K != 1 or pts.dim() != 2 or pts.shape[1] != 3:
        raise _lib.ObjnerfError("field_grad_layerwise: one network, pts [N, 3]")
    n, dev = int(pts.shape[0]), pts.device
    alpha, grad = torch.empty(n, device=dev), torch.empty(n, 3, device=dev)
    for lo in range(0, n, max(int(chunk), 1)):
        p = pts[lo:lo + chunk].reshape(1, -1, 3)
        m = int(p.shape[1])
        emb = embed(arena, p)
        a, _, _, _ = mlp_forward(arena, emb)
        _, d_emb = mlp_backward(arena, emb, torch.ones(1, m, device=dev), torch.zeros(1, m, 3, device=dev))
        alpha[lo:lo + m] = a[0]
        grad[lo:lo + m] = embed_backward_pts(arena, p, d_emb)[0]
    return alpha, grad


def field_grad_layerwise_bytes(arena: ParamArena, n: int, chunk: int = 1 << 18) -> int:
    """Device bytes field_grad_layerwise keeps alive for a segment of n pairs, beside the pair buffers."""
    if n <= 0:
        return 0
    m = min(int(n), int(chunk))
    net = arena.net.c()
    ws = int(lib().objnerf_mlp_backward_workspace_bytes(C.byref(net), 1, m, 0)) + \
        int(lib().objnerf_eval_workspace_bytes(C.byref(net), 1, m))
    return ws + m * 4 * (3 + 2 * 129 + 1 + 3 + 1 + 3 + 3)         # (+ the weight-gradient arena: a constant, not per pair)


def mappoints_gather(pts: torch.Tensor, seg_pt: torch.Tensor, obj_center: float) -> torch.Tensor:
    """pts [seg_pt [i]] - obj_center for a contiguous slice of pair_pt -> [n, 3]."""
    pts, seg_pt = _req(pts, torch.float32, "pts"), _req(seg_pt, torch.int32, "seg_pt")
    n = int(seg_pt.shape[0])
    out = torch.empty(n, 3, device=pts.device)
    if n:
        check(lib().objnerf_mappoints_gather(n, _ptr(seg_pt), _ptr(pts), float(obj_center), _ptr(out), _stream()),
              "objnerf_mappoints_gather")
    return out


def mapalign_select(n_points: int, pair_pt, pair_alpha, pair_grad, g_min: float, best) -> None:
    """One atomicMin per pair into best [N] (int64 storage of the unsigned keys, filled with -1 = all ones by the caller):
    bits 62..31 the bits of |alpha / max(|grad|, g_min)|, bits 30..0 the pair."""
    pair_pt = _req(pair_pt, torch.int32, "pair_pt")
    pair_alpha, pair_grad = _req(pair_alpha, torch.float32, "pair_alpha"), _req(pair_grad, torch.float32, "pair_grad")
    if _req(best, torch.int64, "best") is not best or tuple(best.shape) != (int(n_points),) or n_points < 1:
        raise _lib.ObjnerfError("mapalign_select: best must be a contiguous int64 [N >= 1]")
    if not g_min > 0:
        raise _lib.ObjnerfError(f"mapalign_select: g_min = {g_min}")
    M = _pair_shapes("mapalign_select", pair_pt, pair_alpha, pair_grad)
    check(lib().objnerf_mapalign_select(int(n_points), M, _ptr(pair_pt) if M else None, _ptr(pair_alpha) if M else None,
                                        _ptr(pair_grad) if M else None, float(g_min), _ptr(best), _stream()),
          "objnerf_mapalign_select")


def mapalign_key_encode(d_abs: np.ndarray, pair: np.ndarray) -> np.ndarray:
    """The key objnerf_mapalign_select offers (host side, for tests and tools): uint64."""
    bits = np.ascontiguousarray(np.abs(d_abs), np.float32).view(np.uint32).astype(np.uint64)
    return (bits << np.uint64(31)) | np.asarray(pair, np.uint64)


def mapalign_key_decode(key: np.ndarray):
    """-> (|d| fp32, pair int64; -1 for the caller's fill)."""
    key = np.asarray(key).astype(np.uint64)
    free = (key >> np.uint64(63)) != 0
    d = ((key >> np.uint64(31)) & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.float32)
    pair = (key & np.uint64(0x7FFFFFFF)).astype(np.int64)
    return np.where(free, np.float32(np.inf), d), np.where(free, -1, pair)


def mapalign_resolve(best, seg_off, pair_alpha, pair_grad, g_min: float, want_pair: bool = False):
    """best [N] -> (obj int32 [N] (-1: in no box), pair int32 [N] | None, d [N] (+inf), alpha [N], grad [N, 3] (0))."""
    best, seg_off = _req(best, torch.int64, "best"), _req(seg_off, torch.int64, "seg_off")
    pair_alpha, pair_grad = _req(pair_alpha, torch.float32, "pair_alpha"), _req(pair_grad, torch.float32, "pair_grad")
    N, K, M, dev = int(best.shape[0]), int(seg_off.shape[0]) - 1, int(pair_alpha.shape[0]), best.device
    if best.dim() != 1 or N < 1 or K < 1 or tuple(pair_grad.shape) != (M, 3):
        raise _lib.ObjnerfError("mapalign_resolve: best [N >= 1], seg_off [K + 1], pair_alpha [M], pair_grad [M, 3]")
    obj = torch.empty(N, dtype=torch.int32, device=dev)
    pair = torch.empty(N, dtype=torch.int32, device=dev) if want_pair else None
    d, alpha, grad = torch.empty(N, device=dev), torch.empty(N, device=dev), torch.empty(N, 3, device=dev)
    check(lib().objnerf_mapalign_resolve(N, K, M, _ptr(best), _ptr(seg_off), _ptr(pair_alpha) if M else None,
                                         _ptr(pair_grad) if M else None, float(g_min), _ptr(obj), _ptr(pair), _ptr(d),
                                         _ptr(alpha), _ptr(grad), _stream()), "objnerf_mapalign_resolve")
    return obj, pair, d, alpha, grad


def mapalign_transform(pts: torch.Tensor, T) -> torch.Tensor:
    """float32(R p + t) for pts [N, 3] fp32 and a 4 x 4 (or 3 x 4) host matrix T, formed in fp64 on the device."""
    pts = _req(pts, torch.float32, "pts")
    if pts.dim() != 2 or pts.shape[1] != 3 or pts.shape[0] < 1:
        raise _lib.ObjnerfError(f"mapalign_transform: pts [N >= 1, 3], got {tuple(pts.shape)}")
    rows = np.asarray(T, np.float64)[:3, :4].reshape(-1)
    if rows.shape != (12,) or not np.isfinite(rows).all():
        raise _lib.ObjnerfError("mapalign_transform: T must be a finite 4 x 4 matrix")
    out = torch.empty_like(pts)
    check(lib().objnerf_mapalign_transform(int(pts.shape[0]), _ptr(pts), (C.c_double * 12)(*rows.tolist()), _ptr(out),
                                           _stream()), "objnerf_mapalign_transform")
    return out


def mapalign_accumulate(pts, obj, alpha, grad, pivot, tau: float, g_min: float, out=None) -> torch.Tensor:
    """-> 29 doubles on the device: over the points with obj >= 0 and |d| <= tau the 21 upper entries of sum J J^T, the 6
    of sum J d, sum d^2 and the inlier count; J = [(q - pivot) x n, n], everything in fp64 from the fp32 values.  The
    order of every sum depends on N alone."""
    pts, obj = _req(pts, torch.float32, "pts"), _req(obj, torch.int32, "obj")
    alpha, grad = _req(alpha, torch.float32, "alpha"), _req(grad, torch.float32, "grad")
    N, dev = int(pts.shape[0]), pts.device
    if pts.dim() != 2 or pts.shape[1] != 3 or N < 1 or tuple(obj.shape) != (N,) or tuple(alpha.shape) != (N,) or \
            tuple(grad.shape) != (N, 3):
        raise _lib.ObjnerfError("mapalign_accumulate: pts [N >= 1, 3], obj [N], alpha [N], grad [N, 3]")
    if not (g_min > 0 and tau >= 0):
        raise _lib.ObjnerfError(f"mapalign_accumulate: tau = {tau}, g_min = {g_min}")
    piv = (C.c_double * 3)(*[float(x) for x in pivot])
    nbytes = int(lib().objnerf_mapalign_workspace_bytes(N))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if out is None:
        out = torch.empty(MAPALIGN_SUMS, dtype=torch.float64, device=dev)
    check(lib().objnerf_mapalign_accumulate(N, _ptr(pts), _ptr(obj), _ptr(alpha), _ptr(grad), piv, float(tau), float(g_min),
                                            _ptr(ws), nbytes, _ptr(out), _stream()), "objnerf_mapalign_accumulate")
    return out


# ------------------------------------------------------------------------- geometry evaluation (objnerf_mapeval.hip)
NEAREST_CELL_FACTOR = 1.0       # cell side = this x the typical sample spacing (profiles/mapeval_bench.txt)
_MESH_STATUS = ((1, "a face names a vertex outside [0, V)"), (2, "a face has a non-finite area"),
                (4, "a segment asks for samples but has no area"))


def _offsets(off, total: int, name: str) -> torch.Tensor:
    off = torch.as_tensor(off, dtype=torch.int64).cpu()
    if off.dim() != 1 or off.numel() < 2 or int(off[0]) != 0 or int(off[-1]) != total or bool((off[1:] < off[:-1]).any()):
        raise _lib.ObjnerfError(f"{name}: offsets must rise from 0 to {total}")
    return off


def mesh_sample(verts: torch.Tensor, faces: torch.Tensor, face_off, samp_off, seed: int = 0, out=None):
    """objnerf_mesh_sample: area-weighted points on S meshes stored back to back -> (pts fp64 [N, 3], tri int32 [N] = the
    global face row).  verts fp64 [V, 3], faces int32 [F, 3] (global vertex rows), face_off / samp_off [S + 1].  Sample i
    of mesh s depends on (seed, s, i) only.  out: (pts, tri) to write into."""
    verts = _req(verts, torch.float64, "mesh_sample: verts")
    faces = _req(faces, torch.int32, "mesh_sample: faces")
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise _lib.ObjnerfError("mesh_sample: expected verts [V, 3] and faces [F, 3]")
    V, F, dev = int(verts.shape[0]), int(faces.shape[0]), verts.device
    if faces.device != dev:
        raise _lib.ObjnerfError("mesh_sample: verts and faces on different devices")
    foff = _offsets(face_off, F, "mesh_sample: face_off")
    S = foff.numel() - 1
    soff = torch.as_tensor(samp_off, dtype=torch.int64).cpu()
    if soff.numel() != S + 1:
        raise _lib.ObjnerfError("mesh_sample: face_off and samp_off must have one entry per mesh, plus one")
    N = int(soff[-1]) if soff.numel() else 0
    soff = _offsets(soff, N, "mesh_sample: samp_off")
    if max(V, F, N) >= 2 ** 31:
        raise _lib.ObjnerfError("mesh_sample: at most 2^31 - 1 vertices, faces and samples")
    if out is None:
        pts = torch.empty(N, 3, dtype=torch.float64, device=dev)
        tri = torch.empty(N, dtype=torch.int32, device=dev)
    else:
        pts, tri = _req(out[0], torch.float64, "mesh_sample: out pts"), _req(out[1], torch.int32, "mesh_sample: out tri")
        if tuple(pts.shape) != (N, 3) or tuple(tri.shape) != (N,) or pts is not out[0] or tri is not out[1]:
            raise _lib.ObjnerfError("mesh_sample: out must be contiguous (pts [N, 3], tri [N])")
    nbytes = int(lib().objnerf_mesh_sample_workspace_bytes(F, S))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    foff_dev, soff_dev = foff.to(dev), soff.to(dev)          # (held in names: a temporary's block is reused by the next)
    check(lib().objnerf_mesh_sample(V, F, S, N, _ptr(verts) if V else None, _ptr(faces) if F else None, _ptr(foff_dev),
                                    _ptr(soff_dev), int(seed) & (2 ** 64 - 1), _ptr(ws), nbytes,
                                    _ptr(pts) if N else None, _ptr(tri) if N else None, _ptr(status), _stream()),
          "objnerf_mesh_sample")
    st = int(status.item())
    if st:
        raise _lib.ObjnerfError("mesh_sample: " + "; ".join(msg for bit, msg in _MESH_STATUS if st & bit))
    return pts, tri


class NearestPlan:
    """The sorted cell keys of S reference point sets: query() then finds exact nearest points for any number of query
    sets.  cell: the grid's cell side (any value > 0 gives the same result; it decides the speed only); None: taken
    from the sets' extents and counts as NEAREST_CELL_FACTOR x the spacing of that many points spread over the surface
    of each set's box (the median over the sets)."""

    def __init__(self, ref: torch.Tensor, r_off, cell: Optional[float] = None):
        self.ref, self.off, self.n = _point_sets(ref, r_off, "nearest: ref")
        self.S = self.off.numel() - 1
        self.dev = self.ref.device
        self.off_dev = self.off.to(self.dev)
        self.keys = self.perm = None
        self.mins = torch.zeros(self.S, 3, dtype=torch.float64, device=self.dev)
        self.cell = float(cell) if cell is not None else (self._auto_cell() if self.n else 1.0)
        if not (self.cell > 0.0 and np.isfinite(self.cell)):
            raise _lib.ObjnerfError("nearest: cell must be positive")
        if self.n:
            keys, self.mins = cell_keys(self.ref, self.off, self.cell, 0.0, "nearest: ref")
            self.keys, self.perm = _sort_in_segments(keys, self.off, self.dev)

    def _auto_cell(self) -> float:
        b = point_bounds(self.ref, self.off).cpu().numpy()
        cnt = (self.off[1:] - self.off[:-1]).numpy().astype(np.float64)
        ok = cnt > 0
        if not np.isfinite(b[ok]).all():
            raise _lib.ObjnerfError("nearest: ref: a point is not finite")
        e = b[ok, 3:] - b[ok, :3]
        area = 2.0 * (e[:, 0] * e[:, 1] + e[:, 1] * e[:, 2] + e[:, 2] * e[:, 0])
        spacing = np.sqrt(area / cnt[ok])
        spacing = spacing[spacing > 0]
        cell = NEAREST_CELL_FACTOR * float(np.median(spacing)) if spacing.size else 1.0
        return max(cell, float(e.max()) / 2.0 ** 20, float(np.finfo(np.float64).tiny))

    def query(self, qry: torch.Tensor, q_off, max_rings: int = 0, out=None):
        """objnerf_nearest -> (d2 fp64 [nq] = the smallest squared distance to a reference point of the same segment,
        idx int64 [nq] = the smallest row of ref that attains it; +inf and -1 for an empty reference segment).
        max_rings: the last ring of cells the per-query search visits before brute force takes over (0 = the library's
        default; the result does not depend on it); out: (d2, idx) to write into."""
        qry, qoff, nq = _point_sets(qry, q_off, "nearest: qry")
        if qoff.numel() != self.S + 1:
            raise _lib.ObjnerfError("nearest: ref and qry must have the same number of segments")
        if qry.device != self.dev:
            raise _lib.ObjnerfError("nearest: ref and qry on different devices")
        if out is None:
            d2 = torch.empty(nq, dtype=torch.float64, device=self.dev)
            idx = torch.empty(nq, dtype=torch.int64, device=self.dev)
        else:
            d2, idx = _req(out[0], torch.float64, "nearest: out d2"), _req(out[1], torch.int64, "nearest: out idx")
            if tuple(d2.shape) != (nq,) or tuple(idx.shape) != (nq,) or d2 is not out[0] or idx is not out[1]:
                raise _lib.ObjnerfError("nearest: out must be contiguous (d2 [nq], idx [nq])")
        if nq == 0:
            return d2, idx
        qoff_dev = qoff.to(self.dev)
        nbytes = int(lib().objnerf_nearest_workspace_bytes(nq, self.S))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        status = torch.empty(1, dtype=torch.int32, device=self.dev)
        check(lib().objnerf_nearest(self.n, nq, self.S, _ptr(self.ref) if self.n else None, _ptr(self.off_dev),
                                    _ptr(self.keys), _ptr(self.perm), _ptr(self.mins), self.cell, _ptr(qry), _ptr(qoff_dev),
                                    int(max_rings), _ptr(ws), nbytes, _ptr(d2), _ptr(idx), _ptr(status), _stream()),
              "objnerf_nearest")
        if int(status.item()) != 0:
            raise _lib.ObjnerfError("nearest: a query point is not finite")
        return d2, idx


def nearest(qry: torch.Tensor, q_off, ref: torch.Tensor, r_off, cell: Optional[float] = None):
    """For every query point of segment s the nearest point of reference segment s -> (d2, idx); see NearestPlan."""
    _req(qry, torch.float64, "nearest: qry")
    return NearestPlan(ref, r_off, cell).query(qry, q_off)


def seg_stats(d: torch.Tensor, off, thresholds=(), out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """objnerf_seg_stats -> fp64 [S, 5 + T]: per segment of d (fp64 [n]) the number of finite entries, of non-finite
    ones, the sum, the sum of squares and the maximum of the finite ones, then the number of finite d < thr per threshold
    (at most 4).  Summed in a fixed order: two calls give the same bits.  out: the tensor to write into."""
    d = _req(d, torch.float64, "seg_stats: d")
    if d.dim() != 1:
        raise _lib.ObjnerfError("seg_stats: expected d [n]")
    n, dev = int(d.shape[0]), d.device
    o = _offsets(off, n, "seg_stats: off")
    thr = [float(t) for t in thresholds]
    if len(thr) > 4:
        raise _lib.ObjnerfError("seg_stats: at most 4 thresholds")
    S = o.numel() - 1
    if out is None:
        out = torch.empty(S, 5 + len(thr), dtype=torch.float64, device=dev)
    elif _req(out, torch.float64, "seg_stats: out") is not out or tuple(out.shape) != (S, 5 + len(thr)):
        raise _lib.ObjnerfError("seg_stats: out must be contiguous [S, 5 + T]")
    arr = (C.c_double * max(len(thr), 1))(*thr)
    off_dev = o.to(dev)
    check(lib().objnerf_seg_stats(n, S, _ptr(d) if n else None, _ptr(off_dev), len(thr), arr, _ptr(out), _stream()),
          "objnerf_seg_stats")
    return out


# ------------------------------------------------------------------------- culling meshes to what the frames observed
VIEWS_MAX_BATCH = 256           # frames per objnerf_vertex_views call; longer batches are chunked
_CULL_RULES = {"all": 0, "any": 1}      # OBJNERF_CULL_ALL / OBJNERF_CULL_ANY


def vertex_views(verts: torch.Tensor, T_CW: torch.Tensor, depth: torch.Tensor, intrinsics, z_min: float = 0.0,
                 eps: float = 0.05, margin: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """objnerf_vertex_views: the number of frames that see each vertex -> int32 [V].  verts fp64 [V, 3]
    (world), T_CW fp64 [B, 3, 4] = the upper rows of inverse(T_WC) per frame, depth fp32 [B, W, H] (metres, 0 = invalid),
    intrinsics (fx, fy, cx, cy).  out: an int32 [V] tensor the counts are ADDED to (the caller zeroes it once and streams
    a sequence through in batches); None: a fresh zeroed one."""
    verts = _req(verts, torch.float64, "vertex_views: verts")
    T_CW = _req(T_CW, torch.float64, "vertex_views: T_CW")
    depth = _req(depth, torch.float32, "vertex_views: depth")
    if verts.dim() != 2 or verts.shape[1] != 3:
        raise _lib.ObjnerfError("vertex_views: expected verts [V, 3]")
    if T_CW.dim() != 3 or tuple(T_CW.shape[1:]) != (3, 4):
        raise _lib.ObjnerfError("vertex_views: expected T_CW [B, 3, 4]")
    if depth.dim() != 3 or depth.shape[0] != T_CW.shape[0] or depth.shape[1] < 1 or depth.shape[2] < 1:
        raise _lib.ObjnerfError("vertex_views: expected depth [B, W, H] with one image per pose")
    V, B, W, H, dev = int(verts.shape[0]), int(T_CW.shape[0]), int(depth.shape[1]), int(depth.shape[2]), verts.device
    if T_CW.device != dev or depth.device != dev:
        raise _lib.ObjnerfError("vertex_views: verts, T_CW and depth on different devices")
    if V >= 2 ** 31 or W >= 2 ** 31 or H >= 2 ** 31:
        raise _lib.ObjnerfError("vertex_views: at most 2^31 - 1 vertices, columns and rows")
    fx, fy, cx, cy = (float(x) for x in intrinsics)
    margin = int(margin)
    if margin < 0:
        raise _lib.ObjnerfError("vertex_views: margin must not be negative")
    if out is None:
        out = torch.zeros(V, dtype=torch.int32, device=dev)
    elif _req(out, torch.int32, "vertex_views: out") is not out or tuple(out.shape) != (V,) or out.device != dev:
        raise _lib.ObjnerfError("vertex_views: out must be contiguous int32 [V] on the vertices' device")
    for b0 in range(0, B, VIEWS_MAX_BATCH):
        b1 = min(B, b0 + VIEWS_MAX_BATCH)
        check(lib().objnerf_vertex_views(V, b1 - b0, W, H, _ptr(verts) if V else None, _ptr(T_CW[b0:b1]),
                                         _ptr(depth[b0:b1]), fx, fy, cx, cy, float(z_min), float(eps), margin,
                                         _ptr(out) if V else None, _stream()), "objnerf_vertex_views")
    return out


def mesh_compact(keep_v: torch.Tensor, faces: torch.Tensor, rule: str = "all", out=None) -> Dict[str, torch.Tensor]:
    """objnerf_mesh_cull_count / _emit: the sub-mesh a vertex mask keeps.  keep_v uint8 or bool [V], faces int32 [F, 3];
    rule "all": a face stays iff its three corners are kept, "any": iff at least one is.  -> {"new_of_old" int32 [V]
    (-1 = dropped), "old_of_new" int32 [Vn], "faces" int32 [Fn, 3] re-indexed, "face_old" int32 [Fn]}: the kept faces
    in their original order and exactly the vertices they use, in ascending original order.  Raises if a face names a
    vertex outside [0, V).  Synchronises the stream once (the two totals are read back to size the outputs).
    out: a dict of the four tensors to write into (their sizes must be the counted ones)."""
    if rule not in _CULL_RULES:
        raise ValueError(f"mesh_compact: rule {rule!r}: 'all' or 'any' expected")
    if keep_v.dtype == torch.bool and keep_v.is_cuda:
        keep_v = keep_v.contiguous().view(torch.uint8)
    keep_v = _req(keep_v, torch.uint8, "mesh_compact: keep_v")
    faces = _req(faces, torch.int32, "mesh_compact: faces")
    if keep_v.dim() != 1 or faces.dim() != 2 or faces.shape[1] != 3:
        raise _lib.ObjnerfError("mesh_compact: expected keep_v [V] and faces [F, 3]")
    V, F, dev, r = int(keep_v.shape[0]), int(faces.shape[0]), keep_v.device, _CULL_RULES[rule]
    if faces.device != dev:
        raise _lib.ObjnerfError("mesh_compact: keep_v and faces on different devices")
    if max(V, F) >= 2 ** 31:
        raise _lib.ObjnerfError("mesh_compact: at most 2^31 - 1 vertices and faces")
    nbytes = int(lib().objnerf_mesh_cull_workspace_bytes(V, F))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    kp, fp = _ptr(keep_v) if V else None, _ptr(faces) if F else None
    check(lib().objnerf_mesh_cull_count(V, F, r, kp, fp, _ptr(ws), nbytes, _ptr(counts), _ptr(status), _stream()),
          "objnerf_mesh_cull_count")
    Vn, Fn = (int(x) for x in counts.tolist())                # the one host sync
    if int(status.item()):
        raise _lib.ObjnerfError("mesh_compact: a face names a vertex outside [0, V)")
    shapes = {"new_of_old": (V,), "old_of_new": (Vn,), "faces": (Fn, 3), "face_old": (Fn,)}
    if out is None:
        res = {k: torch.empty(s, dtype=torch.int32, device=dev) for k, s in shapes.items()}
    else:
        res = {k: out[k] for k in shapes}
        for k, s in shapes.items():
            if _req(res[k], torch.int32, f"mesh_compact: out {k}") is not res[k] or tuple(res[k].shape) != s or res[k].device != dev:
                raise _lib.ObjnerfError(f"mesh_compact: out[{k!r}] must be contiguous int32 {list(s)}")
    p = {k: (_ptr(t) if t.numel() else None) for k, t in res.items()}
    check(lib().objnerf_mesh_cull_emit(V, F, r, kp, fp, _ptr(ws), nbytes, Vn, Fn, p["new_of_old"], p["old_of_new"],
                                       p["faces"], p["face_old"], _stream()), "objnerf_mesh_cull_emit")
    return res


# ------------------------------------------------------------- a novel view of the whole map (objnerf_mapview.hip)
# additive under ABI 14; map_view.MapView drives these
VIEW_MAX_ENTRIES = 2 ** 32 - 1          # the merge keys hold an entry of the CSR in 32 bits
VIEW_TILE_GROUPS = 4                    # 16-ray groups per tile of render_fwd_segmented: one per wave of a workgroup


def _view_inputs(T_WC, boxes, dirs_C, name):
    dirs_C, boxes = _req(dirs_C, torch.float32, f"{name}: dirs_C"), _req(boxes, torch.float32, f"{name}: boxes")
    if dirs_C.dim() != 2 or dirs_C.shape[1] != 3 or dirs_C.shape[0] < 1 or boxes.dim() != 2 or boxes.shape[1] != 16 or \
            boxes.shape[0] < 1:
        raise _lib.ObjnerfError(f"{name}: dirs_C [P >= 1, 3], boxes [K >= 1, 16]")
    T_WC = _req(T_WC, torch.float32, f"{name}: T_WC")
    if tuple(T_WC.shape) != (4, 4) or T_WC.device != dirs_C.device or boxes.device != dirs_C.device:
        raise _lib.ObjnerfError(f"{name}: T_WC [4, 4], on the device of dirs_C and boxes")
    return T_WC, boxes, dirs_C


def view_rays_count(T_WC: torch.Tensor, boxes: torch.Tensor, dirs_C: torch.Tensor):
    """The camera rays dirs_C [P, 3] (p = w * H + h) of one view against K boxes at once.  boxes [K, 16]: T_OC rows 0..2 |
    extent / 2 | unused (map_view.view_box_record).  -> (seg_off int64 [K + 1] on the device, the same as a list, the
    workspace view_rays_emit needs); an object with at most one hit has an empty segment.  Synchronises once: seg_off is
    read back, so that the outputs of M = seg[-1] entries can be allocated to their exact size."""
    T_WC, boxes, dirs_C = _view_inputs(T_WC, boxes, dirs_C, "view_rays_count")
    return _csr_count("view_rays", "P", int(dirs_C.shape[0]), int(boxes.shape[0]), T_WC, boxes, dirs_C)


def view_rays_emit(T_WC: torch.Tensor, boxes: torch.Tensor, dirs_C: torch.Tensor, ws: torch.Tensor, M: int):
    """After view_rays_count on the same inputs -> (pix int32 [M], dirs_W [M, 3], near [M], far [M]): object-major,
    ascending in the pixel inside an object; per entry the numbers ops.box_rays gives that (pixel, box)."""
    T_WC, boxes, dirs_C = _view_inputs(T_WC, boxes, dirs_C, "view_rays_emit")
    M = int(M)
    if M > VIEW_MAX_ENTRIES:
        raise _lib.ObjnerfError(f"view_rays_emit: {M} (pixel, object) entries do not fit 32 bits")
    dev = dirs_C.device
    return _csr_emit("view_rays", int(dirs_C.shape[0]), int(boxes.shape[0]), (T_WC, boxes, dirs_C), ws, M,
                     (torch.empty(M, dtype=torch.int32, device=dev), torch.empty(M, 3, device=dev),
                      torch.empty(M, device=dev), torch.empty(M, device=dev)))


def render_tiles(rows, tile_groups: int = VIEW_TILE_GROUPS) -> np.ndarray:
    """The work list of render_fwd_segmented.  rows: (arena row, rays of its segment) in the order to render.  -> int32
    [T, 3]: arena row, first 16-ray group counted from the segment's start, groups (<= tile_groups).  Every group of
    every segment is in exactly one tile, a tile belongs to one row, the tiles of a row are adjacent and ascending; an
    empty segment has no tile."""
    tile_groups = int(tile_groups)
    if tile_groups < 1:
        raise ValueError(f"render_tiles: tile_groups = {tile_groups}")
    parts = []
    for row, n in rows:
        groups = (int(n) + 15) // 16
        if groups <= 0:
            continue
        first = np.arange(0, groups, tile_groups, dtype=np.int64)
        t = np.empty((first.shape[0], 3), np.int64)
        t[:, 0], t[:, 1], t[:, 2] = int(row), first, np.minimum(tile_groups, groups - first)
        parts.append(t)
    if not parts:
        return np.zeros((0, 3), np.int32)
    tiles = np.concatenate(parts)
    if tiles.max() >= 2 ** 31:
        raise _lib.ObjnerfError("render_tiles: a tile field does not fit 32 bits")
    return tiles.astype(np.int32)


def render_fwd_segmented(arena: ParamArena, origin: torch.Tensor, dirs_W: torch.Tensor, near: torch.Tensor,
                         far: torch.Tensor, rows, u: Optional[torch.Tensor] = None, n_bins: int = 150,
                         seed: Optional[int] = None, out=None, _workgroups: int = 0, want_hfeat: bool = False):
    """ops.render_fwd (fp32, no feature hidden unless want_hfeat) over the segments of several hidden-32 objects in ONE
    launch (objnerf_render_fwd_segmented).  arena: the stacked arena of those objects; dirs_W [M, 3], near, far [M]: the CSR of
    view_rays_emit; rows: per object to render (arena row, seg_lo, seg_hi, u_lo, draw) -- its entries of the CSR, the row
    of u [*, n_bins] its first ray reads (None or < 0: drawn in the kernel under (seed, draw)), the Philox draw counter.
    -> dict(depth [M], opacity [M], rgb [M, 3]) (`out`: write into these); entries outside the rows' segments are left
    as they are.  Per entry bit-equal to ops.render_fwd on the object's own rays.  _workgroups: internal, the number of
    persistent workgroups (0: two per compute unit).  want_hfeat: also "hfeat" [M, 32], the composited feature hidden
    (render_fwd's "vals") of every rendered entry, through objnerf_render_fwd_segmented_feat; the other three outputs
    keep their bits."""
    if arena.net.hidden != 32:
        raise ObjnerfError("render_fwd_segmented: a stacked arena of hidden-32 objects")
    dirs_W = _req(dirs_W, torch.float32, "dirs_W")
    near, far = _req(near, torch.float32, "near"), _req(far, torch.float32, "far")
    dev, M = dirs_W.device, int(near.shape[0])
    if tuple(dirs_W.shape) != (M, 3) or int(far.shape[0]) != M or M > VIEW_MAX_ENTRIES:
        raise ObjnerfError("render_fwd_segmented: dirs_W [M, 3], near [M], far [M], M < 2^32")
    u_rows = 0
    if u is not None:
        u = _req(u, torch.float32, "u")
        if u.dim() != 2 or int(u.shape[1]) != int(n_bins):
            raise ObjnerfError(f"render_fwd_segmented: u [*, {n_bins}], got {tuple(u.shape)}")
        u_rows = int(u.shape[0])
    table = np.zeros((arena.K, 4), np.int64)
    table[:, 2] = -1
    work = []
    for row, lo, hi, u_lo, draw in rows:
        row, lo, hi = int(row), int(lo), int(hi)
        u_lo = -1 if (u_lo is None or u is None) else int(u_lo)
        if not (0 <= row < arena.K) or not (0 <= lo <= hi <= M) or (u_lo >= 0 and u_lo + hi - lo > u_rows):
            raise ObjnerfError(f"render_fwd_segmented: row {row} [{lo}, {hi}) u_lo {u_lo} outside the arena, the CSR or u")
        table[row] = (lo, hi, u_lo, int(draw) & 0x1FFFFFFF)
        work.append((row, hi - lo))
    if len(set(r for r, _ in work)) != len(work):
        raise ObjnerfError("render_fwd_segmented: an arena row is listed twice")
    tiles = render_tiles(work)
    if out is None:
        out = {"depth": torch.empty(M, device=dev), "opacity": torch.empty(M, device=dev), "rgb": torch.empty(M, 3, device=dev)}
    if want_hfeat and "hfeat" not in out:
        out["hfeat"] = torch.empty(M, 32, device=dev)
    for k, shp in (("depth", (M,)), ("opacity", (M,)), ("rgb", (M, 3))) + ((("hfeat", (M, 32)),) if want_hfeat else ()):
        if _req(out[k], torch.float32, f"out {k}") is not out[k] or tuple(out[k].shape) != shp or out[k].device != dev:
            raise ObjnerfError(f"render_fwd_segmented: out[{k!r}] must be contiguous fp32 {list(shp)}")
    if tiles.shape[0] == 0 or M == 0:
        return out
    origin = origin.to(dev, torch.float32).contiguous()
    table_d, tiles_d = torch.from_numpy(table).to(dev), torch.from_numpy(tiles).to(dev)
    net = arena.net.c()
    if want_hfeat:
        check(lib().objnerf_render_fwd_segmented_feat(C.byref(net), arena.K, int(tiles.shape[0]), int(n_bins), M,
                                                      _ptr(arena.params), arena.p_stride, _ptr(arena.scale), _ptr(origin),
                                                      _ptr(table_d), _ptr(tiles_d), _ptr(dirs_W), _ptr(near), _ptr(far),
                                                      _ptr(u), u_rows, _seed_of(seed), _ptr(out["depth"]),
                                                      _ptr(out["opacity"]), _ptr(out["rgb"]), _ptr(out["hfeat"]),
                                                      int(_workgroups), _stream()), "objnerf_render_fwd_segmented_feat")
        return out
    check(lib().objnerf_render_fwd_segmented(C.byref(net), arena.K, int(tiles.shape[0]), int(n_bins), M, _ptr(arena.params),
                                             arena.p_stride, _ptr(arena.scale), _ptr(origin), _ptr(table_d), _ptr(tiles_d),
                                             _ptr(dirs_W), _ptr(near), _ptr(far), _ptr(u), u_rows, _seed_of(seed),
                                             _ptr(out["depth"]), _ptr(out["opacity"]), _ptr(out["rgb"]), int(_workgroups),
                                             _stream()), "objnerf_render_fwd_segmented")
    return out


def view_merge(seg_off: torch.Tensor, pix, depth, opacity, rgb, near, far, info: torch.Tensor, P: int,
               any_background: Optional[bool] = None):
    """The z-buffer merge of train.py:581-598 in closed form over the CSR of a view (objnerf_view_merge).  info [K, 2]
    int32: background flag, the id written into the mask-id image.  -> dict(rgb uint8 [P, 3], maskid int32 [P] (0 =
    nothing painted), depth [P] (100 = no foreground), winner int32 [P] (the painter's entry, -1 = none)).
    any_background: whether info flags any object (None: read from info, which synchronises); False skips launch (b)."""
    seg_off, info = _req(seg_off, torch.int64, "seg_off"), _req(info, torch.int32, "info")
    K, dev, M, P = int(seg_off.shape[0]) - 1, seg_off.device, int(depth.shape[0]), int(P)
    if tuple(info.shape) != (K, 2) or M > VIEW_MAX_ENTRIES:
        raise ObjnerfError("view_merge: info [K, 2], M < 2^32")
    pix = _req(pix, torch.int32, "pix")
    depth, opacity, rgb = _req(depth, torch.float32, "depth"), _req(opacity, torch.float32, "opacity"), _req(rgb, torch.float32, "rgb")
    near, far = _req(near, torch.float32, "near"), _req(far, torch.float32, "far")
    if any(int(t.shape[0]) != M for t in (pix, opacity, rgb, near, far)) or tuple(rgb.shape) != (M, 3):
        raise ObjnerfError("view_merge: pix, depth, opacity, near, far [M], rgb [M, 3]")
    best_fg = torch.empty(P, dtype=torch.int64, device=dev)
    best_bg = torch.empty(P, dtype=torch.int32, device=dev)
    out = {"rgb": torch.empty(P, 3, dtype=torch.uint8, device=dev), "maskid": torch.empty(P, dtype=torch.int32, device=dev),
           "depth": torch.empty(P, device=dev), "winner": torch.empty(P, dtype=torch.int32, device=dev)}
    if any_background is None:
        any_background = bool(info[:, 0].any())
    p = (lambda t: _ptr(t) if M else None)
    check(lib().objnerf_view_merge(P, K, M, _ptr(seg_off), p(pix), p(depth), p(opacity), p(rgb), p(near), p(far), _ptr(info),
                                   1 if any_background else 0, _ptr(best_fg), _ptr(best_bg), _ptr(out["rgb"]),
                                   _ptr(out["maskid"]), _ptr(out["depth"]), _ptr(out["winner"]), _stream()),
          "objnerf_view_merge")
    return out


VIEW_QUERY_MAX = 16                     # queries per objnerf_view_query launch (one MFMA tile of dot products)


def _view_heads(heads, C_: int, dev):
    """heads: per object (of_w [C, H], of_b [C], hfeat [n_rows, H] | None, row0) -> (the ctypes array, its device copy)."""
    arr = (_lib.ViewHead * len(heads))()
    for k, (of_w, of_b, hfeat, row0) in enumerate(heads):
        of_w, of_b = _req(of_w, torch.float32, f"heads[{k}] of_w"), _req(of_b, torch.float32, f"heads[{k}] of_b")
        H = int(of_w.shape[1]) if of_w.dim() == 2 else 0
        if of_w.dim() != 2 or int(of_w.shape[0]) != C_ or tuple(of_b.shape) != (C_,):
            raise ObjnerfError(f"view_query: heads[{k}]: of_w [{C_}, H], of_b [{C_}]")
        if hfeat is not None:
            hfeat = _req(hfeat, torch.float32, f"heads[{k}] hfeat")
            if hfeat.dim() != 2 or int(hfeat.shape[1]) != H:
                raise ObjnerfError(f"view_query: heads[{k}]: hfeat [n_rows, {H}], got {tuple(hfeat.shape)}")
        if of_w.device != dev or of_b.device != dev or (hfeat is not None and hfeat.device != dev):
            raise ObjnerfError(f"view_query: heads[{k}] is not on {dev}")
        heads[k] = (of_w, of_b, hfeat, row0)                     # (keeps a contiguous copy alive through the call)
        arr[k] = _lib.ViewHead(_ptr(of_w), _ptr(of_b), _ptr(hfeat) if hfeat is not None and hfeat.numel() else None,
                               int(row0), int(hfeat.shape[0]) if hfeat is not None else 0, H, 0)
    return arr, torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)


def view_query(seg_off: torch.Tensor, pix: torch.Tensor, opacity: torch.Tensor, winner: torch.Tensor, heads,
               queries: Optional[torch.Tensor] = None, pixels: Optional[torch.Tensor] = None, want_sims: bool = True,
               want_best: bool = True, _workgroups: int = 0) -> Dict[str, Optional[torch.Tensor]]:
    """The part feature F = of_w . h + of_b * opacity of the entry that painted each pixel of a merged view, never stored
    densely (objnerf_view_query).  seg_off [K + 1], pix [M], opacity [M]: the CSR of the view; winner int32 [P] from
    view_merge; heads: per object (of_w [C, H], of_b [C], hfeat [n_rows, H] | None, row0) -- hfeat row (entry - row0) is
    the composited feature hidden of that entry, None = the object serves nothing; H a multiple of 32, mixed in one call;
    the three tensors 16-byte aligned.
    queries [Q, C], 1 <= Q <= 16, unit length (the caller normalises) -> "sims" [Q, P] (want_sims), "label" int32 [P]
    (the first arg-max), "best" [P] (want_best); NaN / -1 where nothing painted.
    pixels int [n] (p = w * H + h) -> "feat" [n, C], the raw F; zeros for a pixel out of range or unpainted."""
    seg_off, winner = _req(seg_off, torch.int64, "seg_off"), _req(winner.reshape(-1), torch.int32, "winner")
    pix, opacity = _req(pix, torch.int32, "pix"), _req(opacity, torch.float32, "opacity")
    K, dev, M, P = int(seg_off.shape[0]) - 1, seg_off.device, int(pix.shape[0]), int(winner.shape[0])
    heads = list(heads)
    if len(heads) != K or K < 1 or int(opacity.shape[0]) != M or M > VIEW_MAX_ENTRIES:
        raise ObjnerfError("view_query: one head per object of seg_off [K + 1]; pix, opacity [M], M < 2^32")
    if queries is None and pixels is None:
        raise ObjnerfError("view_query: neither queries nor pixels")
    Q, C_ = 1, int(heads[0][0].shape[0])
    out = {"sims": None, "label": None, "best": None, "feat": None}
    if queries is not None:
        queries = _req(queries, torch.float32, "queries")
        if queries.dim() != 2 or int(queries.shape[1]) != C_:
            raise ObjnerfError(f"view_query: queries [Q, {C_}], got {tuple(queries.shape)}")
        Q = int(queries.shape[0])               # (the library rejects Q outside 1 .. VIEW_QUERY_MAX)
        out["label"] = torch.empty(P, dtype=torch.int32, device=dev)
        out["sims"] = torch.empty(max(Q, 0), P, device=dev) if want_sims else None
        out["best"] = torch.empty(P, device=dev) if want_best else None
    n = 0
    if pixels is not None:
        if not pixels.is_cuda or pixels.dim() != 1 or pixels.dtype not in (torch.int32, torch.int64):
            raise ObjnerfError("view_query: pixels: a flat int32 / int64 GPU tensor")
        # (a pixel index outside int32 is outside [0, P) too: it maps to -1 and gets a zero row)
        pixels = torch.where((pixels >= 0) & (pixels < P), pixels, torch.full_like(pixels, -1)).to(torch.int32).contiguous()
        n = int(pixels.shape[0])
        out["feat"] = torch.empty(n, C_, device=dev)
    arr, table = _view_heads(heads, C_, dev)
    p = (lambda t: _ptr(t) if M else None)
    check(lib().objnerf_view_query(P, K, M, C_, Q, _ptr(seg_off), p(pix), p(opacity), _ptr(winner), _ptr(table),
                                   C.addressof(arr), _ptr(queries), _ptr(out["sims"]), _ptr(out["label"]), _ptr(out["best"]),
                                   n, _ptr(pixels) if n else None, _ptr(out["feat"]) if n else None, int(_workgroups),
                                   _stream()), "objnerf_view_query")
    return out


VIEW_EVAL_TILE = 32                     # OBJNERF_VIEW_EVAL_TILE: objnerf_view_compare's tiles are this many pixels square
VIEW_EVAL_LDS_ROWS = 64                 # OBJNERF_VIEW_EVAL_LDS_ROWS: up to this G the tables are reduced in LDS first
VIEW_EVAL_MAX_ROWS = 32767
VIEW_EVAL_COLS = 9


def view_compare(rgb_r: torch.Tensor, depth_r: torch.Tensor, id_r: torch.Tensor, painted: Optional[torch.Tensor],
                 rgb_g: torch.Tensor, depth_g: torch.Tensor, id_g: torch.Tensor, lut: torch.Tensor, G: int,
                 acc: torch.Tensor, conf: Optional[torch.Tensor] = None, want_ssim_map: bool = False,
                 _workgroups: int = 0) -> Optional[torch.Tensor]:
    """One frame of a rendered view against the sequence's frame (objnerf_view_compare; the columns, the exact-integer SSIM
    and the lut rule stand in include/objnerf_hip.h).  rgb_* uint8 [W, H, 3], depth_* fp32 [W, H], id_* int32 [W, H],
    painted uint8 / bool [W, H] or None (every pixel painted); lut int32 [n_lut]: id -> row in [0, G), anything else = no
    row.  acc int64 [G + 1, 9] and conf int64 [G, G + 1] (or None) are ADDED TO, never cleared.  -> ssim_map fp32 [W, H]
    (NaN outside the interior) with want_ssim_map, else None.  The tables do not depend on _workgroups (0 = default)."""
    rgb_r, rgb_g = _req(rgb_r, torch.uint8, "rgb_r"), _req(rgb_g, torch.uint8, "rgb_g")
    if rgb_r.dim() != 3 or int(rgb_r.shape[2]) != 3 or rgb_g.shape != rgb_r.shape:
        raise ObjnerfError(f"view_compare: rgb_r, rgb_g uint8 [W, H, 3], got {tuple(rgb_r.shape)}, {tuple(rgb_g.shape)}")
    W, H, dev, G = int(rgb_r.shape[0]), int(rgb_r.shape[1]), rgb_r.device, int(G)
    depth_r, depth_g = _req(depth_r, torch.float32, "depth_r"), _req(depth_g, torch.float32, "depth_g")
    id_r, id_g, lut = _req(id_r, torch.int32, "id_r"), _req(id_g, torch.int32, "id_g"), _req(lut, torch.int32, "lut")
    if painted is not None:
        if painted.dtype == torch.bool:
            painted = painted.contiguous().view(torch.uint8)
        painted = _req(painted, torch.uint8, "painted")
    for name, t in (("depth_r", depth_r), ("depth_g", depth_g), ("id_r", id_r), ("id_g", id_g), ("painted", painted)):
        if t is not None and (tuple(t.shape) != (W, H) or t.device != dev):
            raise ObjnerfError(f"view_compare: {name} [{W}, {H}] on {dev}, got {tuple(t.shape)} on {t.device}")
    if W < 1 or H < 1 or W * H > 0x7fffffff or not 1 <= G <= VIEW_EVAL_MAX_ROWS or lut.dim() != 1 or lut.device != dev:
        raise ObjnerfError("view_compare: W, H >= 1, W * H < 2^31, 1 <= G <= 32767, lut int32 [n_lut]")
    # (the kernel adds into these in place: a copy made by .contiguous() would be lost, so they are checked, not fixed)
    if not (acc.is_cuda and acc.dtype == torch.int64 and acc.is_contiguous() and tuple(acc.shape) == (G + 1, VIEW_EVAL_COLS)
            and acc.device == dev):
        raise ObjnerfError(f"view_compare: acc: a contiguous int64 [{G + 1}, {VIEW_EVAL_COLS}] on {dev}")
    if conf is not None and not (conf.is_cuda and conf.dtype == torch.int64 and conf.is_contiguous()
                                 and tuple(conf.shape) == (G, G + 1) and conf.device == dev):
        raise ObjnerfError(f"view_compare: conf: a contiguous int64 [{G}, {G + 1}] on {dev}")
    ssim_map = torch.empty(W, H, device=dev) if want_ssim_map else None
    n_lut = int(lut.shape[0])
    check(lib().objnerf_view_compare(W, H, _ptr(rgb_r), _ptr(depth_r), _ptr(id_r), _ptr(painted), _ptr(rgb_g), _ptr(depth_g),
                                     _ptr(id_g), _ptr(lut) if n_lut else None, n_lut, G, _ptr(acc), _ptr(conf),
                                     _ptr(ssim_map), int(_workgroups), _stream()), "objnerf_view_compare")
    return ssim_map


# ---------------------------------------------------------------------------------------------------
# a navigation volume of the map (objnerf_mapvolume.hip; map_volume.MapVolume drives these).  dims = (nx, ny, nz), volumes
# are [nz, ny, nx]; cost is kept as int32 storage of the unsigned values (-1 = 0xFFFFFFFF, not reached)
VOLUME_MAX_AXIS = 1024
VOLUME_MAX_VOXELS = 2 ** 31 - 1
VOLUME_ROUND_BATCH = 16


def volume_check_dims(dims) -> Tuple[int, int, int]:
    d = tuple(int(v) for v in dims)
    if len(d) != 3 or min(d) < 1 or max(d) > VOLUME_MAX_AXIS or d[0] * d[1] * d[2] > VOLUME_MAX_VOXELS:
        raise ObjnerfError(f"map volume: dims {d}: every axis in [1, {VOLUME_MAX_AXIS}], at most 2^31 - 1 voxels")
    return d


def _volume(t: torch.Tensor, dims, name: str) -> torch.Tensor:
    t = _req(t, torch.int32, name)
    if tuple(t.shape) != (dims[2], dims[1], dims[0]):
        raise ObjnerfError(f"map volume: {name} [{dims[2]}, {dims[1]}, {dims[0]}], got {tuple(t.shape)}")
    return t


def volume_centres(dims, origin, voxel: float, z0: int, nzs: int, device) -> torch.Tensor:
    """The fp32 centres [nzs * ny * nx, 3] of the z-planes [z0, z0 + nzs): origin + (float(i) + 0.5f) * voxel."""
    nx, ny, nz = volume_check_dims(dims)
    if not (0 <= z0 and 0 <= nzs and z0 + nzs <= nz) or not float(voxel) > 0:
        raise ObjnerfError(f"volume_centres: planes [{z0}, {z0 + nzs}) of {nz}, voxel {voxel}")
    out = torch.empty(nzs * ny * nx, 3, device=device)
    org = (C.c_float * 3)(*[float(v) for v in origin])
    check(lib().objnerf_volume_centres(nx, ny, nz, int(z0), int(nzs), org, float(voxel), _ptr(out) if nzs else None,
                                       _stream()), "objnerf_volume_centres")
    return out


def volume_project(label: torch.Tensor, dims, axis: int) -> torch.Tensor:
    """label [nz, ny, nx] -> the axis (0 = x, 1 = y, 2 = z) collapsed to length 1: the first occupied label of a column."""
    nx, ny, nz = volume_check_dims(dims)
    label = _volume(label, (nx, ny, nz), "label")
    if axis not in (0, 1, 2):
        raise ObjnerfError(f"volume_project: axis {axis}")
    od = [nx, ny, nz]
    od[axis] = 1
    out = torch.empty(od[2], od[1], od[0], dtype=torch.int32, device=label.device)
    check(lib().objnerf_volume_project(nx, ny, nz, int(axis), _ptr(label), _ptr(out), _stream()), "objnerf_volume_project")
    return out


def volume_clearance(label: torch.Tensor, dims):
    """-> (dist2 int32 [nz, ny, nx], site int32 [nz, ny, nx]): the exact squared distance to the nearest occupied voxel and
    its linear index (the lowest among equals); INT32_MAX / -1 without an occupied voxel."""
    nx, ny, nz = volume_check_dims(dims)
    label = _volume(label, (nx, ny, nz), "label")
    d, s, td, ts = (torch.empty_like(label) for _ in range(4))
    check(lib().objnerf_volume_clearance(nx, ny, nz, _ptr(label), _ptr(d), _ptr(s), _ptr(td), _ptr(ts), _stream()),
          "objnerf_volume_clearance")
    return d, s


def volume_round_cap(traversable: int) -> int:
    """The hard cap of reach's round loop.  After round r every voxel whose shortest path crosses fewer than r tile borders
    is final; a shortest path is simple, so it crosses fewer borders than there are traversable voxels;
    one more round finds nothing to lower."""
    return int(traversable) + 2


def volume_reach(label: torch.Tensor, dist2: torch.Tensor, dims, r2: int, start_voxel: int, stats: Optional[dict] = None,
                 batch: int = VOLUME_ROUND_BATCH) -> torch.Tensor:
    """cost int32 storage [nz, ny, nx] of the unsigned path costs from start_voxel (a traversable voxel: the caller checks).
    Rounds go out in batches; the changed words are read back once per batch.  stats receives rounds / batches."""
    nx, ny, nz = volume_check_dims(dims)
    label, dist2 = _volume(label, (nx, ny, nz), "label"), _volume(dist2, (nx, ny, nz), "dist2")
    dev, n, r2 = label.device, nx * ny * nz, int(r2)
    if not 0 <= int(start_voxel) < n or not 0 <= r2 <= 0x7fffffff or batch < 1:
        raise ObjnerfError(f"volume_reach: start voxel {start_voxel} of {n}, r2 = {r2}, batch = {batch}")
    trav = int(((label < 0) & (dist2 >= r2)).sum())
    if 5 * trav >= 2 ** 32 - 6:
        raise ObjnerfError(f"volume_reach: {trav} traversable voxels: a path cost may not fit 32 bits")
    T = int(lib().objnerf_volume_reach_tiles(nx, ny, nz))
    cost = torch.full((nz, ny, nx), -1, dtype=torch.int32, device=dev)
    active = torch.zeros(2, T, dtype=torch.int32, device=dev)
    sx, sy, sz = start_voxel % nx, (start_voxel // nx) % ny, start_voxel // (nx * ny)
    ntx, nty = (nx + 7) // 8, (ny + 7) // 8
    cost.view(-1)[start_voxel] = 0
    active[0, ((sz // 8) * nty + sy // 8) * ntx + sx // 8] = 1
    changed = torch.empty(batch, dtype=torch.int32, device=dev)
    cap, rounds, batches = volume_round_cap(trav), 0, 0
    while True:
        changed.zero_()
        check(lib().objnerf_volume_reach_rounds(nx, ny, nz, _ptr(label), _ptr(dist2), r2, _ptr(cost), _ptr(active), rounds,
                                                batch, _ptr(changed), _stream()), "objnerf_volume_reach_rounds")
        ch = changed.tolist()                   # the one read-back of the batch
        batches += 1
        if 0 in ch:                             # a round that lowered nothing: it and every later one were empty
            rounds += ch.index(0) + 1
            break
        rounds += batch
        if rounds > cap:
            raise ObjnerfError(f"volume_reach: not settled after {rounds} rounds (the cap of this grid is {cap})")
    if stats is not None:
        stats["rounds"], stats["batches"], stats["round_cap"], stats["traversable"] = rounds, batches, cap, trav
    return cost


def volume_goals(label, dist2, site, cost, dims, r2: int, K: int) -> torch.Tensor:
    """-> table int64 [K] (storage of the unsigned keys dist2 << 32 | voxel; -1 = all ones: no goal)."""
    nx, ny, nz = volume_check_dims(dims)
    label, dist2, site, cost = (_volume(t, (nx, ny, nz), nm) for t, nm in ((label, "label"), (dist2, "dist2"),
                                                                          (site, "site"), (cost, "cost")))
    if K < 1:
        raise ObjnerfError(f"volume_goals: K = {K}")
    table = torch.full((int(K),), -1, dtype=torch.int64, device=label.device)
    check(lib().objnerf_volume_goals(nx, ny, nz, int(K), _ptr(label), _ptr(dist2), _ptr(site), _ptr(cost), int(r2),
                                     _ptr(table), _stream()), "objnerf_volume_goals")
    return table


def volume_paths(label, dist2, cost, dims, r2: int, goals: torch.Tensor, cap: int, out: Optional[torch.Tensor] = None):
    """goals int32 [G] -> (out int32 [G, cap] (or the caller's contiguous buffer of at least G * cap words), len int32 [G]:
    negative where the path has more than cap voxels)."""
    nx, ny, nz = volume_check_dims(dims)
    label, dist2, cost = (_volume(t, (nx, ny, nz), nm) for t, nm in ((label, "label"), (dist2, "dist2"), (cost, "cost")))
    goals = _req(goals, torch.int32, "goals").reshape(-1)
    G, cap = int(goals.shape[0]), int(cap)
    if cap < 0 or G * max(cap, 1) > 0x7fffffff:
        raise ObjnerfError(f"volume_paths: cap = {cap}, G = {G}")
    if out is None:
        out = torch.full((G, cap), -1, dtype=torch.int32, device=label.device)
    elif not (out.is_cuda and out.dtype == torch.int32 and out.is_contiguous() and out.numel() >= G * cap):
        raise ObjnerfError(f"volume_paths: out: a contiguous int32 buffer of at least {G * cap} words")
    ln = torch.zeros(G, dtype=torch.int32, device=label.device)
    check(lib().objnerf_volume_paths(nx, ny, nz, _ptr(label), _ptr(dist2), int(r2), _ptr(cost), G, _ptr(goals) if G else None,
                                     cap, _ptr(out) if cap and G else None, _ptr(ln) if G else None, _stream()),
          "objnerf_volume_paths")
    return out, ln


# ---------------------------------------------------------------------------------------------------
# part regions: connected patches of a part query on the map's meshes (objnerf_mapregions.hip; query.MapQuery.part_regions
# and map_regions.py drive these).  The rules stand in include/objnerf_hip.h.
REGION_ROW = 32                         # OBJNERF_REGION_ROW
REGION_MAX_Q = 16
REGION_STATUS_BAD_ID, REGION_STATUS_CROSS, REGION_STATUS_NONFINITE = 1, 2, 4


def regions_workspace_bytes(V: int, F: int, S: int) -> int:
    """0 for sizes out of range (V in [1, 2^31), F in [0, 2^31), S in [1, 65535])."""
    if not (-2 ** 63 <= V < 2 ** 63 and -2 ** 63 <= F < 2 ** 63 and -2 ** 31 <= S < 2 ** 31):
        return 0
    return int(lib().objnerf_regions_workspace_bytes(int(V), int(F), int(S)))


def _regions_mesh(vert_off, face_off, faces, sims):
    vert_off, face_off = _req(vert_off, torch.int64, "vert_off"), _req(face_off, torch.int64, "face_off")
    faces, sims = _req(faces, torch.int32, "faces"), _req(sims, torch.float32, "sims")
    S = int(vert_off.shape[0]) - 1
    if vert_off.dim() != 1 or S < 1 or tuple(face_off.shape) != (S + 1,):
        raise ObjnerfError("part regions: vert_off, face_off int64 [S + 1], S >= 1")
    if sims.dim() != 2 or faces.dim() != 2 or int(faces.shape[1]) != 3:
        raise ObjnerfError("part regions: sims [V, Q], faces [F, 3]")
    if any(t.device != sims.device for t in (vert_off, face_off, faces)):
        raise ObjnerfError(f"part regions: every tensor on {sims.device}")
    return vert_off, face_off, faces, sims, S


def regions_label(vert_off: torch.Tensor, face_off: torch.Tensor, faces: torch.Tensor, sims: torch.Tensor, q: int,
                  thr: torch.Tensor, vmax: Optional[int] = None, status: Optional[torch.Tensor] = None,
                  ws: Optional[torch.Tensor] = None):
    """-> (root int32 [V], label int32 [V], reg_off int64 [S + 1], status int32 [1]), all on the device: nothing is read
    back.  vmax: the largest vertex count of an object (None: read from vert_off, which synchronises).  ws: a uint8 buffer
    of regions_workspace_bytes(V, F, S), else one is made."""
    vert_off, face_off, faces, sims, S = _regions_mesh(vert_off, face_off, faces, sims)
    thr = _req(thr, torch.float32, "thr")
    V, Q, F, dev = int(sims.shape[0]), int(sims.shape[1]), int(faces.shape[0]), sims.device
    if tuple(thr.shape) != (S,) or thr.device != dev:
        raise ObjnerfError(f"regions_label: thr fp32 [{S}] on {dev}")
    if vmax is None:
        vmax = int((vert_off[1:] - vert_off[:-1]).max())
    if ws is None:
        ws = torch.empty(max(regions_workspace_bytes(V, F, S), 1), dtype=torch.uint8, device=dev)
    ws = _req(ws, torch.uint8, "ws")
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    status = _req(status, torch.int32, "status")
    root = torch.empty(max(V, 1), dtype=torch.int32, device=dev)[:V]
    label = torch.empty(max(V, 1), dtype=torch.int32, device=dev)[:V]
    reg_off = torch.empty(S + 1, dtype=torch.int64, device=dev)
    check(lib().objnerf_regions_label(V, F, S, int(vmax), Q, int(q), _ptr(vert_off), _ptr(face_off),
                                      _ptr(faces) if F else None, _ptr(sims), _ptr(thr), _ptr(ws), int(ws.numel()),
                                      _ptr(root), _ptr(label), _ptr(reg_off), _ptr(status), _stream()),
          "objnerf_regions_label")
    return root, label, reg_off, status


def regions_table(vert_off: torch.Tensor, face_off: torch.Tensor, verts: torch.Tensor, faces: torch.Tensor,
                  sims: torch.Tensor, q: int, root: torch.Tensor, label: torch.Tensor, R: int,
                  status: torch.Tensor) -> torch.Tensor:
    """-> table int64 [R, REGION_ROW] on the device (the columns: include/objnerf_hip.h); status is OR-ed into."""
    vert_off, face_off, faces, sims, S = _regions_mesh(vert_off, face_off, faces, sims)
    verts = _req(verts, torch.float64, "verts")
    root, label, status = _req(root, torch.int32, "root"), _req(label, torch.int32, "label"), _req(status, torch.int32, "status")
    V, Q, F, dev, R = int(sims.shape[0]), int(sims.shape[1]), int(faces.shape[0]), sims.device, int(R)
    if tuple(verts.shape) != (V, 3) or tuple(root.shape) != (V,) or tuple(label.shape) != (V,) or status.numel() < 1:
        raise ObjnerfError(f"regions_table: verts fp64 [{V}, 3], root, label int32 [{V}], status int32 [1]")
    if any(t.device != dev for t in (verts, root, label, status)):
        raise ObjnerfError(f"regions_table: every tensor on {dev}")
    table = torch.empty(max(R, 0), REGION_ROW, dtype=torch.int64, device=dev)
    check(lib().objnerf_regions_table(V, F, S, Q, int(q), _ptr(vert_off), _ptr(face_off), _ptr(verts),
                                      _ptr(faces) if F else None, _ptr(sims), _ptr(root), _ptr(label), R,
                                      _ptr(table) if R > 0 else None, _ptr(status), _stream()), "objnerf_regions_table")
    return table


# ---------------------------------------------------------------------------------------------------
# a rasteriser for the map's meshes (objnerf_mapraster.hip; map_raster.MapRaster drives these).  The rules stand in
# include/objnerf_hip.h.
RASTER_STATS = ("small", "large", "no_sample", "z_near", "bound", "degenerate", "bad_index", "hidden")
RASTER_STATUS_BAD_ID = 1
RASTER_SMALL_MAX = 0x7fffffff           # _small_box: every face takes the small path (0: every face the large one)
RASTER_MAX_SIDE = 65536


def raster_workspace_bytes(V: int, F: int) -> int:
    """0 for sizes out of range (V, F in [0, 2^31))."""
    if not (-2 ** 63 <= V < 2 ** 63 and -2 ** 63 <= F < 2 ** 63):
        return 0
    return int(lib().objnerf_raster_workspace_bytes(int(V), int(F)))


def _raster_mesh(verts, faces, face_off, W, H, what):
    verts, faces = _req(verts, torch.float64, f"{what}: verts"), _req(faces, torch.int32, f"{what}: faces")
    face_off = _req(face_off, torch.int64, f"{what}: face_off")
    if verts.dim() != 2 or int(verts.shape[1]) != 3 or faces.dim() != 2 or int(faces.shape[1]) != 3:
        raise ObjnerfError(f"{what}: verts fp64 [V, 3], faces int32 [F, 3]")
    S = int(face_off.shape[0]) - 1
    if face_off.dim() != 1 or S < 0 or S > 65535:
        raise ObjnerfError(f"{what}: face_off int64 [S + 1], 0 <= S <= 65535")
    V, F, W, H = int(verts.shape[0]), int(faces.shape[0]), int(W), int(H)
    if F > 0 and (S < 1 or V < 1):
        raise ObjnerfError(f"{what}: {F} faces need at least one object and one vertex")
    if not (1 <= W <= RASTER_MAX_SIDE and 1 <= H <= RASTER_MAX_SIDE and W * H <= 0x7fffffff):
        raise ObjnerfError(f"{what}: W, H in [1, {RASTER_MAX_SIDE}], got {W} x {H}")
    if faces.device != verts.device or face_off.device != verts.device:
        raise ObjnerfError(f"{what}: every tensor on {verts.device}")
    return verts, faces, face_off, V, F, S, W, H


def raster_visibility(verts: torch.Tensor, faces: torch.Tensor, face_off: torch.Tensor, hide: torch.Tensor,
                      T_CW: torch.Tensor, intrinsics, W: int, H: int, z_near: float = 0.05,
                      status: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None, _small_box: int = -1,
                      _passes: int = 0):
    """objnerf_raster_visibility -> (key int64 [W, H]: the bits of the unsigned keys, -1 = nothing drawn; stats int64 [8]
    (RASTER_STATS); status int32 [1]; ws: the workspace, which raster_resolve reads), all on the device.  verts fp64
    [V, 3], faces int32 [F, 3], face_off int64 [S + 1], hide uint8 [S], T_CW fp64 [3, 4] = inverse(T_WC)[:3] on the
    device, intrinsics (fx, fy, cx, cy).  _small_box, _passes: see the header (negative / 0: the default)."""
    verts, faces, face_off, V, F, S, W, H = _raster_mesh(verts, faces, face_off, W, H, "raster_visibility")
    hide, T_CW = _req(hide, torch.uint8, "raster_visibility: hide"), _req(T_CW, torch.float64, "raster_visibility: T_CW")
    dev = verts.device
    if tuple(hide.shape) != (S,) or tuple(T_CW.shape) != (3, 4) or hide.device != dev or T_CW.device != dev:
        raise ObjnerfError(f"raster_visibility: hide uint8 [{S}], T_CW fp64 [3, 4] on {dev}")
    fx, fy, cx, cy = (float(x) for x in intrinsics)
    if not float(z_near) > 0.0:
        raise ObjnerfError(f"raster_visibility: z_near {z_near} must be positive")
    if not -2 ** 31 <= int(_small_box) <= RASTER_SMALL_MAX:
        raise ObjnerfError(f"raster_visibility: _small_box {_small_box}")
    need = raster_workspace_bytes(V, F)
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    ws = _req(ws, torch.uint8, "raster_visibility: ws")
    if ws.numel() < need or ws.device != dev:
        raise ObjnerfError(f"raster_visibility: ws: {need} bytes on {dev}")
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    status = _req(status, torch.int32, "raster_visibility: status")
    key = torch.empty(W, H, dtype=torch.int64, device=dev)
    stats = torch.empty(len(RASTER_STATS), dtype=torch.int64, device=dev)
    check(lib().objnerf_raster_visibility(V, F, S, W, H, _ptr(verts) if V else None, _ptr(faces) if F else None,
                                          _ptr(face_off), _ptr(hide) if S else None, _ptr(T_CW), fx, fy, cx, cy,
                                          float(z_near), int(_small_box), int(_passes), _ptr(ws), int(ws.numel()), _ptr(key), _ptr(stats),
                                          _ptr(status), _stream()), "objnerf_raster_visibility")
    return key, stats, status, ws


def raster_resolve(verts: torch.Tensor, faces: torch.Tensor, face_off: torch.Tensor, ids: torch.Tensor,
                   colors: torch.Tensor, ws: torch.Tensor, key: torch.Tensor, cam, ambient: float = 0.35,
                   shading: bool = True, background=(255, 255, 255)) -> Dict[str, torch.Tensor]:
    """objnerf_raster_resolve over the keys and the workspace of raster_visibility (same mesh) -> dict(rgb uint8
    [W, H, 3], maskid int32 [W, H], depth fp32 [W, H], winner, face, vertex int32 [W, H], counts int64 [S]) on the device.
    ids int32 [S], colors fp32 [V, 3], cam: the camera centre (T_WC[:3, 3]) as three numbers, background: (r, g, b)."""
    key = _req(key, torch.int64, "raster_resolve: key")
    if key.dim() != 2:
        raise ObjnerfError("raster_resolve: key int64 [W, H]")
    verts, faces, face_off, V, F, S, W, H = _raster_mesh(verts, faces, face_off, key.shape[0], key.shape[1], "raster_resolve")
    ids, colors = _req(ids, torch.int32, "raster_resolve: ids"), _req(colors, torch.float32, "raster_resolve: colors")
    ws = _req(ws, torch.uint8, "raster_resolve: ws")
    dev = verts.device
    if tuple(ids.shape) != (S,) or tuple(colors.shape) != (V, 3):
        raise ObjnerfError(f"raster_resolve: ids int32 [{S}], colors fp32 [{V}, 3]")
    if any(t.device != dev for t in (ids, colors, ws, key)):
        raise ObjnerfError(f"raster_resolve: every tensor on {dev}")
    if ws.numel() < raster_workspace_bytes(V, F):
        raise ObjnerfError("raster_resolve: ws is not the workspace of raster_visibility for this mesh")
    cam = [float(x) for x in cam]
    bg = [int(x) for x in background]
    if len(cam) != 3 or len(bg) != 3 or any(not 0 <= b <= 255 for b in bg) or not 0.0 <= float(ambient) <= 1.0:
        raise ObjnerfError("raster_resolve: cam [3], background three values in 0..255, ambient in [0, 1]")
    out = dict(rgb=torch.empty(W, H, 3, dtype=torch.uint8, device=dev), maskid=torch.empty(W, H, dtype=torch.int32, device=dev),
               depth=torch.empty(W, H, dtype=torch.float32, device=dev), winner=torch.empty(W, H, dtype=torch.int32, device=dev),
               face=torch.empty(W, H, dtype=torch.int32, device=dev), vertex=torch.empty(W, H, dtype=torch.int32, device=dev),
               counts=torch.empty(S, dtype=torch.int64, device=dev))
    check(lib().objnerf_raster_resolve(V, F, S, W, H, _ptr(verts) if V else None, _ptr(faces) if F else None, _ptr(face_off),
                                       _ptr(ids) if S else None, _ptr(colors) if V else None, _ptr(ws), int(ws.numel()),
                                       _ptr(key), cam[0], cam[1], cam[2], float(ambient), int(bool(shading)),
                                       (bg[0] << 16) | (bg[1] << 8) | bg[2], _ptr(out["rgb"]), _ptr(out["maskid"]),
                                       _ptr(out["depth"]), _ptr(out["winner"]), _ptr(out["face"]), _ptr(out["vertex"]),
                                       _ptr(out["counts"]) if S else None, _stream()), "objnerf_raster_resolve")
    return out


# ---------------------------------------------------------------------------------------------------
# ray casting over the map's meshes (objnerf_maprays.hip; map_rays.MapRays drives these).  The rules stand in
# include/objnerf_hip.h.
RAYS_STATS = ("rays", "hits", "bad_rays", "node_visits", "face_tests")
RAYS_STATUS_BAD_ID = 1
RAYS_STATUS_BAD_RAY = 2
RAYS_LEAF_DEFAULT = 4                   # an ASSUMED default
RAYS_EMPTY = -1                         # the bits of the all-ones key as int64
RAYS_NODE_BYTES = 32


def rays_workspace_bytes(F: int, leaf: int = -1) -> int:
    """0 for sizes out of range (F in [0, 2^31), leaf >= 1 or negative for the default)."""
    if not (-2 ** 63 <= F < 2 ** 63 and -2 ** 31 <= leaf < 2 ** 31):
        return 0
    return int(lib().objnerf_rays_workspace_bytes(int(F), int(leaf)))


def rays_node_count(F: int, leaf: int = -1) -> int:
    """2 P: the nodes at the start of the workspace (heap order, node 0 unused), 32 bytes each."""
    leaf = RAYS_LEAF_DEFAULT if leaf < 0 else int(leaf)
    n, P = max(-(-int(F) // leaf), 1), 1
    while P < n:
        P *= 2
    return 2 * P


def _rays_mesh(verts, faces, face_off, leaf, what):
    verts, faces = _req(verts, torch.float64, f"{what}: verts"), _req(faces, torch.int32, f"{what}: faces")
    face_off = _req(face_off, torch.int64, f"{what}: face_off")
    if verts.dim() != 2 or int(verts.shape[1]) != 3 or faces.dim() != 2 or int(faces.shape[1]) != 3:
        raise ObjnerfError(f"{what}: verts fp64 [V, 3], faces int32 [F, 3]")
    S = int(face_off.shape[0]) - 1
    if face_off.dim() != 1 or S < 0 or S > 65535:
        raise ObjnerfError(f"{what}: face_off int64 [S + 1], 0 <= S <= 65535")
    V, F = int(verts.shape[0]), int(faces.shape[0])
    if F > 0 and (S < 1 or V < 1):
        raise ObjnerfError(f"{what}: {F} faces need at least one object and one vertex")
    if faces.device != verts.device or face_off.device != verts.device:
        raise ObjnerfError(f"{what}: every tensor on {verts.device}")
    leaf = int(leaf)
    if not (leaf < 0 or 1 <= leaf <= 0x7fffffff):
        raise ObjnerfError(f"{what}: leaf {leaf}: at least 1 (negative: the default)")
    return verts, faces, face_off, V, F, S, leaf


def _rays_pad(pad, what):
    pad = float(pad)
    if not (pad >= 0.0 and pad != float("inf")):
        raise ObjnerfError(f"{what}: pad {pad} must be finite and not negative")
    return pad


def rays_scene_box(verts: torch.Tensor):
    """The box of the finite coordinates of verts fp64 [V, 3] -> (lo [3], hi [3]) as Python floats; (0, 0) on an axis
    without a finite value."""
    big = torch.finfo(torch.float64).max
    fin = torch.isfinite(verts)
    if verts.shape[0] == 0:
        return [0.0] * 3, [0.0] * 3
    lo = torch.where(fin, verts, torch.full_like(verts, big)).amin(dim=0).tolist()
    hi = torch.where(fin, verts, torch.full_like(verts, -big)).amax(dim=0).tolist()
    for k in range(3):
        if lo[k] > hi[k]:
            lo[k] = hi[k] = 0.0
    return lo, hi


def rays_default_pad(verts: torch.Tensor) -> float:
    """2^-20 times the largest finite extent of verts (an ASSUMED default)."""
    lo, hi = rays_scene_box(verts)
    return max(h - l for l, h in zip(lo, hi)) * 2.0 ** -20


def rays_build(verts: torch.Tensor, faces: torch.Tensor, face_off: torch.Tensor, pad: float, leaf: int = -1,
               ws: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None, box=None, _stage: int = 0,
               _codes: Optional[torch.Tensor] = None, _order: Optional[torch.Tensor] = None):
    """objnerf_rays_build, both stages with the stable sort of the codes between them -> (ws uint8: the hierarchy that
    rays_cast walks, status int32 [1]: bit 0 = a face with an id outside [0, V)).  verts fp64 [V, 3], faces int32
    [F, 3], face_off int64 [S + 1] on the device; box: (lo [3], hi [3]) of the scene (None: rays_scene_box(verts)).
    _stage (tools/rays_bench.py): 1 -> the codes int64 [F] alone; 2 -> stage 2 alone on _order."""
    verts, faces, face_off, V, F, S, leaf = _rays_mesh(verts, faces, face_off, leaf, "rays_build")
    pad = _rays_pad(pad, "rays_build")
    dev = verts.device
    lo, hi = rays_scene_box(verts) if box is None else ([float(x) for x in box[0]], [float(x) for x in box[1]])
    if len(lo) != 3 or len(hi) != 3:
        raise ObjnerfError("rays_build: box (lo [3], hi [3])")
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    status = _req(status, torch.int32, "rays_build: status")
    if _stage not in (0, 1, 2):
        raise ObjnerfError(f"rays_build: _stage {_stage}")

    def call(stage, codes, order, wsp):
        check(lib().objnerf_rays_build(stage, V, F, S, leaf, _ptr(verts) if V else None, _ptr(faces) if F else None,
                                       _ptr(face_off), pad, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], _ptr(codes),
                                       _ptr(order), _ptr(wsp), int(wsp.numel()) if wsp is not None else 0, _ptr(status),
                                       _stream()), "objnerf_rays_build")

    if _stage in (0, 1):
        codes = torch.empty(F, dtype=torch.int64, device=dev) if _codes is None else _req(_codes, torch.int64, "rays_build: codes")
        if tuple(codes.shape) != (F,) or codes.device != dev:
            raise ObjnerfError(f"rays_build: codes int64 [{F}] on {dev}")
        call(1, codes if F else None, None, None)
        if _stage == 1:
            return codes
        _order = torch.sort(codes, stable=True)[1]
    order = _req(_order, torch.int64, "rays_build: order")
    if tuple(order.shape) != (F,) or order.device != dev:
        raise ObjnerfError(f"rays_build: order int64 [{F}] on {dev}")
    need = rays_workspace_bytes(F, leaf)
    if ws is None:
        ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    ws = _req(ws, torch.uint8, "rays_build: ws")
    if need == 0 or ws.numel() < need or ws.device != dev:
        raise ObjnerfError(f"rays_build: ws: {need} bytes on {dev}")
    call(2, None, order if F else None, ws)
    return ws, status


def rays_cast(verts: torch.Tensor, faces: torch.Tensor, face_off: torch.Tensor, hide: torch.Tensor, ws: torch.Tensor,
              pad: float, origins: torch.Tensor, dirs: torch.Tensor, t_min=0.0, t_max=float("inf"), leaf: int = -1,
              any_hit: bool = False, status: Optional[torch.Tensor] = None, _fixed_order: bool = False):
    """objnerf_rays_cast over the hierarchy of rays_build (same mesh, pad and leaf) -> (key int64 [N]: the bits of the
    unsigned keys, -1 = no hit (any_hit: hit uint8 [N] instead); stats int64 [5] (RAYS_STATS); status int32 [1]: bits are
    OR-ed in).  origins, dirs fp64 [N, 3]; t_min, t_max: numbers, or fp64 [N] device tensors; hide uint8 [S]."""
    verts, faces, face_off, V, F, S, leaf = _rays_mesh(verts, faces, face_off, leaf, "rays_cast")
    pad = _rays_pad(pad, "rays_cast")
    dev = verts.device
    hide, ws = _req(hide, torch.uint8, "rays_cast: hide"), _req(ws, torch.uint8, "rays_cast: ws")
    o, d = _req(origins, torch.float64, "rays_cast: origins"), _req(dirs, torch.float64, "rays_cast: dirs")
    if o.dim() != 2 or int(o.shape[1]) != 3 or o.shape != d.shape:
        raise ObjnerfError("rays_cast: origins, dirs fp64 [N, 3]")
    N = int(o.shape[0])
    if N > 0x7fffffff:
        raise ObjnerfError(f"rays_cast: {N} rays: at most 2^31 - 1")
    need = rays_workspace_bytes(F, leaf)
    if tuple(hide.shape) != (S,) or need == 0 or ws.numel() < need:
        raise ObjnerfError(f"rays_cast: hide uint8 [{S}], ws: the {need} bytes of rays_build for this mesh and leaf")
    win, per = [], []
    for name, w in (("t_min", t_min), ("t_max", t_max)):
        if isinstance(w, torch.Tensor):
            w = _req(w, torch.float64, f"rays_cast: {name}")
            if tuple(w.shape) != (N,) or w.device != dev:
                raise ObjnerfError(f"rays_cast: {name}: a number or fp64 [{N}] on {dev}")
            win.append(0.0 if name == "t_min" else float("inf"))
            per.append(w)
        else:
            win.append(float(w))
            per.append(None)
    if not win[0] >= 0.0 or win[1] != win[1]:
        raise ObjnerfError(f"rays_cast: t_min {win[0]} must not be negative, t_max {win[1]} not a NaN")
    if any(t.device != dev for t in (hide, ws, o, d)):
        raise ObjnerfError(f"rays_cast: every tensor on {dev}")
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    status = _req(status, torch.int32, "rays_cast: status")
    out = torch.empty(N, dtype=torch.uint8 if any_hit else torch.int64, device=dev)
    stats = torch.empty(len(RAYS_STATS), dtype=torch.int64, device=dev)
    check(lib().objnerf_rays_cast((1 if any_hit else 0) | (2 if _fixed_order else 0), V, F, S, leaf, N,
                                  _ptr(verts) if V else None, _ptr(faces) if F else None, _ptr(hide) if S else None, _ptr(ws),
                                  int(ws.numel()), pad, _ptr(o) if N else None, _ptr(d) if N else None, win[0], win[1],
                                  _ptr(per[0]), _ptr(per[1]), None if any_hit or not N else _ptr(out),
                                  _ptr(out) if any_hit and N else None, _ptr(stats), _ptr(status), _stream()),
          "objnerf_rays_cast")
    return out, stats, status


def rays_resolve(verts: torch.Tensor, faces: torch.Tensor, face_off: torch.Tensor, ids: torch.Tensor,
                 origins: torch.Tensor, dirs: torch.Tensor, key: torch.Tensor) -> Dict[str, torch.Tensor]:
    """objnerf_rays_resolve over the keys of a first-hit rays_cast (same mesh and rays) -> dict(hit uint8 [N], t fp32 [N],
    face, winner, maskid, vertex int32 [N], bary fp64 [N, 2], point, normal fp64 [N, 3]) on the device."""
    verts, faces, face_off, V, F, S, _ = _rays_mesh(verts, faces, face_off, 1, "rays_resolve")
    dev = verts.device
    ids, key = _req(ids, torch.int32, "rays_resolve: ids"), _req(key, torch.int64, "rays_resolve: key")
    o, d = _req(origins, torch.float64, "rays_resolve: origins"), _req(dirs, torch.float64, "rays_resolve: dirs")
    if o.dim() != 2 or int(o.shape[1]) != 3 or o.shape != d.shape:
        raise ObjnerfError("rays_resolve: origins, dirs fp64 [N, 3]")
    N = int(o.shape[0])
    if tuple(ids.shape) != (S,) or tuple(key.shape) != (N,) or N > 0x7fffffff:
        raise ObjnerfError(f"rays_resolve: ids int32 [{S}], key int64 [{N}]")
    if any(t.device != dev for t in (ids, key, o, d)):
        raise ObjnerfError(f"rays_resolve: every tensor on {dev}")
    e = lambda shape, dt: torch.empty(*shape, dtype=dt, device=dev)
    out = dict(hit=e((N,), torch.uint8), t=e((N,), torch.float32), face=e((N,), torch.int32), winner=e((N,), torch.int32),
               maskid=e((N,), torch.int32), vertex=e((N,), torch.int32), bary=e((N, 2), torch.float64),
               point=e((N, 3), torch.float64), normal=e((N, 3), torch.float64))
    p = (lambda t: _ptr(t)) if N else (lambda t: None)
    check(lib().objnerf_rays_resolve(V, F, S, N, _ptr(verts) if V else None, _ptr(faces) if F else None, _ptr(face_off),
                                     _ptr(ids) if S else None, p(o), p(d), p(key), p(out["hit"]), p(out["t"]), p(out["face"]),
                                     p(out["winner"]), p(out["maskid"]), p(out["vertex"]), p(out["bary"]), p(out["point"]),
                                     p(out["normal"]), _stream()), "objnerf_rays_resolve")
    return out
