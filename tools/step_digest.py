"""Diagnostic: SHA-256 digests of a fixed list of seeded cases on the layer-wise path, through whatever library
OBJNERF_LIB names.  A host-side refactor that leaves the kernels alone is correct exactly when it enqueues the same
kernels with the same arguments; every reduction on these paths is the ordered slab form, so that shows as equal bits.
Run it once per library, each in a fresh process, and compare the lines (profiles/gemm_interface_refactor.txt):

    OBJNERF_LIB=/path/to/other/libobjnerf_hip.so python tools/step_digest.py > other.txt
    python tools/step_digest.py > this.txt && diff other.txt this.txt

A training case digests gradients, parameters and moments after the step, loss terms and status; an inference case
its outputs.  The "ray loss" cases (profiles/ray_loss_refactor.txt) take one step through every kernel that composites a
ray and evaluates the loss, at the smallest shape that selects it; each names the kernel its launch code picks.  Every
object's labels hold 0, 1 and 2.  `--repeat` runs every case twice in the process and reports a case whose two digests differ (such a case
is not bit-reproducible to begin with)."""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from openobj_amd import init as obj_init  # noqa: E402
from openobj_amd import ops, optim, synthetic  # noqa: E402

DEV = "cuda"


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()[:32]


def arena_of(K, H, C, seed=21):
    st = obj_init.init_stacked(K, H, C, seed=seed)
    arena = ops.ParamArena(K, ops.NetShape(H, C, 6), DEV)
    arena.load_stacked([q.clone() for q in st])
    arena.scale.fill_(5.0)
    return arena


def train_case(H, K, R, n1, n2, feat, mode="fp32", C=512, with_optim=False, context=True, labels012=False):
    """One training step from a 0xA5-filled workspace.  labels012: every object's labels hold 0, 1 and 2."""
    arena = arena_of(K, H, C)
    b = synthetic.random_batch(K, R, n1, n2, seed=78 + R, feat_dim=C if feat else 0)
    b["labels"][:, 0] = 1
    b["labels"][:, R - 1] = 1
    if labels012:
        b["labels"][:, 1] = 0
        b["labels"][:, 2] = 2
        assert all(set(row.tolist()) == {0, 1, 2} for row in b["labels"])
    keys = ["pts", "z", "gt_depth", "gt_rgb", "labels"] + (["gt_feat"] if feat else [])
    batch = {k: torch.as_tensor(b[k]).to(DEV) for k in keys}
    ws = ops.TrainWorkspace(arena, K, R, n1 + n2, feat, precision=mode)
    for buf in (ws.buf, getattr(ws, "buf2", None)):
        if buf is not None:
            buf.fill_(0xA5)
    if not context:
        ws.context = None
    opt = optim.ArenaAdamW(arena) if with_optim else None
    ops.train_step(arena, ws, batch, with_feat=feat, bf16=mode, optim=opt)
    torch.cuda.synchronize()
    out = [ws.grads, arena.params, ws.loss_terms, ws.status]
    if opt is not None:
        out += [opt.exp_avg, opt.exp_avg_sq, opt._banks]
    return sha(*out)


def loss_case(feat, K=2, R=24, S=16, C=64):
    """ops.step_batch_loss (loss_kernel) on materialised tensors; with pred_feat its C-wide feature term runs."""
    b = synthetic.random_batch(K, R, S // 4, S - S // 4, seed=91, feat_dim=C if feat else 0)
    b["labels"][:, :3] = [1, 0, 2]
    g = torch.Generator().manual_seed(92)
    alpha = torch.randn(K, R, S, generator=g).to(DEV)
    color = torch.rand(K, R, S, 3, generator=g).to(DEV)
    pred = torch.randn(K, R, S, C, generator=g).to(DEV) if feat else None
    t = {k: torch.as_tensor(b[k]).to(DEV) for k in ["z", "gt_depth", "gt_rgb", "labels"] + (["gt_feat"] if feat else [])}
    out = ops.step_batch_loss(alpha, color, t["gt_depth"], t["gt_rgb"], t["labels"], t["z"], gt_feat=t.get("gt_feat"),
                              pred_feat=pred)
    torch.cuda.synchronize()
    return sha(*[out[k] for k in ("total", "terms", "d_alpha", "d_color", "d_pred_feat", "status") if out[k] is not None])


def points(K, N, seed):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(K, N, 3, generator=g) - 0.5) * 2.0).to(DEV)


def eval_case(H, clip):
    arena = arena_of(2, H, 512)
    out = ops.eval_points(arena, points(2, 300, 5), want_hfeat=clip, want_clip=clip)
    torch.cuda.synchronize()
    return sha(*[t for t in out if t is not None])


def backward_case(H, clip):
    K, N = 2, 300
    arena = arena_of(K, H, 512)
    emb = ops.embed(arena, points(K, N, 6))
    g = torch.Generator().manual_seed(7)
    d_alpha = torch.randn(K, N, generator=g).to(DEV)
    d_color = torch.randn(K, N, 3, generator=g).to(DEV)
    d_clip = torch.randn(K, N, 512, generator=g).to(DEV) if clip else None
    grads, d_emb = ops.mlp_backward(arena, emb, d_alpha, d_color, d_clip)
    torch.cuda.synchronize()
    return sha(grads, d_emb)


def head_case():
    K, N = 2, 300
    arena = arena_of(K, 128, 512)
    g = torch.Generator().manual_seed(8)
    hfeat = torch.randn(K, N, 128, generator=g).to(DEV)
    weight = torch.rand(K, N, generator=g).to(DEV)
    out = ops.feature_head(arena, hfeat, weight)
    torch.cuda.synchronize()
    return sha(out)


def cases():
    c = []
    # one-launch iteration, hidden 128 (train_step_small)
    c.append(("small128 A fp32 K1 R24 S16 optim", lambda: train_case(128, 1, 24, 4, 12, False, "fp32", with_optim=True)))
    c.append(("small128 A bf16 K3 R10 S64 feat C64 optim", lambda: train_case(128, 3, 10, 16, 48, True, "bf16", C=64, with_optim=True)))
    c.append(("small128 A bf16 K3 R10 S64 feat C64", lambda: train_case(128, 3, 10, 16, 48, True, "bf16", C=64)))
    c.append(("small128 A fp16 K3 R10 S64 feat C64 optim", lambda: train_case(128, 3, 10, 16, 48, True, "fp16", C=64, with_optim=True)))
    # two-launch small path, hidden 128, S = 80
    for mode in ("fp32", "bf16"):
        for feat in (False, True):
            for ctx in (True, False):
                c.append((f"small128 B {mode} K2 R6 S80{' feat' if feat else ''}{'' if ctx else ' no-context'}",
                          lambda mode=mode, feat=feat, ctx=ctx: train_case(128, 2, 6, 20, 60, feat, mode, context=ctx)))
    # general fp32 chain
    for feat in (False, True):
        for ctx in (True, False):
            c.append((f"chain fp32 H64 K2 R24 S16{' feat' if feat else ''}{'' if ctx else ' no-context'}",
                      lambda feat=feat, ctx=ctx: train_case(64, 2, 24, 4, 12, feat, "fp32", context=ctx)))
    c.append(("chain fp32 H288 K1 R16 S16", lambda: train_case(288, 1, 16, 4, 12, False, "fp32")))
    # 16-bit chain, hidden 256, S = 80
    for R in (64, 16):
        for mode in ("bf16", "fp16"):
            for feat in (False, True):
                c.append((f"chain {mode} H256 K1 R{R} S80{' feat' if feat else ''}",
                          lambda R=R, mode=mode, feat=feat: train_case(256, 1, R, 20, 60, feat, mode)))
    # helpers
    for H in (32, 128, 256):
        for clip in (False, True):
            c.append((f"eval_points H{H}{' clip' if clip else ''}", lambda H=H, clip=clip: eval_case(H, clip)))
    for H in (32, 128):
        for clip in (False, True):
            c.append((f"mlp_backward H{H}{' d_clip' if clip else ''}", lambda H=H, clip=clip: backward_case(H, clip)))
    c.append(("feature_head weight", head_case))
    c.append(("fused32 fp32 K2 R24 S16 feat", lambda: train_case(32, 2, 24, 4, 12, True, "fp32")))
    c.append(("fused256 bf16 K1 R33 S32 feat", lambda: train_case(256, 1, 33, 8, 24, True, "bf16")))
    # ---- ray loss: one case per kernel that composites a ray (the kernel named is the one the launch code selects)
    for S, ss in ((16, 0), (64, 64)):
        for feat in (False, True):
            kern = f"train_fused32_kernel<{'true' if feat else 'false'}, false, {ss}>"
            c.append((f"ray loss: fp32 H32 K2 R24 S{S}{' feat' if feat else ''} [{kern}]",
                      lambda S=S, feat=feat: train_case(32, 2, 24, S // 4, S - S // 4, feat, "fp32", labels012=True)))
    for S in (16, 64):
        for feat in (False, True):
            kern = (f"train_fused_bf16_kernel<{'true' if feat else 'false'}>" if S != 64 else
                    "train_fused_bf16v2f_kernel" if feat else "train_fused_bf16v2_kernel")
            c.append((f"ray loss: bf16 H32 K2 R24 S{S}{' feat' if feat else ''} [{kern}]",
                      lambda S=S, feat=feat: train_case(32, 2, 24, S // 4, S - S // 4, feat, "bf16", labels012=True)))
    for mode, ot in (("bf16", "__bf16"), ("fp16", "_Float16")):
        for feat in (False, True):
            kern = f"fwd256_kernel<{ot}, 32, 4, true>" if feat else f"fwdr256_kernel<{ot}, 32>"
            c.append((f"ray loss: {mode} H256 K1 R33 S32{' feat' if feat else ''} [{kern}]",
                      lambda mode=mode, feat=feat: train_case(256, 1, 33, 8, 24, feat, mode, labels012=True)))
    for S, rt in ((16, 5), (64, 4)):        # (RT = 4 when the workgroup's rays x S fit 64 rows: sf_rays_per_wg)
        for feat in (False, True):
            kern = f"train_small_kernel<{rt}, false, {'true' if feat else 'false'}>"
            c.append((f"ray loss: fp32 H128 K1 R24 S{S}{' feat C64' if feat else ''} [{kern}]",
                      lambda S=S, feat=feat: train_case(128, 1, 24, S // 4, S - S // 4, feat, "fp32", C=64, labels012=True)))
    for feat in (False, True):
        c.append((f"ray loss: step_batch_loss K2 R24 S16{' pred_feat C64' if feat else ''} [loss_kernel]",
                  lambda feat=feat: loss_case(feat)))
    return c


def main():
    repeat = "--repeat" in sys.argv[1:]
    only = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--only=")]      # --only=TEXT: cases whose name holds it
    for name, fn in cases():
        if only and not any(o in name for o in only):
            continue
        d = fn()
        note = ""
        if repeat and fn() != d:
            note = "  NOT-REPRODUCIBLE"
        print(f"{name}: {d}{note}", flush=True)


if __name__ == "__main__":
    main()
