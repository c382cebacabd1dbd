"""Meshing on the GPU (Trainer.meshing, trainer.py:46-103): grid evaluation, marching cubes (objnerf_mesh.hip, count
+ scan + 2 emits), the vertex re-query (colour + 512-d feature) and the whole call, at grid_dim 128 and 256 for the
hidden-32 object network and the hidden-128 background network.  Prints one JSON line.  Run on the GPU box."""
import json
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openobj_amd import cfg as ocfg, ops, render_rays, trainer  # noqa: E402

dev = "cuda:0"
HBM_TBPS = 6.3             # measured device copy rate (MI355X_MICROARCH.md)


def timed(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def gpu_ms(fn, reps=10):
    fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def extraction_kernels_ms(vol):
    """count + scan + emit (4 launches) without the host read-back of V / F between them."""
    from openobj_amd._lib import lib
    d = vol.shape[0]
    nb = int(lib().objnerf_mc_workspace_bytes(d))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    cnt = torch.empty(2, dtype=torch.int64, device=dev)
    lib().objnerf_mc_count(d, 0.5, vol.data_ptr(), ws.data_ptr(), nb, cnt.data_ptr(), ops._stream())
    V, F = (int(x) for x in cnt.tolist())
    v = torch.empty(V, 3, device=dev)
    n = torch.empty(V, 3, device=dev)
    f = torch.empty(F, 3, dtype=torch.int32, device=dev)

    def run():
        lib().objnerf_mc_count(d, 0.5, vol.data_ptr(), ws.data_ptr(), nb, cnt.data_ptr(), ops._stream())
        lib().objnerf_mc_emit(d, 0.5, 0, vol.data_ptr(), ws.data_ptr(), nb, V, F, v.data_ptr(), n.data_ptr(),
                              f.data_ptr(), ops._stream())
    return gpu_ms(run), V, F


def skimage_ms(vol_np):
    try:
        import skimage.measure as m
    except ImportError:
        return "not available"
    t0 = time.perf_counter()
    m.marching_cubes(vol_np, 0.5, gradient_direction="ascent")
    return 1e3 * (time.perf_counter() - t0)


def main():
    out = {"metric": "meshing", "hbm_tbps_bound": HBM_TBPS, "cases": []}
    box = types.SimpleNamespace(center=np.array([0.1, -0.2, 0.3]), R=np.eye(3), extent=np.array([1.0, 0.8, 1.2]))
    for hidden in (32, 128):
        c = ocfg.Config(ocfg.replica_room0_config(train_device=dev))
        c.obj_id = 1 if hidden == 32 else 0
        c.hidden_feature_size = hidden
        torch.manual_seed(0)
        t = trainer.Trainer(c)
        oc = torch.tensor([0.1, -0.2, 0.3])
        for dim in (128, 256):
            scale = torch.from_numpy(box.extent / (2 * t.bound_extent)).float()
            T = torch.eye(4)
            T[:3, 3] = torch.from_numpy(box.center).float()
            pc = render_rays.make_3D_grid([-1., 1.], dim, dev, scale=scale, transform=T).view(-1, 3) - oc.to(dev)
            grid_ms = gpu_ms(lambda: t._eval_grid(pc), reps=3)
            occ = t._eval_grid(pc)[0].view(dim, dim, dim).contiguous()
            frac = float((occ > 0.5).float().mean())
            ext_ms, V, F = extraction_kernels_ms(occ)
            ext_call_ms = timed(lambda: ops.marching_cubes(occ))
            verts = ops.marching_cubes(occ)[0]
            rq_ms = timed(lambda: t.eval_points(verts), reps=3) if V else 0.0
            e2e_ms = timed(lambda: t.meshing(box, oc, grid_dim=dim, save_pcd=False, save_mesh=True, if_color=True,
                                             if_part=True), reps=3)
            n = dim ** 3
            # volume read 3x (count, verts, faces; neighbours from cache), base array written + read, outputs
            bytes_ = 3 * 4 * n + 2 * 2 * n + V * 24 + F * 12
            case = dict(hidden=hidden, dim=dim, occupied=round(frac, 4), V=V, F=F, grid_eval_ms=round(grid_ms, 3),
                        extraction_ms=round(ext_ms, 4), extraction_call_ms=round(ext_call_ms, 3),
                        requery_ms=round(rq_ms, 3), meshing_e2e_ms=round(e2e_ms, 2), extraction_bytes=bytes_,
                        extraction_hbm_bound_ms=round(bytes_ / (HBM_TBPS * 1e12) * 1e3, 4),
                        extraction_frac_of_bound=round(bytes_ / (HBM_TBPS * 1e12) * 1e3 / ext_ms, 3),
                        skimage_cpu_ms=skimage_ms(occ.cpu().numpy()))
            out["cases"].append(case)
            print(json.dumps(case), file=sys.stderr, flush=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
