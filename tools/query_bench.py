"""Map-query timings (objnerf_query.hip) -> profiles/query_bench.json.

    python tools/query_bench.py [--out profiles/query_bench.json] [--reps 10]

At one object (100 k x 512) and at the native map (51 such objects): the projection at Q = 1 and 16 (cosine) against
6.3 TB/s of HBM, the moments against the 157 TF fp32 MFMA peak (2 V D^2 flop, D(D+1)/2 columns pairs counted once:
the kernel computes the upper tiles only), the host eigensolve, a whole part query and a whole PCA colouring end to
end, and the baselines: F.cosine_similarity on the device, sklearn's StandardScaler + PCA(3) per object on the CPU.

    python tools/query_bench.py --compact [--out profiles/query_compact_bench.txt] [--reps 20]

The compact map at the native size: a synthetic feature hidden [51 x 100 k, 32] and one head per
object -> ops.part_rows per object, the stored bytes, the part-query pass at Q = 1 and 16 and the PCA colouring end to
end over the rows, and the same figures of the dense map of the very same features (ops.part_expand of the rows) from
the same run."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openobj_amd import ops, query  # noqa: E402

HBM = 6.3e12
F32_MFMA = 157.3e12


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ts = []
    for _ in range(reps):
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        ts.append(ev[0].elapsed_time(ev[1]) * 1e-3)
    return float(np.median(ts))


def one(S, n, D, reps, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    common = torch.randn(D, device=dev, generator=g)
    f = common + 0.5 * torch.randn(S * n, D, device=dev, generator=g)
    f = f / f.norm(dim=1, keepdim=True)
    off = torch.arange(S + 1, dtype=torch.int64) * n
    V = S * n
    r = {"S": S, "rows_per_object": n, "D": D}
    for Q in (1, 16):
        W = torch.randn(D, Q, device=dev, generator=g)
        t = timed(lambda: ops.segment_project(f, off, W, cosine=True), reps)
        by = V * D * 4 + V * Q * 4
        r[f"project_q{Q}_s"] = t
        r[f"project_q{Q}_hbm_fraction"] = by / t / HBM
    t = timed(lambda: ops.segment_moments(f, off), max(2, reps // 2))
    fl = 2.0 * V * D * (D + 1) / 2
    r["moments_s"] = t
    r["moments_mfma_fraction"] = fl / t / F32_MFMA
    mean, sc = ops.segment_moments(f, off)
    m64, s64 = mean.cpu().numpy(), sc.cpu().numpy()
    st = {}
    query.pca_weights(m64, s64, [n] * S, st)
    r["eigh_s"] = st["eigh_s"]
    r["eigh_s_per_object"] = st["eigh_s"] / S
    # whole part query (one object chosen) and whole PCA colouring through MapQuery, packed buffer reused
    mq = query.MapQuery.__new__(query.MapQuery)
    mq.all_obj, mq.keys, mq.dev, mq.D, mq.V = {}, list(range(S)), torch.device(dev), D, V
    mq.seg_host = off.numpy()
    mq.seg_off = off.to(dev)
    mq.part_feat = f
    mq.rgb = torch.zeros(V, 4, dtype=torch.uint8, device=dev)
    mq.ranked = list(range(S))
    mq.clip = torch.randn(S, 512, device=dev, generator=g)
    mq.caption = torch.randn(S, 384, device=dev, generator=g)
    cq, sq, pq = np.random.randn(512), np.random.randn(384), np.random.randn(D)

    def part_query():
        mq.color_by_part_query(cq, sq, pq, 1)
        torch.cuda.synchronize()
    r["part_query_end_to_end_s"] = timed(part_query, reps)

    def pca():
        mq.color_by_partfeat()
        torch.cuda.synchronize()
    r["pca_coloring_end_to_end_s"] = timed(pca, 2)
    # baselines
    q = torch.from_numpy(pq.astype(np.float32)).to(dev)
    r["torch_cosine_one_object_s"] = timed(lambda: torch.nn.functional.cosine_similarity(q[None], f[:n], dim=-1), reps)
    r["torch_cosine_all_objects_s"] = timed(lambda: torch.nn.functional.cosine_similarity(q[None], f, dim=-1), reps)
    try:
        from sklearn.decomposition import PCA
        from sklearn.preprocessing import StandardScaler
        X = f[:n].cpu().numpy()
        t0 = time.perf_counter()
        PCA(n_components=3).fit_transform(StandardScaler().fit_transform(X))
        r["sklearn_pca_per_object_s"] = time.perf_counter() - t0
    except ImportError:
        r["sklearn_pca_per_object_s"] = None
    del f
    torch.cuda.empty_cache()
    return r


def _bare_query(S, n, D, dev):
    mq = query.MapQuery.__new__(query.MapQuery)
    off = torch.arange(S + 1, dtype=torch.int64) * n
    mq.all_obj, mq.keys, mq.dev, mq.D, mq.V = {}, list(range(S)), torch.device(dev), D, S * n
    mq.seg_host = off.numpy()
    mq.seg_off = off.to(dev)
    mq.rgb = torch.zeros(S * n, 4, dtype=torch.uint8, device=dev)
    mq.ranked = list(range(S))
    return mq


def compact(S, n, H, D, reps, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    V = S * n
    common = torch.randn(H, device=dev, generator=g)
    h = (common + 0.5 * torch.randn(V, H, device=dev, generator=g)).abs()
    heads = torch.randn(S, D, H + 1, device=dev, generator=g) * (2.0 / (D + H)) ** 0.5
    buf = torch.zeros(V, H + ops.PART_ROW_PAD, device=dev)
    f = torch.empty(V, D, device=dev)
    w0, b0 = heads[0, :, :H].contiguous(), heads[0, :, H].contiguous()
    r = {"S": S, "rows_per_object": n, "H": H, "D": D,
         "part_rows_per_object_s": timed(lambda: ops.part_rows(h[:n], w0, b0, out=buf[:n]), reps)}
    r["part_rows_per_object_hbm_fraction"] = n * (2 * H + 4) * 4 / r["part_rows_per_object_s"] / HBM
    for s in range(S):
        ops.part_rows(h[s * n:(s + 1) * n], heads[s, :, :H].contiguous(), heads[s, :, H].contiguous(),
                      out=buf[s * n:(s + 1) * n])
        f[s * n:(s + 1) * n] = ops.part_expand(buf[s * n:(s + 1) * n, :H + 1], heads[s])
    del h
    cm, dm = _bare_query(S, n, D, dev), _bare_query(S, n, D, dev)
    dm.part_feat = f
    cm.part_feat = None
    cm.heads = [heads[s] for s in range(S)]
    cm.heads64 = [heads[s].cpu().numpy().astype(np.float64) for s in range(S)]
    cm.compact = [{"s0": 0, "s1": S, "K": H + 1, "buf": buf, "seg": cm.seg_off}]
    r["store_bytes"] = {"compact": cm.store_bytes(), "dense": dm.store_bytes()}
    r["store_ratio"] = dm.store_bytes() / cm.store_bytes()
    for name, mq, row in (("dense", dm, D), ("compact", cm, H + ops.PART_ROW_PAD)):
        for Q in (1, 16):
            q = torch.randn(Q, D, device=dev, generator=g)
            t = timed(lambda: mq.part_similarity(q), reps)
            r[f"{name}_part_query_q{Q}_s"] = t
            r[f"{name}_part_query_q{Q}_hbm_fraction"] = (V * row * 4 + V * Q * 4) / t / HBM

        def pca():
            mq.color_by_partfeat()
            torch.cuda.synchronize()
        r[f"{name}_pca_coloring_end_to_end_s"] = timed(pca, 2 if name == "dense" else reps)
        st = {}
        mq.color_by_partfeat(st)
        r[f"{name}_pca_eigh_s"] = st["eigh_s"]
    for Q in (1, 16):           # the device pass alone: the per-segment columns already formed and uploaded
        W = cm._columns(cm.compact[0], [np.random.randn(H + 1, Q) for _ in range(S)])
        t = timed(lambda: ops.segment_project(buf, cm.seg_off, W), reps)
        r[f"compact_project_q{Q}_s"] = t
        r[f"compact_project_q{Q}_hbm_fraction"] = (V * (H + ops.PART_ROW_PAD) * 4 + V * Q * 4) / t / HBM
    for Q in (1, 16):
        r[f"part_query_q{Q}_speedup"] = r[f"dense_part_query_q{Q}_s"] / r[f"compact_part_query_q{Q}_s"]
    r["pca_coloring_speedup"] = r["dense_pca_coloring_end_to_end_s"] / r["compact_pca_coloring_end_to_end_s"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--compact", action="store_true", help="the compact map against the dense one (DESIGN.md 4.25)")
    a = ap.parse_args()
    dev = "cuda:0"
    if a.compact:
        res = {"device": torch.cuda.get_device_name(0), "hbm_peak_Bps": HBM, "reps": a.reps or 20,
               "native_map": compact(51, 100_000, 32, 512, a.reps or 20, dev)}
        out = a.out or os.path.join(ROOT, "profiles", "query_compact_bench.txt")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as fh:
            fh.write("python tools/query_bench.py --compact\n" + json.dumps(res, indent=1) + "\n")
        print(json.dumps(res, indent=1))
        return
    a.out = a.out or os.path.join(ROOT, "profiles", "query_bench.json")
    a.reps = a.reps or 10
    res = {"device": torch.cuda.get_device_name(0), "hbm_peak_Bps": HBM, "fp32_mfma_peak_flops": F32_MFMA,
           "one_object": one(1, 100_000, 512, a.reps, dev), "native_map": one(51, 100_000, 512, a.reps, dev)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
