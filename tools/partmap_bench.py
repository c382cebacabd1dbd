"""Compact part-level feature maps at the reference's native shape: a 1200 x 680 camera, down_sample 5 (240 x 136 part
maps), M = 100 masks per frame, C = 512, K = 50 objects, 500 x 24 rays per object and sampler call.  Reports
  * the builder per frame (python -m openobj_amd.part_maps: strided masks -> index kernel -> compaction; and with --dense),
  * per-frame ingest from pageable host memory, dense ([W', H', C] copied into the mapper's buffer, a fresh host
    tensor per repetition) against compact (PartStore.append: into a store with room, and into a new store),
  * bytes on disk and on the device per frame, both forms, as the files and buffers of this run have them,
  * the stacked sampler launch with the dense gather and with the gather through the index, alternating in one process.
Every time is the median of 3 after a warm-up (min and max beside it), a host clock around work that ends in a device
synchronise.  Prints one JSON line; --out FILE also writes it there.  Run on the GPU."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openobj_amd import ops  # noqa: E402
from openobj_amd import part_maps as pm  # noqa: E402

W, H, DOWN, M, C = 1200, 680, 5, 100, 512
K, N_FRAMES, N_PX, F_SLOTS, PART_FRAMES = 50, 500, 24, 8, 8


def timed(fn, reps=3):
    fn()                                            # warm-up: code objects, allocator
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def synthetic_masks(rs):
    """SAM-like input of one frame: M rectangles of 2 - 25 % of the image side, fp16 features, scores."""
    seg = np.zeros((M, H, W), bool)
    for m in range(M):
        h, w = rs.randint(H // 50, H // 4), rs.randint(W // 50, W // 4)
        y, x = rs.randint(0, H - h), rs.randint(0, W - w)
        seg[m, y:y + h, x:x + w] = True
    return {"segmentation": seg, "stability_score": rs.uniform(0.9, 1.0, M), "feat": rs.randn(M, C).astype(np.float16)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(0)
    out = {"W": W, "H": H, "down_sample": DOWN, "masks": M, "C": C, "K": K, "rays_per_object": N_FRAMES * N_PX}

    # ---- the builder
    frame = synthetic_masks(rs)
    out["build_compact"] = timed(lambda: pm.build_frame(frame, DOWN, dev))
    out["build_with_dense"] = timed(lambda: pm.build_frame(frame, DOWN, dev, dense=True))
    masks_dev = torch.from_numpy(pm.strided_masks(frame, DOWN)).to(dev)
    out["index_kernel_call"] = timed(lambda: ops.part_index(masks_dev))
    index, table, dense = pm.build_frame(frame, DOWN, dev, dense=True)
    out["masks_used"] = int(table.shape[0])
    out["uncovered_fraction"] = round(float((index < 0).mean()), 4)

    # ---- bytes on disk
    with tempfile.TemporaryDirectory() as tmp:
        pm.save_compact(os.path.join(tmp, "0.npz"), index, table)
        np.save(os.path.join(tmp, "0.npy"), dense)
        out["disk_bytes_compact"] = os.path.getsize(os.path.join(tmp, "0.npz"))
        out["disk_bytes_dense"] = os.path.getsize(os.path.join(tmp, "0.npy"))

    # ---- ingest from host memory: what mapping.ingest does with the frame's part map
    part_host = torch.from_numpy(dense.transpose(1, 0, 2).copy())                   # [W', H', C] as dataset.py returns it
    idx_host, tab_host = pm.shifted(index, table)
    idx_host = idx_host.t().contiguous()
    buf = torch.empty((PART_FRAMES,) + tuple(part_host.shape), device=dev)

    # every repetition copies from a host tensor made for it, so that no repetition finds its source pages already
    # touched by an earlier copy; the clones are made before the clock starts
    fresh = iter([part_host.clone() for _ in range(4)])

    def ingest_dense():
        buf[0] = next(fresh).to(dev)

    def ingest_compact_first():                     # a new store: buffer allocation and zero fill included
        pm.PartStore(dev).append(idx_host, tab_host)

    steady = pm.PartStore(dev)
    for _ in range(9):                              # past both buffers' growth steps: the next four appends find room
        steady.append(idx_host, tab_host)

    def ingest_compact():                           # the steady state: appended to a store that has room
        if steady.n_frames == steady._index_buf.shape[0] or steady.n_rows + tab_host.shape[0] > steady._table_buf.shape[0]:
            raise RuntimeError("the steady-state store would grow")
        steady.append(idx_host, tab_host)

    out["host_memory"] = "pageable (torch.from_numpy / clone, not pinned)"
    out["ingest_dense"] = timed(ingest_dense)
    out["ingest_compact_new_store"] = timed(ingest_compact_first)
    out["ingest_compact"] = timed(ingest_compact)

    # ---- the two stores the sampler reads: PART_FRAMES frames, each with its own masks
    store = pm.PartStore(dev)
    for f in range(PART_FRAMES):
        fr = synthetic_masks(rs)
        i_f, t_f, _ = pm.build_frame(fr, DOWN, dev)
        i_s, t_s = pm.shifted(i_f, t_f)
        store.append(i_s.t().contiguous(), t_s)
    dense_all = store.dense()                                                       # [frames, W', H', C]
    out["device_bytes_per_frame_compact"] = store.nbytes() // PART_FRAMES
    out["device_bytes_per_frame_dense"] = dense_all.numel() * 4 // PART_FRAMES
    out["table_rows"] = int(store.n_rows)

    # ---- the stacked sampler launch, K objects
    gen = torch.Generator(device=dev).manual_seed(1)
    stores = []
    for _ in range(K):
        rgbs = torch.randint(0, 255, (F_SLOTS, W, H, 4), dtype=torch.uint8, device=dev, generator=gen)
        depth = 1.0 + 2.0 * torch.rand(F_SLOTS, W, H, device=dev, generator=gen)
        t_wc = torch.eye(4, device=dev).repeat(F_SLOTS, 1, 1)
        bbox = torch.tensor([[100.0, 700.0, 80.0, 500.0]], device=dev).repeat(F_SLOTS, 1)
        stores.append((rgbs, depth, t_wc, bbox))
    table_kf = ops.keyframe_table(stores)
    cache = ops.rays_dirs(W, H, 600.0, 600.0, 599.5, 339.5, dev)
    meta = torch.tensor([[F_SLOTS, F_SLOTS - 2, F_SLOTS - 1, k] for k in range(K)], dtype=torch.int32, device=dev)
    use_frame = np.tile(np.arange(F_SLOTS, dtype=np.float64) * 10, (K, 1))          # slot s holds dataset frame 10 s

    def sample(src):
        return ops.sample_rays_seeded(table_kf, F_SLOTS, W, H, cache, meta, N_FRAMES, N_PX, 1, 9, 0.1, 0.05, seed=3,
                                      draw=5, partfeat=(src, use_frame, 10, DOWN))

    a, b = sample(dense_all), sample(store)
    assert torch.equal(a["partfeat"], b["partfeat"]) and bool(a["partfeat"].any())
    del a, b
    runs = {"dense": [], "indexed": []}
    for _ in range(3):                                                              # alternating, same process
        for name, src in (("dense", dense_all), ("indexed", store)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sample(src)
            torch.cuda.synchronize()
            runs[name].append(1e3 * (time.perf_counter() - t0))
    for name, ts in runs.items():
        out["sampler_" + name] = {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3),
                                  "max_ms": round(max(ts), 3)}
    out["sampler_out_bytes"] = K * N_FRAMES * N_PX * C * 4
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
