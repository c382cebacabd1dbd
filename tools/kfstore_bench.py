"""Dense against cropped keyframe stores (openobj_amd/kf_store.py) at the native shape: a 1200 x 680 camera, K = 50
objects, 20 keyframe slots each, 2-D boxes of 40 - 400 px a side; inside a box an ellipse of "this
object" pixels with a ring of unknown ones, depth in U(0.5, 6) m with 5 % zeros.  Both kinds are filled from the same
20 frames and measured in the same process, alternating:

  * store bytes (keyframe pixels held on the device),
  * ingest of one frame into all K objects, twice: the launch alone (objnerf_ingest_frame / objnerf_ingest_frame_crops on
    an item table that is already on the device: what the kernels write) and the whole call (ops.ingest_frame /
    ops.ingest_frame_crops: rects, reservations, the ctypes item table and its pageable upload, then the launch; the
    stream is idle while the host works, so this figure is mostly host time),
  * the stacked seeded pool draw, 500 x 24 rays per object (objnerf_sample_rays_stacked / objnerf_sample_rays_crops),
  * the keyframe scan of the bounds (objnerf_voxel_scan, all 20 slots of every object).

Every time is between two HIP events on the stream, after a warm-up, the median of --runs (default 20) runs; the whole
measurement is repeated --repeats (default 5) times and the spread (max - min) / median of the dense store's medians
over the repeats stands beside each figure: a cropped figure may exceed the dense one by no more than that.
Writes the report to --out (default profiles/kfstore_bench.txt) and prints it.  Run on the GPU."""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openobj_amd import _lib, ops  # noqa: E402
from openobj_amd.kf_store import KeyframeCropStore, crop_rect  # noqa: E402

W, H, K, F = 1200, 680, 50, 20
N_FRAMES, N_PX = 500, 24
INTR = (600.0, 600.0, 599.5, 339.5)


def make_frame(rs, dev):
    """One frame: (rgb u8 [W,H,3], depth [W,H], inst int32 [W,H]) on the device and the K boxes."""
    rgb = torch.from_numpy(rs.randint(0, 256, (W, H, 3)).astype(np.uint8)).to(dev)
    depth = rs.uniform(0.5, 6.0, (W, H)).astype(np.float32)
    depth[rs.rand(W, H) < 0.05] = 0.0
    inst = np.zeros((W, H), np.int32)
    boxes = []
    for k in range(K):
        bw, bh = rs.randint(40, 401), rs.randint(40, 401)
        x0, y0 = rs.randint(0, W - bw), rs.randint(0, H - bh)
        boxes.append([float(x0), float(x0 + bw - 1), float(y0), float(y0 + bh - 1)])
        xx, yy = np.mgrid[0:bw, 0:bh]
        r = ((xx - (bw - 1) / 2) / (bw / 2)) ** 2 + ((yy - (bh - 1) / 2) / (bh / 2)) ** 2
        patch = inst[x0:x0 + bw, y0:y0 + bh]
        patch[r <= 1.0] = -1                                    # the ring of unknown pixels ...
        patch[r <= 0.81] = k + 1                                # ... around the object's own
    return rgb, torch.from_numpy(depth).to(dev), torch.from_numpy(inst).to(dev), boxes


def event_ms(fn, runs, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "kfstore_bench.txt"))
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(1234)
    lib = _lib.lib()
    twc = torch.eye(4, device=dev)

    dense = [(torch.empty(F, W, H, 4, dtype=torch.uint8, device=dev), torch.empty(F, W, H, device=dev),
              torch.empty(F, 4, 4, device=dev), torch.empty(F, 4, device=dev)) for _ in range(K)]
    crops = [KeyframeCropStore(F, W, H, dev) for _ in range(K)]
    outside = torch.zeros(K, dtype=torch.int32, device=dev)
    frames = [make_frame(rs, dev) for _ in range(F)]

    def ingest_dense(slot):
        rgb, depth, inst, boxes = frames[slot]
        ops.ingest_frame(rgb, depth, inst, twc, [(dense[k], slot, k + 1, boxes[k]) for k in range(K)])

    def ingest_crops(slot):
        rgb, depth, inst, boxes = frames[slot]
        ops.ingest_frame_crops(rgb, depth, inst, twc, [(crops[k], slot, k + 1, boxes[k]) for k in range(K)], outside)

    for slot in range(F):                                       # fill both kinds (the arenas reach their final size here)
        ingest_dense(slot)
        ingest_crops(slot)
    torch.cuda.synchronize()
    assert outside.tolist() == [0] * K
    versions = [c.version for c in crops]
    bytes_dense = sum(s[0].numel() + 4 * s[1].numel() for s in dense)
    bytes_crop = sum(c.nbytes for c in crops)
    px_crop = sum(int(c.rect_host[:, 2:].prod(axis=1).sum()) for c in crops)
    for k in (0, K - 1):                                        # the two kinds hold the same pixels inside the rects
        for slot in (0, F - 1):
            x0, y0, cw, ch = crop_rect(frames[slot][3][k], W, H)
            rgbs, d = crops[k].frame(slot)
            assert torch.equal(rgbs[x0:x0 + cw, y0:y0 + ch], dense[k][0][slot, x0:x0 + cw, y0:y0 + ch])
            assert torch.equal(d[x0:x0 + cw, y0:y0 + ch], dense[k][1][slot, x0:x0 + cw, y0:y0 + ch])

    # ---- the sampler's and the scan's arguments
    tab_d, tab_c = ops.keyframe_table(dense), ops.keyframe_table(crops)
    cache = ops.rays_dirs(W, H, *INTR, dev)
    meta = torch.tensor([[F - 1, F - 3, F - 2, k + 1] for k in range(K)], dtype=torch.int32, device=dev)

    def draw(table):
        return ops.sample_rays_seeded(table, F, W, H, cache, meta, N_FRAMES, N_PX, 1, 9, 0.1, 0.05, seed=42, draw=7)

    a, b = draw(tab_d), draw(tab_c)
    for key in a:
        assert (a[key] is None and b[key] is None) or torch.equal(a[key], b[key]), key
    del a, b

    nk = torch.full((K,), F, dtype=torch.int32, device=dev)
    poses = torch.eye(4, dtype=torch.float64, device=dev).repeat(K, F, 1, 1).contiguous()
    nb = int(lib.objnerf_voxel_workspace_bytes(K, F, W, H))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    total = torch.empty(K, dtype=torch.int64, device=dev)
    minmax = torch.empty(K, 6, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def scan(table):
        cropped = table.shape[1] == 5
        va = _lib.VoxelArgs(K, F, W, H, *INTR, 0.05, None if cropped else table.data_ptr(), nk.data_ptr(),
                            poses.data_ptr(), table.data_ptr() if cropped else None)
        _lib.check(lib.objnerf_voxel_scan(C.byref(va), ws.data_ptr(), nb, total.data_ptr(), minmax.data_ptr(), st),
                   "objnerf_voxel_scan")

    scan(tab_d)
    tot_d, mm_d = total.clone(), minmax.clone()
    scan(tab_c)
    assert torch.equal(total, tot_d) and torch.equal(minmax, mm_d) and int(tot_d.sum()) > 0
    points = int(tot_d.sum())

    # ---- item tables resident on the device, one per slot and kind: the ingest launch without its host preparation
    def item_table(rows, struct):
        arr = (struct * K)(*rows)
        return torch.from_numpy(np.frombuffer(arr, dtype=np.uint8).copy()).to(dev)

    f4, i4 = C.c_float * 4, C.c_int32 * 4
    items_d = [item_table([_lib.IngestItem(*[t.data_ptr() for t in dense[k]], slot, k + 1, f4(*frames[slot][3][k]))
                           for k in range(K)], _lib.IngestItem) for slot in range(F)]
    items_c = [item_table([_lib.IngestCropItem(_lib.KfCrops(*crops[k].descriptor()), slot, k + 1, f4(*frames[slot][3][k]),
                                               i4(*crop_rect(frames[slot][3][k], W, H))) for k in range(K)],
                          _lib.IngestCropItem) for slot in range(F)]

    def launch_dense(slot):
        rgb, depth, inst, _ = frames[slot]
        _lib.check(lib.objnerf_ingest_frame(W, H, rgb.data_ptr(), depth.data_ptr(), inst.data_ptr(), twc.data_ptr(), K,
                                            items_d[slot].data_ptr(), st), "objnerf_ingest_frame")

    def launch_crops(slot):
        rgb, depth, inst, _ = frames[slot]
        _lib.check(lib.objnerf_ingest_frame_crops(W, H, rgb.data_ptr(), depth.data_ptr(), inst.data_ptr(), twc.data_ptr(), K,
                                                  items_c[slot].data_ptr(), outside.data_ptr(), st),
                   "objnerf_ingest_frame_crops")

    # ---- timing: dense and cropped alternate inside every repeat
    slots = iter(range(10 ** 9))
    work = {"ingest_launch_ms": (lambda: launch_dense(next(slots) % F), lambda: launch_crops(next(slots) % F)),
            "ingest_call_ms": (lambda: ingest_dense(next(slots) % F), lambda: ingest_crops(next(slots) % F)),
            "pool_draw_ms": (lambda: draw(tab_d), lambda: draw(tab_c)),
            "bounds_scan_ms": (lambda: scan(tab_d), lambda: scan(tab_c))}
    res = {name: {"dense": [], "crop": []} for name in work}
    for _ in range(args.repeats):
        for name, (fd, fc) in work.items():
            res[name]["dense"].append(event_ms(fd, args.runs))
            res[name]["crop"].append(event_ms(fc, args.runs))
    torch.cuda.synchronize()
    assert [c.version for c in crops] == versions and outside.tolist() == [0] * K       # no arena moved while timing

    lines = ["keyframe stores, dense against crop: %d x %d camera, K = %d objects, F = %d slots, boxes 40 - 400 px a side"
             % (W, H, K, F),
             "device: %s; times between HIP events, median of %d runs after 3 warm-up runs, %d repeats, dense and crop"
             % (torch.cuda.get_device_name(0), args.runs, args.repeats),
             "alternating in one process; spread = (max - min) / median of the dense store's medians over the repeats",
             "",
             "store bytes   dense %d (%.1f MB per object)   crop %d (%.1f MB per object)   ratio %.1f x"
             % (bytes_dense, bytes_dense / K / 1e6, bytes_crop, bytes_crop / K / 1e6, bytes_dense / bytes_crop),
             "              pixels inside the rects: %d (%.1f %% of the arena's capacity); points of the scan: %d"
             % (px_crop, 100.0 * px_crop * 8 / bytes_crop, points),
             ""]
    ok = True
    for name, r in res.items():
        md, mc = statistics.median(r["dense"]), statistics.median(r["crop"])
        spread = (max(r["dense"]) - min(r["dense"])) / md
        within = mc <= md * (1.0 + spread)
        ok = ok and within
        lines.append("%-20s dense %9.4f ms (spread %5.1f %%)   crop %9.4f ms   crop / dense %.3f   %s"
                     % (name, md, 100 * spread, mc, mc / md, "within the spread" if within else "SLOWER THAN THE SPREAD"))
        lines.append("%-20s dense medians %s" % ("", " ".join("%.4f" % v for v in r["dense"])))
        lines.append("%-20s crop medians  %s" % ("", " ".join("%.4f" % v for v in r["crop"])))
    lines.append("")
    lines.append("pool draw: %d x %d rays per object, seeded, origins + directions form, the whole ops call" % (N_FRAMES, N_PX))
    lines.append("ingest_launch: one frame into all %d objects, the launch alone, item table resident on the device" % K)
    lines.append("ingest_call: the same through ops.ingest_frame / ops.ingest_frame_crops: host preparation (rects,")
    lines.append("reservations, ctypes item table, pageable upload) runs between the two events on an idle stream and is")
    lines.append("most of the figure; the cropped call does more of it (a rect and a reservation per item)")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
