"""Scoring rendered map views against the frames of the sequence on the GPU: PSNR, an exact-integer SSIM, the depth
error against the sensor's depth and the 2-D instance confusion of the mask-id image (objnerf_view_compare, DESIGN.md
4.26).  The reference's `cfg.if_render` loop (train.py:550-612) writes rgb_ / depth_ / maskid_<id>.png to be compared
with the input by eye; this compares them.

    python -m openobj_amd.map_view_eval --logdir DIR --config scene.json [--frames a:b:s] --out DIR [--bg-ids 0]
                                        [--device cuda:0] [--write-images] [--ssim-maps] [--renders DIR] [--depth-scale S]

Without --renders every selected sample is rendered with MapView and scored on the device against the dataset's sample
(image, depth, obj); with --renders DIR the rgb_ / depth_ / maskid_<id>.png of DIR are scored instead -- an earlier
map_view run, or the reference's own output.  An 8-bit depth_<id>.png holds whole metres: depth is scored from files only
when --depth-scale S says they are the 16-bit round(depth * S) images (a saturated 65535 reads as "nothing wrote depth").
Mask ids above 255 wrapped in those files; the report says so when the map holds one.

Everything accumulated is an integer (ViewEval.acc [G + 1, 9], .conf [G, G + 1]; the columns stand in
include/objnerf_hip.h), so a sequence's tables are the same bytes in every run, grid and frame order, and
eval_views.json, derived from them in fp64 on the host, is the same file."""
from __future__ import annotations

import argparse
import json
import math
import os
from typing import Dict, Iterable, List, Optional

import numpy as np
import torch

from . import _lib, map_points, ops

TAPS = (67, 498, 2359, 7167, 13960, 17434, 13960, 7167, 2359, 498, 67)      # sum 2^16; the header gives the derivation
Q_ONE = 4294967296.0          # 2^32: q of a pixel whose windows are identical
DEPTH_ONE = 1048576.0         # 2^20: column 6 counts metres in these units
NO_DEPTH = 100.0              # what a pixel no foreground object wrote holds (train.py:566)
MAX_ID = 1 << 24              # the lut is dense over [0, max id]
COLUMNS = ("n", "n_painted", "se", "se_painted", "n_depth_gt", "n_depth", "depth_sum", "n_ssim", "q_sum")


def build_lut(ids: Iterable[int]) -> np.ndarray:
    """ids (distinct, 0 <= id < 2^24; their order is the row order) -> lut int32 [max id + 1], -1 where an id has no row."""
    ids = [int(i) for i in ids]
    if not ids:
        raise ValueError("ViewEval: no id")
    if len(set(ids)) != len(ids):
        raise ValueError("ViewEval: duplicate ids")
    if min(ids) < 0 or max(ids) >= MAX_ID:
        raise ValueError(f"ViewEval: ids must lie in [0, {MAX_ID})")
    if len(ids) > ops.VIEW_EVAL_MAX_ROWS:
        raise ValueError(f"ViewEval: more than {ops.VIEW_EVAL_MAX_ROWS} ids")
    lut = np.full(max(ids) + 1, -1, np.int32)
    lut[ids] = np.arange(len(ids), dtype=np.int32)
    return lut


def _ratio(a: float, b: float) -> float:
    return float("nan") if b == 0 else a / b


def figures(row) -> Dict[str, float]:
    """One row of acc (or a sum of rows), nine integers -> the derived figures in fp64.  An empty row gives NaN."""
    n, n_p, se, se_p, n_dg, n_d, d_sum, n_s, q_sum = (int(v) for v in row)

    def psnr(count, err):
        if count == 0:
            return float("nan")
        return float("inf") if err == 0 else 10.0 * math.log10(65025.0 * 3.0 * float(count) / float(err))

    return {"psnr": psnr(n, se), "psnr_painted": psnr(n_p, se_p), "ssim": _ratio(float(q_sum), float(n_s) * Q_ONE),
            "depth_l1": _ratio(float(d_sum), DEPTH_ONE * float(n_d)), "depth_coverage": _ratio(float(n_d), float(n_dg)),
            "painted_share": _ratio(float(n_p), float(n))}


def derive(acc: np.ndarray, conf: np.ndarray, ids: List[int], depth_scored: bool = True) -> dict:
    """The integer tables -> the report: "image" (the column sums), "per_id" (one entry per id, with its iou), "other"
    (row G: the pixels whose ground-truth id has no row), miou and accuracy through map_points.miou, and the tables."""
    acc, conf = np.asarray(acc, np.int64), np.asarray(conf, np.int64)
    G = len(ids)
    if acc.shape != (G + 1, len(COLUMNS)) or conf.shape != (G, G + 1):
        raise ValueError(f"derive: acc [{G + 1}, {len(COLUMNS)}], conf [{G}, {G + 1}], got {acc.shape}, {conf.shape}")

    def fig(row):
        f = figures(row)
        if not depth_scored:
            f["depth_l1"] = f["depth_coverage"] = None
        return f

    m = map_points.miou(torch.from_numpy(conf))
    iou = [float(v) for v in m["iou"]]
    per_id = {}
    for r, i in enumerate(ids):
        per_id[int(i)] = dict(fig(acc[r]), iou=iou[r])
    return {"image": fig(acc.sum(0)), "per_id": per_id, "other": fig(acc[G]), "iou": iou, "miou": float(m["miou"]),
            "accuracy": float(m["accuracy"]), "acc": acc, "conf": conf, "ids": [int(i) for i in ids]}


class ViewEval:
    def __init__(self, ids: Iterable[int], device="cuda:0", per_frame: bool = False):
        """ids: the ids that get a row of the tables, in row order.  per_frame: also keep every frame's whole-image
        integers (.frame_rows(): one [9] copy per frame)."""
        self.ids = [int(i) for i in ids]
        self.G = len(self.ids)
        self.device = dev = torch.device(device)
        self.lut = torch.from_numpy(build_lut(self.ids)).to(dev)
        self.acc = torch.zeros(self.G + 1, ops.VIEW_EVAL_COLS, dtype=torch.int64, device=dev)
        self.conf = torch.zeros(self.G, self.G + 1, dtype=torch.int64, device=dev)
        self.per_frame, self._frames = bool(per_frame), []
        self.n_frames, self.depth_scored, self.ssim_map = 0, True, None

    @classmethod
    def from_map(cls, mv, per_frame: bool = False) -> "ViewEval":
        """The ids the mask-id image of a MapView can hold: the second column of mv.info, duplicates (two objects of one
        class) once, in first-seen order.  (An object that writes id 0 shares it with "nothing painted".)"""
        seen = []
        for i in mv.info[:, 1].cpu().tolist():
            if i not in seen:
                seen.append(int(i))
        return cls(seen, mv.device, per_frame=per_frame)

    def _dev(self, t, dtype):
        t = t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t))
        return t.to(self.device, dtype).contiguous()

    def _add(self, rgb_r, depth_r, id_r, painted, rgb_g, depth_g, id_g, ssim_map, _workgroups):
        acc = torch.zeros_like(self.acc) if self.per_frame else self.acc
        self.ssim_map = ops.view_compare(rgb_r, depth_r, id_r, painted, rgb_g, depth_g, id_g, self.lut, self.G, acc,
                                         self.conf, want_ssim_map=ssim_map, _workgroups=_workgroups)
        if self.per_frame:
            self.acc += acc
            self._frames.append(acc.sum(0))
        self.n_frames += 1

    def add(self, view: Dict[str, torch.Tensor], frame: dict, ssim_map: bool = False, _workgroups: int = 0) -> None:
        """view: the dict of MapView.render(to_host=False); frame: image uint8 [W, H, 3], depth fp32 [W, H], obj int32
        [W, H] as a dataset sample holds them.  The view is only read.  ssim_map: keep this frame's map in .ssim_map."""
        self._add(self._dev(view["rgb"], torch.uint8), self._dev(view["depth"], torch.float32),
                  self._dev(view["maskid"], torch.int32), (view["winner"] >= 0).to(self.device),
                  self._dev(frame["image"], torch.uint8), self._dev(frame["depth"], torch.float32),
                  self._dev(frame["obj"], torch.int32), ssim_map, _workgroups)

    def add_images(self, rgb_r, depth_r, id_r, rgb_g, depth_g, id_g, ssim_map: bool = False, _workgroups: int = 0) -> None:
        """The same for arrays that come from files ([W, H(, 3)]); there is no winner, so every pixel counts as painted.
        depth_r None: the files hold no usable depth -- the depth figures of the whole result are reported as None."""
        rgb_r = self._dev(rgb_r, torch.uint8)
        if depth_r is None:
            self.depth_scored = False
            depth_r = torch.full(rgb_r.shape[:2], NO_DEPTH, device=self.device)
        self._add(rgb_r, self._dev(depth_r, torch.float32), self._dev(id_r, torch.int32), None,
                  self._dev(rgb_g, torch.uint8), self._dev(depth_g, torch.float32), self._dev(id_g, torch.int32),
                  ssim_map, _workgroups)

    def frame_rows(self) -> np.ndarray:
        """int64 [n_frames, 9]: every frame's whole-image integers (per_frame=True)."""
        if not self.per_frame:
            raise _lib.ObjnerfError("ViewEval: built without per_frame=True")
        if not self._frames:
            return np.zeros((0, ops.VIEW_EVAL_COLS), np.int64)
        return torch.stack(self._frames).cpu().numpy()

    def result(self) -> dict:
        """Reads the tables back once -> derive(); with per_frame also "per_frame": a list of figures()."""
        res = derive(self.acc.cpu().numpy(), self.conf.cpu().numpy(), self.ids, self.depth_scored)
        res["frames"] = self.n_frames
        if self.per_frame:
            rows = self.frame_rows()
            res["frame_rows"] = rows
            res["per_frame"] = [figures(r) for r in rows]
            if not self.depth_scored:
                for f in res["per_frame"]:
                    f["depth_l1"] = f["depth_coverage"] = None
        return res


# ----------------------------------------------------------------------------------------------------------------- CLI
def read_view(renders: str, frame_id: int, depth_scale: Optional[float]):
    """rgb_ / depth_ / maskid_<id>.png as map_view.write_view (and train.py:599-611) writes them, back in [W, H]:
    -> (rgb uint8 [W, H, 3], depth fp32 [W, H] | None, maskid int32 [W, H]).  Depth only with depth_scale, from a 16-bit
    file; its saturated value 65535 reads as NO_DEPTH."""
    from PIL import Image

    def png(name):
        f = os.path.join(renders, f"{name}_{frame_id}.png")
        if not os.path.exists(f):
            raise FileNotFoundError(f"--renders: {f} is missing")
        return np.asarray(Image.open(f))

    rgb, mid = png("rgb"), png("maskid")
    if rgb.ndim != 3 or rgb.shape[2] != 3 or rgb.dtype != np.uint8 or mid.shape != rgb.shape[:2]:
        raise ValueError(f"--renders: frame {frame_id}: rgb [H, W, 3] uint8 and maskid [H, W], got {rgb.shape}, {mid.shape}")
    depth = None
    if depth_scale is not None:
        raw = png("depth")
        if raw.dtype != np.uint16 or raw.shape != mid.shape:
            raise ValueError(f"--renders: --depth-scale needs 16-bit depth PNGs [H, W], frame {frame_id} holds {raw.dtype} {raw.shape}")
        depth = (raw.astype(np.float64) / float(depth_scale)).astype(np.float32)
        depth[raw == 65535] = NO_DEPTH
        depth = np.ascontiguousarray(depth.T)
    return np.ascontiguousarray(rgb.transpose(1, 0, 2)), depth, np.ascontiguousarray(mid.astype(np.int32).T)


def ssim_png(ssim_map: np.ndarray) -> np.ndarray:
    """uint8 [H, W]: rint(255 * clip(ssim, 0, 1)), 0 outside the interior."""
    v = np.nan_to_num(np.asarray(ssim_map, np.float64), nan=0.0)
    return np.ascontiguousarray(np.rint(np.clip(v, 0.0, 1.0) * 255.0).astype(np.uint8).T)


def _plain(v):
    """JSON without NaN / Infinity tokens: NaN -> null, +-inf -> "inf" / "-inf"; arrays -> lists."""
    if isinstance(v, dict):
        return {str(k): _plain(x) for k, x in v.items()}
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, float):
        if math.isnan(v):
            return None
        if math.isinf(v):
            return "inf" if v > 0 else "-inf"
    return v


def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m openobj_amd.map_view_eval", description=__doc__.splitlines()[0])
    ap.add_argument("--logdir", required=True, help="reads DIR/ckpt/<id>/obj_<id>.pth: the map, and the ids that get a row")
    ap.add_argument("--config", required=True, help="the scene's config (dataset path, format, camera)")
    ap.add_argument("--frames", default=None, help="a:b:s over the samples of the config's dataset (default: all)")
    ap.add_argument("--out", required=True, help="eval_views.json (and the images asked for) go here")
    ap.add_argument("--bg-ids", type=int, nargs="*", default=[0])
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--write-images", action="store_true", help="also write the rendered rgb_ / depth_ / maskid_<id>.png")
    ap.add_argument("--ssim-maps", action="store_true", help="write ssim_<id>.png, 8 bits, [H, W]")
    ap.add_argument("--renders", default=None, help="score the PNGs of DIR instead of rendering")
    ap.add_argument("--depth-scale", type=float, default=None,
                    help="the depth PNGs are 16-bit round(depth * S): read (--renders) or written (--write-images) so")
    return ap


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)
    if a.renders and a.write_images:
        ap.error("--write-images renders; it cannot go with --renders")
    if a.depth_scale is not None and not (a.renders or a.write_images):
        ap.error("--depth-scale needs --renders or --write-images")
    if a.depth_scale is not None and not a.depth_scale > 0:
        ap.error("--depth-scale must be positive")
    if a.renders and not os.path.isdir(a.renders):
        ap.error(f"--renders: {a.renders} is no directory")
    from . import dataset, map_view, vmap
    from .cfg import Config
    from .render_view import ViewBuffers
    frames_of = lambda n: map_view.parse_frames(a.frames, n)
    try:
        frames_of(1)
    except ValueError as e:
        ap.error(str(e))
    c = Config(a.config)
    if c.dataset_format not in ("Replica", "ScanNet"):
        raise ValueError("Dataset format {} not found".format(c.dataset_format))
    ds = (dataset.Replica if c.dataset_format == "Replica" else dataset.ScanNet)(c)
    mv = map_view.MapView.from_logdir(a.logdir, a.device, bg_ids=a.bg_ids)
    ev = ViewEval.from_map(mv, per_frame=True)
    rays = None if a.renders else vmap.cameraInfo(c).rays_dir_cache
    os.makedirs(a.out, exist_ok=True)
    frame_ids = []
    for i in frames_of(len(ds)):
        frame_id = int(ds.start + i * ds.stride)
        sample = ds[i]
        if a.renders:
            rgb, depth, mid = read_view(a.renders, frame_id, a.depth_scale)
            ev.add_images(rgb, depth, mid, sample["image"], sample["depth"], sample["obj"], ssim_map=a.ssim_maps)
        else:
            view = mv.render(np.asarray(sample["T"], np.float32), rays, to_host=False)
            ev.add(view, sample, ssim_map=a.ssim_maps)
            if a.write_images:
                buf = ViewBuffers.__new__(ViewBuffers)
                buf.rgb, buf.maskid, buf.depth = (view[k].cpu().numpy() for k in ("rgb", "maskid", "depth"))
                map_view.write_view(a.out, frame_id, buf, a.depth_scale)
        if a.ssim_maps:
            from PIL import Image
            Image.fromarray(ssim_png(ev.ssim_map.cpu().numpy())).save(os.path.join(a.out, f"ssim_{frame_id}.png"))
        frame_ids.append(frame_id)
        f = figures(ev._frames[-1].cpu().numpy())
        depth_txt = f"depth L1 {f['depth_l1']:.4f} m over {f['depth_coverage']:.3f}" if ev.depth_scored else "depth not scored"
        print(f"frame {frame_id}: PSNR {f['psnr']:.3f} dB, SSIM {f['ssim']:.5f}, {depth_txt}, painted {f['painted_share']:.3f}")
    res = ev.result()
    report = {"frames": frame_ids, "ids": res["ids"], "taps": list(TAPS), "columns": list(COLUMNS),
              "source": "renders" if a.renders else "map_view", "depth_scored": ev.depth_scored,
              "ids_wrapped": bool(a.renders and max(res["ids"]) > 255),
              "image": res["image"], "other": res["other"], "per_id": res["per_id"], "miou": res["miou"],
              "accuracy": res["accuracy"], "acc": res["acc"], "conf": res["conf"],
              "per_frame": res["per_frame"], "frame_rows": res["frame_rows"]}
    if report["ids_wrapped"]:
        print("note: the map holds ids above 255, which wrapped in maskid_<id>.png")
    with open(os.path.join(a.out, "eval_views.json"), "w") as fh:
        json.dump(_plain(report), fh, indent=1, sort_keys=True)
        fh.write("\n")
    img = res["image"]
    print(f"{len(frame_ids)} frames: PSNR {img['psnr']:.3f} dB, SSIM {img['ssim']:.5f}, mIoU {res['miou']:.4f}, "
          f"accuracy {res['accuracy']:.4f}")
    return res


if __name__ == "__main__":
    main()
