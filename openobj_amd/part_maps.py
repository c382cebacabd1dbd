"""Part-level feature maps (the reference's partlevel/sam_clip_dir.py) from the masks on, in a compact form.

    python -m openobj_amd.part_maps --masks-dir DIR --output-dir OUT --down-sample 5 [--dense]

The reference runs SAM's automatic mask generator on a frame, CLIP on a 1.3x crop around every mask, and writes a dense
[H/d, W/d, C] fp32 image: per down-sampled pixel the CLIP feature of the LAST mask that covers it, times that mask's
stability score, or zeros (sam_clip_dir.py:113-133).  Like mask_graph, this stage keeps the foundation models outside:
what they return is the input, one file per frame, DIR/<frame>.npz, masks in SAM's order (the order decides the result):

    segmentation        [M, H, W] bool        (or segmentation_strided [M, H/d, W/d], already mask[::d, ::d])
    stability_score     [M]
    feat                [M, C] fp16 | fp32, as clip_model.encode_image gave it for crop_box(bbox) of the image
    bbox [M, 4] XYWH, predicted_iou [M]       optional, not used here (see below)

Semantics, the reference's, quirks included:
  * every mask is used: the predicted_iou > 0.9 filter of :89-93 builds `post_masks`, which nothing reads;
  * table row i = (feat_i * float(stability_i)).float(): the product is formed in the feature's own dtype, then widened;
  * a later mask overwrites an earlier one, nothing is accumulated (`per_pixel_weight_sum` is computed and never used:
    there is no normalisation); uncovered pixels are zero;
  * H % d != 0 or W % d != 0 raises ValueError (there mask[::d] has one more row than the output and the boolean
    indexing raises);
  * M = 0 gives an all-zero map (index all -1, an empty table).  The reference fails on `mask_feature_all[0]` there.

A frame with M masks holds at most M + 1 distinct vectors, so the output OUT/<frame>.npz (named by the input's stem) is
    index  int16 [H/d, W/d]   row of `table`, -1 = none
    table  fp32  [M_used, C]  rows no pixel refers to are dropped, the rest renumbered in ascending mask order
and table[index] (zeros at -1) IS the reference's array, bit for bit.  --dense also writes that array as OUT/<frame>.npy,
produced on the device (objnerf_part_dense).  The reference names its files str(idx * skip) + '.npy' for the images
natsorted(input_image)[0:-1:skip], skip = 10 (:69-71, :133): which frames to process and how to name them is the caller's
business here -- name the input files by the dataset frame id that dataset.py looks up (partlevel/<frame>.npz).

The index image comes from objnerf_part_index (a thread per pixel scanning the masks last to first); dataset.py reads the
.npz, mapping.py keeps the frames in a PartStore (one index image per frame + one shared row table on the device) and the
sampler gathers through the index (ops._partfeat_fields, ABI 12): the dense map never exists.
"""
import argparse
import glob
import os
import re
from typing import Optional

import numpy as np
import torch

from . import ops

INDEX_DTYPE = np.int16          # on-disk index image: M_used <= 32767


def crop_box(bbox_xywh, height: int, width: int):
    """The crop CLIP is run on for a mask with SAM's XYWH box (bbox_getter, sam_clip_dir.py:42-59): the box grown to 1.3x
    its size, half of the growth on each side, each side's share cut at the image border -> [x0, y0, x1, y1] for
    image[y0:y1, x0:x1].  Both roundings are Python's round (half to even), as there.  Pure host arithmetic, offered so
    that whoever runs CLIP crops the same pixels."""
    x, y, w, h = bbox_xywh

    def grown(lo, size, limit):
        grow = round((round(size * 1.3) - size) / 2)            # per side, before clipping
        hi = lo + size
        return lo - min(grow, lo), hi + min(grow, limit - hi)

    x0, x1 = grown(x, w, width)
    y0, y1 = grown(y, h, height)
    return [x0, y0, x1, y1]


def strided_masks(frame, down_sample: int) -> np.ndarray:
    """The masks of one input file on the stride: uint8 [M, H/d, W/d] (mask[::d, ::d], :121)."""
    d = int(down_sample)
    if "segmentation_strided" in frame:
        m = np.asarray(frame["segmentation_strided"])
    else:
        seg = np.asarray(frame["segmentation"])
        if seg.ndim != 3:
            raise ValueError("segmentation must be [M, H, W]")
        if seg.shape[1] % d or seg.shape[2] % d:
            raise ValueError("image %d x %d is no multiple of down_sample %d (the reference's mask indexing raises)"
                             % (seg.shape[1], seg.shape[2], d))
        m = seg[:, ::d, ::d]
    if m.ndim != 3:
        raise ValueError("masks must be [M, H', W']")
    return np.ascontiguousarray(m != 0).view(np.uint8)


def feature_table(feat, stability_score) -> torch.Tensor:
    """Row i = (feat_i * float(stability_i)).float() (:123-124) for all masks: fp32 [M, C] on the host."""
    feat = torch.as_tensor(np.asarray(feat))
    score = np.asarray(stability_score).reshape(-1)
    if feat.dim() != 2 or feat.shape[0] != score.shape[0] or not feat.is_floating_point():
        raise ValueError("feat [M, C] floating point and stability_score [M] expected")
    rows = [(feat[i] * float(score[i])).float() for i in range(feat.shape[0])]
    return torch.stack(rows) if rows else torch.zeros(0, feat.shape[1])


def compact(index: np.ndarray, table: np.ndarray):
    """Drop the table rows no pixel refers to and renumber the rest in ascending order of their mask number."""
    used = np.unique(index[index >= 0])
    if used.size > np.iinfo(INDEX_DTYPE).max:
        raise ValueError("more than %d masks in one frame" % np.iinfo(INDEX_DTYPE).max)
    remap = np.full(table.shape[0] + 1, -1, np.int64)         # (the last entry serves index -1)
    remap[used] = np.arange(used.size)
    return remap[index].astype(INDEX_DTYPE), np.ascontiguousarray(table[used])


def build_frame(frame, down_sample: int, device="cuda:0", dense: bool = False):
    """One frame's masks -> (index int16 [H', W'], table fp32 [M_used, C], dense fp32 [H', W', C] | None)."""
    masks = strided_masks(frame, down_sample)
    table = feature_table(frame["feat"], frame["stability_score"])
    if table.shape[0] != masks.shape[0]:
        raise ValueError("%d masks but %d features" % (masks.shape[0], table.shape[0]))
    dev = torch.device(device)
    index = ops.part_index(torch.from_numpy(masks).to(dev))
    idx16, tab = compact(index.cpu().numpy(), table.numpy())
    out = None
    if dense:
        out = ops.part_dense(*shifted(idx16, tab, dev)).cpu().numpy()
    return idx16, tab, out


def shifted(index, table, device=None):
    """The stored pair in the form the kernels and the sampler take: (index + 1 as int32, 0 = none; table with a zero
    row in front), as tensors (on `device` if given)."""
    idx = torch.from_numpy(np.asarray(index).astype(np.int32) + 1)
    table = torch.from_numpy(np.asarray(table, dtype=np.float32))
    tab = torch.cat([torch.zeros(1, table.shape[1]), table])
    return (idx, tab) if device is None else (idx.to(device), tab.to(device))


def save_compact(path: str, index, table) -> None:
    np.savez(path, index=np.asarray(index, dtype=INDEX_DTYPE), table=np.asarray(table, dtype=np.float32))


def load_compact(path: str):
    """-> (index int16 [H', W'], table fp32 [M_used, C]) of a file this module wrote."""
    with np.load(path) as d:
        index, table = d["index"], d["table"]
    if index.ndim != 2 or table.ndim != 2 or (index.size and int(index.max()) >= table.shape[0]) or \
            (index.size and int(index.min()) < -1):
        raise ValueError("%s: index [H', W'] into table [M, C] expected" % path)
    return index, table


def densify_host(index, table) -> np.ndarray:
    """table[index] with zeros at -1 on the host: the reference's dense array (for the loaders that resample it)."""
    idx, tab = shifted(index, table)
    return tab.numpy()[idx.numpy()]


class PartStore:
    """The part maps of a run on the device: `index` int32 [frames, W', H'] of GLOBAL row numbers into `table` fp32
    [rows, C], whose row 0 is zero (a pixel no mask covers).  Both buffers double their capacity when full, like the
    mapper's dense buffer; the views `index` / `table` cover what has been appended."""

    def __init__(self, device):
        self.device = torch.device(device)
        self._index_buf: Optional[torch.Tensor] = None
        self._table_buf: Optional[torch.Tensor] = None
        self.n_frames = 0
        self.n_rows = 0
        self.index: Optional[torch.Tensor] = None
        self.table: Optional[torch.Tensor] = None

    def append(self, part_index, part_table) -> None:
        """One frame: part_index int32 [W', H'] (0 = none, r = row r of part_table), part_table fp32 [M + 1, C] whose
        row 0 is zero.  The frame's rows 1 .. M go behind the table, its non-zero indices move by their base row."""
        idx = torch.as_tensor(part_index)
        tab = torch.as_tensor(part_table)
        if idx.dtype != torch.int32 or idx.dim() != 2 or tab.dtype != torch.float32 or tab.dim() != 2 or tab.shape[0] < 1:
            raise ops.ObjnerfError("PartStore.append: index int32 [W', H'] and table fp32 [M + 1, C] expected")
        if self._index_buf is not None and (tuple(idx.shape) != tuple(self._index_buf.shape[1:]) or
                                            tab.shape[1] != self._table_buf.shape[1]):
            raise ops.ObjnerfError("PartStore.append: the frame's shape differs from the stored frames'")
        idx, tab = idx.to(self.device), tab.to(self.device)
        if self._index_buf is None:
            self._index_buf = torch.empty((8,) + tuple(idx.shape), dtype=torch.int32, device=self.device)
            self._table_buf = torch.zeros(max(64, 2 * tab.shape[0]), tab.shape[1], device=self.device)
            self.n_rows = 1                                     # row 0: zeros
        if self.n_frames == self._index_buf.shape[0]:
            grown = torch.empty((2 * self.n_frames,) + tuple(idx.shape), dtype=torch.int32, device=self.device)
            grown[:self.n_frames] = self._index_buf
            self._index_buf = grown
        m = tab.shape[0] - 1
        if self.n_rows + m > self._table_buf.shape[0]:
            grown = torch.zeros(max(2 * self._table_buf.shape[0], self.n_rows + m), tab.shape[1], device=self.device)
            grown[:self.n_rows] = self._table_buf[:self.n_rows]
            self._table_buf = grown
        base = self.n_rows - 1
        self._index_buf[self.n_frames] = torch.where(idx > 0, idx + base, torch.zeros_like(idx))
        self._table_buf[self.n_rows:self.n_rows + m] = tab[1:]
        self.n_frames += 1
        self.n_rows += m
        self.index = self._index_buf[:self.n_frames]
        self.table = self._table_buf[:self.n_rows]

    def nbytes(self) -> int:
        """Device bytes in use (index images + table rows)."""
        return 0 if self.index is None else self.index.numel() * 4 + self.table.numel() * 4

    def dense(self) -> torch.Tensor:
        """The dense [frames, W', H', C] tensor this store stands for (objnerf_part_dense; tests and diagnostics)."""
        return ops.part_dense(self.index, self.table)


def _natural_key(path):
    return [int(t) if t.isdigit() else t for t in re.split(r"(\d+)", os.path.basename(path))]


def main(argv=None):
    ap = argparse.ArgumentParser(description="Compact part-level feature maps from SAM masks and CLIP features (MI355X).")
    ap.add_argument("--masks-dir", required=True, help="one <frame>.npz per frame (see the module docstring)")
    ap.add_argument("--output-dir", required=True)
    ap.add_argument("--down-sample", type=int, required=True, help="the mapper's part_down (5)")
    ap.add_argument("--dense", action="store_true", help="also write the reference's dense <frame>.npy")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    if args.down_sample <= 0:
        raise ValueError("--down-sample must be positive")
    files = sorted(glob.glob(os.path.join(args.masks_dir, "*.npz")), key=_natural_key)
    if not files:
        raise FileNotFoundError("no .npz file in " + args.masks_dir)
    os.makedirs(args.output_dir, exist_ok=True)
    for path in files:
        stem = os.path.splitext(os.path.basename(path))[0]
        with np.load(path) as frame:
            index, table, dense = build_frame(frame, args.down_sample, args.device, args.dense)
        save_compact(os.path.join(args.output_dir, stem + ".npz"), index, table)
        if dense is not None:
            np.save(os.path.join(args.output_dir, stem + ".npy"), dense)
        print("%s: %d x %d, %d masks in use" % (stem, index.shape[0], index.shape[1], table.shape[0]), flush=True)
    return len(files)


if __name__ == "__main__":
    main()
