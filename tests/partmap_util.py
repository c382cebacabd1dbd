"""Test helper for the part-level feature maps: the reference's mask loop (partlevel/sam_clip_dir.py:118-125) restated
in numpy on the CPU, and a writer of part files -- the reference's dense .npy and the compact .npz -- from the same
synthetic masks.  Nothing here uses openobj_amd: it is what the package is checked against."""
import os

import numpy as np


def scaled_row(feat_i, score):
    """(feat_i * float(score)).float() of :123-124: the product in the feature's own dtype (a 16-bit product is formed
    in fp32 and rounded to 16 bits, as torch does), then widened to fp32."""
    prod = feat_i.astype(np.float32) * np.float32(score)
    return prod.astype(feat_i.dtype).astype(np.float32)


def reference_loop(masks, feat, score):
    """masks [M, H', W'] bool (already mask[::d, ::d]), feat [M, C], score [M] -> the dense fp32 [H', W', C] array the
    reference saves: mask after mask is assigned, a later one overwrites an earlier one, uncovered pixels stay zero."""
    out = np.zeros(masks.shape[1:] + (feat.shape[1],), np.float32)
    for i in range(masks.shape[0]):
        out[masks[i].astype(bool)] = scaled_row(feat[i], score[i])
    return out


def last_mask(masks):
    """int32 [H', W']: the number of the last mask that covers each pixel, -1 where none does."""
    idx = np.full(masks.shape[1:], -1, np.int32)
    for i in range(masks.shape[0]):
        idx[masks[i].astype(bool)] = i
    return idx


def compact_of(masks, feat, score):
    """-> (index int16 [H', W'] into table, -1 = none; table fp32 [M_used, C]) with unused rows dropped."""
    idx = last_mask(masks)
    used = sorted(set(idx[idx >= 0].tolist()))
    new = {m: r for r, m in enumerate(used)}
    index = np.array([[new.get(int(v), -1) for v in row] for row in idx], np.int16).reshape(idx.shape)
    table = np.stack([scaled_row(feat[m], score[m]) for m in used]) if used else np.zeros((0, feat.shape[1]), np.float32)
    return index, table


def synthetic_frame(rs, H, W, M, C, dtype=np.float32):
    """M random rectangles (some overlapping, in a fixed order) with seeded features and scores."""
    seg = np.zeros((M, H, W), bool)
    for m in range(M):
        h, w = rs.randint(3, max(4, H // 2)), rs.randint(3, max(4, W // 2))
        y, x = rs.randint(0, H - h + 1), rs.randint(0, W - w + 1)
        seg[m, y:y + h, x:x + w] = True
    return {"segmentation": seg, "stability_score": rs.uniform(0.85, 1.0, M),
            "feat": rs.randn(M, C).astype(dtype)}


def write_part_files(root, frame_ids, H, W, down, C, form, seed=0, n_masks=(3, 6, 4)):
    """root/partlevel/<frame>.npy (form "dense") or <frame>.npz (form "compact") for every frame id, from the same
    seeded masks whatever the form.  Returns the per-frame (index, table) pairs."""
    assert form in ("dense", "compact") and H % down == 0 and W % down == 0
    os.makedirs(os.path.join(root, "partlevel"), exist_ok=True)
    rs = np.random.RandomState(seed)
    out = []
    for k, fid in enumerate(frame_ids):
        fr = synthetic_frame(rs, H, W, n_masks[k % len(n_masks)], C)
        masks = fr["segmentation"][:, ::down, ::down]
        if form == "dense":
            np.save(os.path.join(root, "partlevel", "%d.npy" % fid),
                    reference_loop(masks, fr["feat"], fr["stability_score"]))
        index, table = compact_of(masks, fr["feat"], fr["stability_score"])
        if form == "compact":
            np.savez(os.path.join(root, "partlevel", "%d.npz" % fid), index=index, table=table)
        out.append((index, table))
    return out
