"""Map export for the open-vocabulary viewer: visualization/gen_map_vis.py:82-146 over the checkpoints the mapper writes
(mapping.py save_checkpoints: <logdir>/ckpt/<obj_id>/obj_<id>.pth).

    python -m openobj_amd.map_vis --logdir DIR [--grid-dim 128] [--device cuda:0] [--compact]

For every object whose checkpoint carries a box: Trainer.meshing(box, obj_center, grid_dim, save_mesh, if_color,
if_part) on the GPU, the part feature L2-normalised per vertex, and the reference's per-object dict (clip_feat,
caption_feat, class_id, mesh, color, part_feat) collected into <logdir>/map_vis.pkl.gz; each mesh is also written to
<logdir>/map_vis/obj_<id>.ply.  The boxes are the ones the mapper fitted to each object's keyframes before writing the
checkpoint (sceneObject.get_bound, vmap.py:287-384; `python -m openobj_amd.mapping` does it for every checkpoint).
Objects whose checkpoint carries no box (too few keyframe points to fit one, as in the reference) are skipped with a
message, as are objects whose network meshes to nothing.

--compact (export(..., compact=True)) writes <logdir>/map_vis_compact.pkl.gz instead: the same dict per object without
part_feat and with part_rows [V, H+1] fp32 and part_head [C, H+1] fp32 -- the unit part feature of vertex v is
part_head . part_rows[v]: 33 floats a vertex at hidden 32 instead of 512.  The 512-d feature is never
formed: Trainer.meshing(part_compact=True).  A vertex whose feature is exactly zero gets a finite row (s = 1e8) there,
where the dense export's f / |f| is NaN.  The .ply files are the same."""
from __future__ import annotations

import argparse
import gzip
import os
import pickle
from typing import Dict, Optional

import numpy as np
import torch

from . import cfg as ocfg
from . import trainer


def load_object(ckpt_file: str, device: str):
    """-> (Trainer with the checkpoint's weights, checkpoint dict)."""
    ck = torch.load(ckpt_file, map_location="cpu", weights_only=False)
    fc = ck["FC_state_dict"]
    c = ocfg.Config(ocfg.replica_room0_config(train_device=device))
    c.obj_id = int(ck["obj_id"])
    c.hidden_feature_size = int(fc["in_layer.0.weight"].shape[0])
    c.clip_point_feature_size = int(fc["out_clip.weight"].shape[0])
    c.obj_scale = float(ck["obj_scale"])
    t = trainer.Trainer(c)
    with torch.no_grad():
        sd = t.fc_occ_map.state_dict()
        for k, v in fc.items():
            sd[k].copy_(v)
        t.pe.B_layer.weight.copy_(ck["PE_state_dict"]["B_layer.weight"])
    return t, ck


def iter_checkpoints(logdir: str, device: str):
    """The objects of <logdir>/ckpt/<id>/obj_<id>.pth in ascending id order that have a checkpoint with a box (the others
    are skipped with a message) -> (obj_id, Trainer, checkpoint dict, box), one object loaded at a time."""
    ckpt_dir = os.path.join(logdir, "ckpt")
    ids = sorted(int(d) for d in os.listdir(ckpt_dir) if os.path.isdir(os.path.join(ckpt_dir, d)) and d.isdigit())

    def load():             # (the directory is listed at the call, the objects are loaded as the caller iterates)
        for obj_id in ids:
            f = os.path.join(ckpt_dir, str(obj_id), f"obj_{obj_id}.pth")
            if not os.path.exists(f):
                print("ckpt not exist ", f)
                continue
            t, ck = load_object(f, device)
            box = ck.get("bbox")
            if box is None:
                print(f"obj {obj_id}: the checkpoint carries no box, skipped")
                continue
            yield obj_id, t, ck, box
    return load()


COMPACT_FILE = "map_vis_compact.pkl.gz"
DENSE_FILE = "map_vis.pkl.gz"


def export(logdir: str, grid_dim: int = 128, device: str = "cuda:0", obj_center: float = 0.0,
           compact: bool = False) -> Optional[Dict]:
    ply_dir = os.path.join(logdir, "map_vis")
    os.makedirs(ply_dir, exist_ok=True)
    all_obj = {}
    for obj_id, t, ck, box in iter_checkpoints(logdir, device):
        res = t.meshing(box, torch.tensor(obj_center), grid_dim=grid_dim, save_pcd=False, save_mesh=True,
                        if_color=True, if_part=True, part_compact=compact)
        if res is None or len(res) != 3 or res[1] is None:
            print(f"obj {obj_id}: no surface, skipped")
            continue
        _, mesh, part_feat = res
        all_obj[obj_id] = {
            "clip_feat": ck.get("clip_feat"),
            "caption_feat": ck.get("caption_feat"),
            "class_id": ck.get("semantic_id"),
            "mesh": mesh,
            "color": mesh.visual.vertex_colors,
        }
        if compact:
            rows, head = part_feat
            all_obj[obj_id]["part_rows"] = np.ascontiguousarray(rows.cpu().numpy())
            all_obj[obj_id]["part_head"] = np.ascontiguousarray(head.cpu().numpy())
        else:
            part_feat = part_feat.cpu().numpy()
            part_feat = part_feat / np.linalg.norm(part_feat, axis=-1, keepdims=True)   # gen_map_vis.py:121
            all_obj[obj_id]["part_feat"] = part_feat
        mesh.export(os.path.join(ply_dir, f"obj_{obj_id}.ply"))
        print(f"obj {obj_id}: {len(mesh.vertices)} vertices, {len(mesh.faces)} faces")
    path = os.path.join(logdir, COMPACT_FILE if compact else DENSE_FILE)
    with gzip.open(path, "wb") as fh:
        pickle.dump(all_obj, fh)
    print(path)
    return all_obj


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--logdir", required=True)
    ap.add_argument("--grid-dim", type=int, default=128)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--compact", action="store_true", help="write map_vis_compact.pkl.gz (rows + head per object)")
    a = ap.parse_args(argv)
    export(a.logdir, a.grid_dim, a.device, compact=a.compact)


if __name__ == "__main__":
    main()
