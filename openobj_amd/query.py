"""Open-vocabulary object and part queries over the exported map: the numerical core of
visualization/vis_interaction.py on the GPU (objnerf_query.hip, ABI 10).

MapQuery(all_obj) takes the dict map_vis.export returns (or map_vis.pkl.gz holds), keeps its order as the reference's
list_of_keys (:129) and packs every object's unit part features once into one device buffer with segment offsets.
Every colouring returns device colours [V_total, 3] fp32 in that packed order; MapQuery.split cuts them per object.

  object_similarity      0.2 cos_sbert + 0.8 cos_clip over the objects (:364-375)
  color_by_object_query  sim_and_update (:322-354): top-k objects red, the rest darkened RGB; top_num = 0: every
                         object in the "rainbow" colour of its normalised similarity
  color_by_part_query    sim_and_update_part (:378-438): the part query's cosine against every vertex of the top-k
                         objects, min-max normalised per object, "rainbow"; the rest darkened RGB
  part_similarity        the cosine of Q <= 16 part queries against every vertex, one pass over the buffer
  color_by_partfeat      StandardScaler + PCA(3) + joint min-max per object (:205-216, :308-320): segment moments on
                         the GPU, the 512 x 512 eigenproblem per object on the host (numpy.linalg.eigh), the projection
                         and the colours on the GPU
  color_by_rgb / color_by_class / color_by_instance (:263-306)
  hidden_sets            the ceiling / "most" index lists and the axis-aligned boxes (:146-190)

Departures from the reference: an object whose checkpoint carries no clip or caption feature
is left out of the ranking (never a top-k object, coloured like a non-selected one) where the reference would raise;
PCA takes the exact top three eigenvectors with sklearn 1.3.2's u-based sign rule (the reference's sklearn takes the
randomized, unseeded solver at these shapes); instance colours come from a fixed golden-ratio palette (distinctipy's
call in the reference is unseeded).  The CLIP / SBERT text encoders stay outside: the query embeddings are inputs.
"""
from __future__ import annotations

import colorsys
import time
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib, ops

DARK = 0.5          # brightness of a non-selected object (:348, :402)
RGB_FACTOR = 0.8    # color_by_rgb (:300)
SBERT_W, CLIP_W = 0.2, 0.8      # :375, :435


# ------------------------------------------------------------------------------------------------ host bookkeeping
def reduce_object_features(all_obj: Dict, eps: float = 0.2, min_samples: int = 2):
    """(:192-204) -> (positions of the objects that carry both features, clip [N, Dc], caption [N, Ds]) fp32 numpy;
    2-D features are reduced with get_majority_cluster_mean(eps, min_samples)."""
    from .mapping import get_majority_cluster_mean
    pos, clip, cap = [], [], []
    for i, k in enumerate(all_obj):
        c, s = all_obj[k].get("clip_feat"), all_obj[k].get("caption_feat")
        if c is None or s is None:
            continue
        c, s = np.asarray(c, np.float64), np.asarray(s, np.float64)
        if c.ndim == 2:
            c = get_majority_cluster_mean(c, eps, min_samples)
        if s.ndim == 2:
            s = get_majority_cluster_mean(s, eps, min_samples)
        pos.append(i)
        clip.append(c.reshape(-1))
        cap.append(s.reshape(-1))
    if not pos:
        return [], np.zeros((0, 0), np.float32), np.zeros((0, 0), np.float32)
    return pos, np.stack(clip).astype(np.float32), np.stack(cap).astype(np.float32)


def top_positions(sim: torch.Tensor, ranked: Sequence[int], top_num: int) -> List[int]:
    """similarities.topk(top_num) (:328, :383) over the ranked objects -> their positions in the map's order."""
    if top_num <= 0 or len(ranked) == 0:
        return []
    idx = torch.topk(sim, min(int(top_num), len(ranked))).indices.tolist()
    return [ranked[i] for i in idx]


def instance_palette(n: int, pastel_factor: float = 0.5) -> np.ndarray:
    """[n, 3] fp64: hue i * golden ratio (mod 1) at full saturation and value, mixed towards white as distinctipy's
    pastel_factor does ((c + p) / (1 + p)).  Deterministic, unlike the reference's unseeded distinctipy.get_colors."""
    out = np.empty((n, 3))
    for i in range(n):
        out[i] = colorsys.hsv_to_rgb((i * 0.6180339887498949) % 1.0, 1.0, 1.0)
    return (out + pastel_factor) / (1.0 + pastel_factor)


def load_color_yaml(path: str):
    """The reference's replica_color.yaml (:62-67) -> (mapping, mapped_colors)."""
    import yaml
    with open(path) as fh:
        data = yaml.safe_load(fh)
    return data["mapping"], data["mapped_colors"]


def class_colors(all_obj: Dict, mapping, mapped_colors) -> np.ndarray:
    """color_by_class (:277-291): mapped_colors[mapping[class_id + 1]] per object -> [K, 3] fp64."""
    return np.array([mapped_colors[mapping[int(all_obj[k]["class_id"]) + 1]] for k in all_obj], np.float64).reshape(-1, 3)


def hidden_sets(all_obj: Dict, dataset_name: Optional[str] = "Replica", scene_name: str = "room_0") -> Dict:
    """(:146-190) -> {"ceiling": positions of the meshes whose lowest vertex is above the scene's height (1; room_2
    -0.5; office_0 0.5), "most": positions of everything but the wall class (93, Scannet 1; scene 611: every key but
    46), "boxes": [(min xyz, max xyz)] per mesh, "hidden": what the viewer removes by default (the ceiling set for
    Replica, :181-184; nothing otherwise)}."""
    height = {"room_2": -0.5, "office_0": 0.5}.get(scene_name, 1)
    wall_id = 1 if dataset_name == "Scannet" else 93
    ceiling, most, boxes = [], [], []
    for idx, k in enumerate(all_obj):
        v = np.asarray(all_obj[k]["mesh"].vertices, np.float64).reshape(-1, 3)
        if len(v) and v[:, 2].min() > height:
            ceiling.append(idx)
        if scene_name == "611":
            if k != 46:
                most.append(idx)
        elif all_obj[k]["class_id"] is None or int(all_obj[k]["class_id"]) + 1 != wall_id:
            most.append(idx)
        boxes.append((v.min(axis=0), v.max(axis=0)) if len(v) else (np.zeros(3), np.zeros(3)))
    return {"ceiling": ceiling, "most": most, "boxes": boxes,
            "hidden": list(ceiling) if dataset_name == "Replica" else []}


def pca_weights(mean: np.ndarray, scatter: np.ndarray, counts: Sequence[int], stats: Optional[Dict] = None):
    """StandardScaler + PCA(3) of every segment from its moments (fp64): std = sqrt(diag(scatter) / n) (ddof 0, 0 -> 1),
    the correlation matrix scatter / (n std std^T), its top three eigenvectors V3 (numpy.linalg.eigh, descending
    eigenvalues) -> W = V3 / std [S, D, 3], b = -mean . W [S, 3] (fp64): scores = f . W + b."""
    S, D = mean.shape
    W = np.zeros((S, D, 3))
    b = np.zeros((S, 3))
    t0 = time.perf_counter()
    for s in range(S):
        n = int(counts[s])
        if n == 0:
            continue
        std = np.sqrt(np.maximum(np.diag(scatter[s]), 0.0) / n)
        std[std == 0.0] = 1.0
        R = scatter[s] / n / np.outer(std, std)
        _, U = np.linalg.eigh(R)
        k = min(3, D)
        W[s, :, :k] = U[:, ::-1][:, :k] / std[:, None]
        b[s] = -mean[s] @ W[s]
    if stats is not None:
        stats["eigh_s"] = time.perf_counter() - t0
    return W, b


# ------------------------------------------------------------------------------------------------ the device side
class MapQuery:
    def __init__(self, all_obj: Dict, device="cuda:0", eps: float = 0.2, min_samples: int = 2):
        self.all_obj = all_obj
        self.keys = list(all_obj.keys())
        self.dev = torch.device(device)
        pf = [np.asarray(all_obj[k]["part_feat"]) for k in self.keys]
        widths = {p.shape[1] for p in pf if p.ndim == 2 and len(p)}
        if len(widths) > 1:
            raise ValueError(f"MapQuery: part features of different widths {sorted(widths)}")
        self.D = widths.pop() if widths else 0
        counts = [len(p) for p in pf]
        self.seg_host = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.V = int(self.seg_host[-1])
        self.seg_off = torch.from_numpy(self.seg_host).to(self.dev)
        self.part_feat = torch.empty(self.V, max(self.D, 1), device=self.dev)
        self.rgb = torch.empty(self.V, 4, dtype=torch.uint8, device=self.dev)
        for s, k in enumerate(self.keys):
            r0, r1 = int(self.seg_host[s]), int(self.seg_host[s + 1])
            if r1 == r0:
                continue
            self.part_feat[r0:r1].copy_(torch.from_numpy(np.ascontiguousarray(pf[s], np.float32)))
            c = np.asarray(all_obj[k]["color"], np.uint8).reshape(r1 - r0, -1)
            self.rgb[r0:r1, : c.shape[1]].copy_(torch.from_numpy(np.ascontiguousarray(c)))
        ranked, clip, cap = reduce_object_features(all_obj, eps, min_samples)
        self.ranked = ranked                     # positions (in the map's order) that take part in the ranking
        self.clip = torch.from_numpy(clip).to(self.dev)
        self.caption = torch.from_numpy(cap).to(self.dev)
        self.last_ranking = None

    @property
    def S(self) -> int:
        return len(self.keys)

    def split(self, colors: torch.Tensor) -> List[torch.Tensor]:
        """[V_total, 3] -> one [n_k, 3] view per object, in the map's order."""
        return [colors[int(self.seg_host[s]):int(self.seg_host[s + 1])] for s in range(self.S)]

    # -------------------------------------------------------------------------------------------- helpers
    def _query(self, q, width: int, name: str) -> torch.Tensor:
        t = torch.as_tensor(np.asarray(q, np.float32)).reshape(-1).to(self.dev)
        if t.numel() != width:
            raise ValueError(f"{name}: width {t.numel()} does not match the map's {width}")
        return t / t.norm(dim=-1, keepdim=True)             # :366, :370, :430

    def _colors(self, modes, factor=None, constant=None, column=None, proj=None, minmax=None) -> torch.Tensor:
        f = np.full(self.S, RGB_FACTOR) if factor is None else factor
        return ops.vertex_colors(self.seg_off, modes, self.V, rgb=self.rgb, factor=f, constant=constant, column=column,
                                 proj=proj, minmax=minmax, out=torch.empty(self.V, 3, device=self.dev))

    def _rainbow(self, values: torch.Tensor) -> torch.Tensor:
        """The "rainbow" colour of a few values min-max normalised together (:329-332) -> [n, 3] device."""
        n = values.numel()
        v = values.reshape(n, 1).float().contiguous()
        mm = torch.stack([v.min(), v.max()]).reshape(1, 1, 2)
        return ops.vertex_colors(torch.tensor([0, n]), [_lib.COLOR_RAINBOW], n, column=[0], proj=v, minmax=mm,
                                 out=torch.empty(n, 3, device=self.dev))

    # -------------------------------------------------------------------------------------------- queries
    def object_similarity(self, clip_q, sbert_q) -> torch.Tensor:
        """0.2 cos(sbert_q, caption) + 0.8 cos(clip_q, clip) per ranked object (self.ranked order), device fp32."""
        N = len(self.ranked)
        if N == 0:
            return torch.zeros(0, device=self.dev)
        cq = self._query(clip_q, self.clip.shape[1], "clip query")
        sq = self._query(sbert_q, self.caption.shape[1], "sbert query")
        seg = torch.tensor([0, N])
        s_sbert = ops.segment_project(self.caption, seg, sq[:, None], cosine=True)[0][:, 0]
        s_clip = ops.segment_project(self.clip, seg, cq[:, None], cosine=True)[0][:, 0]
        return s_sbert * SBERT_W + s_clip * CLIP_W

    def ranking(self, sim: torch.Tensor):
        """[(key, similarity)] of the ranked objects, most similar first."""
        v = sim.detach().cpu().numpy()
        order = np.argsort(-v, kind="stable")
        return [(self.keys[self.ranked[i]], float(v[i])) for i in order]

    def color_by_object_query(self, clip_q, sbert_q, top_num: int = 0) -> torch.Tensor:
        sim = self.object_similarity(clip_q, sbert_q)
        self.last_ranking = self.ranking(sim)
        modes = np.full(self.S, _lib.COLOR_RGB, np.int32)
        const = np.zeros((self.S, 3), np.float32)
        if top_num != 0:
            for p in top_positions(sim, self.ranked, top_num):
                modes[p] = _lib.COLOR_CONSTANT
                const[p] = (1.0, 0.0, 0.0)
        elif len(self.ranked):
            cols = self._rainbow(sim).cpu().numpy()
            for i, p in enumerate(self.ranked):
                modes[p] = _lib.COLOR_CONSTANT
                const[p] = cols[i]
        return self._colors(modes, factor=np.full(self.S, DARK), constant=const)

    def part_similarity(self, part_q, objects: Optional[Sequence[int]] = None):
        """cosine of part_q [Q, D] (Q <= 16) against the vertices of `objects` (positions; None: all, one pass) ->
        (sims [V_total, Q] device fp32, minmax [S, Q, 2]); rows and minmax of objects left out are NaN."""
        q = part_q if torch.is_tensor(part_q) else torch.as_tensor(np.asarray(part_q, np.float32))
        q = q.to(device=self.dev, dtype=torch.float32)
        q = q.reshape(1, -1) if q.dim() == 1 else q
        if q.shape[1] != self.D:
            raise ValueError(f"part query: width {q.shape[1]} does not match the map's {self.D}")
        W = q.t().contiguous()
        if objects is None:
            return ops.segment_project(self.part_feat, self.seg_off, W, cosine=True)
        out = torch.full((self.V, q.shape[0]), float("nan"), device=self.dev)
        mm = torch.full((self.S, q.shape[0], 2), float("nan"), device=self.dev)
        for p in objects:
            r0, r1 = int(self.seg_host[p]), int(self.seg_host[p + 1])
            _, m = ops.segment_project(self.part_feat[r0:r1], torch.tensor([0, r1 - r0]), W, cosine=True,
                                       out=out[r0:r1])
            mm[p] = m[0]
        return out, mm

    def color_by_part_query(self, clip_q, sbert_q, part_q, top_num: int = 1) -> torch.Tensor:
        sim = self.object_similarity(clip_q, sbert_q)
        self.last_ranking = self.ranking(sim)
        top = top_positions(sim, self.ranked, top_num)
        pq = self._query(part_q, self.D, "part query")
        proj, mm = self.part_similarity(pq[None], objects=top)
        modes = np.full(self.S, _lib.COLOR_RGB, np.int32)
        modes[top] = _lib.COLOR_RAINBOW
        return self._colors(modes, factor=np.full(self.S, DARK), column=np.zeros(self.S, np.int32), proj=proj,
                            minmax=mm)

    def color_by_partfeat(self, stats: Optional[Dict] = None) -> torch.Tensor:
        mean, scatter = ops.segment_moments(self.part_feat, self.seg_off)
        W, b = pca_weights(mean.cpu().numpy(), scatter.cpu().numpy(), np.diff(self.seg_host), stats)
        proj, mm = ops.segment_project(self.part_feat, self.seg_off, torch.from_numpy(W).float(),
                                       torch.from_numpy(b).float())
        return self._colors(np.full(self.S, _lib.COLOR_PCA, np.int32), proj=proj, minmax=mm)

    def color_by_rgb(self) -> torch.Tensor:
        return self._colors(np.full(self.S, _lib.COLOR_RGB, np.int32))

    def _constant(self, cols: np.ndarray) -> torch.Tensor:
        return self._colors(np.full(self.S, _lib.COLOR_CONSTANT, np.int32), constant=np.asarray(cols, np.float32))

    def color_by_class(self, mapping, mapped_colors=None) -> torch.Tensor:
        """mapping + mapped_colors as the reference's YAML holds them, or mapping = the path of that YAML."""
        if isinstance(mapping, str):
            mapping, mapped_colors = load_color_yaml(mapping)
        return self._constant(class_colors(self.all_obj, mapping, mapped_colors))

    def color_by_instance(self) -> torch.Tensor:
        return self._constant(instance_palette(self.S))

    def hidden_sets(self, dataset_name: Optional[str] = "Replica", scene_name: str = "room_0") -> Dict:
        return hidden_sets(self.all_obj, dataset_name, scene_name)


__all__ = ["MapQuery", "hidden_sets", "instance_palette", "class_colors", "load_color_yaml", "pca_weights",
           "reduce_object_features", "top_positions"]
