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
  part_regions           beyond the viewer: the connected surface patches a part query selects, with area, centroid,
                         normal, axes and peak (objnerf_mapregions.hip, map_regions.py)

A compact map (map_vis.export(compact=True): part_rows [V, H + 1] and part_head [C, H + 1] per object instead of
part_feat, the unit feature being part_head . part_rows[v]) is taken the same way and answers
the same calls from the rows: the 512-d features are never packed.  MapQuery.features(ids) expands single rows.

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


def pca_weights_lowrank(mean_r: Sequence[np.ndarray], scatter_r: Sequence[np.ndarray], heads: Sequence[np.ndarray],
                        counts: Sequence[int], stats: Optional[Dict] = None):
    """pca_weights for features that are linear in stored rows, X = r A^T (A = heads[s] [C, K], K = H + 1), from the
    moments of r alone (fp64): per segment, with m = mean_r[s] [K], S = scatter_r[s] [K, K] = sum (r - m)(r - m)^T,
      std_c = sqrt(a_c^T S a_c / n)  (0 -> 1; a negative rounding residue counts as 0),     D = diag(std)
      S / n = L L^T  from numpy.linalg.eigh of the K x K matrix (negative eigenvalues clamped to 0),
      B = D^-1 A L  [C, K]: the correlation matrix of X is B B^T, whose non-zero spectrum is that of B^T B [K, K];
      (lambda, V) the top three eigenpairs of B^T B,  U = B V / sqrt(lambda)  (unit eigenvectors of B B^T),
      W = U / std,  P = A^T W [K, 3],  b = -(A m) . W [3]:   scores = X W - (A m) W = r P + b.
    A component with lambda <= 1e-12 lambda_0 (or lambda_0 = 0) gets zero weights.  Sequences (the segments may have
    different K) -> (P: list of [K_s, 3], b: [S, 3]); arrays [S, K], [S, K, K], [S, C, K] work as well and then P
    stacks to [S, K, 3]."""
    S = len(counts)
    P, b = [], np.zeros((S, 3))
    t0 = time.perf_counter()
    for s in range(S):
        A = np.asarray(heads[s], np.float64)
        K = A.shape[1]
        Ps = np.zeros((K, 3))
        P.append(Ps)
        n = int(counts[s])
        if n == 0:
            continue
        Sn = np.asarray(scatter_r[s], np.float64) / n
        m = np.asarray(mean_r[s], np.float64)
        std = np.sqrt(np.maximum(np.einsum("ck,kl,cl->c", A, Sn, A), 0.0))
        std[std == 0.0] = 1.0
        w, E = np.linalg.eigh(Sn)
        L = E * np.sqrt(np.maximum(w, 0.0))
        B = (A @ L) / std[:, None]
        lam, V = np.linalg.eigh(B.T @ B)
        lam, V = lam[::-1], V[:, ::-1]
        k = min(3, K)
        keep = [j for j in range(k) if lam[0] > 0.0 and lam[j] > 1e-12 * lam[0]]
        if not keep:
            continue
        W = (B @ V[:, keep]) / np.sqrt(lam[keep]) / std[:, None]
        Ps[:, keep] = A.T @ W
        b[s, keep] = -(A @ m) @ W
    if stats is not None:
        stats["eigh_s"] = time.perf_counter() - t0
    if len({p.shape for p in P}) == 1 and S:
        P = np.stack(P)
    return P, b


def compact_layout(all_obj: Dict):
    """Host-only checks of a map dict -> None for a dense map (every object carries part_feat), else per object
    (rows [V, H + 1] fp32, head [C, H + 1] fp32) of a compact one.  ValueError: the two kinds mixed, a head that does not
    match its rows, heads of different C."""
    kinds = {"part_rows" in o for o in all_obj.values()}
    if len(kinds) > 1 or any("part_rows" in o and "part_feat" in o for o in all_obj.values()):
        raise ValueError("MapQuery: the map mixes dense (part_feat) and compact (part_rows) objects")
    if not kinds or kinds == {False}:
        return None
    out, Cs = [], set()
    for k, o in all_obj.items():
        if o.get("part_head") is None:
            raise ValueError(f"MapQuery: object {k} carries part_rows without part_head")
        rows, head = np.asarray(o["part_rows"], np.float32), np.asarray(o["part_head"], np.float32)
        if rows.ndim != 2 or head.ndim != 2 or rows.shape[1] != head.shape[1] or rows.shape[1] < 2:
            raise ValueError(f"MapQuery: object {k}: part_rows {rows.shape} does not match part_head {head.shape}")
        Cs.add(head.shape[0])
        out.append((rows, head))
    if len(Cs) > 1:
        raise ValueError(f"MapQuery: part heads of different widths {sorted(Cs)}")
    return out


# ------------------------------------------------------------------------------------------------ the device side
class MapQuery:
    """A dense map (part_feat per object) or a compact one (part_rows + part_head per object): the
    compact map keeps rows [V, H + 1] with f^ = head . row per vertex, one buffer of row stride H + 4 per contiguous
    run of objects of equal H, and answers every query from the rows -- a part query is the affine projection of the
    rows on head^T q^, the PCA colouring needs the moments of the rows and a (H + 1)-wide eigenproblem per object."""
    compact = None                  # the runs of a compact map (_init_compact); None: a dense map

    def __init__(self, all_obj: Dict, device="cuda:0", eps: float = 0.2, min_samples: int = 2):
        self.all_obj = all_obj
        self.keys = list(all_obj.keys())
        self.dev = torch.device(device)
        layout = compact_layout(all_obj)
        if layout is not None:
            self._init_compact(layout)
            self._init_objects(eps, min_samples)
            return
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
        self._init_objects(eps, min_samples)

    def _init_compact(self, layout) -> None:
        """layout: compact_layout's (rows, head) per object -> self.compact: one record per contiguous run of objects of
        equal width (s0, s1: the objects; buf [V_run, H + 4] device, zero in the padding; seg: the run's own offsets)."""
        self.D = int(layout[0][1].shape[0])
        counts = [len(r) for r, _ in layout]
        self.seg_host = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.V = int(self.seg_host[-1])
        self.seg_off = torch.from_numpy(self.seg_host).to(self.dev)
        self.part_feat = None
        self.rgb = torch.empty(self.V, 4, dtype=torch.uint8, device=self.dev)
        self.heads64 = [h.astype(np.float64) for _, h in layout]
        self.heads = [torch.from_numpy(np.ascontiguousarray(h)).to(self.dev) for _, h in layout]
        self.compact = []
        s0 = 0
        while s0 < self.S:
            K = layout[s0][1].shape[1]
            s1 = s0 + 1
            while s1 < self.S and layout[s1][1].shape[1] == K:
                s1 += 1
            r0, r1 = int(self.seg_host[s0]), int(self.seg_host[s1])
            buf = torch.zeros(r1 - r0, K - 1 + ops.PART_ROW_PAD, device=self.dev)
            for s in range(s0, s1):
                a, b = int(self.seg_host[s]) - r0, int(self.seg_host[s + 1]) - r0
                if b > a:
                    buf[a:b, :K].copy_(torch.from_numpy(np.ascontiguousarray(layout[s][0])))
            self.compact.append({"s0": s0, "s1": s1, "K": K, "buf": buf,
                                 "seg": torch.from_numpy(self.seg_host[s0:s1 + 1] - r0).to(self.dev)})
            s0 = s1
        for s, k in enumerate(self.keys):
            r0, r1 = int(self.seg_host[s]), int(self.seg_host[s + 1])
            if r1 > r0:
                c = np.asarray(self.all_obj[k]["color"], np.uint8).reshape(r1 - r0, -1)
                self.rgb[r0:r1, : c.shape[1]].copy_(torch.from_numpy(np.ascontiguousarray(c)))

    def _init_objects(self, eps: float, min_samples: int) -> None:
        all_obj = self.all_obj
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
        if self.compact is not None:
            return self._part_similarity_compact(q, objects)
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

    # -------------------------------------------------------------------------------------------- part regions
    _mesh_dev = None                # the packed meshes on the device, built by the first part_regions call

    def mesh_buffers(self):
        """-> (verts fp64 [V, 3] in packed map order, faces int32 [F, 3] of packed vertex ids, face_off int64 [S + 1],
        anchors fp64 numpy [S, 3]: the first vertex of every object), on the device, from all_obj[k]["mesh"].  Built on
        first use and kept: constructing a MapQuery uploads none of it."""
        if self._mesh_dev is not None:
            return self._mesh_dev
        vs, fs, foff, anchors = [], [], [0], np.zeros((self.S, 3))
        for s, k in enumerate(self.keys):
            m = self.all_obj[k]["mesh"]
            v = np.asarray(m.vertices, np.float64).reshape(-1, 3)
            f = np.asarray(m.faces, np.int64).reshape(-1, 3)
            n = int(self.seg_host[s + 1] - self.seg_host[s])
            if len(v) != n:
                raise ValueError(f"MapQuery: object {k}: the mesh has {len(v)} vertices, the part features {n}")
            if len(f) and (f.min() < 0 or f.max() >= n):
                raise ValueError(f"MapQuery: object {k}: a face names a vertex outside the mesh")
            if n:
                anchors[s] = v[0]
            vs.append(v)
            fs.append(f + int(self.seg_host[s]))
            foff.append(foff[-1] + len(f))
        if self.V > 0x7fffffff or foff[-1] > 0x7fffffff:
            raise ValueError("MapQuery: more than 2^31 - 1 vertices or faces")
        verts = torch.from_numpy(np.ascontiguousarray(np.concatenate(vs) if vs else np.zeros((0, 3)))).to(self.dev)
        faces = torch.from_numpy(np.ascontiguousarray((np.concatenate(fs) if fs else np.zeros((0, 3))).astype(np.int32)))
        self._mesh_dev = (verts, faces.to(self.dev), torch.tensor(foff, dtype=torch.int64, device=self.dev), anchors)
        return self._mesh_dev

    def part_regions(self, part_q, objects: Optional[Sequence[int]] = None, frac: float = 0.75,
                     min_cos: Optional[float] = None, min_area: float = 0.0, min_vertices: int = 1):
        """The connected surface patches of a part query -> map_regions.PartRegions.  A vertex of object s is selected
        iff its cosine with part_q is >= thr[s]; two selected vertices are connected iff a face of the mesh names both.
        thr[s] = fp32(mn + fp32(frac * fp32(mx - mn))) over the object's own minimum and maximum, i.e. the vertices the
        rainbow colouring shows at or above frac; with min_cos given, thr[s] = min_cos.  frac = 0.75 is an ASSUMED
        default, not a measured one.  objects: positions in the map's order (None: all); the others select nothing.
        min_area [m^2] / min_vertices drop small regions on the host; label is remapped to the rows that stay.
        Labelling, the compaction of the roots and the integer table run on the device (ops.regions_label /
        regions_table); R is read back once, then the table."""
        from . import map_regions as mr
        if min_cos is None and not 0.0 <= float(frac) <= 1.0:
            raise ValueError(f"part_regions: frac {frac} outside [0, 1]")
        if objects is not None:
            objects = [int(p) for p in objects]
            if any(not 0 <= p < self.S for p in objects):
                raise ValueError(f"part_regions: objects {objects}: positions in [0, {self.S})")
        pq = self._query(part_q, self.D, "part query")
        empty = mr.regions_from_table(np.zeros((0, mr.ROW), np.int64), np.zeros((max(self.S, 1), 3)), self.keys)
        if self.V == 0 or self.S == 0:
            return mr.PartRegions(torch.full((self.V,), -1, dtype=torch.int32, device=self.dev), empty,
                                  np.full(self.S, np.nan, np.float32))
        sims, mm = self.part_similarity(pq[None], objects=objects)
        thr = mr.thresholds(mm[:, 0].cpu().numpy(), frac, min_cos, objects)
        verts, faces, face_off, anchors = self.mesh_buffers()
        root, label, reg_off, status = ops.regions_label(self.seg_off, face_off, faces, sims, 0,
                                                         torch.from_numpy(thr).to(self.dev),
                                                         vmax=max(int(np.diff(self.seg_host).max()), 1))
        R = int(reg_off[-1])                                               # the one read-back before the table
        table = ops.regions_table(self.seg_off, face_off, verts, faces, sims, 0, root, label, R, status)
        fields = mr.regions_from_table(table.cpu().numpy(), anchors, self.keys)
        keep, remap = mr.filter_rows(fields["area"], fields["n_vertices"], min_area, min_vertices)
        if len(keep) != R:
            fields = {f: v[keep] for f, v in fields.items()}
            label = torch.from_numpy(remap).to(self.dev)[label.long()]     # (-1 indexes remap's last entry, -1)
        return mr.PartRegions(label, fields, thr, int(status.item()))

    # -------------------------------------------------------------------------------------------- the compact map
    def _columns(self, run, cols) -> torch.Tensor:
        """cols: per object of the run [K, Q] fp64 -> [n, H + 4, Q] fp32 on the device (zero rows for the padding)."""
        K, Q = run["K"], cols[0].shape[1]
        W = np.zeros((len(cols), K - 1 + ops.PART_ROW_PAD, Q), np.float32)
        for i, c in enumerate(cols):
            W[i, :K] = c                                              # the one rounding of head^T q^
        return torch.from_numpy(W).to(self.dev)

    def _part_similarity_compact(self, q: torch.Tensor, objects):
        qn = q.detach().cpu().numpy().astype(np.float64)
        qn = qn / np.maximum(np.linalg.norm(qn, axis=1, keepdims=True), 1e-8)       # objnerf_project's convention
        Q = qn.shape[0]
        full = objects is None
        out = torch.empty(self.V, Q, device=self.dev) if full else torch.full((self.V, Q), float("nan"), device=self.dev)
        mm = torch.empty(self.S, Q, 2, device=self.dev) if full else torch.full((self.S, Q, 2), float("nan"),
                                                                               device=self.dev)
        for run in self.compact:
            s0, s1 = run["s0"], run["s1"]
            r0 = int(self.seg_host[s0])
            if full:
                W = self._columns(run, [self.heads64[s].T @ qn.T for s in range(s0, s1)])
                _, m = ops.segment_project(run["buf"], run["seg"], W, out=out[r0:int(self.seg_host[s1])])
                mm[s0:s1] = m
                continue
            for p in objects:
                if not s0 <= p < s1:
                    continue
                a, b = int(self.seg_host[p]), int(self.seg_host[p + 1])
                if b == a:                                            # an empty object: the projection's own answer
                    mm[p, :, 0], mm[p, :, 1] = float("inf"), float("-inf")
                    continue
                W = self._columns(run, [self.heads64[p].T @ qn.T])
                _, m = ops.segment_project(run["buf"][a - r0:b - r0], torch.tensor([0, b - a]), W, out=out[a:b])
                mm[p] = m[0]
        return out, mm

    def _color_by_partfeat_compact(self, stats: Optional[Dict] = None) -> torch.Tensor:
        proj = torch.empty(self.V, 3, device=self.dev)
        mm = torch.empty(self.S, 3, 2, device=self.dev)
        eigh_s = 0.0
        for run in self.compact:
            s0, s1, K = run["s0"], run["s1"], run["K"]
            mean, scatter = ops.segment_moments(run["buf"], run["seg"])
            st = {}
            P, b = pca_weights_lowrank(mean[:, :K].cpu().numpy(), scatter[:, :K, :K].cpu().numpy(),
                                       self.heads64[s0:s1], np.diff(self.seg_host[s0:s1 + 1]), st)
            eigh_s += st["eigh_s"]
            _, m = ops.segment_project(run["buf"], run["seg"], self._columns(run, list(P)),
                                       torch.from_numpy(b).float(),
                                       out=proj[int(self.seg_host[s0]):int(self.seg_host[s1])])
            mm[s0:s1] = m
        if stats is not None:
            stats["eigh_s"] = eigh_s
        return self._colors(np.full(self.S, _lib.COLOR_PCA, np.int32), proj=proj, minmax=mm)

    def features(self, vertex_ids) -> torch.Tensor:
        """The unit part features [n, D] of the vertices vertex_ids (packed map order); a zero row for an id outside
        [0, V).  The dense map gathers its rows, the compact one expands them (ops.part_expand, per object hit)."""
        ids = torch.as_tensor(vertex_ids, dtype=torch.int64).reshape(-1).to(self.dev)
        n = int(ids.numel())
        out = torch.zeros(n, max(self.D, 1), device=self.dev)
        ok = (ids >= 0) & (ids < self.V)
        if n == 0 or not bool(ok.any()):
            return out
        if self.compact is None:
            out[ok] = self.part_feat[ids[ok]]
            return out
        seg = torch.bucketize(ids, self.seg_off[1:], right=True)          # the object of every valid id
        for s in torch.unique(seg[ok]).tolist():
            sel = torch.nonzero(ok & (seg == s)).reshape(-1)
            run = next(r for r in self.compact if r["s0"] <= s < r["s1"])
            a = int(self.seg_host[s]) - int(self.seg_host[run["s0"]])
            rows = run["buf"][a:a + int(self.seg_host[s + 1] - self.seg_host[s]), :run["K"]]
            out[sel] = ops.part_expand(rows, self.heads[s], ids[sel] - int(self.seg_host[s]))
        return out

    def store_bytes(self) -> int:
        """Device bytes of the packed part features: V x D fp32 (dense), or the padded rows plus the heads (compact)."""
        if self.compact is None:
            return int(self.V) * int(self.D) * 4
        return sum(r["buf"].numel() * 4 for r in self.compact) + sum(h.numel() * 4 for h in self.heads)

    def color_by_partfeat(self, stats: Optional[Dict] = None) -> torch.Tensor:
        if self.compact is not None:
            return self._color_by_partfeat_compact(stats)
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
           "pca_weights_lowrank", "compact_layout", "reduce_object_features", "top_positions"]
