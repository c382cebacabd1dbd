"""Trainer -- owns one OccupancyMap + UniDirsEmbed per object (trainer.py:11-128); both modules'
parameters are views of ONE per-object arena block, so update_vmap can gather K of them with a copy."""
import numpy as np
import torch

from . import embedding, model, ops, render_rays, vis
from .mesh import PointCloud


class Trainer:
    def __init__(self, cfg):
        self.obj_id = cfg.obj_id
        self.device = cfg.training_device
        self.hidden_feature_size = cfg.hidden_feature_size        # 32 objects / 128 background
        self.clip_point_feature_size = cfg.clip_point_feature_size
        self.obj_scale = cfg.obj_scale
        self.n_unidir_funcs = cfg.n_unidir_funcs
        self.emb_size1 = 21 * (3 + 1) + 3                         # trainer.py:20
        self.emb_size2 = 21 * (5 + 1) + 3 - self.emb_size1        # trainer.py:21
        self.load_network()
        self.bound_extent = 0.995 if self.obj_id == 0 else 0.9    # trainer.py:25-28
        self.W_vis, self.H_vis = cfg.W, cfg.H
        self.T_WC_gt = None
        self.dirs_C_gt = None
        self.input_pcs = None

    def load_network(self):                                       # trainer.py:36-44
        self.arena = ops.ParamArena(1, ops.NetShape(self.hidden_feature_size, self.clip_point_feature_size,
                                                    self.n_unidir_funcs + 1), self.device)
        self.fc_occ_map = model.OccupancyMap(self.emb_size1, self.emb_size2, hidden_size=self.hidden_feature_size,
                                             clip_size=self.clip_point_feature_size, device=self.device,
                                             _arena=self.arena)
        self.fc_occ_map.apply(model.init_weights)
        self.pe = embedding.UniDirsEmbed(max_deg=self.n_unidir_funcs, scale=self.obj_scale, device=self.device,
                                         _arena=self.arena)

    def eval_points(self, points, chunk_size=300000):
        """points [N,3] -> (occupancy [N], color [N,3], clip [N,C]) or None (trainer.py:105-128).
        One fused launch per chunk: PE + MLP + feature head; occupancy = sigmoid(alpha)."""
        self.arena.scale.fill_(float(self.obj_scale))
        n_chunks = int(np.ceil(points.shape[0] / chunk_size))
        occ, color, clip = [], [], []
        with torch.no_grad():
            for k in range(n_chunks):
                pts = points[k * chunk_size:(k + 1) * chunk_size].reshape(1, -1, 3).to(self.device).contiguous()
                a, c, _, f = ops.eval_points(self.arena, pts, want_clip=True)
                occ.append(ops.occupancy(a[0]))
                color.append(c[0])
                clip.append(f[0])
        occ, color, clip = torch.cat(occ), torch.cat(color), torch.cat(clip)
        if occ.max() == 0:
            print("no occ")
            return None
        return (occ, color, clip)

    def eval_grad(self, points, chunk_size=1 << 18):
        """points [N,3] -> (alpha [N] = 10 * raw of model.py:88, grad [N,3] = d alpha / d points), on the device.  Hidden
        32: the fused kernel of MapPoints (ops.mappoints_grad) over the trivial one-segment list; wider networks: the
        layer-wise chain (ops.field_grad_layerwise) in chunks.  The reference has no counterpart."""
        self.arena.scale.fill_(float(self.obj_scale))
        pts = torch.as_tensor(points).reshape(-1, 3).to(self.device, torch.float32).contiguous()
        n, dev = int(pts.shape[0]), pts.device
        if n == 0:
            return torch.empty(0, device=dev), torch.empty(0, 3, device=dev)
        with torch.no_grad():
            if self.hidden_feature_size != 32:
                return ops.field_grad_layerwise(self.arena, pts, chunk_size)
            boxes = torch.zeros(1, 16, device=dev)                 # never tested here: every point is a pair
            info = torch.zeros(1, 2, dtype=torch.int32, device=dev)
            seg_off = torch.tensor([0, n], dtype=torch.int64, device=dev)
            pair_pt = torch.arange(n, dtype=torch.int32, device=dev)
            alpha, grad = torch.empty(n, device=dev), torch.empty(n, 3, device=dev)
            ops.mappoints_grad(self.arena, pts, boxes, info, seg_off, pair_pt, alpha, grad)
        return alpha, grad

    def eval_points_compact(self, points, chunk_size=300000):
        """points [N,3] -> (occupancy [N], color [N,3], rows [N, H+1], head [C, H+1]) or None: eval_points without the
        C-wide feature.  rows = ops.part_rows of the feature hidden: head . rows[v] is the unit part feature of point v
        (DESIGN.md 4.25)."""
        self.arena.scale.fill_(float(self.obj_scale))
        views = self.arena.views()
        of_w, of_b = views[16][0].contiguous(), views[17][0].contiguous()
        H = int(of_w.shape[1])
        n = int(points.shape[0])
        buf = torch.empty(n, H + ops.PART_ROW_PAD, device=self.device)
        occ, color = [], []
        with torch.no_grad():
            for k in range(0, n, chunk_size):
                pts = points[k:k + chunk_size].reshape(1, -1, 3).to(self.device).contiguous()
                a, c, h, _ = ops.eval_points(self.arena, pts, want_hfeat=True)
                occ.append(ops.occupancy(a[0]))
                color.append(c[0])
                ops.part_rows(h[0], of_w, of_b, out=buf[k:k + chunk_size])
        occ, color = torch.cat(occ), torch.cat(color)
        if occ.max() == 0:
            print("no occ")
            return None
        return occ, color, buf[:, :H + 1], torch.cat([of_w, of_b[:, None]], dim=1)

    def sample_points_bbox(self, bbox, do_eval=True, draws=None):
        """Points inside a known oriented 3-D box along the rays self.T_WC_gt / self.dirs_C_gt
        (trainer.py:130-198).  bbox: anything with .center [3], .R [3,3], .extent [3] (the reference passes an
        open3d OrientedBoundingBox).  draws: optional [n_hit, n_bins] tensor replacing the torch.rand of
        stratified_bins (utils.py:371) -- tests inject the reference's draw.  Sets self.dirs_W, self.origins,
        self.z_vals, self.input_pcs (device tensors) and returns (hit_mask, near[hit], far[hit]) or
        (None, None, None) when at most one ray hits (:164-165)."""
        n_bins = 60 if self.obj_id == 0 else 20                  # :141-144
        if do_eval:
            n_bins = 150
        dev = self.device
        T_WC = torch.as_tensor(self.T_WC_gt[0], dtype=torch.float32).cpu()     # one view: every row is the same pose
        T_WO = torch.eye(4)
        T_WO[:3, :3] = torch.as_tensor(np.asarray(bbox.R))                      # :152-154
        T_WO[:3, 3] = torch.as_tensor(np.asarray(bbox.center))
        T_OC = torch.inverse(T_WO) @ T_WC                                       # :156-157
        half = torch.as_tensor(np.asarray(bbox.extent, np.float64) / 2.0).float()       # :161
        dirs_C = torch.as_tensor(self.dirs_C_gt, dtype=torch.float32).to(dev).reshape(-1, 3)
        dirs_W, near, far, hit = ops.box_rays(T_WC, T_OC, half, dirs_C)
        n_rays = int(hit.sum())
        if n_rays <= 1:
            # (nothing of an earlier call may be served by the lazy z_vals / input_pcs properties after this)
            self._bbox_samples = None
            self._z_vals = self._input_pcs = None
            return None, None, None
        self.dirs_W = dirs_W[hit]
        self.origins = T_WC[:3, 3].to(dev).expand(n_rays, 3)
        near_h, far_h = near[hit].contiguous(), far[hit].contiguous()
        u = None if draws is None else torch.as_tensor(draws).to(dev)     # None: drawn inside the kernel (seeded)
        # z_vals / input_pcs are formed on first access (properties below): the fused renderer (vmap.render_2D_syn ->
        # ops.render_fwd) never needs the [n, 149, 3] point tensor; the same (seed, draw) reproduces the same numbers
        # (the process-wide Philox call counter advances only when this call DRAWS: injected draws leave every later
        # seeded launch on the stream it would have had without this call)
        draw = (ops._next_offset() & 0x1FFFFFFF) if u is None else 0
        self._bbox_samples = dict(origin=T_WC[:3, 3], dirs_W=self.dirs_W.contiguous(), near=near_h, far=far_h, u=u,
                                  n_bins=n_bins, seed=ops._seed_of(None), draw=draw)
        self._z_vals = self._input_pcs = None
        return hit, near_h, far_h

    def _materialise_bbox_samples(self):
        b = self._bbox_samples
        if b is None:
            raise RuntimeError("z_vals / input_pcs: the last sample_points_bbox call found no ray inside the box")
        self._z_vals, self._input_pcs = ops.box_points(b["origin"], b["dirs_W"], b["near"], b["far"], b["u"], b["n_bins"],
                                                       seed=b["seed"], draw=b["draw"])

    @property
    def z_vals(self):                       # trainer.py:175
        if getattr(self, "_z_vals", None) is None:
            self._materialise_bbox_samples()
        return self._z_vals

    @z_vals.setter
    def z_vals(self, v):
        self._z_vals = v

    @property
    def input_pcs(self):                    # trainer.py:176
        if getattr(self, "_input_pcs", None) is None:
            self._materialise_bbox_samples()
        return self._input_pcs

    @input_pcs.setter
    def input_pcs(self, v):
        self._input_pcs = v

    def _eval_grid(self, points, chunk_size=1 << 21):
        """occupancy [N], colour [N,3] on the device, without the 512-d head (trainer.py:64-66 keeps only these two
        of the grid's outputs; at 128^3 the head alone would be a 4.3 GB tensor).  Hidden 32: one fused launch;
        wider networks run layer by layer in chunks that bound the activation workspace."""
        self.arena.scale.fill_(float(self.obj_scale))
        n = points.shape[0]
        step = n if self.hidden_feature_size == 32 else chunk_size
        occ, color = [], []
        with torch.no_grad():
            for k in range(0, n, step):
                pts = points[k:k + step].reshape(1, -1, 3).to(self.device).contiguous()
                a, c, _, _ = ops.eval_points(self.arena, pts)
                occ.append(ops.occupancy(a[0]))
                color.append(c[0])
        return torch.cat(occ), torch.cat(color)

    def meshing(self, bound, obj_center, grid_dim=256, save_pcd=True, save_mesh=True, if_color=False, if_part=False,
                part_compact=False):
        """Trainer.meshing (trainer.py:46-103) with its return shapes: (None, None) when the grid is empty (:63-64),
        None when marching cubes or the vertex re-query fails (:81-84, :95-96), (pcd, None, None) on the save_pcd
        branch (its voxel_down_sample result is discarded there, :70-77), (None, mesh, partfeat) otherwise.
        bound: .center [3], .R [3,3], .extent [3] (an open3d OrientedBoundingBox in the reference).  mesh is a
        mesh.TriMesh, pcd a mesh.PointCloud; partfeat the [V, 512] device feature of the vertices (if_part), or with
        part_compact the pair (rows [V, H+1], head [C, H+1]) of eval_points_compact: the same mesh and colours without
        the 512-d feature."""
        occ_range = [-1., 1.]
        range_dist = occ_range[1] - occ_range[0]
        scene_scale_np = np.asarray(bound.extent) / (range_dist * self.bound_extent)        # :51
        scene_scale = torch.from_numpy(np.asarray(scene_scale_np)).float().to(self.device)
        transform_np = np.eye(4, dtype=np.float32)                                            # :53-56
        transform_np[:3, 3] = np.asarray(bound.center)
        transform_np[:3, :3] = np.asarray(bound.R)
        transform = torch.from_numpy(transform_np).to(self.device)
        grid_pc = render_rays.make_3D_grid(occ_range=occ_range, dim=grid_dim, device=self.device,
                                           scale=scene_scale, transform=transform).view(-1, 3)   # :58-59
        grid_pc -= torch.as_tensor(obj_center, dtype=torch.float32).to(grid_pc.device)        # :60
        occ, colors = self._eval_grid(grid_pc)                                                # :61
        if occ.max() == 0:                                                                    # (eval_points :124-126)
            print("no occ")
            return None, None
        pcd = mesh = partfeat = None
        if save_pcd:                                                                          # :69-77
            mask_valid = occ > 0.5
            pcd = PointCloud(grid_pc[mask_valid].cpu().numpy(), colors[mask_valid].cpu().numpy())
        elif save_mesh:                                                                       # :78-101
            mesh = vis.marching_cubes(occ.view(grid_dim, grid_dim, grid_dim))
            if mesh is None:
                print("marching cube failed")
                return None
            mesh.apply_translation([-0.5, -0.5, -0.5])                                        # :85-90
            mesh.apply_scale(2)
            mesh.apply_scale(scene_scale_np)
            mesh.apply_transform(transform_np)
            if if_color or if_part:
                # the re-query does NOT subtract obj_center (:92), as in the reference
                vertices_pts = torch.from_numpy(np.array(mesh.vertices)).float().to(self.device)
                if if_part and part_compact:
                    ret = self.eval_points_compact(vertices_pts)
                    if ret is None:
                        return None
                    _, color, rows, head = ret
                    partfeat = (rows, head)
                elif if_part:
                    ret = self.eval_points(vertices_pts)
                    if ret is None:
                        return None
                    _, color, clip = ret
                    partfeat = clip
                else:
                    o, color = self._eval_grid(vertices_pts)
                    if o.max() == 0:
                        print("no occ")
                        return None
                if if_color:
                    mesh.visual.vertex_colors = (color * 255).cpu().numpy().astype(np.uint8)  # truncates (:97-99)
        return pcd, mesh, partfeat
