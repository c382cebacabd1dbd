"""The specification of openobj_amd.map_points in plain torch / numpy, and the small scenes its tests share.

Semantics (N world points [N, 3] fp32, K objects in a caller-fixed order, each a network, obj_scale, an oriented box
(center, R, extent), an obj_center offset and a background flag):

* CANDIDATE: point n is a candidate of object k iff |R_k^T (p_n - c_k)| <= extent_k / 2 component-wise, in fp32;
* SCORE: alpha = 10 * raw of OccupancyMap.forward at p_n - obj_center_k (the oracle's chain); occupied: alpha > 0;
* WINNER: only occupied candidates; any occupied foreground candidate beats every background one; the largest alpha wins,
  equal alphas go to the lower position in the list; without an occupied candidate the label is -1, colour and feature
  are 0 and alpha is the largest candidate alpha (-inf without a candidate).

Nothing here imports the product code."""
import functools
import os

import numpy as np
import torch

from oracle import objnerf_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
AMBIGUOUS_CAP = 0.02          # of N
ALPHA_TOL = 1e-4              # what either implementation's alpha may move by (tests/test_hip_parity.py:60)
FACE_MARGIN = 1e-4            # x the smallest extent: how far test points stay from every box face


def _golden(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {k: d[k] for k in d.files}


def _T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


# ------------------------------------------------------------------------------------------------------- the semantics
def box_locals(points, obj, dtype):
    """R^T (p - c) and extent / 2 in `dtype`."""
    p = torch.as_tensor(points).to(dtype)
    c = torch.as_tensor(np.asarray(obj["center"], np.float64)).to(dtype)
    R = torch.as_tensor(np.asarray(obj["R"], np.float64)).to(dtype)
    half = torch.as_tensor(np.asarray(obj["extent"], np.float64)).to(dtype) * 0.5
    return (p - c) @ R, half


def candidate_mask(points, objs):
    """[K, N] bool, the fp32 box test."""
    rows = []
    for o in objs:
        l, half = box_locals(points, o, torch.float32)
        rows.append((l.abs() <= half).all(dim=1))
    return torch.stack(rows)


def face_margin(points, objs):
    """The smallest fp64 distance of a point's local coordinate to a face, over all boxes, in units of the smallest
    extent of all boxes: the fp32 test cannot disagree with the fp64 one while this stays above fp32 rounding."""
    m = np.inf
    ext = min(float(np.min(o["extent"])) for o in objs)
    for o in objs:
        l, half = box_locals(points, o, torch.float64)
        m = min(m, float((l.abs() - half).abs().min()))
    return m / ext


def candidate_lists(cand):
    """[K, N] bool -> (seg_off int64 [K + 1], pair_pt int32 [M]): object-major, ascending in the point index."""
    K = cand.shape[0]
    seg, pts = [0], []
    for k in range(K):
        idx = torch.nonzero(cand[k]).reshape(-1)
        pts.append(idx)
        seg.append(seg[-1] + int(idx.numel()))
    return torch.tensor(seg, dtype=torch.int64), torch.cat(pts).to(torch.int32)


def oracle_eval(points, objs, want_feat=True):
    """Every object on every point through the oracle: alpha [K, N], colour [K, N, 3], clip [K, N, C]."""
    p = torch.as_tensor(points, dtype=torch.float32)
    al, co, fe = [], [], []
    for o in objs:
        emb = O.unidirs_embed(p - torch.tensor(float(o["obj_center"]), dtype=torch.float32), o["B"], float(o["scale"]))
        a, c, f = O.mlp_forward(o["p"], emb, do_clip=want_feat)
        al.append(a.squeeze(-1))
        co.append(c)
        if want_feat:
            fe.append(f)
    return torch.stack(al), torch.stack(co), (torch.stack(fe) if want_feat else None)


def _group_top2(alpha, member):
    """Per point: (largest alpha, its first position, second largest) among the objects flagged in member [K, N]."""
    K = alpha.shape[0]
    a = torch.where(member, alpha, torch.full_like(alpha, -np.inf))
    top, pos = a.max(dim=0)                                     # torch returns the FIRST maximal position
    pos = torch.where(torch.isfinite(top), pos, torch.full_like(pos, -1))
    if K > 1:
        a2 = a.clone()
        a2[pos.clamp(min=0), torch.arange(a.shape[1])] = -np.inf
        second = a2.max(dim=0).values
    else:
        second = torch.full_like(top, -np.inf)
    return top, pos, second


def label_spec(alpha, cand, is_bg, color=None, feat=None):
    """alpha [K, N], cand [K, N] bool, is_bg [K] -> dict(obj int32 [N], alpha [N], color, part_feat, ambiguous bool [N])."""
    is_bg = torch.as_tensor(is_bg, dtype=torch.bool)
    N = alpha.shape[1]
    occ = cand & (alpha > 0)
    fg_top, fg_pos, fg_2nd = _group_top2(alpha, occ & ~is_bg[:, None])
    bg_top, bg_pos, bg_2nd = _group_top2(alpha, occ & is_bg[:, None])
    any_top, _, _ = _group_top2(alpha, cand)
    has_fg, has_bg = fg_pos >= 0, bg_pos >= 0
    obj = torch.where(has_fg, fg_pos, torch.where(has_bg, bg_pos, torch.full_like(fg_pos, -1)))
    out_alpha = torch.where(has_fg, fg_top, torch.where(has_bg, bg_top, any_top))
    # ambiguity: an alpha that decides occupancy within ALPHA_TOL of 0, or the two best of the deciding group closer than
    # 2 ALPHA_TOL (either side may move by ALPHA_TOL).  The groups are taken over ALL candidates, not the occupied ones: a
    # candidate just below 0 may become occupied.
    near0 = cand & (alpha.abs() <= ALPHA_TOL)
    fg_near0 = (near0 & ~is_bg[:, None]).any(dim=0)
    bg_near0 = (near0 & is_bg[:, None]).any(dim=0)
    dec_top = torch.where(has_fg, fg_top, bg_top)
    dec_2nd = torch.where(has_fg, fg_2nd, bg_2nd)
    close = (has_fg | has_bg) & ((dec_top - dec_2nd) < 2 * ALPHA_TOL)
    ambiguous = fg_near0 | (~has_fg & bg_near0) | close
    res = {"obj": obj.to(torch.int32), "alpha": out_alpha, "ambiguous": ambiguous}
    idx = obj.clamp(min=0).long()
    lab = obj >= 0
    ar = torch.arange(N)
    if color is not None:
        res["color"] = torch.where(lab[:, None], color[idx, ar], torch.zeros(N, 3))
    if feat is not None:
        res["part_feat"] = torch.where(lab[:, None], feat[idx, ar], torch.zeros(N, feat.shape[-1]))
    return res


def confusion_spec(pred, gt, n, ignore=-1):
    """Loops, no bincount: [n, n + 1], rows ground truth, columns prediction, last column = predictions outside [0, n)."""
    conf = np.zeros((n, n + 1), np.int64)
    for p, g in zip(np.asarray(pred).reshape(-1), np.asarray(gt).reshape(-1)):
        if g == ignore or g < 0 or g >= n:
            continue
        conf[g, p if 0 <= p < n else n] += 1
    return conf


# ------------------------------------------------------------------------------------------------------------ scenes
def _rotation(rs):
    q, _ = np.linalg.qr(rs.randn(3, 3))
    if np.linalg.det(q) < 0:
        q[:, 2] = -q[:, 2]
    return q


def _net32(k):
    g = _golden("g5_step_s10_feat")
    return dict(p=[_T(g[f"fc0_{i}"][k]) for i in range(18)], B=_T(g["B0"][k]), scale=2.0, hidden=32)


def _net_g2(hidden):
    if hidden not in (32, 128):            # no fixture of this width: the oracle's own initialisation, seeded
        gen = torch.Generator().manual_seed(100 + hidden)
        return dict(p=O.init_object_params(hidden, 512, gen), B=O.icosa_dirs(), scale=2.0, hidden=hidden)
    g = _golden("g2_mlp")
    return dict(p=[_T(g[f"h{hidden}_p{i}"]) for i in range(18)], B=O.icosa_dirs(), scale=2.0, hidden=hidden)


def _obj(net, center, R, extent, obj_id, class_id, obj_center=0.0):
    d = dict(net)
    d.update(center=np.asarray(center, np.float64), R=np.asarray(R, np.float64), extent=np.asarray(extent, np.float64),
             obj_id=obj_id, class_id=class_id, obj_center=obj_center)
    return d


N_MAIN = 3 * 64 + 37
SEED = 11


def _fg_boxes(rs):
    """Four rotated, overlapping boxes around the origin."""
    return [((0.15, 0.0, -0.1), _rotation(rs), (1.3, 1.7, 2.1)),
            ((-0.2, 0.1, 0.15), _rotation(rs), (1.1, 1.5, 1.9)),
            ((0.05, -0.2, 0.1), _rotation(rs), (1.2, 1.4, 2.3)),
            ((0.0, 0.15, -0.15), _rotation(rs), (1.0, 1.6, 2.0))]


def _draw_points(rs, objs, n_pool, lo=-1.3, hi=1.3):
    """A pool of fp32 points in the cube that stay FACE_MARGIN (x 10, for slack) away from every face of every box."""
    pts = rs.uniform(lo, hi, (n_pool, 3)).astype(np.float32)
    ext = min(float(np.min(o["extent"])) for o in objs)
    keep = np.ones(n_pool, bool)
    for o in objs:
        l, half = box_locals(pts, o, torch.float64)
        keep &= ((l.abs() - half).abs().min(dim=1).values.numpy() > 10 * FACE_MARGIN * ext)
    return pts[keep]


@functools.lru_cache(maxsize=None)
def main_scene():
    """Objects [A, EMPTY, B, C, D] (hidden 32: the three networks of g5_step_s10_feat; two of them are rarely occupied, so
    the third also serves D, at another obj_center, to give the winners a contest; EMPTY's box lies outside the cloud)
    and N_MAIN points: 0, 1, 2 and 3 boxes per point all occur, EMPTY's segment is empty and B's has exactly 64 pairs."""
    rs = np.random.RandomState(SEED)
    bx = _fg_boxes(rs)
    objs = [_obj(_net32(0), *bx[0], obj_id=3, class_id=1),
            _obj(_net32(0), (9.0, 9.0, 9.0), _rotation(rs), (0.5, 0.6, 0.7), obj_id=5, class_id=2),
            _obj(_net32(1), *bx[1], obj_id=7, class_id=1),
            _obj(_net32(2), *bx[2], obj_id=9, class_id=4, obj_center=0.25),
            _obj(_net32(2), *bx[3], obj_id=12, class_id=2, obj_center=-0.5)]
    pool = _draw_points(rs, objs, 4000)
    cand = candidate_mask(pool, objs).numpy()
    in_b = cand[2]
    count = cand.sum(0)
    sel_b = np.nonzero(in_b)[0][:64]
    rest = np.nonzero(~in_b)[0]
    # the first points outside B of every multiplicity 0, 1, 2, then the pool's order
    first = [np.nonzero((~in_b) & (count == c))[0][:8] for c in (0, 1, 2)]
    first = np.concatenate(first)
    rest = np.concatenate([first, np.setdiff1d(rest, first, assume_unique=False)])[:N_MAIN - 64]
    idx = rs.permutation(np.concatenate([sel_b, rest]))
    return objs, np.ascontiguousarray(pool[idx])


@functools.lru_cache(maxsize=None)
def background_scene(bg_hidden):
    """[BG, A, B, C, D]: a background box (obj_id 0) that contains the whole cloud, the foreground boxes inside it.
    bg_hidden 32: the hidden-32 weights of g2_mlp; 128: its hidden-128 weights (the merge path); other widths (64, 96:
    the head's other instantiations) are initialised as the reference initialises a network, from a seed."""
    rs = np.random.RandomState(SEED + 1)
    bx = _fg_boxes(rs)
    objs = [_obj(_net_g2(bg_hidden), (0.0, 0.0, 0.0), _rotation(rs), (6.0, 6.0, 6.0), obj_id=0, class_id=0),
            _obj(_net32(0), *bx[0], obj_id=3, class_id=1),
            _obj(_net32(1), *bx[1], obj_id=7, class_id=2),
            _obj(_net32(2), *bx[2], obj_id=9, class_id=4),
            _obj(_net32(2), *bx[3], obj_id=12, class_id=2, obj_center=-0.5)]
    pts = _draw_points(rs, objs, 400)[:N_MAIN]
    return objs, np.ascontiguousarray(pts)


@functools.lru_cache(maxsize=None)
def reference(scene, bg_hidden=32):
    """The specification's answer for a scene, computed once: dict(objs, points, cand, seg_off, pair_pt, alpha [K, N],
    color, feat, spec = label_spec(...))."""
    if scene == "main":
        objs, pts = main_scene()
    elif scene == "cli":                 # three checkpoints: the hidden-128 background and two objects, ids ascending
        objs, pts = background_scene(128)
        objs = [dict(o, obj_center=0.0) for o in (objs[0], objs[1], objs[3])]       # a checkpoint carries no obj_center
    else:
        objs, pts = background_scene(bg_hidden)
    cand = candidate_mask(pts, objs)
    seg_off, pair_pt = candidate_lists(cand)
    alpha, color, feat = oracle_eval(pts, objs)
    is_bg = [o["obj_id"] == 0 for o in objs]
    return dict(objs=objs, points=pts, cand=cand, seg_off=seg_off, pair_pt=pair_pt, alpha=alpha, color=color, feat=feat,
                is_bg=is_bg, spec=label_spec(alpha, cand, is_bg, color, feat))
