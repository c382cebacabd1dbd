"""The mask graph's kernels (objnerf_maskgraph.hip) on the GPU against the numpy / scipy restatement in
tests/maskgraph_util.py: segmented DBSCAN and its fallback policy, the ray / box pass, the cloud overlap, the per-frame
mask clouds, the affinity pass, the comparisons' exact edges and the command line end to end on a synthetic scene."""
import functools
import os

import numpy as np
import pytest
import torch

from openobj_amd import mask_graph as MG
from openobj_amd import ops
try:
    from tests import maskgraph_util as U
except ImportError:          # plain `pytest tests/` puts tests/ itself, not the repository root, on sys.path
    import maskgraph_util as U

pytestmark = pytest.mark.gpu

EPS = 0.05


# ----------------------------------------------------------------------------------------------------------- DBSCAN
def _blobs(rs, sizes, sigmas, span):
    return np.concatenate([rs.randn(n, 3) * s + rs.uniform(0, span, 3) for n, s in zip(sizes, sigmas)])


@functools.lru_cache(maxsize=None)
def _dbscan_case():
    """Segments of 1, 63, 64, 65, 0, 1 000 and 20 000 points; the 1 000 lie in blobs spread over 60 m (1 200 cells of
    0.05 per axis); the 20 000 are blobs of several densities plus uniform noise, shuffled."""
    rs = np.random.RandomState(7)
    segs = [rs.randn(1, 3)]
    for n in (63, 64, 65):
        segs.append(np.concatenate([rs.randn(n - 20, 3) * 0.03, rs.randn(20, 3) * 0.02 + [0.3, 0.0, 0.0]]))
    segs.append(np.zeros((0, 3)))
    far = np.concatenate([rs.randn(50, 3) * 0.02 + np.array([3.0, 3.0, 3.0]) * k for k in range(20)])
    segs.append(far[rs.permutation(len(far))])
    big = np.concatenate([_blobs(rs, [4000, 3000, 3000, 2500, 1500, 500, 300, 200],
                                 [0.10, 0.08, 0.12, 0.15, 0.06, 0.05, 0.04, 0.05], 1.5),
                          rs.uniform(-0.3, 1.8, (5000, 3))])
    segs.append(big[rs.permutation(len(big))])
    off = np.concatenate([[0], np.cumsum([len(s) for s in segs])])
    assert (segs[5].max(0) - segs[5].min(0)).min() > 1024 * EPS
    for s in segs:                                           # no pair at the comparison's edge
        assert U.min_gap_to_radius(s, EPS) > 1e-9
    want = {mp: np.concatenate([U.dbscan_labels(s, EPS, mp) for s in segs]) for mp in (100, 20, 10)}
    return np.concatenate(segs), off, want


@pytest.mark.parametrize("mp", [100, 20, 10])
def test_dbscan_labels_equal_the_restatement(dev, mp):
    pts, off, want = _dbscan_case()
    got = ops.dbscan(torch.from_numpy(pts).to(dev), off, EPS, mp).cpu().numpy()
    w = want[mp]
    print("clusters per segment:", [int(w[a:b].max(initial=-1)) + 1 for a, b in zip(off[:-1], off[1:])],
          "noise:", int((w == -1).sum()), "mismatches:", int((got != w).sum()))
    assert w[off[-2]:].max() >= 1 and (w[off[-2]:] == -1).any()          # several clusters and noise in the large set
    assert np.array_equal(got, w)


def test_dbscan_per_segment_min_points_and_determinism(dev):
    """min_points per set; a set switched off (<= 0) keeps the labels of the previous run; two runs write the same."""
    pts, off, want = _dbscan_case()
    S = len(off) - 1
    plan = ops.DbscanPlan(torch.from_numpy(pts).to(dev), off, EPS)
    first = plan.run(100).cpu().numpy()
    assert np.array_equal(first, want[100])
    mp = np.array([10, 0, 20, 10, 10, 10, 0][:S])
    got = plan.run(mp).cpu().numpy()
    again = ops.DbscanPlan(torch.from_numpy(pts).to(dev), off, EPS)
    again.run(100)
    assert np.array_equal(again.run(mp).cpu().numpy(), got)
    for s in range(S):
        w = want[int(mp[s])] if mp[s] > 0 else want[100]
        assert np.array_equal(got[off[s]:off[s + 1]], w[off[s]:off[s + 1]]), s


@pytest.mark.parametrize("tile", [1024, 4096])
def test_dbscan_root_ranks_carry_across_scan_tiles(dev, tile):
    """256 tile + 300 points in one set: tile + 2 blocks of 256, so a one-workgroup scan of the blocks' root counts in
    tiles of `tile` elements carries from its first tile into a second (4096 = objnerf_wg.h's 1024 threads x 4
    elements; 1024 = a tile of one element a thread).  The points lie site by site in clusters of 4 (1 mm apart, the
    sites 0.5 m = 10 eps apart) and min_points is 3: every point is core, cluster = site, and clusters are numbered by
    their smallest core index (maskgraph_util.dbscan_labels' rule), so labels[i] == i // 4.  A second set of the same
    call holds isolated points only: all noise, and the first set's labels do not move."""
    n1 = 256 * tile + 300
    site = np.arange(n1) // 4
    pts1 = np.stack([site % 65, (site // 65) % 65, site // 4225], 1) * 0.5
    pts1[:, 0] += (np.arange(n1) % 4) * 0.001
    pts2 = _line(50, [100.0, 0.0, 0.0], step=1.0)
    assert n1 // 4 < 65 ** 3
    off = np.array([0, n1, n1 + 50])
    got = ops.dbscan(torch.from_numpy(np.concatenate([pts1, pts2])).to(dev), off, EPS, 3).cpu().numpy()
    assert np.array_equal(got[:n1], site)
    assert (got[n1:] == -1).all()
    alone = ops.dbscan(torch.from_numpy(pts1).to(dev), off[:2], EPS, 3).cpu().numpy()
    assert np.array_equal(alone, got[:n1])


def _line(n, start, step=0.0049):
    return np.asarray(start, np.float64) + np.arange(n)[:, None] * np.array([step, 0.0, 0.0])


def test_denoise_fallback_chain_and_tie_rule(dev):
    """pcd_denoise_dbscan's chain 100 -> 20 -> 10 -> keep all, and Counter.most_common's tie rule: two clusters of 41
    points, the one numbered 1 met first (its border point is row 0)."""
    rs = np.random.RandomState(3)
    tie = np.concatenate([[[5.0 - 0.0055, 0.0, 0.0]], _line(41, [0.0, 0.0, 0.0]), _line(40, [5.0, 0.0, 0.0])])
    clouds = [np.concatenate([rs.randn(400, 3) * 0.02, rs.uniform(-1, 1, (40, 3))]),        # a cluster at 100
              np.concatenate([rs.randn(30, 3) * 0.012, rs.uniform(2, 3, (10, 3))]),         # none at 100, one at 20
              np.concatenate([rs.randn(12, 3) * 0.008, rs.uniform(2, 3, (6, 3))]),          # only at 10
              rs.uniform(0, 5, (7, 3)),                                                     # none: keep all
              tie]
    lab = U.dbscan_labels(tie, EPS, 20)
    assert lab[0] == 1 and (lab == 0).sum() == (lab == 1).sum() == 41 and U.dbscan_labels(tie, EPS, 100).max() == -1
    for c in clouds:
        assert U.min_gap_to_radius(c, EPS) > 1e-9
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    keep, used = MG.denoise_clouds(torch.from_numpy(np.concatenate(clouds)).to(dev), off, EPS, (100, 20, 10))
    assert used.tolist() == [100, 20, 10, 0, 20]
    for s, c in enumerate(clouds):
        assert np.array_equal(keep[off[s]:off[s + 1]], U.denoise(c, EPS, (100, 20, 10))), s
    assert keep[off[4]] and keep[off[4] + 42:off[5]].all() and not keep[off[4] + 1:off[4] + 42].any()


# ------------------------------------------------------------------------------------------------------------ overlap
@pytest.mark.parametrize("C,thr", [(1, 0.02), (2, 0.05), (9, 0.02), (9, 0.05)])
def test_cloud_overlap_counts_equal_ckdtree(dev, C, thr):
    rs = np.random.RandomState(10 + C)
    sizes = [300] if C == 1 else [40, 30000] if C == 2 else [1, 0, 7, 30000, 2000, 500, 64, 65, 9000]
    clouds = []
    for k, n in enumerate(sizes):
        c = rs.uniform(0, 1.2, (n, 3)) * [1.0, 1.0, 0.15] + [0.4 * (k % 3), 0.3 * (k // 3), 0.0]
        clouds.append(c)
    want, gap = U.overlap_counts(clouds, thr)
    assert gap > 1e-12
    off = np.concatenate([[0], np.cumsum(sizes)])
    pts = torch.from_numpy(np.concatenate(clouds)).to(dev)
    got = ops.cloud_overlap(pts, off, thr).cpu().numpy()
    print("counts\n", want)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert np.array_equal(ops.cloud_overlap(pts, off, thr).cpu().numpy(), got)
    if C > 1:
        assert (want[~np.eye(C, dtype=bool)] > 0).any() and (want < np.asarray(sizes)[:, None]).any()
    sim = MG.cloud_similarity(clouds, thr, dev)
    for a in range(C):
        for b in range(a + 1, C):
            if sizes[a] and sizes[b]:
                assert sim[a, b] == sim[b, a] == max(want[a, b] / sizes[a], want[b, a] / sizes[b])


# ---------------------------------------------------------------------------------------------------- ray / box pass
def _ray_case(W, H, N, seed):
    rs = np.random.RandomState(seed)
    F = 3
    depth = rs.randint(800, 4000, (F, H, W)).astype(np.uint16)
    depth[:, ::10, ::10][rs.rand(F, H // 10, W // 10) < 0.15] = 0            # zero-depth rays
    twc = np.tile(np.eye(4), (F, 1, 1))
    for f in range(F):
        q, _ = np.linalg.qr(rs.randn(3, 3))
        twc[f, :3, :3] = q * np.sign(np.linalg.det(q))
        twc[f, :3, 3] = rs.uniform(-0.5, 0.5, 3)
    lo = rs.uniform(-3, 3, (N, 3))
    boxes = np.concatenate([lo, lo + rs.uniform(0.2, 2.5, (N, 3))], axis=1)
    boxes[0] = [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]                             # contains every camera
    if N > 2:
        z = twc[0, :3, 2]                                                    # behind camera 0, and far off every view
        boxes[1] = np.concatenate([twc[0, :3, 3] - 3.0 * z - 0.3, twc[0, :3, 3] - 3.0 * z + 0.3])
        boxes[2] = [50.0, 50.0, 50.0, 50.1, 50.1, 50.1]
    return depth, twc, boxes, (W * 0.9, W * 0.85, W / 2 - 0.5, H / 2 - 0.5)


@pytest.mark.parametrize("W,H,N", [(40, 30, 1), (40, 30, 17), (120, 70, 70), (120, 70, 17)])
def test_ray_boxes_equal_the_restatement(dev, W, H, N):
    depth, twc, boxes, intr = _ray_case(W, H, N, 100 + N + W)
    want, edge = U.ray_boxes(depth, twc, boxes, *intr)
    got = MG.mask_boxes_2d(depth, twc, boxes, intr, dev).cpu().numpy()
    ok = ~edge
    print("excluded", int(edge.sum()), "of", edge.size, "hit boxes", int((want[..., 2] > 0).sum()))
    assert edge.mean() <= 0.02
    assert got.dtype == np.int32 and got.shape == want.shape
    assert np.array_equal(got[ok], want[ok])
    assert (want[:, 0, 2] > 0).all()                                         # the box around the cameras is hit
    if N > 2:
        assert (want[0, 1] == 0).all()                                       # behind the camera: no ray hits
        assert (want[..., 2] > 0).mean() > 0.2 and ((want[..., 2] - want[..., 0]) > 1).any()


def test_ray_boxes_refuse_sizes_not_multiple_of_ten(dev):
    d = torch.zeros(1, 35, 40, dtype=torch.int16, device=dev)
    with pytest.raises(ops.ObjnerfError, match="-22 EINVAL"):
        ops.mask_ray_boxes(d, torch.eye(4, dtype=torch.float64, device=dev)[None], torch.zeros(1, 6, dtype=torch.float64, device=dev),
                           30.0, 30.0, 20.0, 17.0)


# --------------------------------------------------------------------------------- back-projection, histograms, boxes
def _frame_case():
    """40 x 30, four masks: A = a 14 x 12 component (a slanted plane with three outliers 1 m behind it) and a 5 x 5 one
    (under 100 pixels); B = a 15 x 14 patch whose first rows have zero depth; C = entirely on zero depth; D = a lone
    6 x 6 patch (no component of 100 pixels: fewer than 10 points kept)."""
    rs = np.random.RandomState(11)
    H, W = 30, 40
    yy, xx = np.mgrid[0:H, 0:W]
    depth = (1000 + 3 * xx + 2 * yy + rs.randint(0, 3, (H, W))).astype(np.uint16)
    depth[3, 4] = depth[8, 9] = depth[10, 5] = 2100
    depth[0:16, 20:36][0:3] = 0
    depth[24:30, 0:12] = 0
    depth[20, 30] = 65000                                   # past max_depth: zeroed
    bgr = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    A = np.zeros((H, W), bool); A[2:14, 2:16] = True; A[17:22, 14:19] = True
    B = np.zeros((H, W), bool); B[0:14, 20:35] = True
    C = np.zeros((H, W), bool); C[25:29, 1:10] = True
    D = np.zeros((H, W), bool); D[17:23, 28:34] = True
    q, _ = np.linalg.qr(rs.randn(3, 3))
    pose = np.eye(4)
    pose[:3, :3] = q * np.sign(np.linalg.det(q))
    pose[:3, 3] = [0.3, -1.2, 0.7]
    return [A, B, C, D], depth, bgr, pose, 1000.0, (150.0, 145.0, 19.5, 14.5)


@pytest.mark.parametrize("if_filter", [True, False])
def test_frame_masks_points_histograms_boxes(dev, if_filter):
    masks, depth, bgr, pose, scale, intr = _frame_case()
    want = U.project_masks(masks, depth, bgr, pose, scale, intr, if_filter)
    got = MG.project_masks(masks, depth, bgr, pose, scale, intr, dev, if_filter)
    assert want[4].tolist() == [True, True, False, False] and np.array_equal(got[4], want[4])
    assert len(got[0]) == 2
    for k in range(2):
        print("mask", k, "points", len(want[0][k]), "of", int((masks[k] & (depth > 0)).sum()))
        assert np.array_equal(got[0][k], want[0][k])                      # points bit-equal, in order
        assert np.array_equal(got[1][k], want[1][k])                      # boxes bit-equal
        assert got[2][k].dtype == np.float32 and np.array_equal(got[2][k], want[2][k])
        assert got[2][k].sum() == 3 * (masks[k] & (depth > 0)).sum()      # the mask before filtering
        assert np.array_equal(got[3][k], want[3][k])
    if if_filter:
        assert len(want[0][0]) == 14 * 12 - 3 and not want[3][0][17:22, 14:19].any() and not want[3][0][3, 4]
    else:
        assert 10 <= len(want[0][0]) < 14 * 12 and want[3][0][17:22, 14:19].all()


# ------------------------------------------------------------------------------------------------------------ affinity
def _affinity_case(N, dc, dl, F, seed):
    rs = np.random.RandomState(seed)
    K = max(1, N // 4)
    obj = rs.randint(0, K, N)

    def feats(D, noise):
        c = rs.randn(K, D)
        x = c[obj] + noise * rs.randn(N, D)
        return x.astype(np.float32)

    cap, clip = feats(dc, 0.25), feats(dl, 0.25)
    color = np.abs(feats(96, 0.3) * 40).round().astype(np.float32)
    centre = rs.uniform(-2, 2, (K, 3))[obj] + 0.05 * rs.randn(N, 3)
    half = rs.uniform(0.1, 0.4, (N, 3))
    boxes = np.concatenate([centre - half, centre + half], axis=1)
    if N > 2:
        cap[1] = 0.0                                         # a zero-norm feature row: NaN, no edge
        boxes[2, 3] = boxes[2, 0]                            # a zero-volume box
    lo = rs.randint(0, 8, (F, N, 2)) + 3 * (obj % 3)[None, :, None]
    b2 = np.concatenate([lo, lo + rs.randint(0, 6, (F, N, 2))], axis=2).astype(np.int32)
    b2[rs.rand(F, N) < 0.2] = 0                              # no ray hit the mask in that frame
    return boxes, cap, clip, color, b2


def _affinity_fp64(boxes, cap, clip, color, b2, w):
    geo, tcap, tclip = U.geo_matrix(boxes), U.cosine_matrix(cap), U.cosine_matrix(clip)
    tcol, g2 = U.cosine_matrix(color), U.geo2d_mean(b2)
    W = w[0] * geo + w[1] * tcap + w[2] * tclip + w[3] * tcol
    if w[4] != 0:
        W = W + w[4] * g2.astype(np.float64)
    return (geo, tcap, tclip, tcol, g2), W


@pytest.mark.parametrize("N,dc,dl,F", [(1, 96, 384, 1), (15, 384, 512, 2), (16, 98, 96, 7), (17, 512, 384, 2),
                                        (130, 384, 512, 7), (1030, 8, 8, 1)])
def test_affinity_terms_sum_and_edges(dev, N, dc, dl, F):
    """(N = 1030: more rows than 1024, a tile of one element a thread of the one-workgroup scan of the rows' edge
    counts; test_edges_row_offsets_carry_across_scan_tiles passes objnerf_wg.h's tile of 4096.)"""
    boxes, cap, clip, color, b2 = _affinity_case(N, dc, dl, F, 40 + N)
    w = (0.35, 0.3, 0.3, 0.15, 0.2)
    (geo, tcap, tclip, tcol, g2), W64 = _affinity_fp64(boxes, cap, clip, color, b2, w)
    t = lambda a: torch.from_numpy(a).to(dev)
    W, ij, ew, terms = ops.mask_affinity(t(boxes), t(cap), t(clip), t(color), t(b2), w, want_terms=True)
    W, ij, ew, terms = W.cpu().numpy(), ij.cpu().numpy(), ew.cpu().numpy(), terms.cpu().numpy()
    # the 2-D term: the fp32 recurrence, bit for bit; alone (other weights 0) it is W wherever the features are finite
    assert np.array_equal(terms[4], g2)
    W2 = ops.mask_affinity(t(boxes), t(cap), t(clip), t(color), t(b2), (0.0, 0.0, 0.0, 0.0, 1.0))[0].cpu().numpy()
    fin = np.isfinite(tcap) & np.isfinite(tclip) & np.isfinite(tcol)
    assert np.array_equal(W2[fin], g2[fin]) and np.isnan(W2[~fin]).all()
    # cosine terms: 1e-5 x scale of fp64, scale = max(1, max |term|) = 1 (tests/test_query_gpu.py's bound)
    for k, want in ((1, tcap), (2, tclip), (3, tcol)):
        assert np.array_equal(np.isnan(terms[k]), np.isnan(want))
        err = np.nanmax(np.abs(terms[k] - want), initial=0.0)
        print("term", k, "max error", err)
        assert err <= 1e-5
    assert np.abs(terms[0] - geo).max() <= 1e-7              # fp64 arithmetic, rounded once to fp32 (values <= 1)
    if N > 2:
        assert np.isnan(terms[1][1]).all() and (geo[2] == 0).all()
    # W: the weighted sum of the cosine terms' bounds
    bound = 1e-5 * (w[1] + w[2] + w[3])
    assert np.array_equal(np.isnan(W), np.isnan(W64))
    print("W max error", np.nanmax(np.abs(W - W64), initial=0.0), "bound", bound)
    assert np.nanmax(np.abs(W - W64), initial=0.0) <= bound
    # edges: all i < j with W >= 1 in row-major order; pairs within the bound of 1.0 are left out of the comparison
    iu, ju = np.triu_indices(N, 1)
    near = np.abs(W64[iu, ju] - 1.0) <= bound
    assert near.mean() <= 0.01 if N > 1 else True
    want_e = {(a, b) for a, b, nr, v in zip(iu, ju, near, W64[iu, ju]) if not nr and v >= 1.0}
    got_e = [(int(a), int(b)) for a, b in ij]
    assert got_e == sorted(got_e) and all(a < b for a, b in got_e)
    assert np.array_equal(ew, W[ij[:, 0], ij[:, 1]]) if len(ij) else True
    with np.errstate(invalid="ignore"):                      # against the returned W itself: bit for bit, in order
        e_w = np.argwhere(np.triu(W >= 1.0, 1))
    assert np.array_equal(ij, e_w) and np.array_equal(ew, W[e_w[:, 0], e_w[:, 1]])
    skip = {(a, b) for a, b, nr in zip(iu, ju, near) if nr}
    assert set(got_e) - skip == want_e
    print("edges", len(got_e), "of", len(iu), "pairs; left out", int(near.sum()))
    if N >= 15:
        assert 0 < len(want_e) < len(iu)
    # the 2-D weight 0 skips the term: no 2-D boxes needed
    W0 = ops.mask_affinity(t(boxes), t(cap), t(clip), t(color), None, w[:4] + (0.0,))[0].cpu().numpy()
    W064 = _affinity_fp64(boxes, cap, clip, color, b2, w[:4] + (0.0,))[1]
    assert np.nanmax(np.abs(W0 - W064), initial=0.0) <= bound
    again = ops.mask_affinity(t(boxes), t(cap), t(clip), t(color), t(b2), w)
    assert np.array_equal(again[0].cpu().numpy(), W, equal_nan=True) and np.array_equal(again[1].cpu().numpy(), ij)


def test_edges_row_offsets_carry_across_scan_tiles(dev):
    """N = 4100 masks: more rows than the 4096 elements of a tile of the one-workgroup scan of the rows' edge counts
    (objnerf_wg.h: 1024 threads x 4), with edges on both sides of the boundary.  The edges and their order are those of
    the returned W itself, bit for bit: np.argwhere(np.triu(W >= 1, 1)) is row-major."""
    N = 4100
    boxes, cap, clip, color, b2 = _affinity_case(N, 8, 8, 1, 40 + N)
    cap[4097], clip[4097], color[4097], boxes[4097] = cap[4099], clip[4099], color[4099], boxes[4099]   # one object
    t = lambda a: torch.from_numpy(a).to(dev)
    W, ij, ew, _ = ops.mask_affinity(t(boxes), t(cap), t(clip), t(color), t(b2), (0.35, 0.3, 0.3, 0.15, 0.2))
    W, ij, ew = W.cpu().numpy(), ij.cpu().numpy(), ew.cpu().numpy()
    with np.errstate(invalid="ignore"):
        e_w = np.argwhere(np.triu(W >= 1.0, 1))
    assert (e_w[:, 0] < 4096).any() and (e_w[:, 0] >= 4096).any()
    assert np.array_equal(ij, e_w) and np.array_equal(ew, W[e_w[:, 0], e_w[:, 1]])


# ---------------------------------------------------------------------------------------------------------- end to end
E2E_W, E2E_H, E2E_F = 160, 120, 12
E2E_INTR = (140.0, 140.0, 79.5, 59.5)
# axis-aligned boxes (min, max): a wall, the floor and three objects standing on it
E2E_BOXES = {1: ([-3.0, 2.0, 0.0], [3.0, 2.2, 2.5]), 2: ([-3.0, -3.0, -0.2], [3.0, 2.0, 0.0]),
             10: ([-0.9, 0.2, 0.0], [-0.4, 0.7, 0.5]), 11: ([-0.1, 0.6, 0.0], [0.4, 1.1, 0.7]),
             12: ([0.7, 0.0, 0.0], [1.2, 0.5, 0.4])}


def _render(pose):
    """Ray-cast the boxes: per pixel the nearest hit's key and its camera depth in millimetres."""
    fx, fy, cx, cy = E2E_INTR
    v, u = np.mgrid[0:E2E_H, 0:E2E_W]
    d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u, float)], -1) @ pose[:3, :3].T
    o = pose[:3, 3]
    best = np.full((E2E_H, E2E_W), np.inf)
    key = np.zeros((E2E_H, E2E_W), np.int32)
    with np.errstate(all="ignore"):
        for k, (lo, hi) in E2E_BOXES.items():
            t1, t2 = (np.asarray(lo) - o) / d, (np.asarray(hi) - o) / d
            near, far = np.minimum(t1, t2).max(-1), np.maximum(t1, t2).min(-1)
            hit = (near <= far) & (near > 0.05) & (near < best)
            best[hit], key[hit] = near[hit], k
    depth = np.where(np.isfinite(best), np.clip(np.rint(best * 1000.0), 0, 65535), 0).astype(np.uint16)
    return key, depth


def _look_at(eye, target):
    z = np.asarray(target, float) - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, [0.0, 0.0, 1.0]); x /= np.linalg.norm(x)
    y = np.cross(z, x)
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = x, y, z, eye
    return pose


def _write_e2e_inputs(root):
    from PIL import Image
    import pickle
    import yaml
    rs = np.random.RandomState(21)
    unit = lambda a: a / np.linalg.norm(a, axis=-1, keepdims=True)
    capc = {k: c for k, c in zip(E2E_BOXES, unit(rs.randn(5, 32)))}
    clipc = {k: c for k, c in zip(E2E_BOXES, unit(rs.randn(5, 24)))}
    rgbc = {1: (200, 200, 190), 2: (90, 70, 50), 10: (200, 30, 30), 11: (30, 180, 40), 12: (40, 50, 210)}
    for sub in ("depth", "rgb"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    masks, caps, capft, clipft, traj, keys_per_frame = [], [], [], [], [], []
    for f in range(E2E_F):
        a = -0.9 + 1.8 * f / (E2E_F - 1)
        pose = _look_at(np.array([2.6 * np.sin(a), 0.6 - 2.6 * np.cos(a), 1.3]), [0.1, 0.6, 0.3])
        key, depth = _render(pose)
        rgb = np.zeros((E2E_H, E2E_W, 3), np.uint8)
        m_f, c_f, cf_f, cl_f, k_f = [], [], [], [], []
        for k in E2E_BOXES:
            m = key == k
            rgb[m] = np.clip(np.asarray(rgbc[k]) + rs.randint(-12, 13, (int(m.sum()), 3)), 0, 255)
            if m.sum() >= 150:
                m_f.append(m), c_f.append("thing %d" % k), k_f.append(k)
                cf_f.append(unit(capc[k] + 0.02 * rs.randn(32)).astype(np.float32))
                cl_f.append(unit(clipc[k] + 0.02 * rs.randn(24)).astype(np.float32)[None])
        masks.append(m_f), caps.append(c_f), capft.append(cf_f), clipft.append(cl_f), keys_per_frame.append(k_f)
        for sub10 in range(10):                                   # the loader's stride: frames 10 f .. 10 f + 9
            i = 10 * f + sub10
            Image.fromarray(rgb).save(os.path.join(root, "rgb", "rgb_%d.png" % i))
            Image.fromarray(depth).save(os.path.join(root, "depth", "depth_%d.png" % i))
            traj.append(pose.reshape(-1))
    np.savetxt(os.path.join(root, "traj_w_c.txt"), np.stack(traj), delimiter=" ")
    with open(os.path.join(root, "mask_init_all.pkl"), "wb") as fh:
        pickle.dump({"mask": masks, "caption": caps, "capfeat": capft, "clipfeat": clipft}, fh)
    np.savez(os.path.join(root, "bg.npz"), wall=capc[1][None], floor=capc[2][None], ceiling=unit(rs.randn(1, 32)))
    cfg = dict(graph_method="weighted", weight_geo=0.4, weight_cap=0.4, weight_clip=0.3, weight_color=0.2,
               weight_geo_2d=0.1, if_filter=1, if_bg=0, cap_thre=0.8, dis_thre=0.02, weight_pc=0.7, weightcaption=0.7,
               weightcolor=0.7, depth_scale=1000.0, skip=10, use_num=-1, start=0, x_the=0, y_the=0, z_the=0,
               fx=E2E_INTR[0], fy=E2E_INTR[1], cx=E2E_INTR[2], cy=E2E_INTR[3], image_W=E2E_W, image_H=E2E_H, seed=0)
    with open(os.path.join(root, "cfg.yaml"), "w") as fh:
        yaml.safe_dump(cfg, fh)
    return masks, keys_per_frame


def test_end_to_end_cli_ids_dataset_and_determinism(dev, tmp_path):
    """Five boxes (a wall, the floor, three objects) seen from 12 poses, 4 to 5 masks a frame with one noisy feature per
    object, through the command line: one id per object, the wall 1, the floor 2, the written directory read by
    dataset.Replica, a second run byte for byte the same."""
    from openobj_amd import dataset as ods
    from openobj_amd import cfg as ocfg
    root = str(tmp_path / "scene")
    masks, keys = _write_e2e_inputs(root)
    assert all(4 <= len(k) <= 6 for k in keys) and {k for fr in keys for k in fr} == set(E2E_BOXES)
    argv = [os.path.join(root, "cfg.yaml"), "--input-mask", os.path.join(root, "mask_init_all.pkl"), "--dataset-dir", root,
            "--bg-feats", os.path.join(root, "bg.npz")]
    assert MG.main(argv + ["--output-dir", root]) == 0
    second = str(tmp_path / "second")
    assert MG.main(argv + ["--output-dir", second]) == 0
    names = ["object_clipfeat.pkl", "object_capfeat.pkl", "object_caption.pkl"]
    names += ["instance_our/semantic_instance_%d.png" % i for i in range(E2E_F)]
    names += ["class_our/semantic_class_%d.png" % i for i in range(E2E_F)]
    for n in names:
        assert open(os.path.join(root, n), "rb").read() == open(os.path.join(second, n), "rb").read(), n
    assert not os.path.exists(os.path.join(root, "debug"))
    ids, kept_share = {}, []
    for f in range(E2E_F):
        img = ods._read_image(os.path.join(root, "instance_our", "semantic_instance_%d.png" % f))
        for m, k in zip(masks[f], keys[f]):
            got = np.unique(img[m])
            got = got[got != 0]                                    # (pixels the per-mask DBSCAN dropped stay 0)
            assert got.size == 1, (f, k, got)
            ids.setdefault(k, set()).add(int(got[0]))
            kept_share.append(float((img[m] != 0).mean()))         # (a mask keeps its largest DBSCAN cluster only)
    print("ids", ids, "smallest kept share of a mask", min(kept_share))
    assert all(len(v) == 1 for v in ids.values())                  # every mask of an object ends with one id
    assert ids[1] == {1} and ids[2] == {2}
    obj_ids = [next(iter(ids[k])) for k in (10, 11, 12)]
    assert len(set(obj_ids)) == 3 and min(obj_ids) >= 4
    c = ocfg.Config(ocfg.replica_room0_config(train_device="cpu", **{
        "dataset.path": root, "dataset.format": "Replica", "trainer.part_mode": 0, "camera.w": E2E_W, "camera.h": E2E_H,
        "camera.fx": E2E_INTR[0], "camera.fy": E2E_INTR[1], "camera.cx": E2E_INTR[2], "camera.cy": E2E_INTR[3]}))
    ds = ods.Replica(c)
    assert len(ds) == E2E_F
    seen = set()
    for f in (0, 5, 11):
        s = ds[f]
        img = ods._read_image(os.path.join(root, "instance_our", "semantic_instance_%d.png" % f))
        obj = np.asarray(s["obj"]).T
        for k in keys[f]:
            new = next(iter(ids[k]))
            if new == 1:
                assert np.array_equal(obj == 0, img == 1) and 0 in s["obj_clip"]
                continue
            rows, cols = np.nonzero(img == new)                    # dataset.py keeps an object wider and higher than 10 px
            kept = np.ptp(rows) + 1 > 10 and np.ptp(cols) + 1 > 10
            assert (new in s["bbox_dict"]) == kept, (f, k, new)
            if kept:
                seen.add(k)
                assert np.array_equal(obj == new, img == new) and new in s["obj_cap"] and new in s["obj_clip"]
            else:
                assert not (obj == new).any()
    assert {10, 11, 12} <= seen                                    # every object is read back in some sampled frame


# ------------------------------------------------------------------------------------- the comparisons' edges, exactly
def test_dbscan_pair_at_exactly_eps_and_border_between_two_clusters(dev):
    """Exactly representable inputs: a line of points 0.5 apart at eps = 0.5 (d^2 = 0.25 = eps^2: the pair counts, so
    at min_points 3 the inner points are core and the line is one cluster), and a border point within eps of two
    clusters, which takes the lower id."""
    line = np.arange(9)[:, None] * np.array([0.5, 0.0, 0.0])
    want = U.dbscan_labels(line, 0.5, 3)
    assert (want == 0).all()
    got = ops.dbscan(torch.from_numpy(line).to(dev), [0, 9], 0.5, 3).cpu().numpy()
    assert np.array_equal(got, want)
    far = [[-0.02, 0.0, 0.0], [-0.02, 0.01, 0.0], [-0.02, 0.0, 0.01], [-0.02, 0.01, 0.01], [-0.03, 0.0, 0.0], [-0.03, 0.01, 0.0]]
    a = np.array([[0.0, 0.0, 0.0], [0.0, 0.01, 0.0]] + far)
    x = np.concatenate([a * [-1.0, 1.0, 1.0] + [0.08, 0.0, 0.0], [[0.04, 0.002, 0.002]], a])
    assert U.min_gap_to_radius(x, EPS) > 1e-9
    want = U.dbscan_labels(x, EPS, 8)
    assert want[8] == 0 and (want[:8] == 0).all() and (want[9:] == 1).all()
    assert np.array_equal(ops.dbscan(torch.from_numpy(x).to(dev), [0, len(x)], EPS, 8).cpu().numpy(), want)


def test_cloud_overlap_is_strict_at_exactly_the_threshold(dev):
    """d = 0.5 = dis_thre exactly: not counted (the reference's distances < dis_thre); d = 0.25 is."""
    clouds = [np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0]]), np.array([[0.5, 0.0, 0.0], [2.25, 0.0, 0.0]])]
    want, _ = U.overlap_counts(clouds, 0.5)
    assert want.tolist() == [[2, 1], [1, 2]]
    got = ops.cloud_overlap(torch.from_numpy(np.concatenate(clouds)).to(dev), [0, 2, 4], 0.5).cpu().numpy()
    assert np.array_equal(got, want)
