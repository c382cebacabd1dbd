"""GPU: the map-query kernels (objnerf_query.hip, ABI 10) against fp64 and the numpy restatement in
tests/query_util.py, MapQuery's colourings, the planar scene end to end and the native map size."""
import json
import os

import numpy as np
import pytest
import torch

from openobj_amd import _lib, ops, query
try:
    from tests import query_util as QU
except ImportError:          # plain `pytest tests/` puts tests/ itself, not the repository root, on sys.path
    import query_util as QU

pytestmark = pytest.mark.gpu


def _feat(dev, V, D, stride, rs, mean=0.0):
    """[V, D] fp32 device view with row stride `stride` (>= D)."""
    buf = (rs.randn(V, stride) * 0.3 + mean).astype(np.float32)
    return torch.from_numpy(buf).to(dev)[:, :D]


def _segs(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


CASES = [  # (segment sizes, D, Q, row stride, per-segment weights)
    ((1000, 0, 1, 4097, 256), 512, 16, 512, False),
    ((300, 33, 0, 1500), 40, 3, 40, True),
    ((1,), 512, 1, 520, False),
    ((517, 2), 40, 16, 43, False),                   # an unaligned stride: the scalar load path
    ((70, 900), 1024, 5, 1024, True),
    ((255, 257), 7, 2, 9, False),
]


@pytest.mark.parametrize("sizes,D,Q,stride,per", CASES)
@pytest.mark.parametrize("cosine", [True, False])
def test_projection_matches_fp64(dev, sizes, D, Q, stride, per, cosine):
    rs = np.random.RandomState(D + Q + len(sizes))
    off = _segs(sizes)
    V, S = int(off[-1]), len(sizes)
    f = _feat(dev, V, D, stride, rs, mean=0.2)
    W = rs.randn(*((S, D, Q) if per else (D, Q))).astype(np.float32)
    b = None if cosine else rs.randn(*((S, Q) if per else (Q,))).astype(np.float32)
    out, mm = ops.segment_project(f, off, torch.from_numpy(W), None if b is None else torch.from_numpy(b), cosine=cosine)
    out2, mm2 = ops.segment_project(f, off, torch.from_numpy(W), None if b is None else torch.from_numpy(b),
                                    cosine=cosine)
    assert out.cpu().numpy().tobytes() == out2.cpu().numpy().tobytes()
    assert mm.cpu().numpy().tobytes() == mm2.cpu().numpy().tobytes()
    F = f.cpu().numpy().astype(np.float64)
    got, gmm = out.cpu().numpy(), mm.cpu().numpy()
    for s in range(S):
        r0, r1 = off[s], off[s + 1]
        Ws = (W[s] if per else W).astype(np.float64)
        if cosine:
            want = (F[r0:r1] / np.maximum(np.linalg.norm(F[r0:r1], axis=1, keepdims=True), 1e-8)) @ \
                   (Ws / np.maximum(np.linalg.norm(Ws, axis=0, keepdims=True), 1e-8))
            assert np.abs(got[r0:r1] - want).max(initial=0) <= 2e-6
        else:
            want = F[r0:r1] @ Ws + (b[s] if per else b)
            scale = np.abs(want).max(initial=1.0)
            assert np.abs(got[r0:r1] - want).max(initial=0) <= 1e-5 * scale
        if r1 > r0:                                   # the kernel's own output's min / max, exactly
            assert np.array_equal(gmm[s, :, 0], got[r0:r1].min(axis=0))
            assert np.array_equal(gmm[s, :, 1], got[r0:r1].max(axis=0))
        else:
            assert np.all(gmm[s, :, 0] == np.inf) and np.all(gmm[s, :, 1] == -np.inf)


@pytest.mark.parametrize("sizes,D,stride", [((3000, 0, 1, 700), 512, 512), ((129, 40), 40, 44), ((5, 2000), 40, 41),
                                            ((400,), 1000, 1003)])
def test_moments_match_fp64(dev, sizes, D, stride):
    rs = np.random.RandomState(len(sizes) + D)
    off = _segs(sizes)
    f = _feat(dev, int(off[-1]), D, stride, rs, mean=0.6)   # a large common mean, as unit part features have
    mean, sc = ops.segment_moments(f, off)
    mean2, sc2 = ops.segment_moments(f, off)
    assert mean.cpu().numpy().tobytes() == mean2.cpu().numpy().tobytes()
    assert sc.cpu().numpy().tobytes() == sc2.cpu().numpy().tobytes()
    F = f.cpu().numpy().astype(np.float64)
    gm, gs = mean.cpu().numpy(), sc.cpu().numpy()
    for s in range(len(sizes)):
        X = F[off[s]:off[s + 1]]
        if len(X) == 0:
            assert not gm[s].any() and not gs[s].any()
            continue
        m = X.mean(axis=0)
        C = (X - m).T @ (X - m)
        assert np.abs(gm[s] - m).max() <= 1e-5 * np.abs(m).max()
        assert np.abs(gs[s] - C).max() <= 1e-5 * max(np.abs(C).max(), 1e-30)
        assert np.array_equal(gs[s], gs[s].T)


def test_colors_equal_the_restatement_bit_for_bit(dev):
    rs = np.random.RandomState(7)
    sizes = [600, 256, 9, 0, 40, 1, 33]
    off = _segs(sizes)
    V, S, Q = int(off[-1]), len(sizes), 4
    proj = rs.randn(V, Q).astype(np.float32)
    proj[off[1]:off[1] + 256, 1] = (np.arange(256) + 0.5) / 256            # every table entry
    proj[off[1], 1], proj[off[1] + 1, 1] = 0.0, 1.0
    proj[off[2]:off[3], 2] = 0.25                                          # a constant segment: NaN -> (0, 0, 0)
    mm = np.stack([np.stack([proj[off[s]:off[s + 1]].min(axis=0), proj[off[s]:off[s + 1]].max(axis=0)], -1)
                   if sizes[s] else np.tile([np.inf, -np.inf], (Q, 1)) for s in range(S)]).astype(np.float32)
    rgb = rs.randint(0, 256, (V, 4)).astype(np.uint8)
    modes = [_lib.COLOR_RAINBOW, _lib.COLOR_RAINBOW, _lib.COLOR_RAINBOW, _lib.COLOR_RGB, _lib.COLOR_RGB,
             _lib.COLOR_CONSTANT, _lib.COLOR_PCA]
    column = [0, 1, 2, 0, 0, 0, 0]
    factor = [0, 0, 0, 0.5, 0.8, 0, 0]
    const = np.zeros((S, 3), np.float32)
    const[5] = (1.0, 0.0, 0.0)
    args = dict(rgb=torch.from_numpy(rgb).to(dev), factor=factor, constant=const, column=column,
                proj=torch.from_numpy(proj).to(dev), minmax=torch.from_numpy(mm).to(dev))
    got = ops.vertex_colors(off, modes, V, **args).cpu().numpy()
    again = ops.vertex_colors(off, modes, V, **args).cpu().numpy()
    assert got.tobytes() == again.tobytes()
    for s in range(S):
        r0, r1 = off[s], off[s + 1]
        if modes[s] == _lib.COLOR_RAINBOW:
            c = column[s]
            want = QU.rainbow(QU.normalise(proj[r0:r1, c], mm[s, c, 0], mm[s, c, 1]))
        elif modes[s] == _lib.COLOR_RGB:
            want = QU.rgb_colors(rgb[r0:r1], factor[s])
        elif modes[s] == _lib.COLOR_CONSTANT:
            want = np.tile(const[s], (r1 - r0, 1))
        else:
            sc = QU.sign_rule(proj[r0:r1, :3].astype(np.float64))
            want = QU.pca_colors(sc)
            assert np.abs(got[r0:r1] - want).max() <= 1e-6
            continue
        assert got[r0:r1].tobytes() == want.astype(np.float32).tobytes(), s
    assert not got[off[2]:off[3]].any()
    assert len({tuple(x) for x in got[off[1]:off[1] + 256]}) > 200


def _planted(rs, n, D, gap=True):
    """Unit rows around a common mean with a planted spectrum: three strong directions, then a gap."""
    Q, _ = np.linalg.qr(rs.randn(D, D))
    sd = np.concatenate([[3.0, 2.0, 1.5], np.full(D - 3, 0.3)]) * 0.05
    X = rs.randn(n, D) * sd @ Q.T + rs.randn(D)
    return (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)


def _pca_map(rs, sizes, D):
    from openobj_amd.mesh import TriMesh
    out = {}
    for i, n in enumerate(sizes):
        m = TriMesh(rs.rand(n, 3), np.zeros((0, 3), np.int64))
        m.visual.vertex_colors = rs.randint(0, 256, (n, 4)).astype(np.uint8)
        out[i] = {"clip_feat": None, "caption_feat": None, "class_id": 0, "mesh": m, "color": m.visual.vertex_colors,
                  "part_feat": _planted(rs, n, D)}
    return out


def test_pca_colors_match_the_restatement(dev):
    rs = np.random.RandomState(11)
    all_obj = _pca_map(rs, [5000, 800, 2000], 512)
    mq = query.MapQuery(all_obj, dev)
    stats = {}
    cols = mq.color_by_partfeat(stats=stats)
    assert stats["eigh_s"] > 0
    for c, o in zip(mq.split(cols), all_obj.values()):
        X = o["part_feat"].astype(np.float64)
        Z = (X - X.mean(0)) / X.std(0)
        ev = np.linalg.eigvalsh(Z.T @ Z / len(X))[::-1]
        assert ev[2] - ev[3] >= 1e-3 * ev[0]
        want = QU.pca_colors(QU.pca_scores(X))
        assert np.abs(c.cpu().numpy() - want).max() <= 1e-4
    assert mq.color_by_partfeat().cpu().numpy().tobytes() == cols.cpu().numpy().tobytes()


def _check_queries(mq, all_obj, rs, Dc, Ds, D):
    colors = [np.asarray(o["color"]) for o in all_obj.values()]
    _, clip, cap = query.reduce_object_features(all_obj)
    cq, sq, pq = rs.randn(Dc), rs.randn(Ds), rs.randn(D)
    sim = mq.object_similarity(cq, sq)
    simn = sim.cpu().numpy()
    want_sim = QU.object_similarity(cq, sq, clip, cap)
    assert np.abs(simn - want_sim).max() <= 2e-6
    for top in (0, 1, 2):
        got = mq.split(mq.color_by_object_query(cq, sq, top))
        want = QU.object_query_colors(simn, mq.ranked, colors, top)
        for g, w in zip(got, want):
            assert g.cpu().numpy().tobytes() == w.astype(np.float32).tobytes()
    assert [k for k, _ in mq.last_ranking] == [mq.keys[mq.ranked[i]] for i in QU.top_indices(simn, len(simn))]
    for top in (1, 2):
        got = mq.split(mq.color_by_part_query(cq, sq, pq, top))
        tops = [mq.ranked[i] for i in QU.top_indices(simn, top)]
        ps, _ = mq.part_similarity(pq[None] / np.linalg.norm(pq), objects=tops)
        ps = ps[:, 0].cpu().numpy()
        part = {p: ps[mq.seg_host[p]:mq.seg_host[p + 1]] for p in tops}
        for p in tops:                                        # the kernel's similarities against fp64
            X = np.asarray(list(all_obj.values())[p]["part_feat"], np.float64)
            assert np.abs(part[p] - QU.cosine(pq, X)).max() <= 2e-6
        want = QU.part_query_colors(part, tops, colors)
        for g, w in zip(got, want):
            assert g.cpu().numpy().tobytes() == w.astype(np.float32).tobytes()
    full, mm = mq.part_similarity(np.stack([pq, rs.randn(D), rs.randn(D)]))
    assert full.shape == (mq.V, 3) and mm.shape == (mq.S, 3, 2)
    rgb = mq.split(mq.color_by_rgb())
    for g, c in zip(rgb, colors):
        assert g.cpu().numpy().tobytes() == QU.rgb_colors(c, 0.8).astype(np.float32).tobytes()
    inst = mq.split(mq.color_by_instance())
    pal = QU.instance_palette(mq.S)
    for g, c in zip(inst, pal):
        assert np.array_equal(g.cpu().numpy(), np.tile(c.astype(np.float32), (len(g), 1)))


def test_map_queries_match_the_restatement(dev):
    all_obj = QU.synthetic_map(0)
    mq = query.MapQuery(all_obj, dev)
    assert mq.ranked == [0, 1, 3, 4] and mq.V == sum(len(o["part_feat"]) for o in all_obj.values())
    _check_queries(mq, all_obj, np.random.RandomState(1), 512, 384, 512)
    # an object without features is never a top object and stays darkened RGB
    rs = np.random.RandomState(2)
    cols = mq.split(mq.color_by_object_query(rs.randn(512), rs.randn(384), 9))
    assert cols[2].cpu().numpy().tobytes() == QU.rgb_colors(all_obj[16]["color"], 0.5).astype(np.float32).tobytes()
    mapping = {i: i % 5 for i in range(100)}
    mapped = {i: [i / 5, 0.5, 1 - i / 5] for i in range(5)}
    got = mq.split(mq.color_by_class(mapping, mapped))
    for g, c in zip(got, QU.class_colors(all_obj, mapping, mapped)):
        assert np.array_equal(g.cpu().numpy(), np.tile(c.astype(np.float32), (len(g), 1)))


def test_planar_scene_to_queries_end_to_end(dev, tmp_path):
    """The planar helper scene through mapping, compute_bounds and map_vis.export into MapQuery and the CLI."""
    from openobj_amd import dataset as ods
    from openobj_amd import map_query, map_vis, mapping
    from openobj_amd import mesh as omesh
    try:
        from tests import scene_files as SF
        from tests.test_bounds_gpu import _cfg
    except ImportError:
        import scene_files as SF
        from test_bounds_gpu import _cfg
    root = tmp_path / "scene"
    SF.write_scene(str(root), "Replica", n_frames=50)
    c = _cfg(dev, root, **{"render.iters_per_frame": 80})
    torch.manual_seed(5)
    m = mapping.IncrementalMapper(c)
    m.run(ods.init_loader(c, multi_worker=False))
    m.compute_bounds()
    log = tmp_path / "log"
    m.save_checkpoints(str(log), need_bound=True)
    all_obj = map_vis.export(str(log), grid_dim=64, device=str(dev))
    assert len(all_obj) >= 2
    mq = query.MapQuery(all_obj, dev)
    D = mq.D
    Dc = next(np.shape(o["clip_feat"])[-1] for o in all_obj.values() if o["clip_feat"] is not None)
    Ds = next(np.shape(o["caption_feat"])[-1] for o in all_obj.values() if o["caption_feat"] is not None)
    rs = np.random.RandomState(3)
    _check_queries(mq, all_obj, rs, Dc, Ds, D)
    for o, cc in zip(all_obj.values(), mq.split(mq.color_by_partfeat())):
        X = np.asarray(o["part_feat"], np.float64)
        if len(X) > 3:
            assert np.abs(cc.cpu().numpy() - QU.pca_colors(QU.pca_scores(X))).max() <= 1e-3
    np.save(str(tmp_path / "c.npy"), rs.randn(Dc).astype(np.float32))
    np.save(str(tmp_path / "s.npy"), rs.randn(Ds).astype(np.float32))
    np.save(str(tmp_path / "p.npy"), rs.randn(D).astype(np.float32))
    out = tmp_path / "q"
    doc = map_query.main(["--logdir", str(log), "--mode", "part", "--clip-query", str(tmp_path / "c.npy"),
                          "--sbert-query", str(tmp_path / "s.npy"), "--part-query", str(tmp_path / "p.npy"), "--top", "1",
                          "--out", str(out), "--device", str(dev)])
    assert sorted(doc["visible"]) == sorted(int(k) for k in all_obj)
    saved = json.load(open(out / "query.json"))
    assert saved == doc and len(doc["top"]) == 1 and len(doc["ranking"]) == len(mq.ranked)
    for k in all_obj:
        v, _, rgba, f = omesh.read_ply(str(out / f"obj_{k}.ply"))
        assert len(v) == len(all_obj[k]["mesh"].vertices) and rgba is not None
    for mode in ("rgb", "instance", "partpca"):
        d = map_query.main(["--logdir", str(log), "--mode", mode, "--out", str(tmp_path / mode), "--device", str(dev)])
        assert all(os.path.exists(tmp_path / mode / f"obj_{k}.ply") for k in d["visible"])


def test_native_map_size(dev):
    """51 objects x 100 k vertices x 512: the part query, the moments and the PCA projection in one call each."""
    S, n, D = 51, 100_000, 512
    g = torch.Generator(device=dev).manual_seed(0)
    f = torch.randn(S * n, D, device=dev, generator=g)
    f = f / f.norm(dim=1, keepdim=True)
    off = torch.arange(S + 1, dtype=torch.int64) * n
    q = torch.randn(D, 16, device=dev, generator=g)
    out, mm = ops.segment_project(f, off, q, cosine=True)
    mean, sc = ops.segment_moments(f, off)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and torch.isfinite(sc).all()
    k = 37
    X = f[k * n:(k + 1) * n].double()
    ref = torch.nn.functional.cosine_similarity(X, q[:, 3].double()[None], dim=-1)
    assert (out[k * n:(k + 1) * n, 3].double() - ref).abs().max().item() <= 2e-6
    m = X.mean(0)
    C = (X - m).T @ (X - m)
    assert (sc[k] - C).abs().max().item() <= 1e-5 * C.abs().max().item()
