"""GPU: the compact exported map (objnerf_partrows.hip): objnerf_part_rows / objnerf_part_expand
against fp64, the compact MapQuery against the numpy restatement in tests/query_util.py, and the planar scene exported
in both forms end to end."""
import json
import os
import random

import numpy as np
import pytest
import torch

from openobj_amd import _lib, ops, query
try:
    from tests import partcompact_util as PU
    from tests import query_util as QU
except ImportError:          # plain `pytest tests/` puts tests/ itself, not the repository root, on sys.path
    import partcompact_util as PU
    import query_util as QU

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _leave_the_process_as_found():
    """The mapper's Philox draw counter (ops._draw_offset) and the torch / numpy / random generators are process-wide:
    tests that run after this file in the same process train on the draws they would have had without it."""
    draw, py_rng = ops._draw_offset[0], random.getstate()
    cpu_rng, np_rng = torch.get_rng_state(), np.random.get_state()
    gpu_rng = torch.cuda.get_rng_state_all() if torch.cuda.is_available() else None
    yield
    ops._draw_offset[0] = draw
    random.setstate(py_rng)
    torch.set_rng_state(cpu_rng)
    np.random.set_state(np_rng)
    if gpu_rng is not None:
        torch.cuda.set_rng_state_all(gpu_rng)


GATE = 2e-6                  # the project's cosine gate (test_query_gpu.py): |A r - X|_2 bounds the cosine error
                             # against every unit query at once


def _strided(dev, a, stride):
    """[V, D] fp32 device view of a with row stride `stride` (>= D)."""
    buf = torch.zeros(a.shape[0], stride, device=dev)
    buf[:, :a.shape[1]] = torch.from_numpy(a).to(dev)
    return buf[:, :a.shape[1]]


@pytest.mark.parametrize("H,C", [(32, 512), (128, 512), (256, 512), (32, 64)])
@pytest.mark.parametrize("pad", [0, 8])
def test_part_rows_match_fp64(dev, H, C, pad):
    rs = np.random.RandomState(H + C + pad)
    W, b = PU.head(rs, H, C)
    Wd, bd = torch.from_numpy(W).to(dev), torch.from_numpy(b).to(dev)
    for V in (0, 1, 63, 64, 65, 1000):
        h = PU.hidden(rs, V, H)
        if V:
            k = PU.kappa(h, W, b).max()
            assert k <= 16, k
        hd = _strided(dev, h, H + pad)
        rows = ops.part_rows(hd, Wd, bd)
        again = ops.part_rows(hd, Wd, bd)
        assert rows.shape == (V, H + 1) and (V < 2 or rows.stride(0) == H + 4)
        got = rows.cpu().numpy()
        assert got.tobytes() == again.cpu().numpy().tobytes()
        if V == 0:
            continue
        _, A, X = PU.rows64(h, W, b)
        err = np.linalg.norm(got.astype(np.float64) @ A.T - X, axis=1).max()
        print(f"H={H} C={C} stride={H + pad} V={V}: kappa {k:.2f}, max |A r - X|_2 = {err:.3e}")
        assert err <= GATE
        base = rows.as_strided((V, H + 4), (H + 4, 1))                # the padding columns of the buffer: zeros
        assert not base[:, H + 1:].any()


def test_part_rows_zero_feature_gives_a_finite_row(dev):
    rs = np.random.RandomState(0)
    W, _ = PU.head(rs, 32, 64)
    h = PU.hidden(rs, 5, 32)
    h[2] = 0.0
    rows = ops.part_rows(torch.from_numpy(h).to(dev), torch.from_numpy(W).to(dev), torch.zeros(64, device=dev))
    got = rows.cpu().numpy()
    assert np.isfinite(got).all() and not got[2, :32].any() and got[2, 32] == np.float32(1e8)
    feat = ops.part_expand(rows, torch.from_numpy(np.concatenate([W, np.zeros((64, 1), np.float32)], 1)).to(dev))
    assert not feat[2].any() and torch.isfinite(feat).all()


@pytest.mark.parametrize("H,C", [(48, 512), (288, 512), (32, 24), (32, 1040)])
def test_part_rows_reject_unbuilt_widths(dev, H, C):
    with pytest.raises(_lib.ObjnerfError):
        ops.part_rows(torch.zeros(4, H, device=dev), torch.zeros(C, H, device=dev), torch.zeros(C, device=dev))
    with pytest.raises(_lib.ObjnerfError):
        ops.part_expand(torch.zeros(4, H + 1, device=dev), torch.zeros(C, H + 1, device=dev))


def test_part_rows_check_their_arguments(dev):
    z = lambda *s: torch.zeros(*s, device=dev)
    with pytest.raises(_lib.ObjnerfError):
        ops.part_rows(torch.zeros(4, 32), z(64, 32), z(64))            # a host tensor
    with pytest.raises(_lib.ObjnerfError):
        ops.part_rows(z(4, 32), z(64, 64), z(64))                      # the head's H
    with pytest.raises(_lib.ObjnerfError):
        ops.part_rows(z(4, 32), z(64, 32), z(63))
    with pytest.raises(_lib.ObjnerfError):
        ops.part_rows(z(4, 32).double(), z(64, 32), z(64))
    with pytest.raises(_lib.ObjnerfError):
        ops.part_rows(z(4, 32), z(64, 32), z(64), out=z(4, 33))        # not the [V, H + 4] buffer
    with pytest.raises(_lib.ObjnerfError):
        ops.part_expand(z(4, 33), z(64, 32))
    with pytest.raises(_lib.ObjnerfError):
        ops.part_expand(z(4, 33), z(64, 33), index=torch.zeros(2, dtype=torch.int32, device=dev))


@pytest.mark.parametrize("H,C,stride", [(32, 512, 36), (128, 512, 129), (256, 64, 260), (64, 512, 68)])
def test_part_expand_matches_fp64(dev, H, C, stride):
    rs = np.random.RandomState(H + C)
    W, b = PU.head(rs, H, C)
    V = 77
    r, A, _ = PU.rows64(PU.hidden(rs, V, H), W, b)
    r32, A32 = r.astype(np.float32), A.astype(np.float32)
    want = r32.astype(np.float64) @ A32.astype(np.float64).T
    rows, head = _strided(dev, r32, stride), torch.from_numpy(A32).to(dev)
    got = ops.part_expand(rows, head).cpu().numpy()
    assert got.shape == (V, C)
    assert np.linalg.norm(got - want, axis=1).max() <= GATE
    idx = np.array([5, -1, 76, V, 0, 5, 2 ** 40, -2 ** 40, 33] + list(rs.randint(0, V, 60)), np.int64)
    got = ops.part_expand(rows, head, torch.from_numpy(idx).to(dev)).cpu().numpy()
    ok = (idx >= 0) & (idx < V)
    assert not got[~ok].any()
    assert np.linalg.norm(got[ok] - want[idx[ok]], axis=1).max() <= GATE
    assert ops.part_expand(rows, head, torch.zeros(0, dtype=torch.int64, device=dev)).shape == (0, C)
    assert ops.part_expand(rows[:0], head).shape == (0, C)


# ------------------------------------------------------------------------------------------------ MapQuery
SIZES, WIDTHS = (300, 1, 0, 777, 64, 65), (128, 32, 32, 32, 128, 32)


def _check_queries(mq, all_obj, Xs, rs, Dc, Ds):
    """test_query_gpu._check_queries for a compact map: Xs are the fp64 features of its stored rows."""
    D = mq.D
    colors = [np.asarray(o["color"]) for o in all_obj.values()]
    _, clip, cap = query.reduce_object_features(all_obj)
    cq, sq, pq = rs.randn(Dc), rs.randn(Ds), rs.randn(D)
    simn = mq.object_similarity(cq, sq).cpu().numpy()
    assert np.abs(simn - QU.object_similarity(cq, sq, clip, cap)).max() <= GATE
    for top in (0, 1, 2):
        got = mq.split(mq.color_by_object_query(cq, sq, top))
        want = QU.object_query_colors(simn, mq.ranked, colors, top)
        for g, w in zip(got, want):
            assert g.cpu().numpy().tobytes() == w.astype(np.float32).tobytes()
    assert [k for k, _ in mq.last_ranking] == [mq.keys[mq.ranked[i]] for i in QU.top_indices(simn, len(simn))]
    for top in (1, 2):
        got = mq.split(mq.color_by_part_query(cq, sq, pq, top))
        tops = [mq.ranked[i] for i in QU.top_indices(simn, top)]
        ps, _ = mq.part_similarity(mq._query(pq, D, "part query")[None], objects=tops)   # the colouring's own call
        ps = ps[:, 0].cpu().numpy()
        part = {p: ps[mq.seg_host[p]:mq.seg_host[p + 1]] for p in tops}
        for p in tops:                                        # the kernel's similarities against fp64
            assert np.abs(part[p] - QU.cosine(pq, Xs[p])).max(initial=0) <= GATE
        want = QU.part_query_colors(part, tops, colors)
        for g, w in zip(got, want):
            assert g.cpu().numpy().tobytes() == w.astype(np.float32).tobytes()
    rgb = mq.split(mq.color_by_rgb())
    for g, c in zip(rgb, colors):
        assert g.cpu().numpy().tobytes() == QU.rgb_colors(c, 0.8).astype(np.float32).tobytes()
    inst = mq.split(mq.color_by_instance())
    for g, c in zip(inst, QU.instance_palette(mq.S)):
        assert np.array_equal(g.cpu().numpy(), np.tile(c.astype(np.float32), (len(g), 1)))
    mapping = {i: i % 5 for i in range(100)}
    mapped = {i: [i / 5, 0.5, 1 - i / 5] for i in range(5)}
    if all(o["class_id"] is not None for o in all_obj.values()):
        for g, c in zip(mq.split(mq.color_by_class(mapping, mapped)), QU.class_colors(all_obj, mapping, mapped)):
            assert np.array_equal(g.cpu().numpy(), np.tile(c.astype(np.float32), (len(g), 1)))


@pytest.fixture(scope="module")
def small_map():
    return PU.compact_map(0, SIZES, WIDTHS)


def test_compact_part_similarity_matches_fp64(dev, small_map):
    all_obj, Xs = small_map
    mq = query.MapQuery(all_obj, dev)
    off = mq.seg_host
    assert mq.D == 512 and mq.V == sum(SIZES) and mq.S == 6 and mq.seg_off.cpu().tolist() == off.tolist()
    assert [len(c) for c in mq.split(torch.zeros(mq.V, 3))] == list(SIZES)
    rs = np.random.RandomState(1)
    for Q in (1, 3, 16):
        q = rs.randn(Q, 512) * rs.uniform(0.1, 10, (Q, 1))                  # any length: normalised inside
        q[Q - 1] = Xs[3].mean(axis=0)                                        # a segment's mean feature
        for objects in (None, [3, 0], [5], [2]):
            sims, mm = mq.part_similarity(q.astype(np.float32), objects=objects)
            assert sims.shape == (mq.V, Q) and mm.shape == (6, Q, 2)
            s, m = sims.cpu().numpy(), mm.cpu().numpy()
            for p in range(6):
                got = s[off[p]:off[p + 1]]
                if objects is not None and p not in objects:
                    assert np.isnan(got).all() and np.isnan(m[p]).all()
                    continue
                want = np.stack([QU.cosine(q[i].astype(np.float32), Xs[p]) for i in range(Q)], 1)
                assert np.abs(got - want).max(initial=0) <= GATE
                if SIZES[p]:
                    assert np.array_equal(m[p, :, 0], got.min(axis=0)) and np.array_equal(m[p, :, 1], got.max(axis=0))
                else:
                    assert np.all(m[p, :, 0] == np.inf) and np.all(m[p, :, 1] == -np.inf)
            if objects is None:
                assert (s[off[3]:off[4], Q - 1] > 0.8).any()
                assert sims.cpu().numpy().tobytes() == mq.part_similarity(q.astype(np.float32))[0].cpu().numpy().tobytes()
    with pytest.raises(ValueError):
        mq.part_similarity(np.zeros((1, 33), np.float32))


def test_compact_colourings_equal_the_restatement(dev, small_map):
    all_obj, Xs = small_map
    mq = query.MapQuery(all_obj, dev)
    assert mq.ranked == [0, 1, 3, 4, 5]
    _check_queries(mq, all_obj, Xs, np.random.RandomState(1), 512, 384)
    cols = mq.color_by_partfeat()                                            # tiny and empty segments: finite, stable
    assert cols.shape == (mq.V, 3) and torch.isfinite(cols).all()
    assert cols.cpu().numpy().tobytes() == mq.color_by_partfeat().cpu().numpy().tobytes()


def test_compact_features_and_store_bytes(dev, small_map):
    """store_bytes of the compact map is sum(V_s (H_s + 4) 4) plus the heads.  The 1 / 12 bound against the dense store
    is asserted on a hidden-32 map whose vertices outweigh its heads (rows 36 / 512 = 0.070 of the dense bytes, a head
    the bytes of 33 dense vertices): on the six-object map above no layout with H + 4 floats a row can meet it -- its
    rows alone are 78 396 of the dense map's 617 984 floats (0.127; hidden 128 stores 132 floats a vertex), with the six
    heads 0.45."""
    all_obj, Xs = small_map
    mq = query.MapQuery(all_obj, dev)
    X = np.concatenate(Xs)
    ids = np.array([0, 299, 300, 301, 1077, 1078, 1206, mq.V, -1, 2 ** 40, 5, 5] +
                   list(np.random.RandomState(4).randint(0, mq.V, 100)), np.int64)
    got = mq.features(ids).cpu().numpy()
    ok = (ids >= 0) & (ids < mq.V)
    assert got.shape == (len(ids), 512) and not got[~ok].any()
    assert np.linalg.norm(got[ok] - X[ids[ok]], axis=1).max() <= GATE
    assert mq.features([]).shape == (0, 512)
    dense = query.MapQuery(PU.dense_of(all_obj, Xs), dev)
    gd = dense.features(ids).cpu().numpy()
    assert not gd[~ok].any() and np.array_equal(gd[ok], X[ids[ok]].astype(np.float32))
    heads = sum(512 * (H + 1) * 4 for H in WIDTHS)
    assert mq.store_bytes() == sum(n * (H + 4) * 4 for n, H in zip(SIZES, WIDTHS)) + heads
    assert dense.store_bytes() == sum(SIZES) * 512 * 4
    big, bX = PU.compact_map(3, (6000, 3000), (32, 32), missing=())
    cb, db = query.MapQuery(big, dev).store_bytes(), query.MapQuery(PU.dense_of(big, bX), dev).store_bytes()
    assert cb == 9000 * 36 * 4 + 2 * 512 * 33 * 4 and db == 9000 * 512 * 4
    assert cb < db / 12


def test_compact_pca_colors_match_the_restatement(dev):
    all_obj, Xs = PU.compact_map(11, (5000, 800, 64), (32, 128, 32), planted=True)
    mq = query.MapQuery(all_obj, dev)
    stats = {}
    cols = mq.color_by_partfeat(stats=stats)
    assert stats["eigh_s"] > 0
    for c, X in zip(mq.split(cols), Xs):
        assert PU.spectrum_gap_ok(X)
        err = np.abs(c.cpu().numpy() - QU.pca_colors(QU.pca_scores(X))).max()
        print(f"n={len(X)}: PCA colours against the restatement {err:.3e}")
        assert err <= 1e-4
    assert mq.color_by_partfeat().cpu().numpy().tobytes() == cols.cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------------------ end to end
def test_planar_scene_exports_both_forms_end_to_end(dev, tmp_path):
    """The recipe of test_planar_scene_to_queries_end_to_end, exported densely and compactly from the same log."""
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
    dense = map_vis.export(str(log), grid_dim=64, device=str(dev))
    comp = map_vis.export(str(log), grid_dim=64, device=str(dev), compact=True)
    assert os.path.isfile(log / "map_vis.pkl.gz") and os.path.isfile(log / "map_vis_compact.pkl.gz")
    assert len(comp) >= 2 and list(comp) == list(dense)
    Xs = []
    for k, o in comp.items():
        d = dense[k]
        assert "part_feat" not in o and set(o) - {"part_rows", "part_head"} == set(d) - {"part_feat"}
        assert np.array_equal(o["mesh"].vertices, d["mesh"].vertices) and np.array_equal(o["mesh"].faces, d["mesh"].faces)
        assert np.array_equal(np.asarray(o["color"]), np.asarray(d["color"]))
        r, A = o["part_rows"], o["part_head"]
        assert r.dtype == np.float32 and A.dtype == np.float32 and r.flags.c_contiguous
        assert r.shape == (len(d["part_feat"]), A.shape[1]) and A.shape[0] == d["part_feat"].shape[1]
        X = r.astype(np.float64) @ A.astype(np.float64).T
        err = np.linalg.norm(X - np.asarray(d["part_feat"], np.float64), axis=1).max()
        print(f"obj {k}: H = {A.shape[1] - 1}, {len(r)} vertices, max |A r - part_feat|_2 = {err:.3e}")
        assert err <= 4e-6
        Xs.append(X)
    mq = query.MapQuery(comp, dev)
    assert mq.D == query.MapQuery(dense, dev).D and mq.store_bytes() > 0
    Dc = next(np.shape(o["clip_feat"])[-1] for o in comp.values() if o["clip_feat"] is not None)
    Ds = next(np.shape(o["caption_feat"])[-1] for o in comp.values() if o["caption_feat"] is not None)
    rs = np.random.RandomState(3)
    _check_queries(mq, comp, Xs, rs, Dc, Ds)
    for X, d, cc in zip(Xs, dense.values(), mq.split(mq.color_by_partfeat())):
        if len(X) > 3:                                        # against the stored rows' own features and the dense rows
            e_own = np.abs(cc.cpu().numpy() - QU.pca_colors(QU.pca_scores(X))).max()
            e_dense = np.abs(cc.cpu().numpy() - QU.pca_colors(QU.pca_scores(np.asarray(d["part_feat"], np.float64)))).max()
            print(f"PCA colours: {e_own:.3e} against A r, {e_dense:.3e} against the dense part_feat")
            assert e_own <= 1e-3 and e_dense <= 1e-3
    np.save(str(tmp_path / "c.npy"), rs.randn(Dc).astype(np.float32))
    np.save(str(tmp_path / "s.npy"), rs.randn(Ds).astype(np.float32))
    np.save(str(tmp_path / "p.npy"), rs.randn(mq.D).astype(np.float32))
    out = tmp_path / "q"
    doc = map_query.main(["--logdir", str(log), "--compact", "--mode", "part", "--clip-query", str(tmp_path / "c.npy"),
                          "--sbert-query", str(tmp_path / "s.npy"), "--part-query", str(tmp_path / "p.npy"), "--top", "1",
                          "--out", str(out), "--device", str(dev)])
    assert sorted(doc["visible"]) == sorted(int(k) for k in comp)
    assert json.load(open(out / "query.json")) == doc and len(doc["top"]) == 1 and len(doc["ranking"]) == len(mq.ranked)
    for k in comp:
        v, _, rgba, _ = omesh.read_ply(str(out / f"obj_{k}.ply"))
        assert len(v) == len(comp[k]["mesh"].vertices) and rgba is not None
    d = map_query.main(["--logdir", str(log), "--compact", "--mode", "partpca", "--out", str(tmp_path / "pca"),
                        "--device", str(dev)])
    assert all(os.path.exists(tmp_path / "pca" / f"obj_{k}.ply") for k in d["visible"])
    assert os.path.exists(tmp_path / "pca" / "query.json")
