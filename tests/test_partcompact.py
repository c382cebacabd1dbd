"""CPU: the host side of the compact exported map: the low-rank PCA weights against the dense chain
in fp64, the map file, MapQuery's checks before the device and the command line's choice of file."""
import gzip
import os
import pickle

import numpy as np
import pytest

from openobj_amd import map_query, map_vis, query
try:
    from tests import partcompact_util as PU
    from tests import query_util as QU
except ImportError:          # plain `pytest tests/` puts tests/ itself, not the repository root, on sys.path
    import partcompact_util as PU
    import query_util as QU


def _segment(seed, n, H, C=512):
    rs = np.random.RandomState(seed)
    W, b = PU.head(rs, H, C)
    return PU.rows64(PU.hidden(rs, n, H), W, b)


def _scores(r, A, X):
    mr, Sr = PU.moments(r)
    mx, Sx = PU.moments(X)
    P, b = query.pca_weights_lowrank([mr], [Sr], [A], [len(r)])
    Wd, bd = query.pca_weights(mx[None], Sx[None], [len(r)])
    return QU.sign_rule(r @ P[0] + b[0]), QU.sign_rule(X @ Wd[0] + bd[0])


@pytest.mark.parametrize("n,H", [(5000, 32), (800, 128), (64, 32)])
def test_lowrank_pca_equals_the_dense_chain(n, H):
    r, A, X = _segment(n + H, n, H)
    assert PU.spectrum_gap_ok(X)
    low, dense = _scores(r, A, X)
    err = np.abs(low - dense).max()
    print(f"n={n} H={H}: |scores_lowrank - scores_dense| = {err:.3e} of {np.abs(dense).max():.3e}")
    assert err <= 1e-9 * np.abs(dense).max()


def test_lowrank_pca_shapes_and_stats():
    r, A, X = _segment(3, 200, 32, 64)
    mr, Sr = PU.moments(r)
    stats = {}
    P, b = query.pca_weights_lowrank(np.stack([mr, mr]), np.stack([Sr, Sr]), np.stack([A, A]), [200, 0], stats)
    assert P.shape == (2, 33, 3) and b.shape == (2, 3) and stats["eigh_s"] > 0
    assert not P[1].any() and not b[1].any()                         # an empty segment: zero weights


def test_constant_column_takes_std_one():
    rs = np.random.RandomState(5)
    W, b = PU.head(rs, 32, 64)
    W[7], b[7] = 0.0, 0.0                                             # channel 7 of every feature is exactly 0
    r, A, X = PU.rows64(PU.hidden(rs, 500, 32), W, b)
    assert not X[:, 7].any() and PU.spectrum_gap_ok(X)
    low, dense = _scores(r, A, X)
    assert np.isfinite(low).all()
    assert np.abs(low - dense).max() <= 1e-9 * np.abs(dense).max()


@pytest.mark.parametrize("n", [1, 2, 3])
def test_tiny_segments_give_finite_weights(n):
    r, A, _ = _segment(n, n, 32, 64)
    mr, Sr = PU.moments(r)
    P, b = query.pca_weights_lowrank([mr], [Sr], [A], [n])
    assert P[0].shape == (33, 3) and np.isfinite(P[0]).all() and np.isfinite(b).all()
    assert not P[0][:, n - 1:].any()                                  # n rows span at most n - 1 components


def _write(all_obj, logdir, name):
    os.makedirs(logdir, exist_ok=True)
    with gzip.open(os.path.join(logdir, name), "wb") as fh:
        pickle.dump(all_obj, fh)


def test_compact_file_round_trip(tmp_path):
    all_obj, _ = PU.compact_map(0, (30, 0, 7), (32, 32, 128), C=64)
    _write(all_obj, str(tmp_path), map_vis.COMPACT_FILE)
    _, back, _ = map_query._parse(["--logdir", str(tmp_path), "--mode", "rgb", "--out", str(tmp_path / "o"), "--compact"])
    assert list(back) == list(all_obj)
    for k, o in all_obj.items():
        assert "part_feat" not in back[k]
        for key, width in (("part_rows", o["part_head"].shape[1]), ("part_head", o["part_head"].shape[1])):
            assert back[k][key].dtype == np.float32 and back[k][key].shape[1] == width
            assert back[k][key].tobytes() == o[key].tobytes()
    assert query.compact_layout(back) is not None and query.compact_layout(PU.dense_of(all_obj, [
        np.zeros((len(o["part_rows"]), 64)) for o in all_obj.values()])) is None


def test_mapquery_rejects_bad_maps_before_the_device():
    all_obj, Xs = PU.compact_map(1, (5, 4), (32, 32), C=64)
    dense = PU.dense_of(all_obj, Xs)
    k0, k1 = list(all_obj)
    with pytest.raises(ValueError, match="mixes"):
        query.MapQuery({k0: all_obj[k0], k1: dense[k1]}, "cuda:0")
    bad = {k: dict(o) for k, o in all_obj.items()}
    bad[k1]["part_head"] = bad[k1]["part_head"][:, :-1]               # head [C, H] against rows [V, H + 1]
    with pytest.raises(ValueError, match="does not match"):
        query.MapQuery(bad, "cuda:0")
    bad = {k: dict(o) for k, o in all_obj.items()}
    bad[k1]["part_head"] = bad[k1]["part_head"][:48]                  # heads of different C
    with pytest.raises(ValueError, match="different widths"):
        query.MapQuery(bad, "cuda:0")
    bad = {k: dict(o) for k, o in all_obj.items()}
    del bad[k0]["part_head"]
    with pytest.raises(ValueError, match="without part_head"):
        query.MapQuery(bad, "cuda:0")


def test_cli_picks_the_file_and_checks_the_query_width(tmp_path):
    all_obj, Xs = PU.compact_map(2, (6, 3), (32, 128), C=64, Dc=16, Ds=8, missing=())
    both, only_c, only_d = tmp_path / "both", tmp_path / "c", tmp_path / "d"
    _write(all_obj, str(both), map_vis.COMPACT_FILE)
    _write(PU.dense_of(all_obj, Xs), str(both), map_vis.DENSE_FILE)
    _write(all_obj, str(only_c), map_vis.COMPACT_FILE)
    _write(PU.dense_of(all_obj, Xs), str(only_d), map_vis.DENSE_FILE)
    base = ["--mode", "rgb", "--out", str(tmp_path / "o")]
    kind = lambda argv: "part_rows" in next(iter(map_query._parse(argv)[1].values()))
    assert kind(["--logdir", str(both)] + base) is False             # the dense file if present
    assert kind(["--logdir", str(both), "--compact"] + base) is True
    assert kind(["--logdir", str(only_c)] + base) is True            # else the compact one
    assert kind(["--logdir", str(only_d)] + base) is False
    with pytest.raises(SystemExit):
        map_query._parse(["--logdir", str(only_d), "--compact"] + base)
    for name, n in (("c", 16), ("s", 8), ("p64", 64), ("p33", 33)):
        np.save(str(tmp_path / f"{name}.npy"), np.ones(n, np.float32))
    part = lambda logdir, p, *more: map_query._parse(
        ["--logdir", str(logdir), "--mode", "part", "--out", str(tmp_path / "o"), "--clip-query", str(tmp_path / "c.npy"),
         "--sbert-query", str(tmp_path / "s.npy"), "--part-query", str(tmp_path / f"{p}.npy"), *more])
    assert part(only_c, "p64")[2]["part_query"].shape == (64,)       # the head's C, not the row width
    assert part(both, "p64", "--compact")[2]["part_query"].shape == (64,)
    with pytest.raises(SystemExit):
        part(only_c, "p33")
