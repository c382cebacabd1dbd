"""Inputs and fp64 restatements for the compact exported map: test infrastructure only."""
import numpy as np


def head(rs, H, C=512):
    """An out_clip head as the model initialises it: xavier-normal weight [C, H], nn.Linear's uniform bias [C] (fp32)."""
    W = rs.randn(C, H) * np.sqrt(2.0 / (C + H))
    b = rs.uniform(-1.0, 1.0, C) / np.sqrt(H)
    return W.astype(np.float32), b.astype(np.float32)


def hidden(rs, n, H):
    """A feature hidden after its ReLU [n, H] fp32: non-negative, a common offset, three planted directions (strengths
    3 : 2 : 1.5), then a gap to isotropic noise."""
    dirs, _ = np.linalg.qr(rs.randn(H, 3))
    z = rs.randn(n, 3) * np.array([3.0, 2.0, 1.5])
    h = 1.0 + 0.12 * z @ dirs.T + 0.02 * rs.randn(n, H)
    return np.maximum(h, 0.0).astype(np.float32)


def rows64(h, W, b):
    """fp64: (r [n, H + 1], A [C, H + 1], X [n, C] = r A^T the unit features) of fp32 inputs."""
    h, W, b = np.asarray(h, np.float64), np.asarray(W, np.float64), np.asarray(b, np.float64)
    f = h @ W.T + b
    s = 1.0 / np.maximum(np.linalg.norm(f, axis=1, keepdims=True), 1e-8)
    r = np.concatenate([h * s, s], axis=1)
    A = np.concatenate([W, b[:, None]], axis=1)
    return r, A, r @ A.T


def kappa(h, W, b):
    """| |W| |h_v| + |b| |_2 / |W h_v + b|_2 per vertex (fp64): the condition of the head product."""
    h, W, b = np.asarray(h, np.float64), np.asarray(W, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(np.abs(h) @ np.abs(W).T + np.abs(b), axis=1) / np.linalg.norm(h @ W.T + b, axis=1)


def moments(Y):
    Y = np.asarray(Y, np.float64)
    m = Y.mean(axis=0)
    return m, (Y - m).T @ (Y - m)


def spectrum_gap_ok(X):
    """The assertion of test_pca_colors_match_the_restatement: ev[2] - ev[3] >= 1e-3 ev[0] on the correlation matrix."""
    X = np.asarray(X, np.float64)
    sd = X.std(0)
    sd[sd == 0] = 1.0
    Z = (X - X.mean(0)) / sd
    ev = np.linalg.eigvalsh(Z.T @ Z / len(X))[::-1]
    return ev[2] - ev[3] >= 1e-3 * ev[0]


def compact_map(seed, sizes, widths, C=512, Dc=512, Ds=384, missing=(2,), planted=False):
    """A compact all_obj as map_vis.export(compact=True) writes it -> (all_obj, X: per object the fp64 unit features
    of the stored fp32 rows).  Objects at the positions in `missing` carry no clip / caption feature."""
    from openobj_amd.mesh import TriMesh
    rs = np.random.RandomState(seed)
    out, Xs = {}, []
    for p, (n, H) in enumerate(zip(sizes, widths)):
        W, b = head(rs, H, C)
        h = hidden(rs, n, H) if planted else np.abs(0.5 + 0.5 * rs.randn(n, H)).astype(np.float32)
        r, A, _ = rows64(h, W, b)
        r32, A32 = r.astype(np.float32), A.astype(np.float32)
        v = rs.rand(n, 3) + [0, 0, 0.3 * p]
        f = np.arange(3 * (n // 3)).reshape(-1, 3) if n >= 3 else np.zeros((0, 3), np.int64)
        m = TriMesh(v, f)
        m.visual.vertex_colors = rs.randint(0, 256, (n, 4)).astype(np.uint8)
        base_c, base_s = rs.randn(Dc), rs.randn(Ds)
        clip = None if p in missing else np.stack([base_c + 0.01 * rs.randn(Dc) for _ in range(4)] + [rs.randn(Dc) * 5])
        cap = None if p in missing else (base_s + 0.01 * rs.randn(Ds)).astype(np.float32)
        out[10 + 3 * p] = {"clip_feat": clip, "caption_feat": cap, "class_id": p, "mesh": m,
                           "color": m.visual.vertex_colors, "part_rows": r32, "part_head": A32}
        Xs.append(r32.astype(np.float64) @ A32.astype(np.float64).T)
    return out, Xs


def dense_of(all_obj, Xs):
    """The dense map of the same features (part_feat fp32)."""
    out = {}
    for (k, o), X in zip(all_obj.items(), Xs):
        d = {kk: vv for kk, vv in o.items() if kk not in ("part_rows", "part_head")}
        d["part_feat"] = X.astype(np.float32)
        out[k] = d
    return out
