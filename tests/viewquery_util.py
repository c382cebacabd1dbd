"""Helpers of the view-query tests (test infrastructure only): the query of a merged map view stated in numpy fp64,
the fold of the per-object loop extended to carry a feature row per pixel, and the hand-built CSR of the kernel test.

The statement: pixel p is PAINTED by entry e = winner[p] iff 0 <= e < M and pix[e] == p; its object k has
seg[k] <= e < seg[k + 1]; its part feature is F = of_w_k . h + of_b_k * opacity[e] with h = hfeat_k[e - row0_k]
(vmap.py:678: the linear head applied after compositing); sims[q] = (queries[q] . F) / max(|F|, 1e-8); label = the
first arg-max over q.  Nothing painted (or a painter whose object has no hidden rows): NaN, -1, a zero feature row."""
import numpy as np

U24 = 2.0 ** -24


def view_query_ref(seg, pix, opacity, winner, heads, queries=None):
    """seg [K + 1], pix [M], opacity [M], winner [P]; heads: per object (of_w [C, H], of_b [C], hfeat [n, H] | None, row0).
    -> dict(painted [P] bool, F [P, C] fp64 (zeros where not painted), A [P, C] = |of_w| . |h| + |of_b| opacity (the
    scale of F's rounding error), sims [Q, P], label [P] int32, best [P]); the last three only with queries."""
    seg, pix, winner = np.asarray(seg, np.int64), np.asarray(pix, np.int64), np.asarray(winner, np.int64).reshape(-1)
    opacity = np.asarray(opacity, np.float64)
    P, M, C = winner.shape[0], pix.shape[0], np.asarray(heads[0][0]).shape[0]
    w = np.where(winner < 0, winner + (1 << 32), winner)                # (the winner image holds the low 32 bits)
    live = w < M
    live[live] = pix[w[live]] == np.flatnonzero(live)
    F, A, painted = np.zeros((P, C)), np.zeros((P, C)), np.zeros(P, bool)
    obj = np.searchsorted(seg, w, side="right") - 1
    for k, (of_w, of_b, hfeat, row0) in enumerate(heads):
        sel = np.flatnonzero(live & (obj == k))
        if hfeat is None or sel.size == 0:
            continue
        of_w, of_b = np.asarray(of_w, np.float64), np.asarray(of_b, np.float64)
        h, op = np.asarray(hfeat, np.float64)[w[sel] - row0], opacity[w[sel]]
        F[sel] = h @ of_w.T + op[:, None] * of_b[None]
        A[sel] = np.abs(h) @ np.abs(of_w).T + op[:, None] * np.abs(of_b)[None]
        painted[sel] = True
    out = dict(painted=painted, F=F, A=A)
    if queries is not None:
        q = np.asarray(queries, np.float64)
        sims = (q @ F.T) / np.maximum(np.linalg.norm(F, axis=1), 1e-8)[None]
        sims[:, ~painted] = np.nan
        best = np.full(P, np.nan)
        best[painted] = sims[:, painted].max(axis=0)
        out.update(sims=sims, label=first_argmax(sims), best=best)
    return out


def first_argmax(sims):
    """[Q, P] -> int32 [P]: np.argmax over q (the first maximum; the first NaN if there is one), -1 for a column that
    is NaN throughout (nothing painted)."""
    sims = np.asarray(sims)
    lab = np.argmax(sims, axis=0).astype(np.int32)
    lab[np.isnan(sims).all(axis=0)] = -1
    return lab


def dense_then_cosine(seg, pix, opacity, winner, heads, queries):
    """The naive form: walk the ENTRIES, write the 512-d feature of every entry that won its pixel into a dense [P, C]
    image, then torch's cosine_similarity per query over the painted pixels."""
    import torch
    seg, pix, winner = np.asarray(seg, np.int64), np.asarray(pix, np.int64), np.asarray(winner, np.int64).reshape(-1)
    P, C = winner.shape[0], np.asarray(heads[0][0]).shape[0]
    img, painted = np.zeros((P, C)), np.zeros(P, bool)
    for k, (of_w, of_b, hfeat, row0) in enumerate(heads):
        if hfeat is None:
            continue
        for e in range(int(seg[k]), int(seg[k + 1])):
            p = int(pix[e])
            if 0 <= p < P and winner[p] == e:
                img[p] = np.asarray(of_w, np.float64) @ np.asarray(hfeat, np.float64)[e - row0] + \
                    np.asarray(of_b, np.float64) * float(opacity[e])
                painted[p] = True
    q = torch.from_numpy(np.asarray(queries, np.float64))
    sims = np.full((q.shape[0], P), np.nan)
    t = torch.from_numpy(img[painted])
    for i in range(q.shape[0]):
        sims[i, painted] = torch.nn.functional.cosine_similarity(t, q[i][None], dim=1, eps=1e-8).numpy()
    return img, painted, sims


def random_view(rs, K, P, C, widths=(32,), max_seg=40, p_none=0.2):
    """A random small CSR with a valid winner image: K objects over P pixels, each covering a random ascending subset."""
    seg, pix, heads = [0], [], []
    for k in range(K):
        n = int(rs.randint(0, min(P, max_seg) + 1))
        pix.append(np.sort(rs.choice(P, n, replace=False)))
        seg.append(seg[-1] + n)
        H = int(widths[k % len(widths)])
        hf = rs.standard_normal((n, H)).astype(np.float32) if n else None
        heads.append((rs.standard_normal((C, H)).astype(np.float32) / np.sqrt(H), 0.1 * rs.standard_normal(C).astype(np.float32),
                      hf, seg[-2]))
    pix = np.concatenate(pix).astype(np.int32)
    M = pix.shape[0]
    winner = np.full(P, -1, np.int32)
    for p in range(P):
        cand = np.flatnonzero(pix == p)
        if cand.size and rs.uniform() > p_none:
            winner[p] = cand[rs.randint(cand.size)]
    return np.asarray(seg, np.int64), pix, rs.uniform(0.5, 1.0, M).astype(np.float32), winner, heads


def unit_queries(rs, Q, C):
    q = rs.standard_normal((Q, C)).astype(np.float32)
    return q / np.linalg.norm(q, axis=1, keepdims=True)


# The CSR of the kernel test: segments of 1, 15, 16, 17 and 65 entries, then 40 entries of an object that wins nowhere
# (it holds whole 16-entry chunks without a live lane) and 33 entries of a hidden-128 object; object 3 keeps its hidden
# rows in a buffer of its own (row0 = its segment's start), the other hidden-32 objects share one CSR-aligned buffer.
KERNEL_SEGS = (1, 15, 16, 17, 65, 40, 33)
KERNEL_WIDTHS = (32, 32, 32, 32, 32, 32, 128)
KERNEL_P, KERNEL_C = 150, 512
NEVER_WINS = 5


def kernel_case(seed=0):
    """-> dict(seg, pix, opacity, winner, heads (numpy; hfeat of the shared buffer has M rows and row0 = 0), traps):
    every pixel an object covers is won by one of its coverers or by nobody; traps: p_foreign (its winner names an
    entry of ANOTHER pixel: not painted), e_outside (an entry whose pix is outside [0, P))."""
    rs = np.random.RandomState(100 + seed)
    seg = np.concatenate([[0], np.cumsum(KERNEL_SEGS)]).astype(np.int64)
    M, P, C = int(seg[-1]), KERNEL_P, KERNEL_C
    pix = np.concatenate([np.sort(rs.choice(P, n, replace=False)) for n in KERNEL_SEGS]).astype(np.int32)
    obj = np.searchsorted(seg, np.arange(M), side="right") - 1
    e_outside = int(seg[4]) + 20
    pix[e_outside] = P + 7
    winner = np.full(P, -1, np.int32)
    for p in range(P):
        cand = np.flatnonzero((pix == p) & (obj != NEVER_WINS))
        if cand.size and rs.uniform() > 0.15:
            winner[p] = cand[rs.randint(cand.size)]
    free = np.flatnonzero(winner < 0)
    p_foreign = int(free[0])
    winner[p_foreign] = int(np.flatnonzero((pix != p_foreign) & (pix < P))[3])
    shared = rs.standard_normal((M, 32)).astype(np.float32)
    heads = []
    for k, H in enumerate(KERNEL_WIDTHS):
        of_w = (rs.standard_normal((C, H)) / np.sqrt(H)).astype(np.float32)
        of_b = (0.1 * rs.standard_normal(C)).astype(np.float32)
        if H == 32 and k != 3:
            heads.append((of_w, of_b, shared, 0))
        else:
            heads.append((of_w, of_b, rs.standard_normal((KERNEL_SEGS[k], H)).astype(np.float32), int(seg[k])))
    return dict(seg=seg, pix=pix, opacity=rs.uniform(0.5, 1.0, M).astype(np.float32), winner=winner, heads=heads,
                p_foreign=p_foreign, e_outside=e_outside)


def fold_features(buf, results, order, bg_ids, class_of, C):
    """The fold of train.py:581-598 (render_view.ViewBuffers.merge) over per-object results in `order`, extended to carry
    one feature row per pixel.  results: obj_id -> (mask [W, H] bool, depth [n], colour [n, 3], feat [n, C]) or a tuple
    whose depth is None (the object rendered nothing).  -> feat image [W, H, C] (zeros where nothing painted)."""
    img = np.zeros(buf.depth.shape + (C,), np.float32)
    for oid in order:
        mask, depth, colour, feat = results[oid]
        if depth is None:
            continue
        ok = buf.merge(mask, depth, colour, class_of.get(oid, oid), oid in bg_ids)
        this = np.zeros_like(img)
        this[mask] = feat
        img[ok] = this[ok]
    return img
