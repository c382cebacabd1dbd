"""The specification of the ray caster (include/objnerf_hip.h), free of the code under test: numpy fp64,
every operation one numpy call, so it rounds once, as on the device; brute force over every (ray, face) pair; a plain
Python walk of a heap-ordered tree for the CPU tests; the ray sets of tests/test_maprays*.py.  The scenes are those of
mapraster_util.  Test infrastructure only; openobj_amd never imports it."""
import numpy as np

import mapraster_util as RU

EMPTY = np.uint64((1 << 64) - 1)
F64 = np.float64
NAN_BITS = np.uint64(0x7ff8000000000000)
STATUS_BAD_ID, STATUS_BAD_RAY = 1, 2
CHUNK = 256                                                  # rays per block of the brute force


# ------------------------------------------------------------------------------------------------------ specification
def default_pad(verts):
    """2^-20 times the largest finite extent of verts."""
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    ext = 0.0
    for k in range(3):
        c = v[np.isfinite(v[:, k]), k]
        if len(c):
            ext = max(ext, float(c.max() - c.min()))
    return ext * 2.0 ** -20


def face_object(face_off, f):
    return np.searchsorted(np.asarray(face_off), f, side="right") - 1


def prepare(m, pad, hide=None):
    """The per-face part of rule (a) and the padded boxes -> dict(valid bool [F]: ids in range, corners finite, not hidden;
    p0, e1, e2, lo, hi fp64 [F, 3]; obj [F]; status)."""
    verts = np.asarray(m["verts"], np.float64).reshape(-1, 3)
    faces = np.asarray(m["faces"], np.int64).reshape(-1, 3)
    foff = np.asarray(m["face_off"], np.int64)
    V, F, S = len(verts), len(faces), len(foff) - 1
    hide = np.zeros(S, np.uint8) if hide is None else np.asarray(hide, np.uint8)
    in_range = ((faces >= 0) & (faces < V)).all(axis=1)
    safe = np.where(in_range[:, None], faces, 0)
    p = verts[safe] if V else np.zeros((F, 3, 3))
    obj = face_object(foff, np.arange(F)) if F else np.zeros(0, np.int64)
    valid = in_range & np.isfinite(p).all(axis=(1, 2)) & (hide[obj] == 0 if F else True)
    pad = F64(pad)
    with np.errstate(all="ignore"):
        lo = np.minimum(np.minimum(p[:, 0], p[:, 1]), p[:, 2]) - pad
        hi = np.maximum(np.maximum(p[:, 0], p[:, 1]), p[:, 2]) + pad
        e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    return {"valid": valid, "p0": p[:, 0], "e1": e1, "e2": e2, "lo": lo, "hi": hi, "obj": obj, "faces": faces, "verts": verts,
            "face_off": foff, "status": 0 if in_range.all() else STATUS_BAD_ID, "F": F}


def bad_rays(o, d):
    return ~(np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1)) | (d == 0).all(axis=1)


def slab(o, inv, par, lo, hi, t0, t1):
    """o, inv, par [n, 1, 3] (or [3]), lo, hi [1, F, 3] (or [3]), t0, t1 [n, 1] -> (passes, tn)."""
    with np.errstate(all="ignore"):
        a = (lo - o) * inv
        b = (hi - o) * inv
        near = np.where(par, -np.inf, np.fmin(a, b))
        far = np.where(par, np.inf, np.fmax(a, b))
        tn = np.fmax(np.fmax(np.fmax(-np.inf, near[..., 0]), near[..., 1]), near[..., 2])
        tf = np.fmin(np.fmin(np.fmin(np.inf, far[..., 0]), far[..., 1]), far[..., 2])
        inside = (~par | ((lo <= o) & (o <= hi))).all(axis=-1)
        return inside & (tn <= tf) & (tf >= t0) & (tn <= t1), tn


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def triangle(o, d, p0, e1, e2):
    """Sequence (c) -> (accepted, det, U, Vv, T, neg) with det > 0 where accepted."""
    with np.errstate(all="ignore"):
        pv = cross(d, e2)
        det = dot(e1, pv)
        tv = o - p0
        qv = cross(tv, e1)
        U, Vv, T = dot(tv, pv), dot(d, qv), dot(e2, qv)
        neg = det < 0
        det, U, Vv, T = (np.where(neg, -x, x) for x in (det, U, Vv, T))
        ok = (det != 0) & ~np.isnan(det) & (U >= 0) & (Vv >= 0) & (U + Vv <= det)
        return ok, det, U, Vv, T, neg


def windows(n, t_min, t_max):
    return (np.broadcast_to(np.asarray(t_min, np.float64), (n,)).copy(), np.broadcast_to(np.asarray(t_max, np.float64), (n,)).copy())


def pair_hits(P, o, d, t0, t1, sel=None, gates=True, both=False):
    """Rays [n] against the faces `sel` (all) -> (hit bool [n, f], t fp64 [n, f]).  gates=False: sequence (c) and the
    window of (d) alone.  both: -> (hit with the gates, t, hit without them)."""
    sel = slice(None) if sel is None else sel
    with np.errstate(all="ignore"):
        inv = 1.0 / d
        par = ~np.isfinite(inv)
        ok, det, U, Vv, T, _ = triangle(o[:, None], d[:, None], P["p0"][None, sel], P["e1"][None, sel], P["e2"][None, sel])
        t = T / det + 0.0
        hit = ok & P["valid"][None, sel] & (t0[:, None] <= t) & (t <= t1[:, None]) & ~bad_rays(o, d)[:, None]
        plain = hit
        if gates or both:
            passes, tn = slab(o[:, None], inv[:, None], par[:, None], P["lo"][None, sel], P["hi"][None, sel], t0[:, None],
                              t1[:, None])
            hit = hit & passes & (tn <= t)
    return (hit, t, plain) if both else (hit, t)


def keys_of(hit, t, face_ids):
    with np.errstate(all="ignore"):
        bits = t.astype(np.float32).view(np.uint32).astype(np.uint64)
    k = (bits << np.uint64(32)) | face_ids.astype(np.uint64)[None]
    k = np.where(hit, k, EMPTY)
    return k.min(axis=1, initial=EMPTY)


def brute_force(m, o, d, t_min=0.0, t_max=np.inf, pad=None, hide=None, gates=True, count_rejected=False):
    """-> dict(key uint64 [N], bad bool [N], status, P); count_rejected: also `rejected`, the (ray, face) pairs that
    sequence (c) with the window accepts and the gates (b), (d) reject."""
    o, d = np.asarray(o, np.float64).reshape(-1, 3), np.asarray(d, np.float64).reshape(-1, 3)
    pad = default_pad(m["verts"]) if pad is None else pad
    P = prepare(m, pad, m.get("hide") if hide is None else hide)
    n = len(o)
    t0, t1 = windows(n, t_min, t_max)
    key = np.full(n, EMPTY, np.uint64)
    ids = np.arange(P["F"])
    rejected = 0
    for s in range(0, n, CHUNK):
        e = slice(s, s + CHUNK)
        if P["F"]:
            hit, t, plain = pair_hits(P, o[e], d[e], t0[e], t1[e], gates=gates, both=True)
            key[e] = keys_of(hit, t, ids)
            rejected += int((plain & ~hit).sum())
    bad = bad_rays(o, d)
    out = {"key": key, "bad": bad, "status": P["status"] | (STATUS_BAD_RAY if bad.any() else 0), "P": P}
    if count_rejected:
        out["rejected"] = rejected
    return out


def resolve(P, key, o, d, ids):
    """The resolve rule on the keys -> dict(hit, t, face, winner, maskid, vertex, bary, point, normal)."""
    o, d = np.asarray(o, np.float64).reshape(-1, 3), np.asarray(d, np.float64).reshape(-1, 3)
    n = len(key)
    has = key != EMPTY
    f = np.where(has, key & np.uint64(0xFFFFFFFF), 0).astype(np.int64)
    out = {"hit": has.astype(np.uint8), "t": np.full(n, np.inf, np.float32), "face": np.full(n, -1, np.int32),
           "winner": np.full(n, -1, np.int32), "maskid": np.zeros(n, np.int32), "vertex": np.full(n, -1, np.int32),
           "bary": np.full((n, 2), np.nan), "point": np.full((n, 3), np.nan), "normal": np.full((n, 3), np.nan)}
    if not has.any():
        return out
    with np.errstate(all="ignore"):
        _, det, U, Vv, T, neg = triangle(o, d, P["p0"][f], P["e1"][f], P["e2"][f])
        t = T / det + 0.0
        u, v = U / det, Vv / det
        w = (1.0 - u) - v
        nn = cross(P["e1"][f], P["e2"][f])
        nn = np.where(neg[:, None], -nn, nn)
        point = o + t[:, None] * d
    corner = np.zeros(n, np.int64)
    best = w.copy()
    for c, x in ((1, u), (2, v)):
        better = x > best
        corner[better], best[better] = c, x[better]
    winner = face_object(P["face_off"], f)
    ids = np.asarray(ids, np.int32)
    out["t"][has] = (key[has] >> np.uint64(32)).astype(np.uint32).view(np.float32)
    out["face"][has], out["winner"][has] = f[has], winner[has]
    out["maskid"][has] = ids[winner[has]]
    out["vertex"][has] = P["faces"][f, corner][has]
    out["bary"][has] = np.stack([u, v], axis=1)[has]
    out["point"][has], out["normal"][has] = point[has], nn[has]
    return out


def run_spec(m, o, d, t_min=0.0, t_max=np.inf, pad=None, hide=None, ids=None):
    """The whole specification -> resolve()'s dict plus key, status, counters (rays, hits, bad rays)."""
    r = brute_force(m, o, d, t_min, t_max, pad, hide)
    out = resolve(r["P"], r["key"], o, d, m["ids"] if ids is None else ids)
    out.update(key=r["key"], status=r["status"],
               counters=np.array([len(r["key"]), int((r["key"] != EMPTY).sum()), int(r["bad"].sum())], np.int64))
    return out


# ------------------------------------------------------------------------------------------- a plain Python tree walk
def morton(q):
    code = 0
    for b in range(21):
        for k in range(3):
            code |= ((int(q[k]) >> b) & 1) << (3 * b + 2 - k)
    return code


def down32(x):
    f = np.float32(x)
    return np.nextafter(f, np.float32(-np.inf)) if F64(f) > x else f


def up32(x):
    f = np.float32(x)
    return np.nextafter(f, np.float32(np.inf)) if F64(f) < x else f


def build_tree(P, leaf):
    """Morton-sorted faces in groups of `leaf`, a complete tree in heap order with fp32 boxes rounded outward ->
    dict(order, size, lo, hi fp32 [2 size, 3], leaf)."""
    F = P["F"]
    ok = P["valid"]
    fin_lo, fin_hi = P["lo"][ok], P["hi"][ok]
    blo = fin_lo.min(axis=0) if ok.any() else np.zeros(3)
    bhi = fin_hi.max(axis=0) if ok.any() else np.ones(3)
    codes = []
    for f in range(F):
        if not ok[f]:
            codes.append(1 << 63)
            continue
        with np.errstate(all="ignore"):
            q = ((P["lo"][f] + P["hi"][f]) * 0.5 - blo) / (bhi - blo) * 2097152.0
        codes.append(morton(np.clip(np.nan_to_num(q), 0, 2097151).astype(np.int64)))
    order = sorted(range(F), key=lambda f: (codes[f], f))
    n_leaf = max(-(-F // leaf), 1)
    size = 1
    while size < n_leaf:
        size *= 2
    lo = np.full((2 * size, 3), np.inf, np.float32)
    hi = np.full((2 * size, 3), -np.inf, np.float32)
    for i in range(n_leaf):
        fs = [f for f in order[i * leaf:(i + 1) * leaf] if ok[f]]
        if fs:
            l, h = P["lo"][fs].min(axis=0), P["hi"][fs].max(axis=0)
            lo[size + i] = [down32(x) for x in l]
            hi[size + i] = [up32(x) for x in h]
    for n in range(size - 1, 0, -1):
        lo[n], hi[n] = np.minimum(lo[2 * n], lo[2 * n + 1]), np.maximum(hi[2 * n], hi[2 * n + 1])
    return {"order": order, "size": size, "lo": lo, "hi": hi, "leaf": leaf}


def tree_walk(P, tree, o, d, t0, t1):
    """One ray through the tree with the pruning rule of the header -> (key, nodes visited)."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    if bad_rays(o[None], d[None])[0]:
        return EMPTY, 0
    with np.errstate(all="ignore"):
        inv = 1.0 / d
    par = ~np.isfinite(inv)
    t0a, t1a = np.array([t0], np.float64), np.array([t1], np.float64)
    key, best, visits = EMPTY, np.float32(np.inf), 0
    stack = [1]
    while stack:
        n = stack.pop()
        visits += 1
        if tree["lo"][n, 0] > tree["hi"][n, 0]:
            continue
        passes, tn = slab(o, inv, par, tree["lo"][n].astype(np.float64), tree["hi"][n].astype(np.float64), F64(t0), F64(t1))
        if not passes or np.float32(tn) > best:
            continue
        if n >= tree["size"]:
            i = n - tree["size"]
            sel = np.array(tree["order"][i * tree["leaf"]:(i + 1) * tree["leaf"]], np.int64)
            if len(sel):
                hit, t = pair_hits(P, o[None], d[None], t0a, t1a, sel=sel)
                k = keys_of(hit, t, sel)[0]
                if k < key:
                    key, best = k, np.array(k >> np.uint64(32), np.uint32).view(np.float32)
        else:
            stack += [2 * n + 1, 2 * n]
    return key, visits


# --------------------------------------------------------------------------------------------------------- the ray sets
def view_rays(T_WC, intr, W, H):
    """The rasteriser's sample points as rays, restated here: o = the camera centre, d = R ((i - cx) / fx, (j - cy) / fy,
    1), pixel (i, j) at row i H + j."""
    T = np.asarray(T_WC, np.float64)
    fx, fy, cx, cy = (F64(x) for x in intr)
    i, j = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64), indexing="ij")
    x, y = ((i - cx) / fx).reshape(-1), ((j - cy) / fy).reshape(-1)
    R = T[:3, :3]
    d = np.stack([(R[k, 0] * x + R[k, 1] * y) + R[k, 2] for k in range(3)], axis=1)
    return np.broadcast_to(T[:3, 3], d.shape).copy(), d


def edge_midpoints(m):
    f = np.asarray(m["faces"], np.int64).reshape(-1, 3)
    V = len(m["verts"])
    f = f[((f >= 0) & (f < V)).all(axis=1)]
    if not len(f):
        return np.zeros((0, 3))
    e = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1), axis=0)
    v = np.asarray(m["verts"], np.float64)
    return (v[e[:, 0]] + v[e[:, 1]]) * 0.5


def pick(a, n, rs):
    return a if len(a) <= n else a[np.sort(rs.choice(len(a), n, replace=False))]


def special_rays(m, seed=0, n_each=300):
    """Rays through vertices and edge midpoints; axis-parallel rays from points that share coordinates with vertices
    (an infinite inv; a parallel axis exactly on a padded box face); origins on and inside faces; a NaN, an infinite and
    an all-zero direction.  -> (o, d) of about 6 n_each + 8 rays."""
    rs = np.random.RandomState(seed)
    v = np.asarray(m["verts"], np.float64).reshape(-1, 3)
    v = v[np.isfinite(v).all(axis=1)]
    eye = np.asarray(m["cam"], np.float64)
    if not len(v):
        v = np.array([[0.0, 0.0, 0.0], [1.0, 0.5, 0.25]])
    pad = F64(default_pad(m["verts"]))
    os_, ds_ = [], []
    for tgt in (pick(v, n_each, rs), pick(edge_midpoints(m), n_each, rs)):       # through vertices and edge midpoints
        os_.append(np.broadcast_to(eye, tgt.shape).copy())
        ds_.append(tgt - eye)
    pv = pick(v, n_each, rs)                                                     # axis-parallel, sharing two coordinates
    for k, p in enumerate(pv):
        ax, sgn = k % 3, 1.0 if (k // 3) % 2 == 0 else -1.0
        o = p.copy()
        o[ax] -= sgn * 3.0
        if k % 4 == 1:
            o[(ax + 1) % 3] = p[(ax + 1) % 3] - pad                              # exactly on a padded box face
        if k % 4 == 2:
            o[(ax + 2) % 3] = p[(ax + 2) % 3] + pad
        dd = np.zeros(3)
        dd[ax] = sgn * (0.5 + rs.rand())
        os_.append(o[None])
        ds_.append(dd[None])
    pv = pick(v, n_each, rs)                                                     # two parallel axes off, one shared
    o = pv + rs.randn(*pv.shape) * 0.01
    o[:, 2] -= 2.5
    dd = np.zeros_like(pv)
    dd[:, 2] = 1.0
    os_.append(o)
    ds_.append(dd)
    f = np.asarray(m["faces"], np.int64).reshape(-1, 3)
    f = f[((f >= 0) & (f < len(m["verts"]))).all(axis=1)]
    if len(f):
        fv = np.asarray(m["verts"], np.float64)[pick(f, n_each, rs)]
        fv = fv[np.isfinite(fv).all(axis=(1, 2))]
        w = rs.dirichlet((1.0, 1.0, 1.0), len(fv))
        inside = (w[:, :, None] * fv).sum(axis=1)                                # inside a face (up to rounding)
        dirs = rs.randn(len(fv), 3)
        os_ += [inside, fv[:, 0].copy(), (fv[:, 0] + fv[:, 1]) * 0.5]            # on a corner, on an edge
        ds_ += [dirs, rs.randn(len(fv), 3), fv[:, 2] - fv[:, 0]]                 # (the last: inside the face's plane)
    bad_o = np.tile(eye, (8, 1))
    bad_d = np.array([[np.nan, 0, 1], [0, np.inf, 1], [0, 0, 0], [1, -np.inf, 0], [0.1, 0.2, 1.0], [0, 0, 1.0], [0, 0, -0.0],
                      [0.0, 1.0, 0.0]])
    bad_o[4, 1] = np.nan
    bad_o[5, 0] = np.inf
    os_.append(bad_o)
    ds_.append(bad_d)
    return np.concatenate(os_), np.concatenate(ds_)


def scene_rays(m, seed=0, n_each=300):
    """The pixel rays of the scene's camera plus special_rays."""
    o1, d1 = view_rays(m["T_WC"], m["intr"], m["W"], m["H"])
    o2, d2 = special_rays(m, seed, n_each)
    return np.concatenate([o1, o2]), np.concatenate([d1, d2])


def segments_of(m, n=400, seed=1):
    """Segments a -> b as rays (d = b - a, window [0, 1]): from the camera side to behind the meshes, some ending just
    short of and some just beyond a vertex."""
    rs = np.random.RandomState(seed)
    v = np.asarray(m["verts"], np.float64).reshape(-1, 3)
    v = v[np.isfinite(v).all(axis=1)]
    if not len(v):
        v = np.zeros((1, 3))
    tgt = v[rs.randint(len(v), size=n)]
    a = np.asarray(m["cam"], np.float64) + rs.randn(n, 3) * 0.3
    s = np.where(np.arange(n) % 3 == 0, 0.9, np.where(np.arange(n) % 3 == 1, 1.0, 1.5))
    b = a + (tgt - a) * s[:, None]
    return a, b - a


def scene_of(name):
    return RU.bad_index_scene() if name == "bad_index" else RU.make_scenes()[name][0]
