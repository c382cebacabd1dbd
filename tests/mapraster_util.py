"""The specification of the mesh rasteriser (include/objnerf_hip.h), free of the code under test: Python
integers for the edge functions, numpy fp64 scalars for the one depth sequence (every operation is one numpy call, so it
rounds once, as on the device), plain loops over the faces and the pixels of their boxes.  Also the small scenes of
tests/test_mapraster*.py.  Test infrastructure only; openobj_amd never imports it."""
import numpy as np

from mapregions_util import pack, sheet, sheet_xy

BOUND = float(2 ** 25)
EMPTY = (1 << 64) - 1
STATS = ("small", "large", "no_sample", "z_near", "bound", "degenerate", "bad_index", "hidden")
ST = {n: i for i, n in enumerate(STATS)}
SMALL_DEFAULT = 4
F64 = np.float64


# ------------------------------------------------------------------------------------------------------ specification
def world_to_camera(T_WC):
    """The upper 3 x 4 of inverse(T_WC), inverted in fp64."""
    return np.ascontiguousarray(np.linalg.inv(np.asarray(T_WC, np.float64).reshape(4, 4))[:3, :])


def project(verts, T_CW, intr, z_near):
    """-> (X, Y: lists of Python integers (None where dropped), iz fp64 [V], drop int [V]: 0 ok, 1 z_near, 2 bound)."""
    p = np.asarray(verts, np.float64).reshape(-1, 3)
    M = np.asarray(T_CW, np.float64).reshape(12)
    fx, fy, cx, cy = (F64(x) for x in intr)
    with np.errstate(all="ignore"):
        cam = [((M[4 * r] * p[:, 0] + M[4 * r + 1] * p[:, 1]) + M[4 * r + 2] * p[:, 2]) + M[4 * r + 3] for r in range(3)]
        xc, yc, zc = cam
        u = (fx * xc) / zc + cx
        v = (fy * yc) / zc + cy
        X = np.floor(u * 256.0 + 0.5)
        Y = np.floor(v * 256.0 + 0.5)
        front = zc >= F64(z_near)
        inside = (np.abs(X) <= BOUND) & (np.abs(Y) <= BOUND)
        iz = 1.0 / zc
    drop = np.where(~front, 1, np.where(~inside, 2, 0))
    Xi = [int(x) if d == 0 else None for x, d in zip(X, drop)]
    Yi = [int(y) if d == 0 else None for y, d in zip(Y, drop)]
    return Xi, Yi, iz, drop


def edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def setup(X, Y, iz, drop, ids):
    """-> a stats name (the face is not drawn) or dict(x, y: the corners with 1 and 2 swapped where A < 0, iz, A, order:
    the positions 0..2 of the corners in that order)."""
    if any(drop[i] == 1 for i in ids):
        return "z_near"
    if any(drop[i] == 2 for i in ids):
        return "bound"
    x, y = [X[i] for i in ids], [Y[i] for i in ids]
    A = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0])
    if A == 0:
        return "degenerate"
    order = [0, 1, 2] if A > 0 else [0, 2, 1]
    return {"x": [x[k] for k in order], "y": [y[k] for k in order], "iz": [F64(iz[ids[k]]) for k in order], "A": abs(A),
            "order": order}


def box(t, W, H):
    """The sample points inside the face's box, clipped to the screen: pixel i iff min x <= 256 i <= max x."""
    i0, i1 = max(-((-min(t["x"])) // 256), 0), min(max(t["x"]) // 256, W - 1)
    j0, j1 = max(-((-min(t["y"])) // 256), 0), min(max(t["y"]) // 256, H - 1)
    return i0, i1, j0, j1


def weights(t, i, j):
    x, y, px, py = t["x"], t["y"], 256 * i, 256 * j
    return (edge(x[1], y[1], x[2], y[2], px, py), edge(x[2], y[2], x[0], y[0], px, py), edge(x[0], y[0], x[1], y[1], px, py))


def depth_terms(t, w):
    """-> (t_k = w_k iz_k, q = (t0 + t1) + t2)."""
    tk = [F64(w[k]) * t["iz"][k] for k in range(3)]
    return tk, (tk[0] + tk[1]) + tk[2]


def face_object(face_off, f):
    return int(np.searchsorted(np.asarray(face_off), f, side="right")) - 1


def visibility(m, T_CW, intr, W, H, z_near=0.05, hide=None, small=SMALL_DEFAULT, track_w=None):
    """m: dict(verts, faces, face_off) -> (key: a [W][H] list of Python integers, stats [8], status).  track_w: a list
    that receives max |w| over every evaluated sample."""
    verts, faces, foff = m["verts"], np.asarray(m["faces"]).reshape(-1, 3), m["face_off"]
    V, S = len(verts), len(foff) - 1
    hide = np.zeros(S, np.uint8) if hide is None else np.asarray(hide, np.uint8)
    X, Y, iz, drop = project(verts, T_CW, intr, z_near)
    key = [[EMPTY] * H for _ in range(W)]
    stats, status = [0] * 8, 0
    wmax = 0
    for f, ids in enumerate(faces):
        ids = [int(i) for i in ids]
        if any(i < 0 or i >= V for i in ids):
            stats[ST["bad_index"]] += 1
            status |= 1
            continue
        if hide[face_object(foff, f)]:
            stats[ST["hidden"]] += 1
            continue
        t = setup(X, Y, iz, drop, ids)
        if isinstance(t, str):
            stats[ST[t]] += 1
            continue
        i0, i1, j0, j1 = box(t, W, H)
        if i0 > i1 or j0 > j1:
            stats[ST["no_sample"]] += 1
            continue
        stats[ST["small" if i1 - i0 + 1 <= small and j1 - j0 + 1 <= small else "large"]] += 1
        for i in range(i0, i1 + 1):
            for j in range(j0, j1 + 1):
                w = weights(t, i, j)
                wmax = max(wmax, *(abs(x) for x in w))
                if min(w) < 0:
                    continue
                _, q = depth_terms(t, w)
                with np.errstate(all="ignore"):
                    d = np.float32(F64(t["A"]) / q)
                k = (int(d.view(np.uint32)) << 32) | f
                if k < key[i][j]:
                    key[i][j] = k
    if track_w is not None:
        track_w.append(wmax)
    return key, stats, status


def quant(c):
    c = float(c)
    x = (c if c <= 1.0 else 1.0) if c >= 0.0 else 0.0
    return int(np.floor(F64(x) * 255.0 + 0.5))


def shade_of(p0, p1, p2, cam, ambient):
    e1, e2 = p1 - p0, p2 - p0
    g = ((p0 + p1) + p2) / 3.0 - cam
    n = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]])
    dot = (n[0] * g[0] + n[1] * g[1]) + n[2] * g[2]
    nn = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    gg = np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
    den = nn * gg
    if not den > 0.0:
        return F64(1.0)
    a = F64(ambient)
    return a + (F64(1.0) - a) * (np.abs(dot) / den)


def resolve(m, key, T_CW, intr, W, H, z_near, ids, colors, cam, ambient=0.35, shading=True, background=(255, 255, 255)):
    """-> dict(rgb uint8 [W, H, 3], maskid, winner, face, vertex int32 [W, H], depth fp32 [W, H], counts int64 [S],
    point fp64 [W, H, 3]: sum b_k p_k, NaN where nothing is drawn)."""
    verts, faces, foff = np.asarray(m["verts"], np.float64), np.asarray(m["faces"]).reshape(-1, 3), m["face_off"]
    S = len(foff) - 1
    X, Y, iz, drop = project(verts, T_CW, intr, z_near)
    cam = np.asarray(cam, np.float64)
    out = {"rgb": np.zeros((W, H, 3), np.uint8), "maskid": np.zeros((W, H), np.int32), "winner": np.full((W, H), -1, np.int32),
           "face": np.full((W, H), -1, np.int32), "vertex": np.full((W, H), -1, np.int32),
           "depth": np.full((W, H), 100, np.float32), "counts": np.zeros(S, np.int64), "point": np.full((W, H, 3), np.nan)}
    out["rgb"][:] = np.asarray(background, np.uint8)
    col = np.asarray(colors, np.float32).astype(np.float64)
    for i in range(W):
        for j in range(H):
            k = key[i][j]
            if k == EMPTY:
                continue
            f = k & 0xFFFFFFFF
            fid = [int(x) for x in faces[f]]
            t = setup(X, Y, iz, drop, fid)
            s = face_object(foff, f)
            w = weights(t, i, j)
            tk, q = depth_terms(t, w)
            corner = [fid[o] for o in t["order"]]
            best = 0
            for c in (1, 2):
                if tk[c] > tk[best]:
                    best = c
            b = [tk[c] / q for c in range(3)]
            sh = shade_of(verts[fid[0]], verts[fid[1]], verts[fid[2]], cam, ambient) if shading else None
            for ch in range(3):
                c = (b[0] * col[corner[0], ch] + b[1] * col[corner[1], ch]) + b[2] * col[corner[2], ch]
                out["rgb"][i, j, ch] = quant(c * sh if shading else c)
            out["winner"][i, j], out["maskid"][i, j], out["face"][i, j] = s, ids[s], f
            out["vertex"][i, j] = corner[best]
            out["depth"][i, j] = np.array(k >> 32, np.uint32).view(np.float32)
            out["counts"][s] += 1
            out["point"][i, j] = b[0] * verts[corner[0]] + b[1] * verts[corner[1]] + b[2] * verts[corner[2]]
    return out


def key_array(key):
    """The [W][H] list of Python integers -> uint64 [W, H]."""
    return np.array(key, dtype=np.uint64)


def painted(key):
    return sum(k != EMPTY for row in key for k in row)


# ------------------------------------------------------------------------------------------------------------- scenes
W0, H0 = 70, 45
INTR0 = (60.0, 60.0, 34.5, 22.0)


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """T_WC [4, 4] of a camera at eye that looks along +z at target, x to the right, y down."""
    eye, target, up = (np.asarray(a, np.float64) for a in (eye, target, up))
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, y, z, eye
    return T


def sheet_object(w, h, size, centre=(0.0, 0.0, 0.0), tilt=0.0, jitter=0.0, flip=False, seed=0):
    """A w x h vertex sheet of `size` (x, y extent) about centre, rotated by tilt about the x axis, its inner vertices
    jittered by `jitter` cells.  flip: the second triangle of every cell gets the opposite orientation.
    -> (verts fp64 [w h, 3], faces int64 [f, 3])."""
    rs = np.random.RandomState(seed)
    x, y = sheet_xy(w, h)
    gx, gy = x.astype(np.float64), y.astype(np.float64)
    inner = (x > 0) & (x < w - 1) & (y > 0) & (y < h - 1)
    gx = gx + inner * jitter * (rs.rand(w * h) - 0.5)
    gy = gy + inner * jitter * (rs.rand(w * h) - 0.5)
    px = (gx / (w - 1) - 0.5) * size[0]
    py = (gy / (h - 1) - 0.5) * size[1]
    c, s = np.cos(tilt), np.sin(tilt)
    v = np.stack([px, c * py, s * py], axis=1) + np.asarray(centre, np.float64)
    f = sheet(w, h)
    if flip:
        f[1::2] = f[1::2][:, [0, 2, 1]]
    return v, f


def scene(objects, T_WC=None, W=W0, H=H0, intr=INTR0, z_near=0.05, ids=None, hide=None, seed=0, shuffle_seed=None):
    """objects: [(verts, faces)] -> the dict every test takes: the packed mesh (mapregions_util.pack), the camera, random
    fp32 vertex colours."""
    m = pack(objects, shuffle_seed=shuffle_seed) if objects else {
        "verts": np.zeros((0, 3)), "faces": np.zeros((0, 3), np.int32), "vert_off": np.zeros(1, np.int64),
        "face_off": np.zeros(1, np.int64), "perm": []}
    S = len(m["face_off"]) - 1
    T_WC = look_at((0.0, 0.0, -2.0), (0.0, 0.0, 0.0), up=(0.0, -1.0, 0.0)) if T_WC is None else np.asarray(T_WC, np.float64)
    rs = np.random.RandomState(100 + seed)
    m.update(T_WC=T_WC, T_CW=world_to_camera(T_WC), cam=T_WC[:3, 3].copy(), W=W, H=H, intr=tuple(intr), z_near=z_near,
             ids=np.asarray(ids if ids is not None else [3 + 2 * s for s in range(S)], np.int32),
             hide=np.asarray(hide if hide is not None else [0] * S, np.uint8),
             colors=rs.rand(len(m["verts"]), 3).astype(np.float32))
    return m


def overhang_sheet(n=(9, 7), jitter=0.6, tilt=0.5, seed=0):
    """A jittered, tilted sheet of mixed orientations that overhangs the 70 x 45 screen on every side."""
    return scene([sheet_object(n[0], n[1], (3.6, 2.6), tilt=tilt, jitter=jitter, flip=True, seed=seed)], seed=seed)


def make_scenes():
    """name -> (scene, claims): claims names what the scene's test asserts FROM THE SPECIFICATION ALONE: "half" (at least
    half the pixels painted), "both" (a drawn face on either path), and the stats counters that must be non-zero."""
    sc = {}
    sc["dense"] = (overhang_sheet((40, 38), 0.6, 0.5, 1), ("half", "both", "no_sample"))              # 2 886 faces
    sc["coarse"] = (overhang_sheet((5, 4), 0.5, 0.3, 2), ("half", "large"))
    a = sheet_object(14, 11, (3.4, 2.4), tilt=0.45, jitter=0.4, flip=True, seed=3)
    b = sheet_object(12, 13, (3.4, 2.4), tilt=-0.4, jitter=0.4, seed=4)
    sc["interpenetrating"] = (scene([a, b], seed=3), ("half", "both"))
    big = (np.array([[-40.0, -30.0, 0.5], [50.0, -20.0, 0.0], [0.0, 60.0, -0.5]]), np.array([[0, 1, 2]]))
    sc["giant"] = (scene([big], seed=4), ("half", "large"))
    # vertices exactly on sample points and on shared edges: an orthogonal camera pose, fx = z = 2 so that a world unit
    # is one pixel and u * 256 is integral
    T = np.eye(4)
    T[:3, 3] = (0.0, 0.0, -2.0)
    x, y = sheet_xy(25, 17)
    v = np.stack([x * 3.0 - 2.0, y * 3.0 - 2.0, np.zeros(len(x))], axis=1)
    f = sheet(25, 17)
    f[1::2] = f[1::2][:, [0, 2, 1]]
    behind = (np.array([[-4.0, -4.0, 2.0], [160.0, -4.0, 2.0], [-4.0, 120.0, 2.0]]), np.array([[0, 1, 2]]))
    sc["on_samples"] = (scene([(v, f), behind], T_WC=T, intr=(2.0, 2.0, 0.0, 0.0), seed=5), ("half", "both"))
    # two identical faces (a whole sheet twice, as two objects): the lowest id wins
    d = sheet_object(6, 5, (3.6, 2.6), tilt=0.2, seed=6)
    sc["duplicate"] = (scene([d, d], seed=6), ("half", "large"))
    # per-face defects on a sheet that still covers the screen
    base = sheet_object(10, 8, (3.6, 2.6), tilt=0.3, jitter=0.3, flip=True, seed=7)
    v, f = base[0].copy(), base[1].copy()
    v[33] = (0.1, 0.1, -1.99)                                         # a corner behind z_near (the camera is at z = -2)
    sc["z_near"] = (scene([(v, f)], seed=7), ("half", "z_near"))
    v = base[0].copy()
    v[34] = (1.0e7, 0.0, 0.0)                                         # a corner far outside the coordinate bound
    sc["bound"] = (scene([(v, f)], seed=8), ("half", "bound"))
    f2 = np.concatenate([f, [[3, 3, 14], [5, 16, 27]]])               # a repeated corner, and one more ordinary face
    sc["zero_area"] = (scene([(base[0], f2)], seed=9), ("half", "degenerate"))
    v = base[0].copy()
    v[35] = (np.nan, 0.0, 0.0)
    sc["nan"] = (scene([(v, f)], seed=10), ("half", "z_near"))
    hid = sheet_object(4, 4, (3.0, 2.0), centre=(0.0, 0.0, -0.8), seed=11)
    sc["hidden"] = (scene([base, hid], hide=[0, 1], seed=11), ("half", "hidden"))
    sc["empty"] = (scene([], seed=12), ())
    away = look_at((0.0, 0.0, -2.0), (0.0, 0.0, -5.0), up=(0.0, -1.0, 0.0))
    sc["sees_nothing"] = (scene([base], T_WC=away, seed=13), ("z_near",))
    return sc


def bad_index_scene():
    """The `coarse` scene with two faces appended whose ids lie outside [0, V)."""
    m, _ = make_scenes()["coarse"]
    m = dict(m)
    V = len(m["verts"])
    m["faces"] = np.concatenate([m["faces"], np.array([[0, 1, V], [-1, 2, 3]], np.int32)])
    m["face_off"] = m["face_off"].copy()
    m["face_off"][-1] += 2
    return m


def permuted(m, seed=5):
    """The same scene with the faces of every object in another order."""
    out = dict(m)
    rs = np.random.RandomState(seed)
    f = m["faces"].copy()
    for s in range(len(m["face_off"]) - 1):
        a, b = int(m["face_off"][s]), int(m["face_off"][s + 1])
        f[a:b] = f[a:b][rs.permutation(b - a)]
    out["faces"] = f
    return out


def reversed_faces(m):
    out = dict(m)
    out["faces"] = np.ascontiguousarray(m["faces"][:, [0, 2, 1]])
    return out


def run_spec(m, small=SMALL_DEFAULT, shading=True, ambient=0.35, background=(255, 255, 255)):
    """The whole specification on a scene -> resolve()'s dict plus key (uint64 [W, H]), stats, status."""
    key, stats, status = visibility(m, m["T_CW"], m["intr"], m["W"], m["H"], m["z_near"], m["hide"], small)
    out = resolve(m, key, m["T_CW"], m["intr"], m["W"], m["H"], m["z_near"], m["ids"], m["colors"], m["cam"], ambient, shading,
                  background)
    out.update(key=key_array(key), stats=np.array(stats, np.int64), status=status)
    return out
