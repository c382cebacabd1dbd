"""The specification of the part regions (include/objnerf_hip.h), free of the code under test: plain Python
union-find over the face list, the integer table in Python integers from numpy fp64 (every operation of the per-face
sequence is one element-wise numpy call, so it rounds once, as on the device), and a deliberately naive float path for
the sanity bounds.  Test infrastructure only; openobj_amd never imports it."""
import numpy as np

ROW = 32
C_ROOT, C_OBJ, C_NV, C_NF, C_AREA, C_M1, C_NRM, C_MIN, C_MAX, C_PEAK, C_CEN, C_M2 = 0, 1, 2, 3, 4, 5, 8, 11, 14, 17, 18, 21
C_RES = 27
SCALE = np.float64(2.0 ** 44)
LIMIT = np.float64(2.0 ** 62)


# ------------------------------------------------------------------------------------------------------ mesh builders
def sheet(w, h):
    """A w x h vertex sheet (vertex y * w + x), two triangles a cell: (v00, v10, v11), (v00, v11, v01).  The diagonal joins
    (x, y) and (x + 1, y + 1).  -> faces int64 [2 (w - 1)(h - 1), 3] in cell order."""
    f = []
    for y in range(h - 1):
        for x in range(w - 1):
            v = y * w + x
            f += [(v, v + 1, v + w + 1), (v, v + w + 1, v + w)]
    return np.array(f, np.int64).reshape(-1, 3)


def sheet_xy(w, h):
    i = np.arange(w * h)
    return i % w, i // w


def spiral(w, h):
    """bool [h, w]: a one-vertex-wide spiral from (0, 0) inwards whose arms stay at least two apart (so not even the
    diagonal joins two arms): one region that crosses the whole sheet.  A walker goes straight while the next vertex is
    free and the one after it is not part of the path, else it turns right; it stops when it can do neither."""
    m = np.zeros((h, w), bool)
    x, y, dx, dy = 0, 0, 1, 0
    m[0, 0] = True
    inside = lambda i, j: 0 <= i < w and 0 <= j < h
    while True:
        for _ in range(2):
            nx, ny, ax, ay = x + dx, y + dy, x + 2 * dx, y + 2 * dy
            if inside(nx, ny) and not m[ny, nx] and not (inside(ax, ay) and m[ay, ax]):
                x, y = nx, ny
                m[y, x] = True
                break
            dx, dy = -dy, dx
        else:
            return m


def pack(objects, permute_seed=None, shuffle_seed=None):
    """objects: [(verts [n, 3] fp64, faces [f, 3] local ids)] -> dict(verts fp64 [V, 3], faces int32 [F, 3] of packed ids,
    vert_off, face_off int64 [S + 1], perm: per object the new local id of every old one).  permute_seed: a random
    permutation of every object's vertex ids (the root is then not the geometric first vertex); shuffle_seed: a random
    order of every object's faces."""
    vs, fs, voff, foff, perms = [], [], [0], [0], []
    rs_p = np.random.RandomState(permute_seed) if permute_seed is not None else None
    rs_f = np.random.RandomState(shuffle_seed) if shuffle_seed is not None else None
    for v, f in objects:
        v, f = np.asarray(v, np.float64).reshape(-1, 3), np.asarray(f, np.int64).reshape(-1, 3)
        n = len(v)
        perm = rs_p.permutation(n) if rs_p is not None else np.arange(n)
        nv = np.empty_like(v)
        nv[perm] = v
        f = perm[f] if len(f) else f
        if rs_f is not None and len(f):
            f = f[rs_f.permutation(len(f))]
        vs.append(nv)
        fs.append(f + voff[-1])
        perms.append(perm)
        voff.append(voff[-1] + n)
        foff.append(foff[-1] + len(f))
    return {"verts": np.concatenate(vs), "faces": np.concatenate(fs).astype(np.int32).reshape(-1, 3),
            "vert_off": np.array(voff, np.int64), "face_off": np.array(foff, np.int64), "perm": perms}


def per_vertex(m, values):
    """values: per object an array over the ORIGINAL vertex order -> one packed array in the map's (permuted) order."""
    out = []
    for perm, v in zip(m["perm"], values):
        v = np.asarray(v)
        o = np.empty_like(v)
        o[perm] = v
        out.append(o)
    return np.concatenate(out)


# ------------------------------------------------------------------------------------------------------ specification
def selected(sims_col, thr, vert_off):
    """sims fp32 [V], thr fp32 [S]: one fp32 compare; a NaN on either side selects nothing."""
    s = np.asarray(sims_col, np.float32)
    t = np.repeat(np.asarray(thr, np.float32), np.diff(vert_off))
    with np.errstate(invalid="ignore"):
        return s >= t


def face_object(face_off, f):
    return int(np.searchsorted(face_off, f, side="right")) - 1


def valid_faces(m):
    """-> (ok bool [F], status): bit 0 an id outside [0, V), bit 1 an id outside the face's own object."""
    V, faces, voff, foff = len(m["verts"]), m["faces"], m["vert_off"], m["face_off"]
    ok, status = np.ones(len(faces), bool), 0
    S = len(voff) - 1
    for f, ids in enumerate(faces):
        s = min(max(face_object(foff, f), 0), S - 1)
        if any(i < 0 or i >= V for i in ids):
            ok[f], status = False, status | 1
        elif any(i < voff[s] or i >= voff[s + 1] for i in ids):
            ok[f], status = False, status | 2
    return ok, status


def components(m, sel):
    """Plain union-find over the face list -> (root int32 [V]: the smallest packed index of the region, -1 where not
    selected; status)."""
    V = len(m["verts"])
    parent = list(range(V))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    ok, status = valid_faces(m)
    for f, ids in enumerate(m["faces"]):
        if not ok[f]:
            continue
        s = [int(i) for i in ids if sel[i]]
        for a, b in zip(s, s[1:]):
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    root = np.full(V, -1, np.int32)
    for v in range(V):
        if sel[v]:
            root[v] = find(v)
    return root, status


def rows(root, vert_off):
    """-> (reg_off int64 [S + 1], label int32 [V]): the roots in ascending order per object."""
    V = len(root)
    roots = [v for v in range(V) if root[v] == v]
    row_of = {v: i for i, v in enumerate(roots)}
    label = np.array([row_of[r] if r >= 0 else -1 for r in root], np.int32).reshape(V)
    reg_off = np.searchsorted(np.array(roots, np.int64), vert_off, side="left").astype(np.int64)
    return reg_off, label


def f32_key(x):
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return np.where(u & 0x80000000, (~u) & 0xFFFFFFFF, u | 0x80000000).astype(np.uint64)


def q44(x):
    """llrint(x 2^44) as Python integers; non-finite or |x 2^44| >= 2^62 -> 0 and bad."""
    y = np.asarray(x, np.float64) * SCALE
    with np.errstate(invalid="ignore"):
        good = np.abs(y) < LIMIT
    r = np.rint(np.where(good, y, 0.0))
    return [int(v) for v in r], bool((~good).any())


def face_terms(m, fidx):
    """The per-face fp64 sequence for the faces fidx, every line one rounding per element."""
    v, faces, voff, foff = m["verts"], m["faces"], m["vert_off"], m["face_off"]
    obj = np.searchsorted(foff, fidx, side="right") - 1
    an = v[voff[obj]]
    dA, dB, dC = v[faces[fidx, 0]] - an, v[faces[fidx, 1]] - an, v[faces[fidx, 2]] - an
    u, w = dB - dA, dC - dA
    c = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                  u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        area = 0.5 * np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
    return dA, dB, dC, c, area


def table(m, sims_col, root, label):
    """The int64 table [R, 32] of the specification (computed in Python integers) and the status bits."""
    v, faces, voff = m["verts"], m["faces"], m["vert_off"]
    V = len(v)
    R = int(label.max()) + 1 if V else 0
    T = [[0] * ROW for _ in range(R)]
    for r in range(R):
        for c in range(3):
            T[r][C_MIN + c] = 0xFFFFFFFF
    ok, status = valid_faces(m)
    keys = f32_key(v.astype(np.float32))
    skey = f32_key(np.asarray(sims_col, np.float32))
    for i in range(V):
        r = int(label[i])
        if r < 0:
            continue
        if root[i] == i:
            T[r][C_ROOT] = i
            T[r][C_OBJ] = int(np.searchsorted(voff, i, side="right")) - 1
        T[r][C_NV] += 1
        for c in range(3):
            T[r][C_MIN + c] = min(T[r][C_MIN + c], int(keys[i, c]))
            T[r][C_MAX + c] = max(T[r][C_MAX + c], int(keys[i, c]))
        T[r][C_PEAK] = max(T[r][C_PEAK], (int(skey[i]) << 32) | ((~i) & 0xFFFFFFFF))
    fidx = np.array([f for f in range(len(faces)) if ok[f] and all(label[j] >= 0 for j in faces[f])], np.int64)
    if len(fidx):
        dA, dB, dC, c, area = face_terms(m, fidx)
        frow = label[faces[fidx, 0]]
        s = (dA + dB) + dC
        cols, bad = [q44(area)], []
        cols += [q44((area * s[:, j]) / 3.0) for j in range(3)]
        cols += [q44(0.5 * c[:, j]) for j in range(3)]
        for n, r in enumerate(frow):
            T[r][C_NF] += 1
            for k, col in enumerate((C_AREA, C_M1, C_M1 + 1, C_M1 + 2, C_NRM, C_NRM + 1, C_NRM + 2)):
                T[r][col] += cols[k][0][n]
        bad = any(b for _, b in cols)
        cen = np.zeros((R, 3))
        for r in range(R):
            for j in range(3):
                a = np.float64(T[r][C_AREA])
                cen[r, j] = np.float64(T[r][C_M1 + j]) / a if a > 0 else 0.0
        ce = cen[frow]
        eA, eB, eC = dA - ce, dB - ce, dC - ce
        t = (eA + eB) + eC
        n2 = 0
        for j in range(3):
            for k in range(j, 3):
                mjk = ((eA[:, j] * eA[:, k] + eB[:, j] * eB[:, k]) + eC[:, j] * eC[:, k]) + t[:, j] * t[:, k]
                vals, b = q44((area * mjk) / 12.0)
                bad = bad or b
                for n, r in enumerate(frow):
                    T[r][C_M2 + n2] += vals[n]
                n2 += 1
        for j in range(3):
            vals, b = q44((area * t[:, j]) / 3.0)
            bad = bad or b
            for n, r in enumerate(frow):
                T[r][C_RES + j] += vals[n]
        if bad:
            status |= 4
    for r in range(R):
        a = np.float64(T[r][C_AREA])
        for j in range(3):
            T[r][C_CEN + j] = int(np.array(np.float64(T[r][C_M1 + j]) / a if a > 0 else 0.0, np.float64).view(np.int64))
    out = np.zeros((R, ROW), np.int64)
    for r in range(R):
        for c in range(ROW):
            x = T[r][c]
            out[r, c] = x - (1 << 64) if x >= (1 << 63) else x           # (the peak is an unsigned 64-bit number)
    return out, status


# ---------------------------------------------------------------------------------------------- the naive float path
def naive_regions(m, label):
    """Per region: area = sum 0.5 |cross|, centroid = sum area * mean / sum area, in world coordinates, plain numpy."""
    v, faces = m["verts"], m["faces"]
    ok, _ = valid_faces(m)
    R = int(label.max()) + 1 if len(label) else 0
    area, mom, nf = np.zeros(R), np.zeros((R, 3)), np.zeros(R, np.int64)
    for f, ids in enumerate(faces):
        if not ok[f] or any(label[j] < 0 for j in ids):
            continue
        A, B, C = v[ids[0]], v[ids[1]], v[ids[2]]
        a = 0.5 * np.linalg.norm(np.cross(B - A, C - A))
        r = label[ids[0]]
        area[r] += a
        mom[r] += a * (A + B + C) / 3.0
        nf[r] += 1
    with np.errstate(invalid="ignore", divide="ignore"):
        return area, mom / area[:, None], nf


def region_sets(root):
    """The regions as a set of frozensets of vertex ids."""
    d = {}
    for v, r in enumerate(root):
        if r >= 0:
            d.setdefault(int(r), []).append(v)
    return {frozenset(x) for x in d.values()}


# ------------------------------------------------------------------------------------- a map with two planted blobs
BLOBS = ((7.3, 6.1, 2.6), (17.6, 11.4, 1.7))        # (centre x, centre y, sigma) in cells of the planted object's sheet
PLANT_W, PLANT_H, CELL = 26, 18, 0.05


def planted_map(seed=0, H=32, C=512, Dc=64, Ds=48):
    """Two objects as query_util.synthetic_map makes them, but with sheet meshes, in the COMPACT form (part_rows [V, H + 1],
    part_head [C, H + 1]; partcompact_util.dense_of gives the dense map of the same features).  Object 1 (key 13) carries
    the part query as two Gaussian blobs: its unit feature is (b + g(v) q) / sqrt(1 + g^2) with b, q orthonormal and
    g = 2 exp(-d^2 / (2 sigma^2)) summed over the blobs, so cos(feature, q) = g / sqrt(1 + g^2): 0.894 at a centre, ~0
    far away.  Object 0 (key 10) has g = 0.05 everywhere.
    -> (all_obj, X: per object the fp64 unit features of the stored fp32 rows, q [C] fp64, info)."""
    from openobj_amd.mesh import TriMesh
    rs = np.random.RandomState(seed)
    out, Xs = {}, []
    A = rs.randn(C, H + 1) / np.sqrt(C)
    Qm, _ = np.linalg.qr(A)                                  # A = Qm Rm: orthonormal columns of the head's range
    Rm = Qm.T @ A
    rb, rq = np.linalg.solve(Rm, np.eye(H + 1)[0]), np.linalg.solve(Rm, np.eye(H + 1)[1])   # A rb = Qm[:, 0], A rq = Qm[:, 1]
    q = Qm[:, 1]
    sizes = ((12, 9), (PLANT_W, PLANT_H))
    for p, (w, h) in enumerate(sizes):
        x, y = sheet_xy(w, h)
        g = np.full(w * h, 0.05)
        if p == 1:
            g = sum(2.0 * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * s * s)) for cx, cy, s in BLOBS)
        r = (rb[None] + g[:, None] * rq[None]) / np.sqrt(1 + g * g)[:, None]
        r32, A32 = r.astype(np.float32), A.astype(np.float32)
        v = np.stack([x * CELL + 2.0 * p, y * CELL, np.zeros(w * h) + 0.4], axis=1)
        m = TriMesh(v, sheet(w, h))
        m.visual.vertex_colors = rs.randint(0, 256, (w * h, 4)).astype(np.uint8)
        base_c, base_s = rs.randn(Dc), rs.randn(Ds)
        out[10 + 3 * p] = {"clip_feat": np.stack([base_c + 0.01 * rs.randn(Dc) for _ in range(3)]),
                           "caption_feat": (base_s + 0.01 * rs.randn(Ds)).astype(np.float32), "class_id": p, "mesh": m,
                           "color": m.visual.vertex_colors, "part_rows": r32, "part_head": A32}
        Xs.append(r32.astype(np.float64) @ A32.astype(np.float64).T)
        if p == 1:
            info = {"clip_query": base_c.astype(np.float32), "sbert_query": base_s.astype(np.float32), "position": 1,
                    "key": 13, "centres": [(cx * CELL + 2.0, cy * CELL, 0.4) for cx, cy, _ in BLOBS]}
    return out, Xs, q, info
