"""numpy restatements of objnerf_mapeval.hip (include/objnerf_hip.h): brute-force nearest points in the fixed operation
order, the mesh sampler with Python-integer prefix and mulhi, and the metrics of openobj_amd/map_eval.py."""
import numpy as np

S_MESH = 8                  # objnerf_philox.h Stream


def philox4x32_10(ctr, k0, k1):
    """ctr: uint32 [..., 4]; Salmon et al. 2011, 10 rounds."""
    M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
    x, y, z, w = [ctr[..., i].astype(np.uint64) for i in range(4)]
    k0, k1 = np.uint64(k0), np.uint64(k1)
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * x, np.uint64(M1) * z
        x, y, z, w = ((p1 >> np.uint64(32)) ^ y ^ k0) & mask, p1 & mask, ((p0 >> np.uint64(32)) ^ w ^ k1) & mask, p0 & mask
        k0, k1 = (k0 + np.uint64(W0)) & mask, (k1 + np.uint64(W1)) & mask
    return np.stack([x, y, z, w], axis=-1).astype(np.uint32)


def u01(x):
    return (x >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


# ------------------------------------------------------------------------------------------------------------ nearest
def nearest_ref(qry, q_off, ref, r_off, chunk=2048):
    """-> (d2 fp64 [nq], idx int64 [nq]): per segment the minimum of (dx dx + dy dy) + dz dz and the smallest row of ref
    that attains it (np.argmin returns the first); +inf and -1 for an empty reference segment."""
    qry, ref = np.asarray(qry, np.float64).reshape(-1, 3), np.asarray(ref, np.float64).reshape(-1, 3)
    d2 = np.full(len(qry), np.inf)
    idx = np.full(len(qry), -1, np.int64)
    for s in range(len(q_off) - 1):
        r0, r1 = int(r_off[s]), int(r_off[s + 1])
        if r1 == r0:
            continue
        R = ref[r0:r1]
        for a in range(int(q_off[s]), int(q_off[s + 1]), chunk):
            b = min(a + chunk, int(q_off[s + 1]))
            d = R[None, :, :] - qry[a:b, None, :]
            m = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            j = np.argmin(m, axis=1)
            d2[a:b] = m[np.arange(b - a), j]
            idx[a:b] = j + r0
    return d2, idx


def unique_minimum(qry, q_off, ref, r_off, d2, chunk=2048):
    """bool [nq]: exactly one reference row attains d2."""
    out = np.zeros(len(qry), bool)
    for s in range(len(q_off) - 1):
        R = ref[int(r_off[s]):int(r_off[s + 1])]
        for a in range(int(q_off[s]), int(q_off[s + 1]), chunk):
            b = min(a + chunk, int(q_off[s + 1]))
            d = R[None, :, :] - qry[a:b, None, :]
            m = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            out[a:b] = (m == d2[a:b, None]).sum(axis=1) == 1
    return out


# ------------------------------------------------------------------------------------------------------------ sampler
def face_weights(verts, faces):
    """-> (area fp64 [F], q list of Python ints) of one segment's faces."""
    A, B, C = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    e1, e2 = B - A, C - A
    cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    area = 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)
    amax = area.max() if len(area) else 0.0
    if not amax > 0.0:
        return area, [0] * len(area)
    return area, [int(v) for v in np.floor(area / amax * 4294967296.0)]


def mesh_sample_ref(verts, faces, face_off, samp_off, seed):
    """-> (pts fp64 [N, 3], tri int32 [N]); raises ValueError for a segment that asks for samples without area."""
    verts, faces = np.asarray(verts, np.float64), np.asarray(faces, np.int64)
    N = int(samp_off[-1])
    pts, tri = np.zeros((N, 3)), np.zeros(N, np.int32)
    for s in range(len(face_off) - 1):
        f0, f1, s0, s1 = int(face_off[s]), int(face_off[s + 1]), int(samp_off[s]), int(samp_off[s + 1])
        if s1 == s0:
            continue
        _, q = face_weights(verts, faces[f0:f1])
        prefix = [0]
        for v in q:
            prefix.append(prefix[-1] + v)                    # Python integers: exact
        W = prefix[-1]
        if W == 0:
            raise ValueError("no area")
        n = s1 - s0
        ctr = np.stack([np.full(n, s, np.uint32), np.arange(n, dtype=np.uint32), np.zeros(n, np.uint32),
                        np.full(n, S_MESH, np.uint32)], axis=-1)
        r = philox4x32_10(ctr, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
        t = np.array([(((int(x) << 32) | int(y)) * W) >> 64 for x, y in zip(r[:, 0], r[:, 1])], np.uint64)
        k = np.searchsorted(np.array(prefix[:-1], np.uint64), t, side="right") - 1       # prefix[k] <= t < prefix[k + 1]
        fc = faces[f0:f1][k]
        A, B, C = verts[fc[:, 0]], verts[fc[:, 1]], verts[fc[:, 2]]
        u1, u2 = u01(r[:, 2]).astype(np.float64), u01(r[:, 3]).astype(np.float64)
        sq = np.sqrt(u1)
        wa, wb, wc = (1.0 - sq)[:, None], (sq * (1.0 - u2))[:, None], (sq * u2)[:, None]
        pts[s0:s1] = (wa * A + wb * B) + wc * C
        tri[s0:s1] = k + f0
    return pts, tri


# ------------------------------------------------------------------------------------------------------------ metrics
def metrics_ref(d_acc, d_comp, thresholds):
    d_acc, d_comp = np.asarray(d_acc, np.float64), np.asarray(d_comp, np.float64)
    fa, fc = d_acc[np.isfinite(d_acc)], d_comp[np.isfinite(d_comp)]
    a = float(np.mean(fa)) if fa.size else None
    c = float(np.mean(fc)) if fc.size else None
    out = {"accuracy": a, "completion": c, "chamfer": None if a is None or c is None else 0.5 * (a + c),
           "n_pred": int(d_acc.size), "n_gt": int(d_comp.size)}
    for t in thresholds:
        out[f"completion_ratio@{t:g}"] = float(np.count_nonzero(fc < t) / d_comp.size) if d_comp.size else None
    return out
