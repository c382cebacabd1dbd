"""numpy fp64 restatement of the map-query colourings of visualization/vis_interaction.py (test infrastructure only;
openobj_amd never imports it)."""
import colorsys

import numpy as np


def rainbow_lut():
    """matplotlib's "rainbow" _lut[:256, :3]: _cm.py gfunc 33 / 13 / 10 (|2x - 0.5|, sin(pi x), cos(pi x / 2)) at
    np.linspace(0, 1, 256), clipped to [0, 1] (colors.py _create_lookup_table), fp64."""
    x = np.linspace(0, 1, 256)
    return np.clip(np.stack([np.abs(2 * x - 0.5), np.sin(x * np.pi), np.cos(x * np.pi / 2)], axis=1), 0, 1)


def rainbow(x):
    """cmap(x)[..., :3] (:332, :392) for a float32 array: x * 256 in float32, 256 -> 255, x < 0 -> entry 0,
    x * 256 >= 256 -> 255, NaN -> (0, 0, 0) (the bad colour's RGB)."""
    xa = np.array(x, np.float32) * np.float32(256)
    xa[xa == 256] = 255
    under, over, bad = xa < 0, xa >= 256, np.isnan(xa)
    with np.errstate(invalid="ignore"):
        i = xa.astype(int)
    i[under] = 0
    i[over] = 255
    i[bad] = 0
    out = rainbow_lut()[i]
    out[bad] = 0.0
    return out


def normalise(s, mn=None, mx=None):
    """(s - min) / (max - min) in float32 (torch's fp32 ops on the device, :330-331, :389-391)."""
    s = np.asarray(s, np.float32)
    mn = s.min() if mn is None else np.float32(mn)
    mx = s.max() if mx is None else np.float32(mx)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (s - mn) / (mx - mn)


def rgb_colors(color, factor):
    """np.asarray(color)[..., :-1] / 255 * factor (:299-301, :347-349), fp64."""
    return np.asarray(color)[..., :3] / 255 * factor


def cosine(q, F):
    """F.cosine_similarity(q[None], F) in fp64."""
    q = np.asarray(q, np.float64)
    F = np.asarray(F, np.float64)
    return (F / np.maximum(np.linalg.norm(F, axis=-1, keepdims=True), 1e-8)) @ (q / max(np.linalg.norm(q), 1e-8))


def object_similarity(clip_q, sbert_q, clip, caption):
    """:364-375: the queries normalised, 0.2 cos_sbert + 0.8 cos_clip."""
    return 0.2 * cosine(sbert_q, caption) + 0.8 * cosine(clip_q, clip)


def top_indices(sim, top_num):
    return list(np.argsort(-np.asarray(sim), kind="stable")[:top_num]) if top_num else []


def object_query_colors(sim, ranked, colors, top_num):
    """sim_and_update (:322-354) with the unranked objects darkened: per object [n_k, 3] fp64."""
    top = [ranked[i] for i in top_indices(sim, top_num)]
    out = [rgb_colors(c, 0.5) for c in colors]
    if top_num:
        for p in top:
            out[p] = np.tile([1.0, 0.0, 0.0], (len(colors[p]), 1))
    else:
        sc = rainbow(normalise(sim))
        for i, p in enumerate(ranked):
            out[p] = np.tile(sc[i], (len(colors[p]), 1))
    return out


def part_query_colors(part_sims, top, colors):
    """sim_and_update_part (:378-408): part_sims[p] = the per-vertex similarities of top object p (float32)."""
    out = [rgb_colors(c, 0.5) for c in colors]
    for p in top:
        out[p] = rainbow(normalise(part_sims[p]))
    return out


def pca_scores(X):
    """StandardScaler (ddof 0, zero std -> 1) + PCA(3) exact, fp64, with the u-based sign rule (the largest |score| of
    each component positive; sklearn 1.3.2's svd_flip(u_based_decision=True))."""
    X = np.asarray(X, np.float64)
    mu = X.mean(axis=0)
    sd = X.std(axis=0)
    sd[sd == 0] = 1.0
    Z = (X - mu) / sd
    _, _, Vt = np.linalg.svd(Z - Z.mean(axis=0), full_matrices=False)
    return sign_rule(Z @ Vt[:3].T)


def sign_rule(scores):
    scores = np.array(scores, np.float64)
    i = np.argmax(np.abs(scores), axis=0)
    return scores * np.sign(scores[i, np.arange(scores.shape[1])])


def pca_colors(scores):
    """:211-214: one joint min-max over the three columns, clipped to [0, 1]."""
    mn, mx = scores.min(), scores.max()
    return np.clip((scores - mn) / (mx - mn), 0, 1)


def instance_palette(n, pastel_factor=0.5):
    c = np.array([colorsys.hsv_to_rgb((i * 0.6180339887498949) % 1.0, 1.0, 1.0) for i in range(n)]).reshape(-1, 3)
    return (c + pastel_factor) / (1 + pastel_factor)


def class_colors(all_obj, mapping, mapped_colors):
    """color_by_class (:283-288)."""
    return [np.asarray(mapped_colors[mapping[o["class_id"] + 1]], np.float64) for o in all_obj.values()]


def hidden_sets(all_obj, dataset_name, scene_name):
    """:146-190."""
    ceiling, most, boxes = [], [], []
    keys = list(all_obj.keys())
    for idx, k in enumerate(keys):
        v = np.asarray(all_obj[k]["mesh"].vertices)
        height = 1
        if scene_name == "room_2":
            height = -0.5
        if scene_name == "office_0":
            height = 0.5
        if np.min(v[:, 2]) > height:
            ceiling.append(idx)
        wall_id = 93
        if dataset_name == "Scannet":
            wall_id = 1
        if scene_name == "611":
            if keys[idx] != 46:
                most.append(idx)
        elif all_obj[k]["class_id"] + 1 != wall_id:
            most.append(idx)
        boxes.append((v.min(axis=0), v.max(axis=0)))
    return ceiling, most, boxes


def synthetic_map(seed=0, sizes=(300, 1, 5, 777, 64), D=512, Dc=512, Ds=384, missing=(2,), z0=(0.2, 1.5, 0.3, 2.5, 0.0),
                  classes=(3, 92, 5, 0, 7)):
    """A small all_obj as map_vis.export writes it: unit part features around a common mean, 2-D clip / caption
    features (several views, one outlier) for most objects, none for the positions in `missing`."""
    from openobj_amd.mesh import TriMesh
    rs = np.random.RandomState(seed)
    common = rs.randn(D)
    out = {}
    for p, n in enumerate(sizes):
        v = rs.rand(n, 3) + [0, 0, z0[p]]
        f = np.arange(3 * max(n // 3, 0)).reshape(-1, 3) if n >= 3 else np.zeros((0, 3), np.int64)
        m = TriMesh(v, f)
        c = rs.randint(0, 256, (n, 4)).astype(np.uint8)
        m.visual.vertex_colors = c
        pf = (common + 0.3 * rs.randn(n, D)).astype(np.float32)
        pf /= np.linalg.norm(pf, axis=-1, keepdims=True)
        base_c, base_s = rs.randn(Dc), rs.randn(Ds)
        clip = None if p in missing else np.stack([base_c + 0.01 * rs.randn(Dc) for _ in range(4)] + [rs.randn(Dc) * 5])
        cap = None if p in missing else (base_s + 0.01 * rs.randn(Ds)).astype(np.float32)
        out[10 + 3 * p] = {"clip_feat": clip, "caption_feat": cap, "class_id": classes[p], "mesh": m,
                           "color": m.visual.vertex_colors, "part_feat": pf}
    return out
