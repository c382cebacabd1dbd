"""The specification of objnerf_view_compare in torch on the CPU, written from the comment of its declaration in
include/objnerf_hip.h: integer taps, integer moments (int64), one fixed sequence of fp64 operations, integer tables.
Also the canonical float-tap fp64 SSIM of Wang et al. that the integer taps approximate."""
import numpy as np
import torch

TAPS = [67, 498, 2359, 7167, 13960, 17434, 13960, 7167, 2359, 498, 67]
C1, C2 = 6.5025, 58.5225
R = 5


def gaussian():
    """The 11 normalised fp64 taps, sigma 1.5."""
    g = np.exp(-((np.arange(11) - 5.0) ** 2) / (2.0 * 1.5 ** 2))
    return g / g.sum()


def rows_of(ids, lut, G):
    """id image -> row image (int64); G = no row: an id outside [0, n_lut) or whose lut entry is outside [0, G)."""
    ids, lut = torch.as_tensor(ids).long(), torch.as_tensor(lut).long()
    n = int(lut.shape[0])
    inside = (ids >= 0) & (ids < n)
    r = lut[ids.clamp(0, max(n - 1, 0))] if n else torch.zeros_like(ids)
    ok = inside & (r >= 0) & (r < G)
    return torch.where(ok, r, torch.full_like(r, G))


def _window_sums(a, taps):
    """a [W, H, 3] -> [W - 10, H - 10, 3]: sum over the window of taps[i] taps[j] a; first along h, then along w."""
    W, H = a.shape[0], a.shape[1]
    a1 = sum(taps[k] * a[:, k:H - 10 + k] for k in range(11))
    return sum(taps[k] * a1[k:W - 10 + k] for k in range(11))


def integer_ssim(x, y):
    """x, y uint8 [W, H, 3] -> (q int64 [W, H], value fp64 [W, H]): 0 / NaN outside the interior."""
    W, H = int(x.shape[0]), int(x.shape[1])
    q = torch.zeros(W, H, dtype=torch.int64)
    value = torch.full((W, H), float("nan"), dtype=torch.float64)
    if W < 11 or H < 11:
        return q, value
    xi, yi = torch.as_tensor(x).long(), torch.as_tensor(y).long()
    Mx, My = _window_sums(xi, TAPS), _window_sums(yi, TAPS)
    Mxx, Myy, Mxy = _window_sums(xi * xi, TAPS), _window_sums(yi * yi, TAPS), _window_sums(xi * yi, TAPS)
    assert int(Mxx.max()) < 2 ** 48
    S = 2.0 ** -32
    mx, my, exx, eyy, exy = (m.double() * S for m in (Mx, My, Mxx, Myy, Mxy))
    mxmx, mymy, mxmy = mx * mx, my * my, mx * my
    vx, vy, cv = exx - mxmx, eyy - mymy, exy - mxmy
    a1, a2 = (2.0 * mxmy) + C1, (2.0 * cv) + C2
    b1, b2 = (mxmx + mymy) + C1, (vx + vy) + C2
    s = (a1 * a2) / (b1 * b2)
    v = ((s[..., 0] + s[..., 1]) + s[..., 2]) / 3.0
    value[R:W - R, R:H - R] = v
    q[R:W - R, R:H - R] = torch.floor(v * 4294967296.0).long()
    return q, value


def float_ssim(x, y):
    """The canonical definition in fp64 with the normalised Gaussian taps: per-pixel mean over channels [W - 10, H - 10]."""
    g = [float(v) for v in gaussian()]
    xd, yd = torch.as_tensor(x).double(), torch.as_tensor(y).double()
    mx, my = _window_sums(xd, g), _window_sums(yd, g)
    vx = _window_sums(xd * xd, g) - mx * mx
    vy = _window_sums(yd * yd, g) - my * my
    cv = _window_sums(xd * yd, g) - mx * my
    s = ((2 * mx * my + C1) * (2 * cv + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))
    return s.mean(-1)


def compare(rgb_r, depth_r, id_r, painted, rgb_g, depth_g, id_g, lut, G):
    """-> dict(acc int64 [G + 1, 9], conf int64 [G, G + 1], q int64 [W, H], value fp64 [W, H]) of ONE frame."""
    rgb_r, rgb_g = torch.as_tensor(rgb_r), torch.as_tensor(rgb_g)
    W, H = int(rgb_r.shape[0]), int(rgb_r.shape[1])
    depth_r, depth_g = torch.as_tensor(depth_r).float(), torch.as_tensor(depth_g).float()
    pt = torch.ones(W, H, dtype=torch.bool) if painted is None else torch.as_tensor(painted) != 0
    d = rgb_r.long() - rgb_g.long()
    se = (d * d).sum(-1)
    f4 = depth_g > 0
    f5 = f4 & (depth_r < 100)
    e = (depth_r - depth_g).abs().clamp(max=4194304.0)              # one fp32 subtraction
    dq = torch.where(f5, torch.floor(e.double() * 1048576.0), torch.zeros((), dtype=torch.float64)).long()
    q, value = integer_ssim(rgb_r, rgb_g)
    interior = torch.zeros(W, H, dtype=torch.bool)
    if W >= 11 and H >= 11:
        interior[R:W - R, R:H - R] = True
    rg, rp = rows_of(id_g, lut, G), rows_of(id_r, lut, G)
    cols = [torch.ones(W, H, dtype=torch.int64), pt.long(), se, se * pt.long(), f4.long(), f5.long(), dq,
            interior.long(), q]
    acc = torch.zeros(G + 1, 9, dtype=torch.int64)
    for c, v in enumerate(cols):
        acc[:, c].index_add_(0, rg.reshape(-1), v.reshape(-1))
    keep = rg < G
    conf = torch.bincount(rg[keep] * (G + 1) + rp[keep], minlength=G * (G + 1)).reshape(G, G + 1)
    return {"acc": acc, "conf": conf, "q": q, "value": value}


def images(W, H, kind, seed=0):
    """A pair of uint8 [W, H, 3] images: 'smooth' (a gradient plus a slow wave against a shifted copy), 'noisy'
    (smooth plus seeded noise), 'noise' (independent noise), 'inverted', 'constant', 'extreme' (0 against 255),
    'identical'."""
    g = torch.Generator().manual_seed(seed)
    w = torch.arange(W, dtype=torch.float64)[:, None, None]
    h = torch.arange(H, dtype=torch.float64)[None, :, None]
    c = torch.arange(3, dtype=torch.float64)[None, None, :]
    base = 128 + 60 * torch.sin(w / 7.0 + c) + 50 * torch.cos(h / 5.0 - c) + (w + h) * (40.0 / max(W + H, 1))
    u8 = lambda t: t.round().clamp(0, 255).to(torch.uint8)
    if kind == "smooth":
        return u8(base), u8(base * 0.9 + 10)
    if kind == "noisy":
        return u8(base), u8(base + 25 * torch.randn(W, H, 3, generator=g, dtype=torch.float64))
    if kind == "noise":
        return (torch.randint(0, 256, (W, H, 3), generator=g, dtype=torch.uint8),
                torch.randint(0, 256, (W, H, 3), generator=g, dtype=torch.uint8))
    if kind == "inverted":
        x = u8(base + 25 * torch.randn(W, H, 3, generator=g, dtype=torch.float64))
        return x, 255 - x
    if kind == "constant":
        return torch.full((W, H, 3), 90, dtype=torch.uint8), torch.full((W, H, 3), 140, dtype=torch.uint8)
    if kind == "extreme":
        return torch.zeros(W, H, 3, dtype=torch.uint8), torch.full((W, H, 3), 255, dtype=torch.uint8)
    if kind == "identical":
        x = u8(base + 25 * torch.randn(W, H, 3, generator=g, dtype=torch.float64))
        return x, x.clone()
    raise ValueError(kind)


def depths(W, H, seed=0):
    """(depth_r, depth_g) fp32 [W, H] with depth_g == 0, depth_r == 100 and both together on bands of the image."""
    g = torch.Generator().manual_seed(seed + 1000)
    dg = 0.5 + 4 * torch.rand(W, H, generator=g)
    dr = dg + 0.05 * torch.randn(W, H, generator=g)
    dg[::3, ::4] = 0.0                     # invalid sensor depth
    dr[::4, ::3] = 100.0                   # nothing wrote depth (meets dg == 0 at multiples of 12)
    return dr.float().contiguous(), dg.float().contiguous()


def id_images(W, H, values, seed=0, block=3):
    """(id_r, id_g) int32 [W, H]: blocks of `block` pixels drawn from `values`, independently for the two sides."""
    g = torch.Generator().manual_seed(seed + 2000)
    vals = torch.as_tensor(values, dtype=torch.int32)

    def one():
        bw, bh = -(-W // block), -(-H // block)
        pick = torch.randint(0, len(vals), (bw, bh), generator=g)
        return vals[pick].repeat_interleave(block, 0).repeat_interleave(block, 1)[:W, :H].contiguous()

    return one(), one()
