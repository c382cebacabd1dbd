"""Compact part-level feature maps on the GPU: the index and densify kernels (objnerf_partmap.hip) against numpy, the
builder end to end against the reference's saved arrays (fixture G17), the sampler's gather through the index image
against its dense gather (ABI 12), and a mapping run from compact files against the same run from dense files."""
import ctypes as C

import numpy as np
import pytest
import torch

from openobj_amd import _lib
from openobj_amd import cfg as ocfg
from openobj_amd import dataset as ods
from openobj_amd import mapping, ops
from openobj_amd import part_maps as pm
try:
    from tests import partmap_util as PU
    from tests import scene_files as SF
except ImportError:          # plain `pytest tests/` puts tests/ itself, not the repository root, on sys.path
    import partmap_util as PU
    import scene_files as SF

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ the two kernels
@pytest.mark.parametrize("Hp,Wp", [(3, 5), (136, 240)])
@pytest.mark.parametrize("M", [0, 1, 65])
def test_part_index_equals_the_mask_loop(dev, M, Hp, Wp):
    rs = np.random.RandomState(100 * M + Hp)
    masks = rs.rand(M, Hp, Wp) < 0.03                   # sparse: most pixels are decided far down the scan, many by none
    if M:
        masks[0, 0, 0] = True                           # the first mask, seen last by the scan
        masks[:, -1, -1] = False                        # a pixel no mask covers
        masks[M - 1, Hp // 2, :] = True
    want = PU.last_mask(masks)
    got = ops.part_index(torch.from_numpy(masks.view(np.uint8)).to(dev))
    assert got.dtype == torch.int32 and tuple(got.shape) == (Hp, Wp)
    assert np.array_equal(got.cpu().numpy(), want)
    assert int(got[-1, -1]) == -1 and (M == 0 or int(got[Hp // 2, 0]) == M - 1)


@pytest.mark.parametrize("C_", [512, 6])
def test_part_dense_equals_table_lookup(dev, C_):
    """table[index], bit for bit: 16-byte lanes (C = 512) and scalar lanes (C = 6); index values outside the table are
    clamped into it.  The C = 512 table that starts 4 bytes off a 16-byte boundary shows that such a table gives the
    same bytes; it cannot show WHICH lanes copied it, because this GPU also executes unaligned 16-byte loads."""
    rs = np.random.RandomState(C_)
    rows, n = 37, 1000                                  # 250 blocks of four waves
    table = torch.from_numpy(rs.randn(rows + 1, C_).astype(np.float32)).to(dev)
    index = torch.from_numpy(rs.randint(0, rows, (n,)).astype(np.int32)).to(dev)
    index[0], index[-1] = 0, rows - 1
    for tab in (table[:rows], table.reshape(-1)[1:1 + rows * C_].reshape(rows, C_)):       # the second: 4 bytes off
        got = ops.part_dense(index, tab)
        assert got.shape == (n, C_) and torch.equal(got, tab.contiguous()[index.long()])
    bad = index.clone()
    bad[1], bad[2] = -7, rows + 5
    got = ops.part_dense(bad.reshape(10, 100), table[:rows])
    assert got.shape == (10, 100, C_)
    assert torch.equal(got.reshape(n, C_), table[:rows][bad.long().clamp(0, rows - 1)])


@pytest.mark.parametrize("tag", ["fp32", "fp16"])
def test_kernels_reproduce_g17(golden, dev, tag):
    g = golden("g17_partmap")
    frame = {"segmentation": g["segmentation"], "stability_score": g["stability_score"], "feat": g["feat_" + tag]}
    index, table, dense = pm.build_frame(frame, int(g["down_sample"]), dev, dense=True)
    assert dense.dtype == np.float32 and np.array_equal(dense, g["dense_" + tag])
    i2, t2 = PU.compact_of(g["segmentation"][:, ::5, ::5], g["feat_" + tag], g["stability_score"])
    assert index.dtype == np.int16 and np.array_equal(index, i2) and np.array_equal(table, t2)


def test_builder_command_line(golden, dev, tmp_path):
    """python -m openobj_amd.part_maps on the G17 inputs: --dense writes the reference's .npy, the .npz holds the same
    map; a file with the masks already on the stride, and one without masks, work too."""
    g = golden("g17_partmap")
    src, out = tmp_path / "masks", tmp_path / "out"
    src.mkdir()
    common = dict(stability_score=g["stability_score"], bbox=g["bbox"], predicted_iou=g["predicted_iou"])
    np.savez(str(src / "0.npz"), segmentation=g["segmentation"], feat=g["feat_fp32"], **common)
    np.savez(str(src / "10.npz"), segmentation_strided=g["segmentation"][:, ::5, ::5], feat=g["feat_fp16"], **common)
    np.savez(str(src / "20.npz"), segmentation=np.zeros((0, 40, 60), bool), feat=np.zeros((0, 16), np.float32),
             stability_score=np.zeros(0))
    assert pm.main(["--masks-dir", str(src), "--output-dir", str(out), "--down-sample", "5", "--dense",
                    "--device", str(dev)]) == 3
    for stem, tag in (("0", "fp32"), ("10", "fp16")):
        want = g["dense_" + tag]
        got = np.load(str(out / (stem + ".npy")))
        assert got.dtype == np.float32 and np.array_equal(got, want)
        index, table = pm.load_compact(str(out / (stem + ".npz")))
        assert table.shape == (4, 16) and np.array_equal(pm.densify_host(index, table), want)
    index, table = pm.load_compact(str(out / "20.npz"))
    assert (index == -1).all() and table.shape == (0, 16) and not np.load(str(out / "20.npy")).any()
    np.savez(str(src / "30.npz"), segmentation=np.zeros((1, 41, 60), bool), feat=np.zeros((1, 16), np.float32),
             stability_score=np.ones(1))
    with pytest.raises(ValueError):
        pm.main(["--masks-dir", str(src), "--output-dir", str(out), "--down-sample", "5", "--device", str(dev)])


# ------------------------------------------------------------------ the sampler: indexed gather == dense gather
W_, H_, PD, F_, K_ = 20, 15, 5, 3, 2
USE_FRAME = np.array([[0.0, 10, 10], [10, 0, 10]])         # dataset frame of every keyframe slot, per object
KF_IDS = [[0, 1, 2], [1, 2, 0]]
STRIDE = 10


def _gather_setup(dev, C_, n_px, seed):
    """Two objects with three keyframe slots over two part frames whose tables differ in size (3 and 5 rows)."""
    rs = np.random.RandomState(seed)
    gen = torch.Generator().manual_seed(seed)
    stores = []
    for _ in range(K_):
        rgbs = torch.randint(0, 255, (F_, W_, H_, 4), dtype=torch.uint8, generator=gen).to(dev)
        depth = (1.0 + 2.0 * torch.rand(F_, W_, H_, generator=gen)).to(dev)
        t_wc = torch.eye(4).repeat(F_, 1, 1).to(dev)
        bbox = torch.tensor([[0.0, W_, 0.0, H_]]).repeat(F_, 1).to(dev)
        stores.append((rgbs, depth, t_wc, bbox))
    store, dense = pm.PartStore(dev), []
    pw, ph = W_ // PD, H_ // PD
    for m in (3, 5):
        idx = torch.from_numpy(rs.randint(0, m + 1, (pw, ph)).astype(np.int32))
        tab = torch.cat([torch.zeros(1, C_), torch.from_numpy(rs.randn(m, C_).astype(np.float32))])
        if m == 3:
            idx[0, 0] = 0                               # frame 0, pixel (0, 0): no mask
        else:
            idx[pw - 1, ph - 1] = m                     # frame 1, last pixel: the last row of the whole table
        store.append(idx, tab)
        dense.append(tab[idx.long()])                   # the frame's own rows: no base row involved
    dense = torch.stack(dense).to(dev)                  # global_partfeat [2, W', H', C]
    n = 3 * n_px
    S, M = 10, 9
    u_w, u_h = torch.rand(K_, 3, n_px, generator=gen), torch.rand(K_, 3, n_px, generator=gen)
    u_w[0, 0, 0], u_h[0, 0, 0] = 0.5 / W_, 0.5 / H_                       # object 0, ray 0: slot 0 = frame 0, pixel (0, 0)
    u_w[0, 2, -1], u_h[0, 2, -1] = (W_ - 0.5) / W_, (H_ - 0.5) / H_       # its last ray: slot 2 = frame 1, last pixel
    draws = dict(kf_ids=torch.tensor(KF_IDS, dtype=torch.int64), u_w=u_w, u_h=u_h,
                 u=torch.rand(K_, n, S, generator=gen), g=0.03 * torch.randn(K_, n, M, generator=gen))
    draws = {k: v.to(dev) for k, v in draws.items()}
    cache = ops.rays_dirs(W_, H_, 18.0, 18.0, 9.5, 7.0, dev)
    return stores, store, dense, draws, cache


@pytest.mark.parametrize("n_px", [4, 100])                 # 12 rays; 300 rays: across the 256-ray block
@pytest.mark.parametrize("C_", [512, 6])
def test_indexed_gather_equals_dense_gather(dev, C_, n_px):
    stores, store, dense, d, cache = _gather_setup(dev, C_, n_px, seed=7 * C_ + n_px)
    assert store.table.shape == (9, C_) and int(store.index.max()) == 8
    args = (1, 9, 0.1, 0.05)
    names = ["rgb", "depth", "valid", "labels", "pts", "z", "partfeat"]
    table = ops.keyframe_table(stores)
    stacked = {}
    for form, src in (("dense", dense), ("indexed", store)):
        stacked[form] = ops.sample_rays_stacked(table, F_, W_, H_, cache, d["kf_ids"], d["u_w"], d["u_h"], d["u"], d["g"],
                                                *args, partfeat=(src, USE_FRAME, STRIDE, PD))
    for name, a, b in zip(names, stacked["dense"], stacked["indexed"]):
        assert torch.equal(a, b), name
    pf = stacked["indexed"][6]
    assert pf.shape == (K_, 3 * n_px, C_) and pf.abs().sum() > 0
    assert not pf[0, 0].any()                                        # the uncovered pixel: the zero row
    assert torch.equal(pf[0, -1], store.table[-1]) and pf[0, -1].any()   # the last row of the table
    for k in range(K_):                                              # per object, both forms, against the stacked call
        for src in (dense, store):
            one = ops.sample_rays(*stores[k], cache, d["kf_ids"][k], d["u_w"][k], d["u_h"][k], d["u"][k], d["g"][k],
                                  *args, partfeat=(src, USE_FRAME[k], STRIDE, PD))
            for name, a, b in zip(names, stacked["dense"], one):
                assert torch.equal(a[k].reshape(-1), b.reshape(-1).to(a.dtype)), (k, name)


def test_sampler_refuses_bad_part_stores(dev, monkeypatch):
    stores, store, dense, d, cache = _gather_setup(dev, 6, 4, seed=1)
    call = lambda src, uf=USE_FRAME[0]: ops.sample_rays(*stores[0], cache, d["kf_ids"][0], d["u_w"][0], d["u_h"][0],
                                                        d["u"][0], d["g"][0], 1, 9, 0.1, 0.05,
                                                        partfeat=(src, uf, STRIDE, PD))
    with pytest.raises(IndexError):
        call(store, np.array([0, 10, 20]))                 # frame 2 of a store that holds two
    with pytest.raises(IndexError):
        call(pm.PartStore(dev))                            # an empty store
    wrong = pm.PartStore(dev)
    wrong.index, wrong.table = store.index.long(), store.table
    with pytest.raises(_lib.ObjnerfError):
        call(wrong)
    wrong.index, wrong.table = store.index, store.table.reshape(3, 3, 6)
    with pytest.raises(_lib.ObjnerfError):
        call(wrong)
    # the library's own check: part_index set with pf_rows <= 0 is refused before any launch
    real = _lib.lib()

    class ZeroRows:
        def __getattr__(self, name):
            return getattr(real, name)

        def objnerf_sample_rays(self, a, stream):
            assert a._obj.part_index and a._obj.pf_rows == 9
            a._obj.pf_rows = 0
            return real.objnerf_sample_rays(a, stream)

    monkeypatch.setattr(ops, "lib", lambda: ZeroRows())
    with pytest.raises(_lib.ObjnerfError):
        call(store)


def test_kernel_entries_refuse_bad_arguments(dev):
    l = _lib.lib()
    masks = torch.zeros(2, 3, 5, dtype=torch.uint8, device=dev)
    out = torch.full((3, 5), 7, dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert l.objnerf_part_index(2, 3, 5, None, p(out), None) == -22
    assert l.objnerf_part_index(2, 3, 5, p(masks), None, None) == -22
    assert l.objnerf_part_index(-1, 3, 5, p(masks), p(out), None) == -22
    assert l.objnerf_part_index(2, 0, 5, p(masks), p(out), None) == -22
    table = torch.ones(4, 6, device=dev)
    index = torch.zeros(15, dtype=torch.int32, device=dev)
    dense = torch.full((15, 6), 7.0, device=dev)
    assert l.objnerf_part_dense(15, 6, 4, None, p(table), p(dense), None) == -22
    assert l.objnerf_part_dense(15, 6, 4, p(index), None, p(dense), None) == -22
    assert l.objnerf_part_dense(15, 6, 4, p(index), p(table), None, None) == -22
    assert l.objnerf_part_dense(15, 6, 0, p(index), p(table), p(dense), None) == -22
    assert l.objnerf_part_dense(0, 6, 4, p(index), p(table), p(dense), None) == -22
    assert l.objnerf_part_dense(15, 0, 4, p(index), p(table), p(dense), None) == -22
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((dense == 7.0).all())          # nothing was launched
    with pytest.raises(_lib.ObjnerfError):
        ops.part_index(masks.reshape(6, 5))
    with pytest.raises(_lib.ObjnerfError):
        ops.part_dense(index.long(), table)
    with pytest.raises(_lib.ObjnerfError):
        ops.part_dense(index, table.reshape(-1))


# ------------------------------------------------------------------ mapping from compact files == from dense files
def test_mapping_from_compact_files_equals_dense(dev, tmp_path, monkeypatch):
    """The same scene with its part maps once as dense .npy and once as compact .npz (the same synthetic masks), three
    frames of ten iterations under the same seed: identical object and background parameters; the compact run never
    holds a dense map.  (The samplers key their Philox draws on the seed AND on a per-process call counter, so both
    runs start from the same seed and the same counter.)"""
    over = {"dataset.format": "Replica", "trainer.part_mode": 1, "trainer.part_down": 4, "camera.w": SF.W,
            "camera.h": SF.H, "camera.fx": SF.FX, "camera.fy": SF.FY, "camera.cx": SF.CX, "camera.cy": SF.CY,
            "render.iters_per_frame": 10, "render.n_per_optim_bg": 240, "render.depth_range": [0.0, 8.0]}
    runs = {}
    for form in ("dense", "compact"):
        root = tmp_path / form
        SF.write_scene(str(root), "Replica", n_frames=30)
        PU.write_part_files(str(root), [0, 10, 20], SF.H, SF.W, 4, 512, form, seed=11)
        c = ocfg.Config(ocfg.replica_room0_config(train_device=str(dev), **dict(over, **{"dataset.path": str(root)})))
        torch.manual_seed(1234)
        monkeypatch.setattr(ops, "_draw_offset", [0])
        m = mapping.IncrementalMapper(c)
        hist = []
        m.run(ods.init_loader(c, multi_worker=False), n_frames=3, on_frame=lambda f, l: hist.append(l))
        torch.cuda.synchronize()
        runs[form] = (m, hist)
    md, mc = runs["dense"][0], runs["compact"][0]
    assert md.part_store is None and md.global_partfeat.shape == (3, SF.W // 4, SF.H // 4, 512)
    assert mc.global_partfeat is None and mc.part_store.index.shape == (3, SF.W // 4, SF.H // 4)
    assert mc.part_store.table.shape[1] == 512 and mc.part_store.nbytes() < md.global_partfeat.numel() * 4 // 10
    assert torch.equal(mc.part_store.dense(), md.global_partfeat)
    assert list(md.obj_dict) == list(mc.obj_dict) == [4, 7]
    assert torch.equal(md.loop.arena.params, mc.loop.arena.params)
    assert torch.equal(md.scene_bg.trainer.arena.params, mc.scene_bg.trainer.arena.params)
    for h in runs["compact"][1]:
        t = torch.stack(h["obj"])
        assert torch.isfinite(t).all() and (t[:, :, 3] > 0).all()        # the feature term is active
    # one run holds one form
    s = ods.Replica(ocfg.Config(ocfg.replica_room0_config(train_device=str(dev), **dict(
        over, **{"dataset.path": str(tmp_path / "dense")}))))[0]
    with pytest.raises(ValueError):
        mc.ingest(s, 3)
