"""CPU: the cropped keyframe store (openobj_amd/kf_store.py) -- the crop rectangle against the sampler's pixel draw, the
growth rule, the direct (torch slicing) write path replaying the reference's slot trace, and the config key."""
import numpy as np
import pytest
import torch

from conftest import T
from openobj_amd import cfg as ocfg
from openobj_amd import vmap as ovmap
from openobj_amd.kf_store import KeyframeCropStore, crop_rect, grown_cap
from test_reference_pins import _ReplayChoice, _check_trace, _map_cfg, _state_map

W, H = 48, 40

BOXES = [
    ((5.0, 20.0, 3.0, 9.0), (5, 3, 16, 7)),                 # integer
    ((3.7, 11.2, 0.4, 38.9), (3, 0, 9, 39)),                # fractional
    ((0.0, 47.0, 0.0, 39.0), (0, 0, 48, 40)),               # the whole image: touches every border
    ((30.5, 47.0, 12.25, 39.0), (30, 12, 18, 28)),          # ends at the last column and row
    ((7.0, 7.0, 9.0, 9.0), (7, 9, 1, 1)),                   # degenerate: lo == hi
    ((-2.5, 50.0, 38.2, 44.0), (0, 38, 48, 2)),             # past the image: clipped
]


@pytest.mark.parametrize("box,want", BOXES)
def test_crop_rect(box, want):
    assert crop_rect(box, W, H) == want
    assert crop_rect(torch.tensor(box), W, H) == want
    assert crop_rect(np.asarray(box, np.float32), W, H) == want


@pytest.mark.parametrize("box", [b for b, _ in BOXES[:5]])
def test_sampler_draw_lies_inside_crop_rect(box):
    """The sampler's pixel index, restated in fp32 as sample_gather_kernel computes it: fw = u * (hi - lo) + lo (each
    operation rounded to fp32, no contraction), truncated."""
    x0, y0, cw, ch = crop_rect(box, W, H)
    b = np.asarray(box, np.float32)
    rs = np.random.RandomState(7)
    u = np.concatenate([rs.random_sample(9998), [0.0, 1.0 - 2.0 ** -24]]).astype(np.float32)    # [0, 1), both ends
    assert u.max() < 1.0
    for lo, hi, r0, rn in ((b[0], b[1], x0, cw), (b[2], b[3], y0, ch)):
        f = (u * np.float32(hi - lo)).astype(np.float32) + np.float32(lo)
        i = np.trunc(f.astype(np.float32)).astype(np.int64)
        assert i.min() >= r0 and i.max() <= r0 + rn - 1


def test_growth_rule():
    assert [grown_cap(n) for n in (1, 170, 171, 256, 1000, 4096)] == [256, 256, 512, 512, 1536, 6144]
    st = KeyframeCropStore(4, W, H, "cpu")
    assert (st.cap, st.version, st.nbytes) == (0, 0, 0)
    caps = []
    for slot, (cw, ch) in enumerate([(10, 10), (12, 14), (30, 20), (5, 5)]):       # 100, 168, 600, 25 pixels
        st.reserve(slot, (1, 2, cw, ch))
        caps.append((st.cap, st.version))
    # 100 px -> ceil(150 / 256) * 256; 168 fits; 600 -> ceil(900 / 256) * 256; the arena never shrinks
    assert caps == [(256, 1), (256, 1), (1024, 2), (1024, 2)]
    assert st.nbytes == 4 * 1024 * 8 and st.arena.numel() == st.nbytes
    assert st.descriptor() == (st.arena.data_ptr(), 1024, st.rect.data_ptr(), st.t_wc.data_ptr(), st.bbox.data_ptr())
    with pytest.raises(ValueError):
        st.reserve(0, (40, 0, 10, 4))              # leaves the image
    with pytest.raises(IndexError):
        st.reserve(4, (0, 0, 2, 2))


def _frame(rs):
    return (T(rs.randint(0, 256, (W, H, 3)).astype(np.uint8)), T(rs.rand(W, H).astype(np.float32) + 0.5),
            T(rs.randint(0, 3, (W, H)).astype(np.uint8)), T(rs.randn(4, 4).astype(np.float32)))


def test_live_slots_survive_growth_bit_exactly():
    rs = np.random.RandomState(3)
    st = KeyframeCropStore(3, W, H, "cpu")
    boxes = [(4.0, 13.5, 6.0, 14.0), (20.2, 30.0, 1.0, 5.9), (0.0, 47.0, 0.0, 39.0)]      # the last forces a growth
    frames = [_frame(rs) for _ in boxes]
    seen = []
    for slot, (box, (rgb, depth, mask, twc)) in enumerate(zip(boxes, frames)):
        v = st.version
        st.write(slot, rgb, depth, mask, T(np.asarray(box, np.float32)), twc)
        seen.append(st.version)
        if slot == 2:
            assert st.version == v + 1 and st.cap == grown_cap(W * H)
    assert seen == [1, 1, 2]
    for slot, (box, (rgb, depth, mask, twc)) in enumerate(zip(boxes, frames)):
        x0, y0, cw, ch = crop_rect(box, W, H)
        assert st.rect[slot].tolist() == [x0, y0, cw, ch] == st.rect_host[slot].tolist()
        rgbs, d = st.frame(slot)
        want = torch.zeros(W, H, 4, dtype=torch.uint8)
        want[x0:x0 + cw, y0:y0 + ch, :3] = rgb[x0:x0 + cw, y0:y0 + ch]
        want[x0:x0 + cw, y0:y0 + ch, 3] = mask[x0:x0 + cw, y0:y0 + ch]
        want_d = torch.zeros(W, H)
        want_d[x0:x0 + cw, y0:y0 + ch] = depth[x0:x0 + cw, y0:y0 + ch]
        assert torch.equal(rgbs, want) and torch.equal(d, want_d)
        assert torch.equal(st.t_wc[slot], twc) and torch.equal(st.bbox[slot], T(np.asarray(box, np.float32)))


@pytest.mark.parametrize("tag", ["fg_step2p5_buf6", "fg_step1_buf5"])
def test_keyframe_trace_g12_crop_store(golden, monkeypatch, tag):
    """The reference's slot trace through a crop-store object (direct writes, CPU): the bookkeeping is the dense
    object's, and every live slot holds the dense slot's pixels inside its rect."""
    g = golden("g12_keyframes")
    objs = {}
    for kind in ("dense", "crop"):
        cfg, obj_id, n_frames = _map_cfg(g, tag)
        cfg.keyframe_store = kind
        monkeypatch.setattr(ovmap.random, "choice", _ReplayChoice(g, tag))
        so = None
        for i in range(n_frames):
            args = (T(g[f"{tag}_rgb"][i]), T(g[f"{tag}_depth"][i]), _state_map(T(g[f"{tag}_inst"][i]), obj_id),
                    T(g[f"{tag}_bbox"][i]), T(g[f"{tag}_t_wc"][i]), int(g[f"{tag}_frame_ids"][i]))
            if so is None:
                so = ovmap.sceneObject(cfg, obj_id, *args)
            else:
                so.append_keyframe(*args)
            _check_trace(so, g, tag, i)
        objs[kind] = so
    d, c = objs["dense"], objs["crop"]
    assert c.crops is not None and not hasattr(c, "rgbs_batch") and not hasattr(c, "depth_batch")
    assert d.crops is None and c.keyframe_store() is c.crops
    assert list(c.kf_id_dict.items()) == list(d.kf_id_dict.items())
    assert (c.n_keyframes, c.kf_pointer, c.lastest_kf_queue, c.frame_cnt) == \
        (d.n_keyframes, d.kf_pointer, d.lastest_kf_queue, d.frame_cnt)
    live = sorted(set(d.kf_id_dict.values()))
    assert torch.equal(c.t_wc_batch[live], d.t_wc_batch[live]) and torch.equal(c.bbox[live], d.bbox[live])
    Wd, Hd = d.frames_width, d.frames_height
    for slot in live:
        x0, y0, cw, ch = crop_rect(d.bbox[slot], Wd, Hd)
        assert c.crops.rect[slot].tolist() == [x0, y0, cw, ch]
        rgbs, depth = c.crops.frame(slot)
        inside = torch.zeros(Wd, Hd, dtype=torch.bool)
        inside[x0:x0 + cw, y0:y0 + ch] = True
        assert torch.equal(rgbs[inside], d.rgbs_batch[slot][inside])
        assert torch.equal(depth[inside], d.depth_batch[slot][inside])
        assert not rgbs[~inside].any() and not depth[~inside].any()
    # (at this tiny camera the 256-pixel granule of the arena is larger than a frame: no size comparison here)
    assert c.store_bytes() == c.crops.nbytes == c.keyframe_buffer_size * c.crops.cap * 8
    assert d.store_bytes() == d.keyframe_buffer_size * Wd * Hd * 8


def test_background_object_stays_dense(golden):
    g = golden("g12_keyframes")
    tag = "bg_step5_buf20"
    cfg, obj_id, _ = _map_cfg(g, tag)
    cfg.keyframe_store = "crop"
    assert obj_id == 0 and cfg.do_bg
    so = ovmap.sceneObject(cfg, obj_id, T(g[f"{tag}_rgb"][0]), T(g[f"{tag}_depth"][0]),
                           _state_map(T(g[f"{tag}_inst"][0]), obj_id), T(g[f"{tag}_bbox"][0]), T(g[f"{tag}_t_wc"][0]), 0)
    assert so.crops is None and so.rgbs_batch.shape[1:3] == so.depth_batch.shape[1:]


def test_config_key():
    assert ocfg.Config(ocfg.replica_room0_config()).keyframe_store == "dense"        # no key: every shipped config
    assert ocfg.Config(ocfg.replica_room0_config(**{"model.keyframe_store": "crop"})).keyframe_store == "crop"
    assert ocfg.Config(ocfg.replica_room0_config(**{"model.keyframe_store": "dense"})).keyframe_store == "dense"
    with pytest.raises(ValueError):
        ocfg.Config(ocfg.replica_room0_config(**{"model.keyframe_store": "sparse"}))
