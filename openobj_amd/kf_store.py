"""Cropped keyframe store: an object's keyframes kept as the crops the sampler and get_bound can read.

The dense store of sceneObject holds keyframe_buffer_size full frames per object (rgbs_batch [F, W, H, 4] u8 and
depth_batch [F, W, H] fp32: 8 bytes per pixel of the CAMERA).  Of those only the pixels inside the slot's 2-D box are
ever read: the sampler draws `(long)(u * (hi - lo) + lo)` with u in [0, 1) per axis (vmap.py:414-425), and get_bound
reads the pixels whose state byte is 1, which the dataset adapters put inside the box (the box is the instance's own
rectangle, enlarged).  KeyframeCropStore keeps exactly that rectangle per slot, in one byte arena per object:

    arena  u8 [F * cap * 8]   slot s = cap * 4 bytes of rgb + state, then cap floats of depth; the crop row-major
                              [cw][ch], the transposed orientation of the dense store
    rect   int32 [F, 4]       x0, y0, cw, ch of every slot (device; a host copy is kept for growth and frame())
    t_wc   fp32 [F, 4, 4], bbox fp32 [F, 4]   as in the dense store

Growth rule (a contract): a crop of `needed` pixels that does not fit takes the capacity to
ceil(1.5 * needed / 256) * 256 pixels per slot; the slots are copied device to device into the new arena, `version` is
bumped (descriptor tables that hold the arena's address must be rebuilt) and the arena never shrinks.
"""
import math

import numpy as np
import torch

CAP_ALIGN = 256          # pixels: a slot is a multiple of 2 KiB, its depth plane 1 KiB aligned
GROWTH = 1.5


def crop_rect(bbox, W, H):
    """(x0, y0, cw, ch) of a 2-D box [u lo, u hi, v lo, v hi]: columns trunc(b0) .. trunc(b1) and rows trunc(b2) ..
    trunc(b3), inclusive, clipped to the W x H image -- every pixel `(long)(u * (hi - lo) + lo)`, u in [0, 1), can be
    (the sampler's draw), and the pixel of `hi` itself, which the fp32 product can round up to."""
    b = [float(v) for v in (bbox.tolist() if hasattr(bbox, "tolist") else bbox)]
    lim = lambda v, n: min(max(int(math.trunc(v)), 0), n - 1)
    x0, x1 = sorted((lim(b[0], W), lim(b[1], W)))
    y0, y1 = sorted((lim(b[2], H), lim(b[3], H)))
    return x0, y0, x1 - x0 + 1, y1 - y0 + 1


def grown_cap(needed):
    """The growth rule: the capacity (pixels per slot) a store takes when a crop of `needed` pixels does not fit."""
    return int(math.ceil(GROWTH * needed / CAP_ALIGN)) * CAP_ALIGN


class KeyframeCropStore:
    """Keyframe slots of ONE object as crops (see the module text).  t_wc / bbox may be given (sceneObject shares its
    own tensors); otherwise they are allocated here."""

    def __init__(self, n_slots, W, H, device, t_wc=None, bbox=None):
        self.F, self.W, self.H = int(n_slots), int(W), int(H)
        self.device = device
        self.cap = 0
        self.version = 0
        self.arena = torch.empty(0, dtype=torch.uint8, device=device)
        self.rect = torch.zeros(self.F, 4, dtype=torch.int32, device=device)
        self.t_wc = t_wc if t_wc is not None else torch.empty(self.F, 4, 4, dtype=torch.float32, device=device)
        self.bbox = bbox if bbox is not None else torch.empty(self.F, 4, dtype=torch.float32, device=device)
        self.rect_host = np.zeros((self.F, 4), np.int32)       # what `rect` holds (or will, once the launch has run)

    # ---------------------------------------------------------------------------------------------- capacity
    @property
    def nbytes(self):
        """Bytes of keyframe pixels held (the arena; the dense store's counterpart is rgbs_batch + depth_batch)."""
        return self.arena.numel()

    def reserve(self, slot, rect):
        """Make room for `rect` in `slot` and record it on the host.  The device `rect` row is written by whoever
        writes the pixels (write() here, objnerf_ingest_frame_crops on the deferred path)."""
        if not 0 <= slot < self.F:
            raise IndexError("keyframe slot outside the store")
        x0, y0, cw, ch = (int(v) for v in rect)
        if cw < 1 or ch < 1 or x0 < 0 or y0 < 0 or x0 + cw > self.W or y0 + ch > self.H:
            raise ValueError("crop rect outside the image")
        needed = cw * ch
        if needed > self.cap:
            self._grow(grown_cap(needed))
        self.rect_host[slot] = (x0, y0, cw, ch)

    def _grow(self, cap):
        old, old_cap = self.arena, self.cap
        new = torch.empty(self.F * cap * 8, dtype=torch.uint8, device=self.device)
        if old_cap:
            src, dst = old.view(self.F, old_cap * 8), new.view(self.F, cap * 8)
            dst[:, :old_cap * 4] = src[:, :old_cap * 4]                              # rgb + state planes
            dst[:, cap * 4:cap * 4 + old_cap * 4] = src[:, old_cap * 4:]             # depth planes
        self.arena, self.cap = new, cap
        self.version += 1

    # ---------------------------------------------------------------------------------------------- views
    def _planes(self, slot):
        """(rgb + state u8 [cw, ch, 4], depth fp32 [cw, ch]) views of the slot's crop, and its rect."""
        x0, y0, cw, ch = (int(v) for v in self.rect_host[slot])
        o = slot * self.cap * 8
        px = self.arena[o:o + cw * ch * 4].view(cw, ch, 4)
        d = self.arena[o + self.cap * 4:o + self.cap * 4 + cw * ch * 4].view(torch.float32).view(cw, ch)
        return px, d, (x0, y0, cw, ch)

    def write(self, slot, rgb, depth, mask, bbox_2d, t_wc):
        """The direct write path (sceneObject._write_slot with a state mask), in torch slicing: runs on any device."""
        rect = crop_rect(bbox_2d, self.W, self.H)
        self.reserve(slot, rect)
        px, d, (x0, y0, cw, ch) = self._planes(slot)
        px[..., :3] = rgb[x0:x0 + cw, y0:y0 + ch]
        px[..., 3] = mask[x0:x0 + cw, y0:y0 + ch]
        d[...] = depth[x0:x0 + cw, y0:y0 + ch]
        self.rect[slot] = torch.tensor(rect, dtype=torch.int32)
        self.t_wc[slot, ...] = t_wc
        self.bbox[slot, ...] = bbox_2d

    def frame(self, slot):
        """(rgbs [W, H, 4] u8, depth [W, H] fp32) of a slot rebuilt dense, zero outside its rect (tests, debugging)."""
        rgbs = torch.zeros(self.W, self.H, 4, dtype=torch.uint8, device=self.device)
        depth = torch.zeros(self.W, self.H, dtype=torch.float32, device=self.device)
        if self.cap:
            px, d, (x0, y0, cw, ch) = self._planes(slot)
            rgbs[x0:x0 + cw, y0:y0 + ch] = px
            depth[x0:x0 + cw, y0:y0 + ch] = d
        return rgbs, depth

    def descriptor(self):
        """The fields of objnerf_kf_crops: (arena address, cap, rect, t_wc, bbox addresses).  Valid until `version`
        changes; the tensors must stay alive while a kernel uses it."""
        return (self.arena.data_ptr(), self.cap, self.rect.data_ptr(), self.t_wc.data_ptr(), self.bbox.data_ptr())
