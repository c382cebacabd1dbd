#!/usr/bin/env python3
"""Fixture G13B: what the REFERENCE's own sceneObject.load_checkpoints (vmap.py:579-602) makes of a checkpoint written
HERE by openobj_amd.vmap.sceneObject.save_checkpoints (tests/test_reference_pins.py::object_written_here): the checkpoint
entries it reads, the parameter names of its own OccupancyMap / UniDirsEmbed (its load_state_dict is strict, so the file
must carry exactly these), the values those modules hold after the load, and the metadata it takes over.
tests/test_reference_pins.py::test_checkpoint_written_here_loads_in_reference checks the file written there against it.

    python tests/golden/make_g13b_ref_load.py      -> tests/golden/g13b_ref_load.npz

Needs the reference checkout that make_golden.py imports."""
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402
import test_reference_pins as P  # noqa: E402


class ReadLog(dict):
    """The loaded checkpoint, logging every entry the loader reads."""

    def __init__(self, d):
        super().__init__(d)
        self.read = []

    def __getitem__(self, k):
        self.read.append(k)
        return super().__getitem__(k)


def main():
    log = {}
    _load = torch.load

    def load(f, *a, **k):      # (the reference runs torch 2.0.1, where torch.load unpickles numpy arrays by default)
        log["ckpt"] = ReadLog(_load(f, *a, weights_only=False, **k))
        return log["ckpt"]

    with tempfile.TemporaryDirectory() as d:
        _, path = P.object_written_here(d)
        ref = types.SimpleNamespace(trainer=MG.ref_trainer.Trainer(MG.make_cfg(hidden=32, scale=2.0)),
                                    training_device="cpu")
        MG.ref_vmap.torch.load = load
        try:
            assert MG.ref_vmap.sceneObject.load_checkpoints(ref, path) is True
        finally:
            MG.ref_vmap.torch.load = _load
    fc, pe = ref.trainer.fc_occ_map.state_dict(), ref.trainer.pe.state_dict()
    out = {"read": np.array(log["ckpt"].read), "fc_keys": np.array(list(fc)), "pe_keys": np.array(list(pe)),
           "meta": np.array([ref.obj_id, ref.semantic_id, float(ref.trainer.obj_scale)], dtype=np.float64),
           "clip_feat": ref.clip_feat, "caption_feat": ref.caption_feat}
    out.update({f"fc{i}": v for i, v in enumerate(fc.values())})
    out.update({f"pe{i}": v for i, v in enumerate(pe.values())})
    MG.save("g13b_ref_load", **out)


if __name__ == "__main__":
    main()
