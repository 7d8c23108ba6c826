"""helpers shared by the -m gpu tests: move synth batches to the GPU, compare with the oracle"""
import numpy as np
import torch

import oracle_lib as ol


def to_dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def batch_to_dev(b, dev, weights=None):
    w = weights if weights is not None else b.weights
    return dict(ctrl=to_dev(b.ctrl, dev), guide_off=to_dev(b.guide_off, dev), guide_pv=to_dev(b.guide_pv, dev),
                guide_unk=to_dev(b.guide_unk, dev), obs_off=to_dev(b.obs_off, dev), obs=to_dev(b.obs, dev),
                weights=to_dev(w, dev))


def rel_err_per_traj(a, ref):
    B = ref.shape[0]
    return np.abs(a - ref).reshape(B, -1).max(1) / np.abs(ref).reshape(B, -1).max(1)


def is_level(ctrl):
    """the level rule (include/vigo.h), per trajectory"""
    zmin, zmax = ctrl[:, :, 2].min(1), ctrl[:, :, 2].max(1)
    return (zmax - zmin) <= 2.0 ** -40 * np.maximum(1.0, np.maximum(np.abs(zmin), np.abs(zmax)))


def simd_count():
    return 4 * torch.cuda.get_device_properties(torch.device("cuda", 0)).multi_processor_count   # as vigo_create


class emulation:
    """context manager: oracle in device-emulation mode for N control points (fast=True: of VIGO_PREC_F64_FAST)"""

    def __init__(self, N, fast=False):
        self.g, self.ppl = ol.emulation_shape(N)
        self.fast = fast

    def __enter__(self):
        if self.fast:
            ol.oracle().vgo_set_emulation_fast(1)
        ol.set_emulation(self.g, self.ppl)

    def __exit__(self, *a):
        ol.set_emulation(0)
        if self.fast:
            ol.oracle().vgo_set_emulation_fast(0)
