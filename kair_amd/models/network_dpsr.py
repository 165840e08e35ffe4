"""DPSR's super-resolver prior (Zhang, Zuo, Zhang, CVPR 2019); the reference's models/network_dpsr.py (MSRResNet_prior)
restated from upstream cszn/KAIR (the reference sources were not at hand; not checked against them): MSRResNet0's
topology and state_dict keys with in_nc = C + 1 -- the LR image followed by one noise-level channel -- and nc 96.

It shares network_msrresnet.MSRResNet0's implementation (and its departures from the reference) and runs on the same
step program (engine/ressr_engine.py).  The DPSR plug-and-play loop (main_test_dpsr.py) is not built.
"""
from .network_msrresnet import MSRResNet0


class MSRResNet_prior(MSRResNet0):
    NAME = "DPSR MSRResNet_prior"

    def __init__(self, in_nc=4, out_nc=3, nc=96, nb=16, upscale=4, act_mode="R", upsample_mode="upconv",
                 compute_dtype="fp32"):
        super().__init__(in_nc, out_nc, nc, nb, upscale, act_mode, upsample_mode, compute_dtype)
