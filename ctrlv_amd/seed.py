"""`DeviceSeed`: a seed the library draws from on the device (include/ctrlv_hip.h: ctrlv_randn, ctrlv_pipeline_prepare)."""


class DeviceSeed:
    """`generator=DeviceSeed(seed, clip_index0)` of the two pipelines, on the CTRLV_PIPELINE=plan route only: the PIL image goes
    to the driver at its own size, and the Lanczos resize, the two Gaussian draws and the sigma schedule happen in the library
    (PipelinePlan.generate(seed=...)).  The noise of clip i of the call is a pure function of (seed, clip_index0 + i): the same
    clip draws the same noise alone, inside any batch and on any rank.  The default route raises a ValueError for it."""
    __slots__ = ("seed", "clip_index0")

    def __init__(self, seed, clip_index0=0):
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.clip_index0 = int(clip_index0)
        if not 0 <= self.clip_index0 < 2 ** 32:
            raise ValueError(f"DeviceSeed: clip_index0={clip_index0} must fit 32 bits")

    def __repr__(self):
        return f"DeviceSeed({self.seed}, clip_index0={self.clip_index0})"
