"""The reference's two voxel-wise segmentation losses (dram/metrics.py:10-72) on the device, for a target the caller gives:
fine-tuning on real voxel labels, where the fused IntRegRefineLoss (train_step.DeviceIntRegRefineLoss) derives its target
from the prediction itself.  Constructor and call signatures are the reference's; the work is `functional.boot_bce` /
`functional.bce_smooth` (kernels dram_boot_bce_* / dram_bce_smooth_* of csrc/loss.hip).  There is no CPU path.

Neither class fits DataParallelTrainer(loss_fn=...): that contract is two terms, a per-sample sum and a share-weighted batch
mean, and these are a single mean over the whole batch."""
from . import functional as HF


class BootBinCrossEntropy:
    """loss = BootBinCrossEntropy(smoothing)(p, t, voi): p the sigmoid outputs [N,1,D,H,W] (float32, device), t the target
    and voi the volume of interest of the same shape (float32, uint8 or bool).  Returns a 0-dim tensor, differentiable in p.

    Of the reference's two assertions, `t.size() == p.size()` is checked here (and voi's too), as a ValueError.
    `t.sum() <= voi.sum()` would need the two sums on the host, i.e. a device read in a path that has none: it is dropped.
    `class_weights` is accepted and ignored, as in the reference."""

    def __init__(self, smoothing=0.1):
        self.smoothing = smoothing
        self.eps = 1e-7

    def __call__(self, p, t, voi, class_weights=None):
        return HF.boot_bce(p, t, voi, self.smoothing)


class BinaryCrossEntropySmooth:
    """loss = BinaryCrossEntropySmooth(smooth)(probs, targets): probs float32 on the device, targets of the same shape
    (float32, uint8 or bool).  Returns a 0-dim tensor, differentiable in probs.  The reference's size assertion is a
    ValueError here."""

    def __init__(self, smooth):
        self.smooth = smooth
        self.eps = 1e-6

    def __call__(self, probs, targets):
        return HF.bce_smooth(probs, targets, self.smooth)
