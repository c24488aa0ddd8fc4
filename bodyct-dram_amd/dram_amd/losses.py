"""Segmentation losses on the device for a target the caller gives: fine-tuning on real voxel labels, where the fused
IntRegRefineLoss (train_step.DeviceIntRegRefineLoss) derives its target from the prediction itself.  There is no CPU path.

BootBinCrossEntropy and BinaryCrossEntropySmooth are the reference's two voxel-wise losses (dram/metrics.py:10-72) on
probabilities, constructor and call signatures the reference's; the work is `functional.boot_bce` / `functional.bce_smooth`
(kernels dram_boot_bce_* / dram_bce_smooth_* of csrc/loss.hip).  Neither fits DataParallelTrainer(loss_fn=...): that
contract is two terms, a per-sample sum and a share-weighted batch mean, and these are a single mean over the whole batch
whose class-balance weight is a statistic of that batch.

TverskyLoss, SoftDiceLoss and FocalLoss have no reference counterpart.  They take LOGITS, every quantity of theirs is per
sample (include/dram_hip.h, SegOverlap; `functional.seg_overlap`, kernels dram_seg_overlap_*), and the pair of them is
what does fit the trainer: train_step.DeviceSegOverlapLoss."""
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


class TverskyLoss:
    """loss = TverskyLoss(a, b, smooth)(logits, target, voi=None): the mean over samples of 1 - TI_n,
    TI_n = (TP + smooth) / (TP + a FP + b FN + smooth) with the soft counts of sample n inside voi (a weighs false
    positives, b false negatives).  logits [N,1,D,H,W] float32 on the device, target and voi of the same shape (float32,
    uint8 or bool; non-zero is set; voi None: every voxel).  Returns a 0-dim tensor, differentiable in the logits."""

    def __init__(self, a=0.5, b=0.5, smooth=1.0):
        self.a, self.b, self.smooth = a, b, smooth

    def __call__(self, logits, target, voi=None):
        n = max(logits.shape[0], 1)
        return HF.seg_overlap(logits, target, voi, self.a, self.b, self.smooth, 0.5, 0.0)[0] / n


class SoftDiceLoss(TverskyLoss):
    """SoftDiceLoss(smooth) = TverskyLoss(0.5, 0.5, smooth): the mean over samples of 1 - (2 TP + 2 smooth) /
    (sum p + sum t + 2 smooth)."""

    def __init__(self, smooth=1.0):
        super().__init__(0.5, 0.5, smooth)


class FocalLoss:
    """loss = FocalLoss(alpha, gamma)(logits, target, voi=None): the mean over samples of the sample's mean inside voi of
    -alpha_t (1 - p_t)^gamma log p_t (alpha_t = alpha where the target is set, 1 - alpha elsewhere).  gamma = 0 with
    alpha = 0.5 is half the plain binary cross-entropy.  Tensors as TverskyLoss's.  Returns a 0-dim tensor."""

    def __init__(self, alpha=0.5, gamma=2.0):
        self.alpha, self.gamma = alpha, gamma

    def __call__(self, logits, target, voi=None):
        return HF.seg_overlap(logits, target, voi, 0.5, 0.5, 1.0, self.alpha, self.gamma)[1]
