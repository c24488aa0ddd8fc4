"""Device-resident restatement of the reference's training step around DC3D
(`LesionSegChunkTrain.train`, dram/job_runner.py:649-681, with
`IntRegRefineLoss`, dram/metrics.py:311-373) plus the pure data-parallel wrapper that the
reference does not have: one process per GPU, gradients averaged with an RCCL
all-reduce over xGMI.

The loss runs as two fused HIP kernels (csrc/loss.hip: one streaming pass for every sum of the
regression hinge and the bootstrapped BCE, one for the gradient) and -- unlike the reference, which
round-trips every sample through numpy (metrics.py:338-352) -- never synchronises with the host
(`oracle.dram_oracle.fused_loss_math` spells the same fused formulation with torch ops for the CPU tests
against the reference's golden vectors).  The regression targets depend only on the data (lesion
ratio, CT severity score), so they are computed when the batch is built, as the reference's data
loader side would.  The affine-consistency losses build a second, transformed batch inside every call: its targets
come from the device masks by one more kernel pair of csrc/loss.hip (`Batch.on_device`), not from a host loop.

`DeviceIntRegLoss` / `DeviceIntRegAffLoss` are the reference's two losses without the pseudo-label refinement
(metrics.py:75-308: the same hinge plus an entropy term, one more kernel pair of csrc/loss.hip); they take the places of
`DeviceIntRegRefineLoss` / `DeviceIntRegAffRefineLoss` unchanged.

`DeviceSegOverlapLoss` is the supervised one, with no counterpart in the reference: a per-sample Tversky term and a
per-sample focal term on the logits against voxel labels that are GIVEN (`Batch.supervised`), one more kernel pair of
csrc/loss.hip.  It has the same call signature and decomposes over micro-batches and ranks exactly.
"""
import math

import torch
import torch.distributed as dist

# IntRegLoss.ctss_ratio_map (metrics.py:76-83)
CTSS_RATIO_MAP = {0: (0.0, 0.001), 1: (0.001, 0.01), 2: (0.01, 0.05),
                  3: (0.05, 0.35), 4: (0.35, 0.5), 5: (0.5, 1.00001)}


def regression_targets(ctsses, ratio_upper_bound, band_width):
    """IntRegLoss.get_labels (metrics.py:122-138): per-sample [lower, upper] band."""
    out = []
    for ctss, lp in zip(ctsses, ratio_upper_bound):
        lp = float(lp)
        lb, ub = max(0.0, lp - band_width), min(1.0, lp + band_width)
        c_lb, c_ub = CTSS_RATIO_MAP[int(float(ctss))]
        band = (max(c_lb, lb), min(c_ub, ub))
        if band[1] < band[0]:
            if ub <= c_lb:
                band = (lb, ub)
            elif lb >= c_ub:
                band = (c_lb, c_ub)
            else:
                raise RuntimeError("cannot reach here!")
        out.append(band)
    return torch.tensor(out, dtype=torch.float32)


class Batch:
    """One per-rank batch of lobe chunks, already in the post-transform layout the reference's
    train() feeds the model (job_runner.py:658-660): [N,1,D,H,W] float tensors on the device."""

    def __init__(self, images, lobes, lesions, ctss, freq_map, band_width=1e-2):
        self.images, self.lobes, self.lesions = images, lobes, lesions
        self.ctss = [float(c) for c in ctss]
        B = images.shape[0]
        ratio_ub = (lesions * lobes).view(B, -1).sum(-1) / lobes.view(B, -1).sum(-1)
        self.targets = regression_targets(self.ctss, ratio_ub.cpu(), band_width).to(images.device)
        wf = torch.tensor([freq_map[int(c)] for c in self.ctss], dtype=torch.float32)
        self.weight = torch.clamp(wf, 0.2, 0.8).to(images.device)           # metrics.py:172-174
        self.keep = torch.tensor([0.0 if c < 1e-7 else 1.0 for c in self.ctss],
                                 dtype=torch.float32).view(-1, 1, 1, 1, 1).to(images.device)   # metrics.py:326-327

    @classmethod
    def from_chunks(cls, chunks, ctss, freq_map, loader, band_width=1e-2):
        """The batch of raw chunks (dicts of int16 "#image", uint8 "#lobe_reference", optional "#vessel_reference" and
        meta["spacing"], every chunk with its own size) prepared on the device by `loader`, a dram_amd.preprocess.ChunkLoader:
        windowing, fixed-size resample and the pseudo-lesion label of dataset.py:450-486 / job_runner.py:586-597."""
        out = loader(loader.pack(chunks))
        return cls(out["#image"], out["#lobe_reference"], out["#pseudo_lesion_reference"], ctss, freq_map, band_width)

    @classmethod
    def on_device(cls, images, lobes, lesions, ctss_dev, freq_map, band_width=1e-2, ctss=None):
        """A batch whose masks were made on the device (the transformed copy of the affine-consistency losses), built
        WITHOUT a host read: one kernel pair (csrc/loss.hip, dram_intreg_targets) turns the two masks, the int32 device
        tensor `ctss_dev` of the samples' CT severity scores (`ctss_device()` of the batch they came from) and the six
        class frequencies into what `__init__` computes with a device-to-host copy and a Python loop.  For 0/1 masks
        `targets`, `weight` and `keep` carry the same bits as `Batch(...)`'s.  `freq_map` stays on the host (a dict over
        0..5 or a sequence of six floats): it travels with the launch.  Two differences, both outside what a training
        batch holds: a sample with an empty lobe gets NaN targets (the host loop turns the 0/0 into the sample's class
        interval), and a score outside 0..5 gives NaN targets and a NaN weight where the host raises KeyError.
        `ctss`: the host list of the scores where the caller has one (kept as `.ctss`)."""
        from . import functional as HF
        b = object.__new__(cls)
        b.images, b.lobes, b.lesions = images, lobes, lesions
        b.ctss = None if ctss is None else [float(c) for c in ctss]
        freq = [freq_map[k] for k in range(6)]
        b.targets, b.weight, keep = HF.intreg_targets(lobes, lesions, ctss_dev, freq, band_width)
        b.keep = keep.view(-1, 1, 1, 1, 1)
        b._ctss_dev = ctss_dev
        return b

    @classmethod
    def supervised(cls, images, lobes, labels):
        """A batch for supervised fine-tuning (DeviceSegOverlapLoss): the images, the lobe masks and the GIVEN voxel labels,
        which take the place of `lesions`.  No CT severity scores and no host read: `ctss`, `targets`, `weight` and `keep`
        are None, so `micro()` and `augmented()` work and the IntReg losses, which need them, refuse such a batch."""
        b = object.__new__(cls)
        b.images, b.lobes, b.lesions = images, lobes, labels
        b.ctss = b.targets = b.weight = b.keep = b._ctss_dev = None
        return b

    def require_targets(self, who):
        """The IntReg losses' precondition: a batch built from CT severity scores (regression band, class weight, switch)."""
        if self.targets is None or self.weight is None or self.keep is None:
            raise ValueError(f"{who} needs the regression targets of a batch built from CT severity scores; this batch is "
                             f"Batch.supervised(...) and carries voxel labels only (use DeviceSegOverlapLoss)")

    def ctss_device(self):
        """The CT severity scores as an int32 tensor on the batch's device: uploaded at the first call, kept after that
        (micro-batches take slices of it), so that `on_device` batches derived from this one need no upload of their own."""
        dev = getattr(self, "_ctss_dev", None)
        if dev is None and self.ctss is None:
            raise ValueError("this batch has no CT severity scores (Batch.supervised)")
        if dev is None:
            dev = self._ctss_dev = torch.tensor([int(c) for c in self.ctss], dtype=torch.int32).to(self.images.device)
        return dev

    def micro(self, lo, hi):
        b = object.__new__(Batch)
        b.images, b.lobes, b.lesions = self.images[lo:hi], self.lobes[lo:hi], self.lesions[lo:hi]
        b.ctss = None if self.ctss is None else self.ctss[lo:hi]
        b.targets, b.weight, b.keep = (None if v is None else v[lo:hi] for v in (self.targets, self.weight, self.keep))
        dev = getattr(self, "_ctss_dev", None)
        b._ctss_dev = None if dev is None else dev[lo:hi]
        return b

    def augmented(self, aug):
        """This batch after `aug` (an element of dram_amd/augment.py or its EnsembleScanAugmentation): the images go through it as
        "#image", the two masks as "#..._reference", so flips and quarter turns move all three alike while the intensity
        transforms touch the images only.  The regression targets are sums over the chunk, which those moves keep."""
        out = aug({"#image": self.images, "#lobes_reference": self.lobes, "#lesions_reference": self.lesions, "meta": {}})
        b = object.__new__(Batch)
        b.images, b.lobes, b.lesions = out["#image"], out["#lobes_reference"], out["#lesions_reference"]
        b.ctss, b.targets, b.weight, b.keep = self.ctss, self.targets, self.weight, self.keep
        b._ctss_dev = getattr(self, "_ctss_dev", None)
        return b

    def __len__(self):
        return self.images.shape[0]


def synthetic_batch(n, size, seed, device, freq_map=None):
    """images U[0,1) zeroed outside a centred ellipsoid lobe mask
    (semi-axes 0.45*S), lesions = (image > 0.7) & lobe, ctss = n mod 6, frequency map 1/6."""
    D, H, W = (size,) * 3 if isinstance(size, int) else size
    g = torch.Generator(device="cpu").manual_seed(seed)
    zz = (torch.arange(D, dtype=torch.float32) - (D - 1) / 2).view(D, 1, 1) / (0.45 * D)
    yy = (torch.arange(H, dtype=torch.float32) - (H - 1) / 2).view(1, H, 1) / (0.45 * H)
    xx = (torch.arange(W, dtype=torch.float32) - (W - 1) / 2).view(1, 1, W) / (0.45 * W)
    lobe = ((zz ** 2 + yy ** 2 + xx ** 2) < 1.0).float().to(device)
    images = torch.empty((n, 1, D, H, W), dtype=torch.float32, device=device)
    for i in range(n):   # generate on the host one chunk at a time (bounded host memory)
        images[i, 0] = torch.rand((D, H, W), generator=g).to(device) * lobe
    lobes = lobe.view(1, 1, D, H, W).expand(n, 1, D, H, W).contiguous()
    lesions = ((images > 0.7) & (lobes > 0)).float()
    ctss = [float(i % 6) for i in range(n)]
    return Batch(images, lobes, lesions, ctss, freq_map or {k: 1.0 / 6 for k in range(6)})


class DeviceIntRegRefineLoss:
    """IntRegRefineLoss.__call__ (metrics.py:360-373) given the model output `dense` (DC3D returns
    the same tensor as dense_outs and refined_dense_outs).  Returns (reg_loss, seg_loss)."""

    def __init__(self, band_width=1e-2, smoothing=0.1):
        self.band_width, self.smoothing, self.eps = band_width, smoothing, 1e-7

    def __call__(self, dense, batch, refined=None):
        """`refined`: the model's second output when it differs from `dense` (DC3DATGeneric).  Two fused HIP
        kernels (csrc/loss.hip); like every other op of the path there is no CPU fallback (CPU tensors raise)."""
        from . import functional as HF
        batch.require_targets("DeviceIntRegRefineLoss")
        out = HF.intreg_refine_loss(dense, batch.lobes, batch.lesions, batch.keep, batch.targets, batch.weight,
                                    self.smoothing, refined=refined)
        return out[0], out[1]


class DeviceIntRegLoss:
    """IntRegLoss.__call__ (metrics.py:204-210): the interval regression of IntRegRefineLoss without the pseudo-label
    term, plus the entropy of the predicted probabilities (compute_enc_loss, metrics.py:154-156).  The reference takes
    the model's SECOND output for both terms, so `refined` is used when given and `dense` otherwise (DC3D returns one
    tensor twice).  Returns (reg_loss, enc_loss).

    The call signature is DeviceIntRegRefineLoss's, so it goes into DataParallelTrainer(loss_fn=...) as it is.  `enc` is a
    mean over the batch's elements, so the trainer's share = len(micro) / n_global weighting of the second term makes
    micro-batches and ranks of equal chunk size add up to the whole-batch value exactly (unlike seg_loss, no statistic of
    the micro-batch enters it)."""

    def __init__(self, band_width=5e-2):
        self.band_width = band_width

    def __call__(self, dense, batch, refined=None):
        """One fused HIP kernel each way (csrc/loss.hip); no CPU fallback (CPU tensors raise)."""
        from . import functional as HF
        batch.require_targets("DeviceIntRegLoss")
        out = HF.intreg_enc_loss(dense if refined is None else refined, batch.lobes, batch.lesions, batch.targets, batch.weight)
        return out[0], out[1]


class DeviceSegOverlapLoss:
    """Supervised fine-tuning on given voxel labels: the per-sample Tversky and focal terms of include/dram_hip.h
    (SegOverlap; functional.seg_overlap, one HIP kernel each way and a one-block finish) on the model's logits, with
    `batch.lesions` as the target and `batch.lobes` as the volume of interest (a batch of Batch.supervised; any Batch
    works).  `a`, `b` weigh false positives and false negatives (0.5, 0.5: soft Dice), `smooth` is added to numerator and
    denominator, `alpha`, `gamma` are the focal term's.  Returns (tversky_sum, focal_mean):

      tversky_sum = sum over the samples of 1 - TI_n        focal_mean = mean over the samples of F_n

    The call signature is DeviceIntRegLoss's, so it goes into DataParallelTrainer(loss_fn=...) as it is, and `refined` is
    used when given.  Every quantity is per sample -- no statistic of the batch enters either term -- so both terms
    decompose over micro-batches and ranks with NO deviation: the first adds up, the second adds up under the trainer's
    share = len(micro) / n_global weighting.  The first term is therefore a sum over the GLOBAL batch: a mean Dice loss of
    weight w wants loss_factors[0] = w / n_global (the losses.TverskyLoss / SoftDiceLoss / FocalLoss classes return the
    means directly, for use outside the trainer)."""

    def __init__(self, a=0.5, b=0.5, smooth=1.0, alpha=0.5, gamma=2.0):
        self.a, self.b, self.smooth, self.alpha, self.gamma = a, b, smooth, alpha, gamma

    def __call__(self, dense, batch, refined=None):
        """No CPU fallback (CPU tensors raise)."""
        from . import functional as HF
        out = HF.seg_overlap(dense if refined is None else refined, batch.lesions, batch.lobes, self.a, self.b, self.smooth,
                             self.alpha, self.gamma)
        return out[0], out[1]


class DataParallelTrainer:
    """One optimisation step of DC3D on this rank's chunks, optionally as micro-batches with
    gradient accumulation, and -- when torch.distributed is initialised -- an all-reduce of the gradients in a
    few large flat buckets, OVERLAPPED with backward, before the optimiser step.

    What the step computes is rank-count independent: it is the reference's loss on the GLOBAL batch
    (all ranks' chunks), evaluated shard by shard.  `reg_loss` is a sum over samples (metrics.py:177), so
    its gradients add up over micro-batches and ranks; `seg_loss` is a batch mean, so every micro-batch
    enters with its share len(micro) / len(global batch) (its class-balance weight alpha stays a statistic of
    the micro-batch: documented deviation from one huge batch).  The gradients are therefore SUMMED over ranks,
    and W ranks with one shard each reproduce one rank running the same shards as micro-batches
    (tests/test_gpu_dp.py).

    Overlap: the fused engine's backward (dram_amd/engine.py) hands every parameter gradient to
    `grad_sink` the moment it is final -- the head first, then stage by stage, each right after its backward-weights launch.
    During the LAST micro-batch's backward the trainer writes it (plus what earlier micro-batches accumulated) straight into
    its slot of a persistent flat bucket and starts that bucket's asynchronous all-reduce as soon as the bucket is complete:
    RCCL runs it on its own stream beside the remaining backward kernels (the largest gradient, us_modules.0's 768 -> 256
    filter, 21 MB, is ready after ~45 % of backward).  What autograd delivers outside the engine (per-op path, the attention
    module of DC3DATGeneric) joins after backward.  xGMI is point-to-point (7 links/GPU): the 65 MB take < 1 ms as a ring
    all-reduce against a multi-second step, so this hides little here -- it is the stated design and costs nothing.
    Per-rank BatchNorm statistics (the reference's default "bn") need no exchange.  `p.grad` of every parameter is a view
    into its bucket after the step (no per-step torch.cat, no copy back).

    Losses that run the model themselves (`calls_model = True`: DeviceIntRegAffRefineLoss, DeviceIntRegAffLoss, which
    need the model on the batch and on a transformed copy of it) are called as `loss_fn(model, micro_batch, transform=T)`
    instead of on the model's output, and may return any number of terms: `loss_factors` may be the reference's whole
    LOSS_FACTORS ([2.0, 1.0, 0.5, 0.5]), of which the first len(terms) are used (job_runner.py:668-669).  The FIRST term is a
    sum over samples and adds up; EVERY later term (aff, seg, enc) is a batch mean and enters with the micro-batch's share,
    the rule -- and, for statistics of the micro-batch inside such a term, the documented deviation -- of `seg` above.
    `step` returns all terms.  T is drawn ONCE per step (`loss_fn.draw()`) and passed to every micro-batch: a step is one
    transform on the rank's batch, as in the reference.  Such a loss records two forward tapes per backward, so the engine's
    gradient sink would see every parameter twice and `_grad_sink` refuses a second delivery once the bucket is sent: for
    these losses the sink stays off and every bucket is reduced after the last backward, exactly the `overlap=False` path.

    `optimizer` is any torch.optim.Optimizer over the model's parameters; dram_amd.optim.Adam / AdamW / SGD / RAdam /
    AdaBound (one HIP launch per parameter group, bucket views at any offset included) go in unchanged.

    `max_grad_norm` (default None: no clipping, the step as it always was) clips the global gradient norm of kind
    `grad_norm_type` (2.0 or inf) on the device: the norm is that of the SUMMED gradient, after the all-reduce, i.e. of the
    global batch whatever the rank count.  An optimiser with `set_grad_clip` (dram_amd.optim's) takes it into its own step();
    any other one gets dram_amd.optim.clip_grad_norm_ between the all-reduce and its step().  `last_grad_norm` is the 0-dim
    device tensor of the norm before clipping after every step."""

    def __init__(self, model, optimizer, loss_fn=None, loss_factors=(2.0, 1.0), bucket_mb=32, overlap=True, max_grad_norm=None,
                 grad_norm_type=2.0):
        self.model, self.opt = model, optimizer
        self.max_grad_norm, self.grad_norm_type = max_grad_norm, grad_norm_type
        self.last_grad_norm = None
        self._clip_in_opt = max_grad_norm is not None and hasattr(optimizer, "set_grad_clip")
        if self._clip_in_opt:
            optimizer.set_grad_clip(max_grad_norm, grad_norm_type)
        elif max_grad_norm is not None:
            from .optim import _norm_kind
            _norm_kind(grad_norm_type)             # refuse an unsupported norm here, not at the first step
        self.overlap = bool(overlap)               # False: every bucket is reduced after the last backward (A/B, diagnostics)
        self.loss_fn = loss_fn or DeviceIntRegRefineLoss()
        self.calls_model = bool(getattr(self.loss_fn, "calls_model", False))
        self.loss_factors = loss_factors           # LOSS_FACTORS of st_dram_ref.py:42: the first len(terms) are used
        self.world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        self.params = [p for p in model.parameters() if p.requires_grad]
        self.buckets = self._make_buckets(bucket_mb * (1 << 20))
        self._slot = {}                            # id(parameter) -> (bucket index, offset)
        for bi, bucket in enumerate(self.buckets):
            off = 0
            for p in bucket:
                self._slot[id(p)] = (bi, off)
                off += p.numel()
        self._flat = [None] * len(self.buckets)    # persistent flat buffers (allocated at the first reduction)
        self._filled = [set() for _ in self.buckets]
        self._works = [None] * len(self.buckets)
        self.overlapped_buckets = 0                # (diagnostics) buckets whose all-reduce started inside the last backward

    def _make_buckets(self, cap_bytes):
        buckets, cur, size = [], [], 0
        for p in reversed(self.params):            # reverse: roughly the order gradients become ready
            cur.append(p)
            size += p.numel() * 4
            if size >= cap_bytes:
                buckets.append(cur)
                cur, size = [], 0
        if cur:
            buckets.append(cur)
        return buckets

    # ---- gradient exchange
    def _flat_of(self, bi):
        if self._flat[bi] is None:
            p0 = self.buckets[bi][0]
            self._flat[bi] = torch.empty(sum(p.numel() for p in self.buckets[bi]), dtype=p0.dtype, device=p0.device)
        return self._flat[bi]

    def _begin(self):
        for f in self._filled:
            f.clear()
        self._works = [None] * len(self.buckets)

    def _deposit(self, p, g):
        """Write the final gradient of `p` (g, plus whatever p.grad accumulated before; g None: p.grad alone, or zeros) into
        its bucket slot; start the bucket's all-reduce when it is complete."""
        bi, off = self._slot[id(p)]
        view = self._flat_of(bi)[off:off + p.numel()]
        if g is not None and p.grad is not None:
            torch.add(p.grad.reshape(-1), g.reshape(-1), out=view)
        elif g is not None:
            view.copy_(g.reshape(-1))
        elif p.grad is not None:
            if p.grad.data_ptr() != view.data_ptr():
                view.copy_(p.grad.reshape(-1))
        else:
            view.zero_()                            # a parameter without a gradient on this rank still takes part
        self._filled[bi].add(id(p))
        if len(self._filled[bi]) == len(self.buckets[bi]):
            self._works[bi] = dist.all_reduce(self._flat[bi], op=dist.ReduceOp.SUM, async_op=True)

    def _grad_sink(self, p, g):
        """engine.backward's sink during the last micro-batch's backward (see the class docstring)."""
        if id(p) not in self._slot or id(p) in self._filled[self._slot[id(p)][0]]:
            return False
        self._deposit(p, g)
        return True

    def allreduce_gradients(self):
        """Sum the gradients over the ranks (see the class docstring for why a sum): every bucket that backward has not
        already sent is completed from p.grad and sent now; then wait, and point p.grad at the reduced slots."""
        if self.world == 1:
            return
        for bi, bucket in enumerate(self.buckets):
            for p in bucket:
                if id(p) not in self._filled[bi]:
                    self._deposit(p, None)
        for bi, bucket in enumerate(self.buckets):
            self._works[bi].wait()
            off = 0
            for p in bucket:
                n = p.numel()
                p.grad = self._flat[bi][off:off + n].view_as(p)
                off += n
        self._begin()

    def probe(self, batch, micro_batch=None):
        """Forward, loss and backward of the first micro-batch WITHOUT any collective and without the optimiser step, the
        gradients dropped again: "does this micro-batch size fit on this device" as a rank-local question.  A caller with
        several ranks agrees on the answer afterwards (one all-reduce per attempt on every rank, whatever each rank found);
        an out-of-memory error inside `step` instead would leave the ranks with different numbers of collectives issued."""
        n = len(batch)
        mb = n if not micro_batch else min(micro_batch, n)
        self.opt.zero_grad(set_to_none=True)
        try:
            if self.calls_model:
                batch.ctss_device()
            terms = self._terms(batch.micro(0, mb), self.loss_fn.draw() if self.calls_model else None)
            self._weighted(terms, None).backward()
        finally:
            self.opt.zero_grad(set_to_none=True)

    def _terms(self, b, transform):
        """The loss terms of one micro-batch, in either calling convention (see the class docstring)."""
        if self.calls_model:
            return tuple(self.loss_fn(self.model, b, transform=transform))
        dense, refined = self.model(b.images, b.lobes)
        return tuple(self.loss_fn(dense, b, refined=None if refined is dense else refined))

    def _weighted(self, terms, share):
        """sum_k loss_factors[k] * terms[k] (job_runner.py:668-669: the first len(terms) factors); every term but the first
        times `share` where one is given."""
        if len(self.loss_factors) < len(terms):
            raise ValueError(f"the loss returns {len(terms)} terms, loss_factors has {len(self.loss_factors)}")
        loss = self.loss_factors[0] * terms[0]
        for f, t in zip(self.loss_factors[1:], terms[1:]):
            loss = loss + (f * t if share is None else f * t * share)
        return loss

    def step(self, batch, micro_batch=None, global_batch=None):
        """Returns the (detached, device) loss components of this rank's batch, as many as the loss returns: the first
        (reg) summed, every later one weighted by the share of the global batch.  `global_batch`: number of chunks over
        all ranks (default: every rank holds as many as this one)."""
        n = len(batch)
        n_glob = int(global_batch) if global_batch else n * self.world
        mb = n if not micro_batch else min(micro_batch, n)
        self.opt.zero_grad(set_to_none=True)
        self._begin()
        self.overlapped_buckets = 0
        transform = None
        if self.calls_model:
            transform = self.loss_fn.draw()        # ONE transform per step, the same for every micro-batch
            batch.ctss_device()                    # (uploaded once per batch; the micro-batches take slices)
        totals = None
        starts = list(range(0, n, mb))
        for lo in starts:
            b = batch.micro(lo, min(n, lo + mb))
            terms = self._terms(b, transform)
            share = len(b) / n_glob
            loss = self._weighted(terms, share)
            overlap = self.overlap and not self.calls_model and self.world > 1 and lo == starts[-1]
            if overlap:
                self.model.grad_sink = self._grad_sink
            try:
                loss.backward()
            finally:
                if overlap:
                    self.model.grad_sink = None
                    self.overlapped_buckets = sum(w is not None for w in self._works)
            parts = [terms[0].detach()] + [t.detach() * share for t in terms[1:]]
            totals = parts if totals is None else [a + p for a, p in zip(totals, parts)]
        self.allreduce_gradients()
        if self.max_grad_norm is None:
            self.opt.step()
        elif self._clip_in_opt:
            self.opt.step()
            self.last_grad_norm = self.opt.last_grad_norm
        else:
            from .optim import clip_grad_norm_
            self.last_grad_norm = clip_grad_norm_(self.params, self.max_grad_norm, self.grad_norm_type)
            self.opt.step()
        return tuple(totals)


class DeviceIntRegAffRefineLoss:
    """IntRegAffRefineLoss.__call__ (reference dram/metrics.py:376-462) on the device: the interval-regression and
    pseudo-label losses of IntRegRefineLoss on a batch AND on an affinely transformed copy of it, plus the
    consistency terms smooth_l1(T(sigmoid(dense)), sigmoid(dense_T)) and smooth_l1(T(cls), cls_T) inside the
    transformed lobes.  The random transform T (rescale / flip / rot90 drawn as the reference draws them: same
    `random` / `numpy.random` calls in the same order) runs on the OneShot kernels of dram_amd/transforms.py and
    stays differentiable for the predictions.  The model returns (dense, refined, cls) like the 3-output
    variants this loss was written for (metrics.py:432).  Returns (reg, aff, seg) as the reference does."""

    def __init__(self, rescale_jitter, band_width=5e-2, smoothing=0.05, freq_map=None):
        self.rescale_jitter, self.band_width, self.smoothing = rescale_jitter, band_width, smoothing
        self.freq_map = freq_map or {k: 1.0 / 6 for k in range(6)}
        self.loss = DeviceIntRegRefineLoss(band_width, smoothing)

    def get_affine_transform(self):
        """metrics.py:391-416: the three OneShot transforms in a random order, each kept with probability 1/2."""
        import itertools
        import random

        import numpy as np

        from .transforms import Flip3DOneShot, Rescale3DOneShot, Rotate903DOneShot
        pool = [Rescale3DOneShot(self.rescale_jitter, None, mode='size'), Flip3DOneShot(), Rotate903DOneShot()]
        order = list(random.sample(list(itertools.permutations(pool, 3)), 1)[0])
        chosen = [t for t in order if np.random.randint(0, 10) < (10 * 0.5)]

        def apply(sample):
            for t in chosen:
                sample = t(sample)
            return sample
        apply.p = chosen
        return apply

    calls_model = True      # DataParallelTrainer: call loss_fn(model, batch, transform=T), not loss_fn(model(batch), batch)

    def draw(self):
        """One random transform T, for `__call__(..., transform=T)`: every host-side random draw of the loss happens here."""
        return self.get_affine_transform()

    def __call__(self, model, batch, transform=None):
        """`transform`: a T from `draw()` (the trainer passes one T to every micro-batch of a step); None draws one.  With a
        given T the call reads nothing back from the device: the transformed copy's regression targets come from
        `Batch.on_device`, the scores from `batch.ctss_device()` (uploaded once per batch)."""
        from . import functional as HF
        batch.require_targets("DeviceIntRegAffRefineLoss")
        T = self.draw() if transform is None else transform
        aff_images = T({"#image": batch.images})["#image"]
        aff_lobes = T({"#reference": batch.lobes})["#reference"].contiguous()
        aff_lesions = T({"#reference": batch.lesions})["#reference"].contiguous()
        dense, refined, cls = model(batch.images, batch.lobes)
        reg, seg = self.loss(dense, batch, refined=refined)
        probs_T = T({"#image": HF.sigmoid(dense)})["#image"]
        cls_T = T({"#image": cls})["#image"]
        aff = Batch.on_device(aff_images.detach(), aff_lobes, aff_lesions, batch.ctss_device(), self.freq_map,
                              band_width=self.band_width, ctss=batch.ctss)
        a_dense, a_refined, a_cls = model(aff.images, aff.lobes)
        a_reg, a_seg = self.loss(a_dense, aff, refined=a_refined)
        aff_loss = HF.masked_smooth_l1(probs_T, HF.sigmoid(a_dense), aff.lobes)
        aff_loss_cls = HF.masked_smooth_l1(cls_T, a_cls, aff.lobes)
        return (reg + a_reg) / 2.0, (aff_loss + aff_loss_cls) / 2.0, (seg + a_seg) / 2.0


class DeviceIntRegAffLoss:
    """IntRegAffLoss.__call__ (reference dram/metrics.py:245-308) on the device: the interval regression of IntRegLoss on a
    batch AND on an affinely transformed copy of it (compute_reg_loss, metrics.py:191-195: the model's FIRST output), the
    consistency term smooth_l1(T(sigmoid(dense)), sigmoid(dense_T)) inside the transformed lobes, and the entropy of the
    un-transformed probabilities.  T is drawn as get_affine_transform draws it (metrics.py:219-243: the pool and the order of
    the `random` / `numpy.random` calls of DeviceIntRegAffRefineLoss, each transform kept with probability 0.6).  The model
    returns three outputs.  Returns (reg, aff, enc) as the reference does; its `trace` image dumps are not restated."""

    def __init__(self, rescale_jitter, band_width=5e-2, freq_map=None):
        self.rescale_jitter, self.band_width = rescale_jitter, band_width
        self.freq_map = freq_map or {k: 1.0 / 6 for k in range(6)}
        self.loss = DeviceIntRegLoss(band_width)

    def get_affine_transform(self):
        """metrics.py:219-243: the three OneShot transforms in a random order, each kept with probability 0.6."""
        import itertools
        import random

        import numpy as np

        from .transforms import Flip3DOneShot, Rescale3DOneShot, Rotate903DOneShot
        pool = [Rescale3DOneShot(self.rescale_jitter, None, mode='size'), Flip3DOneShot(), Rotate903DOneShot()]
        order = list(random.sample(list(itertools.permutations(pool, 3)), 1)[0])
        chosen = [t for t in order if np.random.randint(0, 10) < 6]

        def apply(sample):
            for t in chosen:
                sample = t(sample)
            return sample
        apply.p = chosen
        return apply

    calls_model = True      # as DeviceIntRegAffRefineLoss

    def draw(self):
        """One random transform T, for `__call__(..., transform=T)`: every host-side random draw of the loss happens here."""
        return self.get_affine_transform()

    def __call__(self, model, batch, transform=None):
        """`transform`: as DeviceIntRegAffRefineLoss.__call__."""
        from . import functional as HF
        batch.require_targets("DeviceIntRegAffLoss")
        T = self.draw() if transform is None else transform
        aff_images = T({"#image": batch.images})["#image"]
        aff_lobes = T({"#reference": batch.lobes})["#reference"].contiguous()
        aff_lesions = T({"#reference": batch.lesions})["#reference"].contiguous()
        dense = model(batch.images, batch.lobes)[0]
        reg, enc = self.loss(dense, batch)
        probs_T = T({"#image": HF.sigmoid(dense)})["#image"]
        aff = Batch.on_device(aff_images.detach(), aff_lobes, aff_lesions, batch.ctss_device(), self.freq_map,
                              band_width=self.band_width, ctss=batch.ctss)
        a_dense = model(aff.images, aff.lobes)[0]
        a_reg, _ = self.loss(a_dense, aff)
        aff_loss = HF.masked_smooth_l1(probs_T, HF.sigmoid(a_dense), aff.lobes)
        return (reg + a_reg) / 2.0, aff_loss, enc
