"""Whole-scan, per-lobe inference on the GPU.

Device-resident restatement of the reference's working inference semantics,
`LesionSegChunkTrain.evaluate_scan` (dram/job_runner.py:720-779): for every lobe label, crop
its bounding box (+5 mm), mask outside-lobe voxels to -2048 HU, window (-1000,-300) -> [0,1],
resample to RESAMPLE_SIZE (80^3), run the model, sigmoid, resize back to the crop size and paste
where the lobe is; then the thresholding of `LesionSegTest.run` (job_runner.py:1003-1005):
Otsu on the 8-bit heat map inside the lungs (`binary_cam`, dram/utils.py:226-242), mask = htp > th.

Differences from the reference, on purpose: the lobes (every non-zero label of the map, like
`np.unique(lobe)[1:]`; normally 5) go through the model in batches of up to 8 chunks; the scan and the label map are uploaded once and every step runs on the device
(the reference round-trips each lobe through numpy and SimpleITK).  The crop -> 80^3 resampling restates the grid of the
reference's call -- sitk.ResampleImageFilter with the identity transform, the crop's own origin and the output spacing
spacing * size_in / size_out, linear, default value 0 (utils.py:371-381) -- from ITK's published semantics: output voxel o
samples continuous input index o * size_in / size_out, zero beyond size_in - 0.5 (csrc/infer.hip:itk_index).  SimpleITK is not
available here, so that step's parity is unpinned; the way back is the reference's own F.interpolate(align_corners=True).

`LobeInference(head="cam")` runs the head of the reference's inference entry point instead (`LesionSegTest.run`,
job_runner.py:985-1004; csrc/infer_cam.hip): the dense output is pooled over the resampled lobe mask, the arg-max is the lobe's
class (torch.max's rule: first of equal maxima, a NaN counts as the maximum), and what is pasted is the ReLU'd map of that
class's channel divided by its maximum over the crop -- zero for class 0, and NaN where the reference gives NaN (a channel that
is <= 0 over the whole crop).  It is meant for `out_ch > 1` models; with one channel every lobe is class 0 and the map is zero.
The result then also holds `lobe_cls` ({label: class}), `pool` ([lobes, out_ch]) and `lobe_mask`; `lobewise_records` turns
`lobe_cls` into the reference's lobe-wise records.

`LobeInference(tta=...)` is test-time augmentation, which the reference does not have: every chunk goes through the model in V
signed-permutation views (`tta_views`; the flips and 90-degree rotations the model is trained to be consistent under), the heat
map is the mean of the V sigmoid maps and the result gains `spread`, their population standard deviation -- both formed at the
chunk's resolution, then resized and pasted like the single-view map (include/dram_hip.h, "test-time augmentation";
csrc/infer_tta.hip).  `tta=None` (the default) is the path described above, unchanged.

`LobeInference(refine=...)` adds an edge-aware refinement of the finished heat map, which the reference does not have either:
the masked 3-D guided filter of `dram_amd.refine`, guided by the scan inside the lobes.  The result gains `htp_refined`,
`threshold_refined` and `mask_refined`, and `post_process` the same judgement of the refined map beside that of the map as it
is.  Whether it improves a metric on real scans has not been measured; with `curves=` a user with labels measures it in one
call.  `refine=None` (the default) changes nothing.
"""
import ctypes
import itertools
import math

import numpy as np
import torch

from . import _lib
from ._lib import call

# IntRegLoss.ctss_ratio_map / ratio_to_label (dram/metrics.py:76-83, 108-114)
CTSS_RATIO_MAP = {0: (0.0, 0.001), 1: (0.001, 0.01), 2: (0.01, 0.05), 3: (0.05, 0.35), 4: (0.35, 0.5), 5: (0.5, 1.00001)}


def ratio_to_label(ratio):
    return [k for k, (lo, hi) in CTSS_RATIO_MAP.items() if lo <= ratio < hi][0]


def otsu_threshold_from_hist(hist):
    """skimage.filters.threshold_otsu on a uint8 image, restated from its published algorithm
    (maximise the between-class variance over the histogram of the occupied value range) and
    evaluated on the 256-bin histogram.  Returns the threshold in 0..255."""
    hist = np.asarray(hist, dtype=np.float64)
    nz = np.nonzero(hist)[0]
    lo, hi = int(nz[0]), int(nz[-1])
    h = hist[lo:hi + 1]
    centers = np.arange(lo, hi + 1, dtype=np.float64)
    w1 = np.cumsum(h)
    w2 = np.cumsum(h[::-1])[::-1]
    m1 = np.cumsum(h * centers) / w1
    m2 = (np.cumsum((h * centers)[::-1]) / w2[::-1])[::-1]
    var12 = w1[:-1] * w2[1:] * (m1[:-1] - m2[1:]) ** 2
    return float(centers[int(np.argmax(var12))])


def binary_cam_threshold(hist, scaler=1.0):
    """`binary_cam` (dram/utils.py:226-242) on the 8-bit histogram: returns th / 255."""
    hist = np.asarray(hist)
    if np.count_nonzero(hist) < 2:                      # only one colour
        return float(np.nonzero(hist)[0][0]) / 255.0
    return min(otsu_threshold_from_hist(hist) * scaler, 255.0) / 255.0


_RESAMPLE_KINDS = {torch.uint8: 0, torch.int16: 1, torch.float32: 2}

TTA_MAX_VIEWS = 48     # DRAM_TTA_MAX_VIEWS (include/dram_hip.h): the signed permutations of three axes


def tta_views(kind):
    """The views of test-time augmentation as a tuple of (perm, flip) pairs in `dram_spatial_permute_flip`'s convention
    (viewed[o] = x[i], i[perm[k]] = flip[k] ? R-1-o[k] : o[k]).
    "flip": the 8 flip combinations under the identity permutation, ordered by the flip bits read as a binary number with z
    the high bit -- the identity first.  "full": all 48 signed permutations, by permutation in lexicographic order, then by
    flips as above -- the identity first.  Anything else is taken as a sequence of (perm, flip) pairs, validated (1 to 48
    views, perm a permutation of (0, 1, 2), flips 0 or 1; a repeated view counts that many times) and returned."""
    flips = [((n >> 2) & 1, (n >> 1) & 1, n & 1) for n in range(8)]
    if isinstance(kind, str):
        if kind == "flip":
            return tuple(((0, 1, 2), f) for f in flips)
        if kind == "full":
            return tuple((p, f) for p in itertools.permutations(range(3)) for f in flips)
        raise ValueError(f"tta_views: unknown kind {kind!r} ('flip', 'full' or a sequence of (perm, flip) pairs)")
    try:
        views = tuple((tuple(perm), tuple(flip)) for perm, flip in kind)
    except TypeError:
        raise ValueError("tta_views: 'flip', 'full' or a sequence of (perm, flip) pairs") from None
    if not 1 <= len(views) <= TTA_MAX_VIEWS:
        raise ValueError(f"tta_views: between 1 and {TTA_MAX_VIEWS} views, got {len(views)}")
    out = []
    for perm, flip in views:
        if len(perm) != 3 or any(isinstance(a, bool) or not isinstance(a, (int, np.integer)) for a in perm) or \
                sorted(int(a) for a in perm) != [0, 1, 2]:
            raise ValueError(f"tta_views: perm {perm!r} is not a permutation of (0, 1, 2)")
        if len(flip) != 3 or any(not isinstance(f, (bool, int, np.integer)) or int(f) not in (0, 1) for f in flip):
            raise ValueError(f"tta_views: flip {flip!r}: three values, each 0 or 1")
        out.append((tuple(int(a) for a in perm), tuple(int(f) for f in flip)))
    return tuple(out)


def resample_volume(vol, spacing, required_spacing, new_size, interpolator="linear"):
    """`utils.resample(narray, spacing, required_spacing=..., new_size=..., interpolator=...)` (dram/utils.py:414-434) of a
    device volume [D,H,W] (uint8 / int16 / float32; the pixel type is kept like sitk's `orig_pixelid`): the grid of
    sitk.ResampleImageFilter restated from ITK's published semantics (csrc/infer.hip: resample_volume_kernel; SimpleITK is not
    available, parity unpinned).  spacing / required_spacing / new_size in (z, y, x) order like the reference's numpy side."""
    if interpolator not in ("nearest", "linear"):
        raise NotImplementedError(f"interpolator {interpolator!r}: the reference's inference uses 'nearest' and 'linear'")
    if vol.dim() != 3 or vol.dtype not in _RESAMPLE_KINDS or not vol.is_cuda:
        raise ValueError("resample_volume: a [D,H,W] uint8 / int16 / float32 tensor on the GPU")
    vol = vol.contiguous()
    size = [int(v) for v in new_size]
    out = torch.empty(size, dtype=vol.dtype, device=vol.device)
    sp_in = (ctypes.c_double * 3)(*[float(v) for v in spacing])
    sp_out = (ctypes.c_double * 3)(*[float(v) for v in required_spacing])
    call("dram_resample_volume", vol.data_ptr(), out.data_ptr(), _RESAMPLE_KINDS[vol.dtype], int(interpolator == "linear"),
         *vol.shape, *size, sp_in, sp_out, torch.cuda.current_stream().cuda_stream)
    return out


def crop_list(boxes, shape, spacing, border, max_labels):
    """The crops from the labels' boxes, boxes[label - 1] = (min z, y, x, max z, y, x) inclusive, min > max for an absent label
    (dram_label_bboxes): one [z0, y0, x0, dz, dy, dx, label] per label present in 1..max_labels, ascending, the box widened by
    ceil(border / spacing) voxels per axis and clipped to the volume (find_crops, utils.py:244-254)."""
    chunks = []
    for label in range(1, max_labels + 1):
        lo, hi = boxes[label - 1][:3], boxes[label - 1][3:]
        if hi[0] < lo[0]:
            continue                                                         # label absent (np.unique(lobe)[1:])
        start, stop = [], []
        for l, h, size, sp in zip(lo, hi, shape, spacing):
            pad = int(math.ceil(border / sp)) if border > 0 else 0
            start.append(max(0, int(l) - pad))
            stop.append(min(int(size), int(h) + 1 + pad))
        chunks.append(start + [b - a for a, b in zip(start, stop)] + [label])
    return chunks


class LobeInference:
    """model: a models.DC3D on the GPU.  run(scan_i16, lobe_u8, spacing) -> dict.  Every label 1..max_labels
    present in the uint8 lobe map is visited in ascending order (evaluate_scan: `np.unique(lobe)[1:]`,
    job_runner.py:729); a label above max_labels raises instead of being silently left out of the heat map.
    head: "sigmoid" (default) pastes sigmoid(dense) like evaluate_scan; "cam" runs the lobe-wise class head of
    LesionSegTest.run (module docstring) and adds lobe_cls / pool / lobe_mask to the result.
    tta: None (default: one view, the path above), "flip", "full" or a sequence of (perm, flip) views (`tta_views`): the chunks
    are cropped once, every view of them goes through the model in batches of `tta_batch` chunks, "htp" is the mean of the
    views' sigmoid maps and the result gains "spread" (float32 [D,H,W], their population standard deviation resized and pasted
    like the heat map, zero outside the lobes) and "views"; "input" stays the canonical chunks.  Only with head="sigmoid".
    refine: None (default), True (the defaults of `dram_amd.refine.refine_heatmap`) or a dict with any of radius_mm, eps, window,
    iterations: once the heat map is complete (either head, with or without tta) it is refined, and the result gains
    "htp_refined", "threshold_refined" (`binary_cam` on the refined map inside the lobes) and "mask_refined"."""

    REFINE_KEYS = ("radius_mm", "eps", "window", "iterations")

    MAX_CHUNKS = 8     # chunks per kernel call / model batch (csrc/infer.hip MAX_CHUNKS)

    def __init__(self, model, resample_size=80, window=(-1000.0, -300.0), border_mm=5.0, max_labels=255,
                 post_window=(-1150, 350), post_scaler=0.75, head="sigmoid", tta=None, tta_batch=8, refine=None):
        if not 1 <= int(max_labels) <= 255:
            raise ValueError("max_labels must be in 1..255 (uint8 label map)")
        if head not in ("sigmoid", "cam"):
            raise ValueError("head must be 'sigmoid' (evaluate_scan) or 'cam' (LesionSegTest.run)")
        self.head = head
        self.views = None if tta is None else tta_views(tta)
        if self.views is not None and head == "cam":
            raise NotImplementedError("tta with head='cam': the class head takes an arg-max per lobe, and how the views' "
                                      "classes are to be combined is not defined; test-time augmentation needs head='sigmoid'")
        if isinstance(tta_batch, bool) or not isinstance(tta_batch, (int, np.integer)) or tta_batch < 1:
            raise ValueError("tta_batch must be a positive integer (chunks per model call)")
        self.tta_batch = int(tta_batch)
        if refine is None or refine is True:
            self.refine = None if refine is None else {}
        elif isinstance(refine, dict) and set(refine) <= set(self.REFINE_KEYS):
            self.refine = dict(refine)
        else:
            raise ValueError(f"refine must be None, True or a dict with keys among {self.REFINE_KEYS}")
        self.model, self.R, self.window, self.border, self.max_labels = model, int(resample_size), window, border_mm, int(max_labels)
        # the brightness gate of LesionSegTest.run: windowing()'s default span (utils.py:189, job_runner.py:1006) and the 0.75
        # on its Otsu threshold (job_runner.py:1007)
        self.post_window, self.post_scaler = (int(post_window[0]), int(post_window[1])), float(post_scaler)

    @torch.no_grad()
    def run(self, scan, lobe, spacing, vessel=None, lesion=None, original_spacing=None, original_size=None, curves=None):
        """`vessel` (uint8 [D,H,W], optional): the vessel mask of LesionSegTest.run; with it (or with `lesion`) the result also
        holds the post-processed mask `mask_post` = mask & (windowed scan > brightness threshold) & ~vessel (job_runner.py:1006-1010).
        `vessel` may also be a callable `fn(scan_dev, lobe_dev, spacing) -> uint8 [D,H,W]` that produces the mask; it is called once
        on the device tensors held here (`dram_amd.vessels.pseudo_vessel_mask`, or a functools.partial of it, fits as it is).
        `lesion` (uint8 [D,H,W], optional): the reference mask; adds iou / iou_post / dice / dice_post (job_runner.py:1033-1037),
        computed at the working resolution unless `original_spacing` and `original_size` ((z, y, x), the scan's metadata) are
        given: then, like job_runner.py:1016-1032, the masks (nearest neighbour), the scan and the heat map (linear) first go
        back to the original grid (`resample_volume`; result key "original": mask / mask_post / lesion / scan / htp there) and
        the four metrics are those of the resampled masks.
        `curves` (a number of bins, optional; needs `lesion`): adds "curves" and "curves_post", the evaluation curves of the heat
        map over all thresholds (see `post_process`)."""
        if curves is not None and lesion is None:
            raise ValueError("curves needs the reference mask: pass lesion=")
        dev = next(self.model.parameters()).device
        scan = torch.as_tensor(scan).to(device=dev, dtype=torch.int16).contiguous()
        lobe = torch.as_tensor(lobe).to(device=dev, dtype=torch.uint8).contiguous()
        if scan.dim() != 3 or scan.shape != lobe.shape:
            raise ValueError("scan and lobe must be [D,H,W] arrays of the same shape")
        if callable(vessel):
            vessel = vessel(scan, lobe, spacing)
        chunks = crop_list(self._label_boxes(lobe), scan.shape, spacing, self.border, self.max_labels)
        out = {"htp": torch.zeros(scan.shape, dtype=torch.float32, device=dev)}
        if self.views is not None:
            out.update(spread=torch.zeros_like(out["htp"]), views=self.views)
        if not chunks:
            return self._empty_result(out)
        self._run_groups(chunks, scan, lobe, out)
        htp = out["htp"]
        th, mask, ssum, n_lung, cls_h = self._judge(htp, lobe, out.pop("cls", None))
        ratio = float(ssum.item()) / max(n_lung, 1)                          # (htp * (lobe>0)).sum() / (lobe>0).sum()
        res = {"htp": htp, "mask": mask, "threshold": th, "lesion_ratio": ratio, "ctss": ratio_to_label(ratio), "chunks": chunks, **out}
        if self.head == "cam":
            res.update(lobe_cls={c[6]: int(k) for c, k in zip(chunks, cls_h)}, pool=torch.cat(out["pool"]))
        refined = None
        if self.refine is not None:
            from .refine import refine_heatmap
            htp_r = refine_heatmap(htp, scan, lobe, spacing, **self.refine)
            th_r, mask_r = self._judge(htp_r, lobe)[:2]
            res.update(htp_refined=htp_r, threshold_refined=th_r, mask_refined=mask_r)
            refined = (htp_r, th_r, mask_r)
        if vessel is not None or lesion is not None or original_size is not None:
            res.update(self.post_process(scan, lobe, htp, th, vessel, lesion, mask, spacing=spacing,
                                         original_spacing=original_spacing, original_size=original_size, curves=curves,
                                         refined=refined))
        return res

    def _label_boxes(self, lobe):
        """dram_label_bboxes on the host, [max_labels, 6]: the only sync before the model (a second small one when labels are capped)."""
        D, H, W = lobe.shape
        boxes = torch.empty(self.max_labels * 6, dtype=torch.int32, device=lobe.device)
        call("dram_label_bboxes", lobe.data_ptr(), boxes.data_ptr(), self.max_labels, D, H, W, torch.cuda.current_stream().cuda_stream)
        top = int(lobe.max()) if self.max_labels < 255 else 0
        if top > self.max_labels:
            raise ValueError(f"lobe map holds label {top} > max_labels={self.max_labels}: it would be left out of the "
                             f"heat map while still counting in the lesion ratio")
        return boxes.cpu().numpy().reshape(self.max_labels, 6)

    def _empty_result(self, out):
        """No label in the map: an all-zero heat map judged by hand (there is no histogram to take a threshold from)."""
        mask = torch.zeros(out["htp"].shape, dtype=torch.uint8, device=out["htp"].device)
        res = {"mask": mask, "threshold": 0.0, "lesion_ratio": 0.0, "ctss": 0, "chunks": [], **out}
        if self.head == "cam":
            res["lobe_cls"] = {}
        if self.refine is not None:
            res.update(htp_refined=torch.zeros_like(out["htp"]), threshold_refined=0.0, mask_refined=torch.zeros_like(mask))
        return res

    def _run_groups(self, chunks, scan, lobe, out):
        """Crops every chunk to R^3 (out["input"]) and takes the chunks through the model and into out["htp"] in groups of up to
        MAX_CHUNKS, by the group method of the head; what else a head produces per chunk joins `out` (its group method says)."""
        R, dev, st = self.R, scan.device, torch.cuda.current_stream().cuda_stream
        D, H, W = scan.shape
        x = out["input"] = torch.empty((len(chunks), 1, R, R, R), dtype=torch.float32, device=dev)
        if self.head == "cam":
            out.update(lobe_mask=torch.empty_like(x), cls=torch.empty(len(chunks), dtype=torch.int32, device=dev),
                       cmax=torch.empty(len(chunks), dtype=torch.float32, device=dev), pool=[])
        group = self._cam_group if self.head == "cam" else self._sigmoid_group if self.views is None else self._tta_group
        was_training = self.model.training
        self.model.eval()
        try:
            for g0 in range(0, len(chunks), self.MAX_CHUNKS):
                grp = chunks[g0:g0 + self.MAX_CHUNKS]
                sl, L = slice(g0, g0 + len(grp)), len(grp)
                carr = (ctypes.c_int * (7 * L))(*[v for c in grp for v in c])
                call("dram_lobe_chunks", scan.data_ptr(), lobe.data_ptr(), x[sl].data_ptr(), carr, L, D, H, W, R,
                     float(self.window[0]), float(self.window[1]), st)
                group(out, sl, lobe, carr, L, D, H, W, st)
        finally:
            self.model.train(was_training)
        out.pop("cmax", None)

    def _judge(self, htp, lobe, ride=None):
        """The judgement of a finished map: `binary_cam` on its 8-bit histogram inside the lungs (job_runner.py:1003-1005), mask =
        htp > threshold.  Returns (threshold, mask, the map's fp64 sum inside the lungs, still on the device, the lungs' voxel
        count, `ride` on the host): a few device integers that ride along with the histogram's read-back, this step's one sync."""
        st = torch.cuda.current_stream().cuda_stream
        hist = torch.empty(256 + (0 if ride is None else len(ride)), dtype=torch.int64, device=htp.device)
        ssum = torch.empty(1, dtype=torch.float64, device=htp.device)
        call("dram_lung_hist256", htp.data_ptr(), lobe.data_ptr(), hist.data_ptr(), ssum.data_ptr(), htp.numel(), st)
        if ride is not None:
            hist[256:].copy_(ride)
        hist_h = hist.cpu().numpy()
        th = binary_cam_threshold(hist_h[:256])
        mask = torch.empty(htp.shape, dtype=torch.uint8, device=htp.device)
        call("dram_threshold_mask", htp.data_ptr(), mask.data_ptr(), float(th), htp.numel(), st)
        return th, mask, ssum, int(hist_h[:256].sum()), hist_h[256:]

    SHEET_TITLES = {"mask": "pred_lesion", "mask_post": "pred_lesion_post", "lesion": "lesion", "htp": "pred_cam"}

    @torch.no_grad()
    def sheet(self, res, scan, lesion=None, original=False, **kw):
        """The screenshot sheet of archive_results (job_runner.py:897-904) from a result of `run`: the windowed scan on top, then
        one row each for res["mask"], res["mask_post"] when the run produced it, `lesion` when given, and res["htp"] through the
        jet map; the slices are taken through the reference's coord_mask, pred > 0 | ref > 0.  `dram_amd.sheet.result_sheet` does
        the work and `kw` goes to it (num_slices, alpha, flip_axis, zoom_size, coord_axis, colormap, style, ...; `titles`
        defaults to the reference's).  original=True draws the original-grid volumes of res["original"] instead (a run with
        original_size=; its resampled scan and reference are used, `scan` and `lesion` are not read).  Returns what result_sheet
        returns: None for an empty coord_mask, else the dict with "sheet" on the device.  `run` and `res` are left as they are."""
        from .sheet import result_sheet
        if original:
            if "original" not in res:
                raise ValueError("sheet: original=True needs a run with original_spacing= and original_size=")
            src = res["original"]
            scan, lesion = src["scan"], src.get("lesion")
        else:
            src = res
            dev = res["htp"].device
            scan = torch.as_tensor(scan).to(device=dev, dtype=torch.int16).contiguous()
            if lesion is not None:
                lesion = torch.as_tensor(lesion).to(device=dev, dtype=torch.uint8).contiguous()
        layers = {"mask": src["mask"], "mask_post": src.get("mask_post"), "lesion": lesion, "htp": src["htp"]}
        names = [k for k in ("mask", "mask_post", "lesion", "htp") if layers[k] is not None]
        kw.setdefault("titles", [self.SHEET_TITLES[k] for k in names])
        coord = [src["mask"]] + ([lesion] if lesion is not None else [])
        return result_sheet(scan, [[layers[k]] for k in names], coord, **kw)

    def _sigmoid_group(self, out, sl, lobe, carr, L, D, H, W, st):
        """evaluate_scan for chunks `sl` of out["input"] (L of them, `carr` their boxes): the model's 2nd output
        (job_runner.py:764), sigmoid, resize, paste into out["htp"].  The other two group methods take the same arguments."""
        _, dense = self.model(out["input"][sl], None)
        call("dram_lobe_paste", dense.contiguous().data_ptr(), lobe.data_ptr(), out["htp"].data_ptr(), carr, L, D, H, W, self.R, st)

    def _tta_group(self, out, sl, lobe, carr, L, D, H, W, st):
        """Test-time augmentation for one group of L chunks (csrc/infer_tta.hip): all V views in one launch, the V * L viewed
        chunks through the model in batches of tta_batch -- a batch may end inside one view and start the next --, then mean
        and spread over the views at the chunk's resolution and both pasted in one walk over the crops (out["spread"])."""
        R, V, xg = self.R, len(self.views), out["input"][sl]
        varr = (ctypes.c_int * (6 * V))(*[a for perm, flip in self.views for a in perm + flip])
        xv = torch.empty((V * L, 1, R, R, R), dtype=torch.float32, device=xg.device)
        call("dram_tta_expand", xg.data_ptr(), xv.data_ptr(), L, R, varr, V, st)
        dense = torch.empty_like(xv)
        for b0 in range(0, V * L, self.tta_batch):
            dense[b0:b0 + self.tta_batch].copy_(self.model(xv[b0:b0 + self.tta_batch], None)[1])
        mean = torch.empty((2, L, R, R, R), dtype=torch.float32, device=xg.device)
        call("dram_tta_combine", dense.data_ptr(), mean[0].data_ptr(), mean[1].data_ptr(), L, R, varr, V, st)
        call("dram_lobe_paste_prob", mean[0].data_ptr(), mean[1].data_ptr(), lobe.data_ptr(), out["htp"].data_ptr(),
             out["spread"].data_ptr(), carr, L, D, H, W, R, st)

    def _cam_group(self, out, sl, lobe, carr, L, D, H, W, st):
        """The lobe-wise class head of LesionSegTest.run (job_runner.py:985-1004) for one batch of L chunks: the model sees the
        image chunk and the resampled lobe mask (out["lobe_mask"]), the dense output is pooled over that mask (out["pool"], one
        [L, C] tensor per group), and the class (out["cls"]), the maximum of its ReLU'd map over the crop (out["cmax"]) and the
        paste follow on the device (csrc/infer_cam.hip)."""
        import models
        R, mg, cls, cmax = self.R, out["lobe_mask"][sl], out["cls"][sl], out["cmax"][sl]
        call("dram_lobe_chunk_masks", lobe.data_ptr(), mg.data_ptr(), carr, L, D, H, W, R, st)
        _, dense = self.model(out["input"][sl], mg)                          # the 2nd output (job_runner.py:985)
        dense = dense.contiguous()
        C = int(dense.shape[1])
        pool = models.pooling_dense_features(dense, mg).contiguous()         # [L, C]: masked mean (models.py:45-47)
        out["pool"].append(pool)
        call("dram_lobe_cam_max", dense.data_ptr(), pool.data_ptr(), carr, L, C, R, cls.data_ptr(), cmax.data_ptr(), st)
        call("dram_lobe_cam_paste", dense.data_ptr(), lobe.data_ptr(), out["htp"].data_ptr(), carr, cls.data_ptr(), cmax.data_ptr(),
             L, C, D, H, W, R, st)

    @torch.no_grad()
    def post_process(self, scan, lobe, htp, th, vessel=None, lesion=None, mask=None, spacing=None, original_spacing=None,
                     original_size=None, curves=None, refined=None):
        """The tail of LesionSegTest.run (job_runner.py:1006-1037) on the device: brightness gate
        `binary_cam(w_scan[lobe > 0], 0.75)` on the scan windowed with windowing()'s default span, lesion_pred_post =
        lesion_pred & (w_scan > th) & ~(vessel > 0), the resampling to the scan's original grid when `original_spacing` /
        `original_size` are given (job_runner.py:1016-1032), and IOU / Dice against the reference lesion mask (utils.py:437-446).
        `curves=nbins` (a power of two in 2..4096; needs `lesion`) adds what the reference does not have, the same judgement at
        every threshold instead of the one Otsu point (`dram_amd.curves.heatmap_curves`: ROC-AUC, average precision, the Dice /
        IoU sweep and its best point, a calibration table; one row per lobe label 1..highest present, then the lungs pooled):
        "curves" for the heat map as it is and "curves_post" with the gate behind `mask_post`, (w_scan > brightness threshold) &
        ~vessel.  Both are computed on the grid of the IoU / Dice metrics: the working grid, or with `original_size` the original
        one, from the linearly resampled heat map and the nearest-resampled reference, lobe map and gate.  On the original grid
        the reported `dice` (of a nearest-resampled mask) is therefore not a point of this curve (a linearly resampled map, then
        thresholded); on the working grid `dice` is the curve's value at the cut below `threshold`, up to the bin width.
        `refined` = (htp_refined, threshold_refined, mask_refined) of a `refine=` run adds, under the same conditions as the keys
        above and computed the same way from the refined map: "mask_refined_post" (the same gate), "iou_refined", "dice_refined",
        "iou_refined_post", "dice_refined_post", "curves_refined", "curves_refined_post", and under "original" "htp_refined"
        (linear), "mask_refined" and "mask_refined_post" (nearest)."""
        if curves is not None and lesion is None:
            raise ValueError("curves needs the reference mask: pass lesion=")
        if (original_spacing is None) != (original_size is None) or (original_size is not None and spacing is None):
            raise ValueError("post_process: spacing, original_spacing and original_size go together")
        dev = htp.device
        st = torch.cuda.current_stream().cuda_stream
        n = htp.numel()
        vessel = None if vessel is None else torch.as_tensor(vessel).to(device=dev, dtype=torch.uint8).contiguous()
        if vessel is not None and vessel.shape != htp.shape:
            raise ValueError("vessel mask and scan must have the same shape")
        hist = torch.empty(256, dtype=torch.int64, device=dev)
        call("dram_scan_hist256", scan.data_ptr(), lobe.data_ptr(), hist.data_ptr(), self.post_window[0], self.post_window[1], n, st)
        th_scan = binary_cam_threshold(hist.cpu().numpy(), self.post_scaler)

        def gated(score, cut):
            post = torch.empty(score.shape, dtype=torch.uint8, device=dev)
            call("dram_lesion_post", score.data_ptr(), scan.data_ptr(), None if vessel is None else vessel.data_ptr(), None,
                 post.data_ptr(), float(cut), self.post_window[0], self.post_window[1], float(th_scan), score.numel(), st)
            return post

        # the heat map as it is and, when given, the refined one; `infix` tells their result keys apart
        judged = [{"infix": "", "htp": htp, "th": th, "mask": mask}]
        if refined is not None:
            judged.append({"infix": "_refined", "htp": refined[0], "th": refined[1], "mask": refined[2]})
        out = {"threshold_scan": th_scan}
        for m in judged:
            m["post"] = out[f"mask{m['infix']}_post"] = gated(m["htp"], m["th"])
            if m["mask"] is None and (lesion is not None or original_size is not None):
                m["mask"] = torch.empty(htp.shape, dtype=torch.uint8, device=dev)
                call("dram_threshold_mask", m["htp"].data_ptr(), m["mask"].data_ptr(), float(m["th"]), n, st)
        if lesion is not None:
            lesion = torch.as_tensor(lesion).to(device=dev, dtype=torch.uint8).contiguous()
            if lesion.shape != htp.shape:
                raise ValueError("lesion mask and scan must have the same shape")
        if original_size is not None:
            back = lambda v, how: resample_volume(v, spacing, original_spacing, original_size, how)
            orig = out["original"] = {"scan": back(scan, "linear")}
            if lesion is not None:
                orig["lesion"] = lesion = back(lesion, "nearest")
            for m in judged:
                m.update(htp=back(m["htp"], "linear"), mask=back(m["mask"], "nearest"), post=back(m["post"], "nearest"))
                orig.update({f"htp{m['infix']}": m["htp"], f"mask{m['infix']}": m["mask"], f"mask{m['infix']}_post": m["post"]})
        if curves is not None:
            from .curves import heatmap_curves
            # the gate alone: with a cut of -inf the prediction term of dram_lesion_post is true wherever the score is not NaN, and a
            # NaN score is in bin 0 (never predicted) with or without a gate
            gate, regions, n_regions = gated(htp, float("-inf")), lobe, max(1, int(lobe.max()))
            if original_size is not None:
                regions, gate = back(lobe, "nearest"), back(gate, "nearest")
            n_cal = min(16, int(curves))
            for m in judged:
                out[f"curves{m['infix']}"] = heatmap_curves(m["htp"], lesion, regions, n_regions, None, curves, n_cal)
                out[f"curves{m['infix']}_post"] = heatmap_curves(m["htp"], lesion, regions, n_regions, gate, curves, n_cal)
        if lesion is not None:
            s = 1e-5                                                        # the smooth term of job_runner.py:1033-1037
            for m in judged:
                counts = torch.empty(8, dtype=torch.int64, device=dev)
                call("dram_mask_overlap", m["mask"].data_ptr(), lesion.data_ptr(), counts.data_ptr(), lesion.numel(), st)
                call("dram_mask_overlap", m["post"].data_ptr(), lesion.data_ptr(), counts[4:].data_ptr(), lesion.numel(), st)
                c = [int(v) for v in counts.cpu()]
                out.update({f"iou{m['infix']}": (c[0] + s) / (c[1] + s), f"dice{m['infix']}": (2.0 * c[0] + s) / (c[2] + c[3] + s),
                            f"iou{m['infix']}_post": (c[4] + s) / (c[5] + s),
                            f"dice{m['infix']}_post": (2.0 * c[4] + s) / (c[6] + c[7] + s)})
        return out


def lobewise_records(result, targets, labels=range(1, 6)):
    """The lobe-wise predictions against the targets that LesionSegTest.run collects (job_runner.py:954-960, 988-992, 1033)
    from the result of a `head="cam"` run.  targets: {label: class}.  Returns (preds, targets, acc): the two lists that feed
    the confusion matrix, one entry per label of `labels`, and the scan's accuracy, np.mean over the lobes that are present.
    An absent lobe contributes its target as its prediction to the lists and nothing to acc; with no lobe present acc is
    NaN (the reference's np.mean of an empty list)."""
    lobe_cls = result["lobe_cls"]
    preds, tgts, accs = [], [], []
    for label in labels:
        target = int(targets[label])
        pred = int(lobe_cls[label]) if label in lobe_cls else target
        preds.append(pred)
        tgts.append(target)
        if label in lobe_cls:
            accs.append(pred == target)
    return preds, tgts, float(np.mean(accs)) if accs else float("nan")


def iou(predict, target, smooth=1e-5):
    """dram/utils.py:437-442."""
    predict, target = np.asarray(predict) > 0, np.asarray(target) > 0
    return (np.logical_and(predict, target).sum() + smooth) / (np.logical_or(predict, target).sum() + smooth)


def dice(predict, target, smooth=1e-5):
    """dram/utils.py:444-446."""
    predict, target = np.asarray(predict) > 0, np.asarray(target) > 0
    inter = np.logical_and(predict, target).sum()
    return (2.0 * inter + smooth) / (predict.sum() + target.sum() + smooth)


def synthetic_ct(shape=(300, 512, 512), spacing=(1.0, 0.7, 0.7), seed=7, n_lesions=20):
    """air -1000, lung parenchyma N(-850,60^2) inside 5 disjoint
    ellipsoid "lobes" labelled 1-5, spherical lesions N(-300,80^2) r in [5,20] voxels, body +40."""
    rng = np.random.default_rng(seed)
    D, H, W = shape
    scan = np.full(shape, 40, dtype=np.int16)
    lobe = np.zeros(shape, dtype=np.uint8)
    zz, yy, xx = np.meshgrid(np.arange(D, dtype=np.float32), np.arange(H, dtype=np.float32),
                             np.arange(W, dtype=np.float32), indexing="ij", sparse=True)
    centres = [(0.30, 0.45, 0.27), (0.62, 0.50, 0.27), (0.28, 0.45, 0.73), (0.52, 0.36, 0.73), (0.74, 0.60, 0.73)]
    radii = [(0.17, 0.22, 0.13), (0.17, 0.24, 0.13), (0.13, 0.20, 0.12), (0.10, 0.14, 0.10), (0.13, 0.20, 0.12)]
    for lab, (c, r) in enumerate(zip(centres, radii), start=1):
        m = (((zz - c[0] * D) / (r[0] * D)) ** 2 + ((yy - c[1] * H) / (r[1] * H)) ** 2 + ((xx - c[2] * W) / (r[2] * W)) ** 2) < 1.0
        m &= lobe == 0
        lobe[m] = lab
    lung = lobe > 0
    scan[lung] = rng.normal(-850, 60, size=int(lung.sum())).astype(np.int16)
    idx = np.argwhere(lung)
    for _ in range(n_lesions):
        cz, cy, cx = idx[rng.integers(len(idx))]
        rad = rng.integers(5, 21) * min(1.0, min(shape) / 300.0)
        z0, z1 = max(0, int(cz - rad)), min(D, int(cz + rad) + 1)
        y0, y1 = max(0, int(cy - rad)), min(H, int(cy + rad) + 1)
        x0, x1 = max(0, int(cx - rad)), min(W, int(cx + rad) + 1)
        sub = ((zz[z0:z1] - cz) ** 2 + (yy[:, y0:y1] - cy) ** 2 + (xx[:, :, x0:x1] - cx) ** 2) < rad ** 2
        sub &= lung[z0:z1, y0:y1, x0:x1]
        scan[z0:z1, y0:y1, x0:x1][sub] = rng.normal(-300, 80, size=int(sub.sum())).astype(np.int16)
    return scan, lobe, spacing
