"""Device chunk loader: from raw ragged chunks to the `[N,1,D,H,W]` float tensors a training step takes.

The reference prepares every chunk on the host in two places (csrc/prep.hip spells the arithmetic):

* `RadboudCOVIDLobeVesselChunk.get_data` (dram/dataset.py:450-486): the pseudo-lesion label of the weak supervision --
  `w_scan = windowing(scan, to_span=(0, 1))`, `_, th = binary_cam(w_scan[lobe > 0], 0.75)` (Otsu inside the lobe),
  `lesion_candidate = (w_scan > th) & (lobe > 0)` -- and the vessel mask `(vessel > 0) & (lobe > 0)`;
* `LesionSegChunkTrain.preprocessing()` (dram/job_runner.py:586-597): `Windowing(min, max)` of "#image", then
  `Resample(mode, factor, size)`: linear for the image, nearest neighbour for every "...reference" key
  (data_transforms.py:183-187); `ToTensor` and `.float().cuda().unsqueeze(1)` follow (job_runner.py:658-660).

`ChunkLoader` does both for a whole batch with three launches and no host synchronisation: the chunks (every one with its own
size) are packed back to back into one pinned host buffer per kind, uploaded with non-blocking copies together with a table of
one 48-byte record per sample, and `dram_chunk_hist256` -> `dram_otsu256` -> `dram_chunk_prepare` produce the batch.  The
pseudo-lesion mask is never written at source resolution: it is evaluated at the nearest source voxel of every output voxel,
which is what the reference's nearest-neighbour resample of the full-resolution mask reads.

Deviation, documented: an empty lobe makes the reference raise `IndexError` (`np.unique(...)[0]` of an empty array in
binary_cam); the device cannot raise without a synchronisation, so that sample's threshold is +inf and it gets no candidates.

The resampling grid is ITK's as `dram_resample_volume` restates it (SimpleITK is not available: parity with the library itself
is unpinned, as everywhere else in the tree); the Otsu threshold is `inference.binary_cam_threshold`'s, bit for bit.
"""
import math

import numpy as np
import torch

from ._lib import call

# one record per sample (csrc/prep.hip: ChunkRec): offset in elements, source size, output-to-input index steps (z, y, x)
TABLE_DTYPE = np.dtype([("off", "<i8"), ("D", "<i4"), ("H", "<i4"), ("W", "<i4"), ("pad", "<i4"),
                        ("sz", "<f8"), ("sy", "<f8"), ("sx", "<f8")])
assert TABLE_DTYPE.itemsize == 48

MAX_WO = 2048            # csrc/prep.hip PREP_MAX_WO


def resample_plan(mode, factor, size, spacing, current_size, rng=np.random):
    """`(required_spacing, new_size)` of `Resample(mode, factor, size).__call__` (dram/data_transforms.py:65-181) for a sample
    with `meta["spacing"] = spacing` and `meta["size"] = current_size`, both in (z, y, x) order: what its calls of
    `utils.resample` hand to sitk.ResampleImageFilter.  `required_spacing` is a list of floats (`factor * spacing` when the
    mode leaves it to utils.resample, utils.py:421-424); `new_size` is a list of ints -- where the mode leaves it None it is
    resample_sitk_image's `ceil(size * (spacing / required_spacing))` (utils.py:365-370).  The two random modes draw from
    `rng.uniform` exactly where the reference draws from `np.random.uniform`.  Unknown modes raise NotImplementedError."""
    size = list(size) if size is not None else None
    if mode == "random_spacing":
        f = rng.uniform(factor[0], factor[1])
        require_spacing, new_size = [f] * len(spacing), None
    elif mode == "fixed_factor":
        require_spacing, new_size = None, None
    elif mode == "fixed_spacing":
        if isinstance(factor, (float, int)):
            require_spacing = [factor] * len(spacing)
        elif isinstance(factor, (tuple, list)):
            require_spacing = factor
        else:
            raise TypeError("fixed_spacing: factor is a number or a tuple / list")       # (the reference: UnboundLocalError)
        new_size = None
    elif mode == "inplane_spacing_only":
        assert len(current_size) == 3
        require_spacing, new_size = [spacing[0], factor[1], factor[2]], None
    elif mode == "inplane_resolution_only":
        assert len(current_size) == 3
        require_spacing = [spacing[0], spacing[1] * current_size[1] / size[1], spacing[2] * current_size[2] / size[2]]
        new_size = [current_size[0], size[1], size[2]]
    elif mode == "inplane_resolution_z_spacing":
        assert len(current_size) == 3
        require_spacing = [factor[0], spacing[1] * current_size[1] / size[1], spacing[2] * current_size[2] / size[2]]
        new_size = [int(round(current_size[0] * spacing[0] / factor[0])), size[1], size[2]]
    elif mode == "inplane_resolution_z_jittering":
        assert len(current_size) == 3
        z_spacing = spacing[0] + rng.uniform(-factor, factor)
        require_spacing = [z_spacing, spacing[1] * current_size[1] / size[1], spacing[2] * current_size[2] / size[2]]
        new_size = [int(round(current_size[0] * spacing[0] / z_spacing)), size[1], size[2]]
    elif mode == "inplane_resolution_min_z_spacing":
        assert len(current_size) == 3
        inplane = [spacing[1] * current_size[1] / size[1], spacing[2] * current_size[2] / size[2]]
        if spacing[0] < factor[0]:
            require_spacing = [factor[0]] + inplane
            new_size = [int(round(current_size[0] * spacing[0] / factor[0])), size[1], size[2]]
        else:
            require_spacing = [spacing[0]] + inplane
            new_size = [current_size[0], size[1], size[2]]
    elif mode == "fixed_spacing_min_in_plane_resolution":
        assert len(current_size) == 3
        f = [factor] * 3 if not isinstance(factor, (tuple, list)) else factor
        new_y_size = int(round(current_size[1] * spacing[1] / f[1]))
        if new_y_size > size[1]:
            require_spacing = [spacing[0], spacing[1] * current_size[1] / size[1], spacing[2] * current_size[2] / size[2]]
            new_size = [current_size[0], size[1], size[2]]
        else:
            require_spacing, new_size = [spacing[0], f[1], f[2]], None
    elif mode == "iso_minimal":
        require_spacing, new_size = [np.min(spacing)] * len(spacing), None
    elif mode == "fixed_output_size":
        ratio = current_size[-1] / size[-1]
        require_spacing = [spacing[-1] * ratio] * len(spacing)
        new_size = size[:]
        new_size[0] = int(round(current_size[0] * spacing[0] / require_spacing[0]))
        new_size[1] = int(round(current_size[1] * spacing[1] / require_spacing[1]))
    elif mode == "fixed_size":
        ratios = np.asarray(current_size) / np.asarray(size)
        require_spacing = (spacing * ratios).tolist()
        new_size = size[:]
    elif mode == "spacing_size_match":
        require_spacing, new_size = factor[:], size[:]
    else:
        raise NotImplementedError
    if require_spacing is None:                                      # utils.resample: req_spacing = factor * orig_spacing
        require_spacing = factor * np.asarray(spacing)
    require_spacing = [float(s) for s in require_spacing]
    if new_size is None:                                             # resample_sitk_image, utils.py:365-370
        new_size = np.asarray(current_size) * (np.asarray(spacing, dtype=np.float64) / np.asarray(require_spacing))
        new_size = np.ceil(new_size).astype(int)
    return require_spacing, [int(s) for s in new_size]


def _as_numpy(v, dtype, what):
    a = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    if a.dtype != dtype:
        raise TypeError(f"{what}: dtype {a.dtype}, expected {np.dtype(dtype)}")
    if a.ndim != 3:
        raise ValueError(f"{what}: a [D,H,W] array, got shape {a.shape}")
    return a


class PackedChunks:
    """What `ChunkLoader.pack` returns: the pinned host buffers (`scans` int16, `lobes` uint8, `vessels` uint8 or None, `table`
    uint8 view of N 48-byte records), their device copies (`d_*`, None when packed without a device), and the per-sample plan
    (`sizes`: output size per sample, `steps`, `offsets`)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __len__(self):
        return len(self.sizes)


class ChunkLoader:
    """`loader(loader.pack(chunks))` -> {"#image", "#lobe_reference", "#pseudo_lesion_reference", "#vessel_reference"?,
    "threshold"}: `[N,1,D,H,W]` float32 device tensors (threshold: `[N]` float64), the chunks windowed to `window`, resampled by
    `Resample(mode, factor, resample_size)` and labelled as get_data labels them (module docstring).  `window`: the
    WINDOWING_MIN / WINDOWING_MAX of the preprocessing, values that fp32 holds exactly; `pseudo_window` / `pseudo_scaler`:
    windowing()'s default span and the 0.75 of dataset.py:461-462."""

    def __init__(self, resample_size, window, pseudo_window=(-1150, 350), pseudo_scaler=0.75, mode="fixed_size", factor=None):
        self.size = [int(v) for v in ((resample_size,) * 3 if isinstance(resample_size, int) else resample_size)]
        if len(self.size) != 3 or min(self.size) <= 0:
            raise ValueError("resample_size: three positive ints (z, y, x)")
        self.window = (float(window[0]), float(window[1]))
        if not self.window[1] > self.window[0]:
            raise ValueError("window: max must exceed min")
        if any(float(np.float32(w)) != w for w in self.window):
            raise ValueError("window: bounds must be exactly representable in float32 (the image is windowed in float32)")
        self.pseudo_window = (int(pseudo_window[0]), int(pseudo_window[1]))
        if not self.pseudo_window[1] > self.pseudo_window[0] or tuple(pseudo_window) != self.pseudo_window:
            raise ValueError("pseudo_window: two integers (HU), max above min")
        self.pseudo_scaler = float(pseudo_scaler)
        self.mode, self.factor = mode, factor

    def plan(self, spacing, current_size, rng=np.random):
        return resample_plan(self.mode, self.factor, self.size, spacing, current_size, rng)

    def pack(self, chunks, device="cuda", rng=np.random):
        """chunks: dicts with "#image" (int16 [D,H,W]), "#lobe_reference" (uint8, same shape), optionally "#vessel_reference"
        (uint8; in all chunks or in none), and meta["spacing"] (z, y, x); numpy arrays or torch tensors.  One pinned host
        buffer per kind plus the table, uploaded to `device` with non-blocking copies (device=None: host side only)."""
        if len(chunks) == 0:
            raise ValueError("pack: no chunks")
        with_vessel = ["#vessel_reference" in c for c in chunks]
        if any(with_vessel) and not all(with_vessel):
            raise ValueError("pack: '#vessel_reference' must be in every chunk or in none")
        arrays, table = [], np.zeros(len(chunks), dtype=TABLE_DTYPE)
        sizes, steps, off = [], [], 0
        for i, c in enumerate(chunks):
            scan = _as_numpy(c["#image"], np.int16, f"chunk {i} '#image'")
            lobe = _as_numpy(c["#lobe_reference"], np.uint8, f"chunk {i} '#lobe_reference'")
            ves = _as_numpy(c["#vessel_reference"], np.uint8, f"chunk {i} '#vessel_reference'") if with_vessel[0] else None
            for name, m in (("#lobe_reference", lobe), ("#vessel_reference", ves)):
                if m is not None and m.shape != scan.shape:
                    raise ValueError(f"chunk {i}: '{name}' has shape {m.shape}, '#image' {scan.shape}")
            spacing = c["meta"]["spacing"]
            if len(spacing) != 3 or not all(float(s) > 0 for s in spacing):
                raise ValueError(f"chunk {i}: meta['spacing'] must be three positive numbers")
            req, new_size = self.plan(spacing, scan.shape, rng)
            step = [float(req[a]) / float(spacing[a]) for a in range(3)]
            if not all(math.isfinite(s) and s > 0 for s in step):
                raise ValueError(f"chunk {i}: resampling steps {step}")
            table[i] = (off, scan.shape[0], scan.shape[1], scan.shape[2], 0, step[0], step[1], step[2])
            arrays.append((scan, lobe, ves))
            sizes.append(tuple(new_size))
            steps.append(tuple(step))
            off += scan.size
        pin = device is not None and torch.cuda.is_available()
        total = off

        def host(dtype):
            return torch.empty(total, dtype=dtype, pin_memory=pin)
        scans, lobes = host(torch.int16), host(torch.uint8)
        vessels = host(torch.uint8) if with_vessel[0] else None
        for rec, (scan, lobe, ves) in zip(table, arrays):
            lo, hi = int(rec["off"]), int(rec["off"]) + scan.size
            scans.numpy()[lo:hi] = scan.reshape(-1)
            lobes.numpy()[lo:hi] = lobe.reshape(-1)
            if ves is not None:
                vessels.numpy()[lo:hi] = ves.reshape(-1)
        tab = torch.empty(table.nbytes, dtype=torch.uint8, pin_memory=pin)
        tab.numpy()[:] = table.view(np.uint8)
        packed = PackedChunks(scans=scans, lobes=lobes, vessels=vessels, table=tab, sizes=sizes, steps=steps,
                              offsets=[int(o) for o in table["off"]], d_scans=None, d_lobes=None, d_vessels=None, d_table=None)
        if device is not None:
            up = lambda t: None if t is None else t.to(device, non_blocking=True)
            packed.d_scans, packed.d_lobes, packed.d_vessels, packed.d_table = up(scans), up(lobes), up(vessels), up(tab)
        return packed

    def __call__(self, packed):
        if len(set(packed.sizes)) != 1:
            raise ValueError(f"mode {self.mode!r} gives the samples different output sizes {sorted(set(packed.sizes))}: they "
                             f"cannot form one batch (use resample_one per sample)")
        if packed.d_scans is None:
            raise ValueError("the chunks were packed without a device (pack(..., device=None))")
        Do, Ho, Wo = packed.sizes[0]
        if Wo > MAX_WO:
            raise ValueError(f"output rows of up to {MAX_WO} voxels, got {Wo}")
        N, dev = len(packed), packed.d_scans.device
        st = torch.cuda.current_stream(dev).cuda_stream
        hist = torch.empty((N, 256), dtype=torch.int64, device=dev)
        th = torch.empty(N, dtype=torch.float64, device=dev)
        out = [torch.empty((N, 1, Do, Ho, Wo), dtype=torch.float32, device=dev) for _ in range(4 if packed.d_vessels is not None else 3)]
        call("dram_chunk_hist256", packed.d_scans.data_ptr(), packed.d_lobes.data_ptr(), packed.d_table.data_ptr(), N,
             hist.data_ptr(), self.pseudo_window[0], self.pseudo_window[1], st)
        call("dram_otsu256", hist.data_ptr(), N, self.pseudo_scaler, th.data_ptr(), st)
        call("dram_chunk_prepare", packed.d_scans.data_ptr(), packed.d_lobes.data_ptr(),
             None if packed.d_vessels is None else packed.d_vessels.data_ptr(), packed.d_table.data_ptr(), th.data_ptr(), N,
             Do, Ho, Wo, self.window[0], self.window[1], self.pseudo_window[0], self.pseudo_window[1], out[0].data_ptr(),
             out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr() if len(out) == 4 else None, st)
        res = {"#image": out[0], "#lobe_reference": out[1], "#pseudo_lesion_reference": out[2], "threshold": th}
        if len(out) == 4:
            res["#vessel_reference"] = out[3]
        return res

    def resample_one(self, sample, rng=np.random):
        """`Resample(mode, factor, size)(sample)` for ONE sample on the device, for the modes whose output size depends on
        the sample: every "#" key goes through `inference.resample_volume` -- nearest neighbour for "reference" / "weight_map"
        keys, linear otherwise (data_transforms.py:183-187), 3-D arrays as they are, 4-D arrays channel by channel; the pixel
        type is kept, as sitk keeps it (uint8 / int16 / float32).  meta: spacing, size, size_before_resample as the
        reference leaves them (data_transforms.py:205-209)."""
        from .inference import resample_volume
        spacing = sample["meta"]["spacing"]
        first = next(v for k, v in sample.items() if "#" in k)
        current = tuple(sample["meta"].get("size", tuple(first.shape[-3:])))
        req, new_size = self.plan(spacing, current, rng)
        out = {}
        for k, v in sample.items():
            if "#" not in k:
                out[k] = v
                continue
            how = "nearest" if ("reference" in k or "weight_map" in k) else "linear"
            t = torch.as_tensor(v).cuda()
            if t.dim() == 4:
                out[k] = torch.stack([resample_volume(c, spacing, req, new_size, how) for c in t], dim=0)
            elif t.dim() == 3:
                out[k] = resample_volume(t, spacing, req, new_size, how)
            else:
                raise NotImplementedError
        out["meta"] = dict(sample["meta"], spacing=tuple(req), size=tuple(new_size), size_before_resample=current)
        return out
