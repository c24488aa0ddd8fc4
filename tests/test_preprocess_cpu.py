"""Host side of the device chunk loader (dram_amd/preprocess.py): the resample plan of every `Resample` mode against what the
reference's own class asked of the resampler (tests/golden/preprocess.json, written by scripts/make_golden_preprocess.py),
the packed buffers and table, and the argument errors.  No kernel is launched."""
import json
import os

import numpy as np
import pytest
import torch

import preprocess_cases as PC
from dram_amd.preprocess import MAX_WO, TABLE_DTYPE, ChunkLoader, resample_plan


def test_resample_plan_matches_the_reference_for_every_mode(golden_dir):
    z = json.load(open(os.path.join(golden_dir, "preprocess.json")))
    cases = z["cases"]
    modes = {c["mode"] for c in cases}
    assert len(modes) == 13 and len(cases) == 45          # every branch of Resample.__call__, three inputs each
    for c in cases:
        if c["seed"] is not None:
            np.random.seed(c["seed"])                      # the two random modes draw from np.random like the reference
        req, new_size = resample_plan(c["mode"], c["factor"], c["size"], np.asarray(c["spacing"]), c["current_size"])
        assert req == c["required_spacing"] == c["meta_spacing"], (c["mode"], req, c["required_spacing"])
        assert new_size == c["new_size"], (c["mode"], new_size, c["new_size"])
        assert all(isinstance(v, float) for v in req) and all(isinstance(v, int) for v in new_size)
        # linear for the image, nearest for "reference" / "weight_map" keys (data_transforms.py:183-187)
        assert c["interpolator"]["#image"] == "linear"
        assert all(v == "nearest" for k, v in c["interpolator"].items() if k != "#image")
    assert z["unknown_mode_raises"] == "NotImplementedError"
    with pytest.raises(NotImplementedError):
        resample_plan("no_such_mode", None, (4, 4, 4), (1.0, 1.0, 1.0), (4, 4, 4))
    # an explicit generator in the place of np.random
    a = resample_plan("random_spacing", (0.9, 1.6), None, (1.0, 0.7, 0.7), (30, 48, 48), rng=np.random.RandomState(5))
    np.random.seed(5)
    assert a == resample_plan("random_spacing", (0.9, 1.6), None, (1.0, 0.7, 0.7), (30, 48, 48))


def test_pack_offsets_table_and_steps():
    chunks = PC.make_chunks()
    loader = ChunkLoader(PC.OUT_SIZES[1], PC.WINDOW)
    packed = loader.pack(chunks, device=None)
    sizes = [int(np.prod(s)) for s in PC.SHAPES]
    offsets = [int(v) for v in np.concatenate([[0], np.cumsum(sizes)[:-1]])]
    assert packed.offsets == offsets and len(packed) == 6
    assert any(o % 8 for o in offsets[1:])                                  # unaligned chunk starts
    assert packed.scans.dtype == torch.int16 and packed.lobes.dtype == torch.uint8 and packed.vessels.dtype == torch.uint8
    assert packed.scans.numel() == packed.lobes.numel() == packed.vessels.numel() == sum(sizes)
    assert packed.table.dtype == torch.uint8 and packed.table.numel() == 6 * 48
    table = packed.table.numpy().view(TABLE_DTYPE)
    n_last_bit = 0
    for i, c in enumerate(chunks):
        lo, hi = offsets[i], offsets[i] + sizes[i]
        assert np.array_equal(packed.scans.numpy()[lo:hi].reshape(PC.SHAPES[i]), c["#image"])
        assert np.array_equal(packed.lobes.numpy()[lo:hi].reshape(PC.SHAPES[i]), c["#lobe_reference"])
        assert np.array_equal(packed.vessels.numpy()[lo:hi].reshape(PC.SHAPES[i]), c["#vessel_reference"])
        rec = table[i]
        assert (int(rec["off"]), int(rec["D"]), int(rec["H"]), int(rec["W"]), int(rec["pad"])) == (lo,) + PC.SHAPES[i] + (0,)
        # Resample('fixed_size'): require_spacing = (spacing * (size_in / size_out)).tolist(); step = required / spacing
        spacing = np.asarray(c["meta"]["spacing"])
        ratios = np.asarray(PC.SHAPES[i]) / np.asarray(PC.OUT_SIZES[1])
        req = (spacing * ratios).tolist()
        for a, name in enumerate(("sz", "sy", "sx")):
            step = float(req[a]) / float(spacing[a])
            assert float(rec[name]) == step == packed.steps[i][a]
            n_last_bit += step != ratios[a]
        assert packed.sizes[i] == PC.OUT_SIZES[1]
    # the chosen inputs exercise the reference's rounding: (spacing * ratio) / spacing is not ratio for some axis
    assert n_last_bit >= 1
    # raw bytes of the first record: int64 offset, 4 x int32, 3 x float64, little endian
    import struct
    first = struct.pack("<q4i3d", 0, 9, 14, 23, 0, *packed.steps[0])
    assert bytes(packed.table.numpy()[:48]) == first
    # torch tensors are taken as well, and the vessel masks are optional
    as_torch = [{k: (torch.from_numpy(v) if k.startswith("#") else v) for k, v in c.items() if k != "#vessel_reference"}
                for c in chunks]
    p2 = loader.pack(as_torch, device=None)
    assert p2.vessels is None and torch.equal(p2.scans, packed.scans) and torch.equal(p2.table, packed.table)


def test_last_bit_steps_exist_for_both_output_sizes():
    """The GPU test's claim that the steps are the reference's `(spacing * ratio) / spacing`, not `ratio`, only bites if the
    two differ somewhere in the chosen inputs."""
    for out in PC.OUT_SIZES:
        n = 0
        for shape, spacing in zip(PC.SHAPES, PC.SPACINGS):
            req, _ = resample_plan("fixed_size", None, out, np.asarray(spacing), shape)
            n += sum(float(req[a]) / float(spacing[a]) != shape[a] / out[a] for a in range(3))
        assert n >= 1, out


def test_row_regime_sizes_are_the_regimes_they_name():
    """rows below 64, spans that are no multiple of 4, an x table longer than one stride, one row per block at the cap; and the
    oracle prepares all six chunks at each size quickly (it is vectorised)."""
    assert [PC.prepare_rows(s) for s in PC.OUT_SIZES] == [(64, 2), (64, 1)]              # what the suite had before
    assert [PC.prepare_rows(s) for s in PC.ROW_REGIME_SIZES] == [(63, 3), (7, 3), (1, 3)]
    rows, blocks = PC.prepare_rows(PC.ROW_REGIME_SIZES[0])
    assert rows * PC.ROW_REGIME_SIZES[0][2] == 2079 and 2079 % 4 and blocks * rows > 2 * 70 > (blocks - 1) * rows
    assert PC.ROW_REGIME_SIZES[1][2] > 256 and PC.ROW_REGIME_SIZES[2][2] == PC.MAX_WO == MAX_WO
    chunks = PC.make_chunks()
    for out in PC.ROW_REGIME_SIZES:
        plan = lambda spacing, size: resample_plan("fixed_size", None, out, spacing, size)
        set_voxels = dict.fromkeys(("#image", "#lobe_reference", "#pseudo_lesion_reference", "#vessel_reference"), 0)
        for c in chunks:
            ref, th = PC.oracle_prepare(c, out, plan)
            assert set(ref) == set(set_voxels) and 0 < th < 1
            assert all(v.shape == out and v.dtype == np.float32 for v in ref.values())
            for k, v in ref.items():
                set_voxels[k] += np.count_nonzero(v)
        print(out, set_voxels)
        assert all(n > 100 for n in set_voxels.values()), (out, set_voxels)     # no output of the batch is all background


def test_hist_chunks_fill_a_second_lap():
    chunks = PC.make_hist_chunks()
    assert [c["#image"].shape for c in chunks] == PC.HIST_SHAPES
    off, size = chunks[0]["#image"].size, chunks[1]["#image"].size
    assert off == 105 and off % 8 and off % 16 and PC.HIST_LAP == 512 * 256 * 8
    start = PC.hist_second_lap_start()
    assert 0 < start < size < start + PC.HIST_LAP and (off + start) % 8 == 0 and (off + start) // 8 - off // 8 == 512 * 256
    lobe = chunks[1]["#lobe_reference"].ravel()
    assert lobe[:start].any() and lobe[start:].any() and not lobe.all() and chunks[0]["#lobe_reference"].any()
    for c in chunks:
        h = PC.hist_expected(c)
        assert h.shape == (256,) and h.sum() == np.count_nonzero(c["#lobe_reference"])
    first, second = (dict(chunks[1], **{"#image": chunks[1]["#image"].ravel()[sl], "#lobe_reference": lobe[sl]})
                     for sl in (slice(0, start), slice(start, None)))
    whole = PC.hist_expected(chunks[1])
    assert np.array_equal(PC.hist_expected(first) + PC.hist_expected(second), whole)
    assert PC.hist_expected(second).sum() > 100 and (PC.hist_expected(first) != whole).any()   # one lap alone is another answer


def test_argument_errors():
    chunks = PC.make_chunks()
    loader = ChunkLoader(PC.OUT_SIZES[0], PC.WINDOW)
    bad = dict(chunks[0])
    bad["#lobe_reference"] = chunks[0]["#lobe_reference"][:, :, :-1]
    with pytest.raises(ValueError, match="shape"):
        loader.pack([bad], device=None)
    bad = dict(chunks[0])
    bad["#image"] = chunks[0]["#image"].astype(np.float32)
    with pytest.raises(TypeError, match="int16"):
        loader.pack([bad], device=None)
    bad = dict(chunks[0])
    bad["#lobe_reference"] = chunks[0]["#lobe_reference"].astype(np.int16)
    with pytest.raises(TypeError, match="uint8"):
        loader.pack([bad], device=None)
    no_vessel = {k: v for k, v in chunks[1].items() if k != "#vessel_reference"}
    with pytest.raises(ValueError, match="every chunk or in none"):
        loader.pack([chunks[0], no_vessel], device=None)
    with pytest.raises(ValueError, match="no chunks"):
        loader.pack([], device=None)
    # a mode whose output size depends on the sample cannot form a batch: the sizes are named
    iso = ChunkLoader(PC.OUT_SIZES[0], PC.WINDOW, mode="fixed_spacing", factor=1.5)
    packed = iso.pack(chunks[:2], device=None)
    assert len(set(packed.sizes)) == 2
    with pytest.raises(ValueError, match=r"different output sizes \[\(5, 7, 11\), \(29, 4, 7\)\]"):
        iso(packed)
    with pytest.raises(ValueError, match="without a device"):
        loader(loader.pack(chunks, device=None))
    with pytest.raises(ValueError, match="float32"):
        ChunkLoader(8, (-1000.1, -300))
    with pytest.raises(ValueError, match="window"):
        ChunkLoader(8, (-300, -1000))
    with pytest.raises(NotImplementedError):
        ChunkLoader(8, PC.WINDOW, mode="no_such_mode").pack(chunks, device=None)


def test_batch_from_chunks_is_a_classmethod_of_batch():
    import inspect
    from dram_amd.train_step import Batch
    assert list(inspect.signature(Batch.from_chunks).parameters) == ["chunks", "ctss", "freq_map", "loader", "band_width"]
    assert inspect.signature(Batch.from_chunks).parameters["band_width"].default == 1e-2
