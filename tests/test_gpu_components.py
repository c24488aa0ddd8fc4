"""csrc/components.hip and dram_amd/lesions.py on the device against the numpy restatement (tests/components_restatement.py,
itself held against scipy.ndimage by tests/test_components_cpu.py): everything here is integers, so every comparison is exact."""
import math

import numpy as np
import pytest
import torch

import component_cases as CC
import component_large_cases as CL
import components_restatement as CR

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()            # a copy: the shared cases are read-only arrays


def _st():
    return torch.cuda.current_stream().cuda_stream


def gpu_label(mask, connectivity):
    from dram_amd._lib import call, lib
    D, H, W = mask.shape
    m = _dev(mask)
    labels = torch.full(mask.shape, -7, dtype=torch.int32, device="cuda")        # poisoned: every voxel must be written
    ws_bytes = lib.dram_cc_ws_bytes(D, H, W)
    ws = torch.full((ws_bytes // 4,), -7, dtype=torch.int32, device="cuda")
    count = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    call("dram_cc_label", m.data_ptr(), labels.data_ptr(), count.data_ptr(), connectivity, D, H, W, ws.data_ptr(), ws_bytes, _st())
    return labels.cpu().numpy(), int(count.item())


def gpu_stats(labels, n, other=None):
    from dram_amd._lib import call
    lab = _dev(labels.astype(np.int32))
    voxels = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    bbox = torch.full((n, 6), -7, dtype=torch.int32, device="cuda")
    hits = None if other is None else torch.full((n,), -7, dtype=torch.int64, device="cuda")
    oth = None if other is None else _dev(other)
    call("dram_cc_stats", lab.data_ptr(), None if oth is None else oth.data_ptr(), n, voxels.data_ptr(), bbox.data_ptr(),
         None if hits is None else hits.data_ptr(), *labels.shape, _st())
    return voxels.cpu().numpy(), bbox.cpu().numpy(), None if hits is None else hits.cpu().numpy()


@pytest.mark.parametrize("connectivity", CC.CONNECTIVITIES)
@pytest.mark.parametrize("name", list(CC.CASES))
def test_cc_label_matches_the_restatement(name, connectivity):
    mask = CC.mask_of(name)
    ref, n_ref = CC.expected(name, connectivity)
    labels, n = gpu_label(mask, connectivity)
    assert n == n_ref
    assert np.array_equal(labels, ref)
    again, n_again = gpu_label(mask, connectivity)
    assert n_again == n and np.array_equal(again, labels)                        # no dependence on the order of the atomics
    if name in CC.KNOWN_COUNTS:
        assert n == CC.KNOWN_COUNTS[name][connectivity]


def test_cc_label_takes_any_non_zero_value_as_set():
    mask = CC.mask_of("random_7x9x11_35") * np.uint8(200)
    labels, n = gpu_label(mask, 2)
    ref, n_ref = CC.expected("random_7x9x11_35", 2)
    assert n == n_ref and np.array_equal(labels, ref)


@pytest.mark.parametrize("with_other", [False, True])
@pytest.mark.parametrize("name", CC.STATS_CASES)
def test_cc_stats_matches_the_restatement(name, with_other):
    labels, n = CC.expected(name, 1)
    other = CC.other_mask(name) if with_other else None
    voxels, bbox, hits = gpu_stats(labels, n, other)
    v_ref, b_ref, h_ref = CR.stats(labels, n, other)
    assert np.array_equal(voxels, v_ref) and np.array_equal(bbox, b_ref)
    assert (hits is None and h_ref is None) or np.array_equal(hits, h_ref)
    assert voxels.sum() == np.count_nonzero(labels)


def test_cc_stats_skips_labels_outside_the_range():
    labels, n = CC.expected("random_16x16x16_20", 1)
    assert n >= 4
    bad = labels.copy()
    bad[0, 0, 0], bad[15, 15, 15], bad[3, 4, 5] = n + 1, np.iinfo(np.int32).max, -3   # none of them may be written through
    other = CC.other_mask("random_16x16x16_20")
    voxels, bbox, hits = gpu_stats(bad, n, other)
    v_ref, b_ref, h_ref = CR.stats(bad, n, other)
    assert np.array_equal(voxels, v_ref) and np.array_equal(bbox, b_ref) and np.array_equal(hits, h_ref)
    # stats of the first n - 2 components only: the two last ones are above the range now and the rest is unchanged
    voxels2, bbox2, _ = gpu_stats(labels, n - 2)
    full = CR.stats(labels, n)
    assert np.array_equal(voxels2, full[0][:n - 2]) and np.array_equal(bbox2, full[1][:n - 2])


def test_cc_relabel_lut_aliasing_and_single_outputs():
    from dram_amd._lib import call
    labels, n = CC.expected("random_5x6x70_35", 1)
    assert n >= 6
    keep = np.arange(n) % 2 == 0                                                 # drops every second component
    ref_labels, n_kept, ref_mask = CR.relabel(labels, n, keep)
    lut = np.zeros(n + 1, dtype=np.int32)
    lut[1:] = np.where(keep, np.cumsum(keep), 0)
    lut_d, nvox = _dev(lut), labels.size

    lab = _dev(labels)
    out = torch.full(labels.shape, -7, dtype=torch.int32, device="cuda")
    msk = torch.full(labels.shape, 9, dtype=torch.uint8, device="cuda")
    call("dram_cc_relabel", lab.data_ptr(), lut_d.data_ptr(), n, out.data_ptr(), msk.data_ptr(), nvox, _st())
    assert np.array_equal(out.cpu().numpy(), ref_labels) and np.array_equal(msk.cpu().numpy(), ref_mask)
    assert np.array_equal(lab.cpu().numpy(), labels)                             # the input is left alone
    # labels only / mask only
    out2 = torch.full(labels.shape, -7, dtype=torch.int32, device="cuda")
    call("dram_cc_relabel", lab.data_ptr(), lut_d.data_ptr(), n, out2.data_ptr(), None, nvox, _st())
    msk2 = torch.full(labels.shape, 9, dtype=torch.uint8, device="cuda")
    call("dram_cc_relabel", lab.data_ptr(), lut_d.data_ptr(), n, None, msk2.data_ptr(), nvox, _st())
    assert torch.equal(out2, out) and torch.equal(msk2, msk)
    # in place
    call("dram_cc_relabel", lab.data_ptr(), lut_d.data_ptr(), n, lab.data_ptr(), None, nvox, _st())
    assert torch.equal(lab, out)
    # a label outside 0..n reads nothing from the table
    bad = labels.copy()
    bad[0, 0, 0], bad[4, 5, 69] = n + 1, -1
    expect = ref_labels.copy()
    expect[0, 0, 0] = expect[4, 5, 69] = 0
    out3 = torch.full(labels.shape, -7, dtype=torch.int32, device="cuda")
    call("dram_cc_relabel", _dev(bad).data_ptr(), lut_d.data_ptr(), n, out3.data_ptr(), None, nvox, _st())
    assert np.array_equal(out3.cpu().numpy(), expect)


@pytest.mark.parametrize("name,connectivity", CL.LABEL_CASES)
def test_cc_label_past_one_scan_lap(name, connectivity):
    """2095 tiles: cc_scan_kernel walks laps of 1024, 1024 and 47 tile counts with its carry, cc_rank / cc_final see block
    offsets and rank codes from every lap (tests/component_large_cases.py; expectations by construction)."""
    mask, ref, n_ref = CL.large(name, connectivity)
    labels, n = gpu_label(mask, connectivity)
    assert n == n_ref
    assert np.array_equal(labels, ref)


@pytest.mark.parametrize("with_other", [False, True])
@pytest.mark.parametrize("name", CL.STATS_CASES)
def test_cc_stats_with_many_components_and_rows_off_the_wave(name, with_other):
    """n far above 256 (cc_stats_init_kernel in many blocks), W = 260 (groups of a wave span rows)."""
    _, labels, n = CL.large(name, 1)
    other = CL.other_mask(CL.LARGE) if with_other else None
    voxels, bbox, hits = gpu_stats(labels, n, other)
    v_ref, b_ref, h_ref = CL.stats(labels, n, other)
    assert np.array_equal(voxels, v_ref) and np.array_equal(bbox, b_ref)
    assert (hits is None and h_ref is None) or np.array_equal(hits, h_ref)


def test_cc_relabel_past_the_grid_cap():
    """16384 x 256 + 300 elements: the second lap of the grid-stride loop, labels outside 0..n in the first block, on both
    sides of the lap seam and in the ragged tail.  Separate outputs, one output at a time, in place; a guard band after
    every output."""
    from dram_amd._lib import call
    labels, lut, n, ref_labels, ref_mask = CL.relabel_case()
    nvox, guard = labels.size, 64
    lut_d = _dev(lut)

    def buffers():
        lab = torch.full((nvox + guard,), -7, dtype=torch.int32, device="cuda")
        lab[:nvox] = _dev(labels)
        return (lab, torch.full((nvox + guard,), -7, dtype=torch.int32, device="cuda"),
                torch.full((nvox + guard,), 9, dtype=torch.uint8, device="cuda"))

    def check(out, msk):
        if out is not None:
            assert np.array_equal(out[:nvox].cpu().numpy(), ref_labels) and bool((out[nvox:] == -7).all())
        if msk is not None:
            assert np.array_equal(msk[:nvox].cpu().numpy(), ref_mask) and bool((msk[nvox:] == 9).all())

    lab, out, msk = buffers()
    call("dram_cc_relabel", lab.data_ptr(), lut_d.data_ptr(), n, out.data_ptr(), msk.data_ptr(), nvox, _st())
    check(out, msk)
    assert np.array_equal(lab[:nvox].cpu().numpy(), labels)                      # the input is left alone
    _, out, msk = buffers()
    call("dram_cc_relabel", lab.data_ptr(), lut_d.data_ptr(), n, out.data_ptr(), None, nvox, _st())
    call("dram_cc_relabel", lab.data_ptr(), lut_d.data_ptr(), n, None, msk.data_ptr(), nvox, _st())
    check(out, msk)
    _, _, msk = buffers()
    call("dram_cc_relabel", lab.data_ptr(), lut_d.data_ptr(), n, lab.data_ptr(), msk.data_ptr(), nvox, _st())   # in place
    check(lab, msk)


def test_remove_small_renumbers_in_the_old_order():
    from dram_amd import component_stats, label_components, remove_small
    mask = np.array(CC.mask_of("random_16x16x16_20"))                            # a host array goes in as it is
    labels, n = label_components(mask, 1)
    ref, n_ref = CC.expected("random_16x16x16_20", 1)
    assert n == n_ref and labels.dtype == torch.int32 and labels.is_cuda and np.array_equal(labels.cpu().numpy(), ref)
    st = component_stats(labels, n)
    v_ref = CR.stats(ref, n)[0]
    assert st["hits"] is None and np.array_equal(st["voxels"], v_ref) and st["bbox"].shape == (n, 6)
    assert 0 < (v_ref >= 2).sum() < n
    out, n_kept, kept = remove_small(labels, n, st["voxels"], 2)
    r_labels, r_n, r_mask = CR.relabel(ref, n, v_ref >= 2)
    assert n_kept == r_n and np.array_equal(out.cpu().numpy(), r_labels) and np.array_equal(kept.cpu().numpy(), r_mask)
    assert kept.dtype == torch.uint8


@pytest.mark.parametrize("offset", [0, 1])
def test_lobe_burden_counts(offset):
    """70,001 voxels: no multiple of any vector width, more than one block; offset 1 takes the buffers off their 16-byte
    alignment (the element-wise path)."""
    from dram_amd._lib import call
    n = 70001
    rng = np.random.default_rng(11)
    values = np.array([0, 1, 2, 3, 4, 5, 255], dtype=np.uint8)
    lobe = np.repeat(rng.choice(values, size=1000), rng.integers(40, 200, size=1000))[:n]   # runs, as a lobe map has them
    assert lobe.size == n and set(np.unique(lobe)) == set(values.tolist())
    lobe[::977] = rng.choice(values, size=lobe[::977].size)                                  # and single odd voxels
    mask = (rng.random(n) < 0.3).astype(np.uint8) * rng.integers(1, 256, size=n).astype(np.uint8)
    lobe_d, mask_d = _dev(np.concatenate([np.zeros(offset, np.uint8), lobe])), _dev(np.concatenate([np.ones(offset, np.uint8), mask]))
    counts = torch.full((256, 2), -7, dtype=torch.int64, device="cuda")
    call("dram_lobe_burden", mask_d.data_ptr() + offset, lobe_d.data_ptr() + offset, counts.data_ptr(), n, _st())
    got = counts.cpu().numpy()
    ref = np.zeros((256, 2), dtype=np.int64)
    for v in values.tolist():
        ref[v] = (np.count_nonzero(lobe == v), np.count_nonzero((lobe == v) & (mask != 0)))
    assert np.array_equal(got, ref) and got[:, 0].sum() == n
    small = CR.burden(mask[:3001], lobe[:3001])                                              # the restatement agrees with the count
    call("dram_lobe_burden", mask_d.data_ptr() + offset, lobe_d.data_ptr() + offset, counts.data_ptr(), 3001, _st())
    assert np.array_equal(counts.cpu().numpy(), small)


def _assert_reports_equal(rep, ref):
    assert rep["n_lesions"] == ref["n_lesions"]
    assert np.array_equal(rep["mask"].cpu().numpy(), ref["mask"]) and rep["mask"].dtype == torch.uint8
    assert np.array_equal(rep["labels"].cpu().numpy(), ref["labels"])
    assert np.array_equal(rep["volumes_ml"], ref["volumes_ml"]) and rep["volumes_ml"].dtype == np.float64
    assert np.array_equal(rep["bboxes"], ref["bboxes"])
    assert rep["lobes"] == ref["lobes"]
    for key in ("n_reference", "n_found", "n_false"):
        assert (key in rep) == (key in ref) and rep.get(key) == ref.get(key)
    if "sensitivity" in ref:
        assert rep["sensitivity"] == ref["sensitivity"] or (math.isnan(rep["sensitivity"]) and math.isnan(ref["sensitivity"]))


def _planted():
    shape = (24, 32, 40)
    lobe = np.zeros(shape, dtype=np.uint8)
    lobe[:, 2:, 0:13], lobe[:, 2:, 13:26], lobe[:, 2:, 26:40] = 1, 2, 3
    blobs = {"a": (slice(2, 6), slice(4, 9), slice(2, 7)), "b": (slice(10, 14), slice(10, 14), slice(3, 6)),
             "c": (slice(3, 8), slice(20, 26), slice(15, 20)), "d": (slice(15, 20), slice(5, 10), slice(14, 24)),
             "e": (slice(12, 18), slice(15, 22), slice(30, 36)), "speck": (20, 28, slice(30, 33))}
    mask = np.zeros(shape, dtype=np.uint8)
    for sl in blobs.values():
        mask[sl] = 1
    reference = np.zeros(shape, dtype=np.uint8)
    reference[3:7, 5:10, 3:8] = 1                          # overlaps a
    for k in "bcd":
        reference[blobs[k]] = 1
    reference[20, 28, 30:34] = 1                           # touched by the speck only: not found once the speck is gone
    reference[21:23, 3:6, 30:34] = 1                       # missed; e has no counterpart: the extra lesion
    return mask, lobe, reference


def test_lesion_report_on_planted_blobs():
    from dram_amd import lesion_report
    mask, lobe, reference = _planted()
    spacing = (1.0, 0.7, 0.7)
    ref = CR.report(mask, lobe, spacing, connectivity=1, min_volume_mm3=2.0, reference=reference)
    # the case is what it is meant to be
    assert CR.label(mask, 1)[1] == 6 and ref["n_lesions"] == 5 and not ref["mask"][20, 28, 30:33].any()
    assert (ref["n_reference"], ref["n_found"], ref["n_false"]) == (6, 4, 1) and sorted(ref["lobes"]) == [1, 2, 3]
    rep = lesion_report(_dev(mask), lobe, spacing, connectivity=1, min_volume_mm3=2.0, reference=reference)
    _assert_reports_equal(rep, ref)
    assert rep["mask"].is_cuda and rep["labels"].is_cuda and rep["labels"].dtype == torch.int32
    assert rep["sensitivity"] == 4 / 6
    # without a reference and without a filter: no detection keys, the speck stays
    plain = lesion_report(mask, lobe, spacing, connectivity=3)
    _assert_reports_equal(plain, CR.report(mask, lobe, spacing, connectivity=3))
    assert plain["n_lesions"] == 6 and "n_reference" not in plain
    # an empty mask and an empty reference
    none = lesion_report(np.zeros_like(mask), lobe, spacing, reference=np.zeros_like(mask))
    assert none["n_lesions"] == 0 and none["n_reference"] == 0 and math.isnan(none["sensitivity"]) and none["n_false"] == 0
    assert none["volumes_ml"].shape == (0,) and none["bboxes"].shape == (0, 6) and not bool(none["mask"].any())
    assert {k: v["ctss"] for k, v in none["lobes"].items()} == {1: 0, 2: 0, 3: 0}


def test_lesion_report_after_lobe_inference():
    """LobeInference.run of a SLIM model, then the report on its post-processed mask: runs on the device tensors of the result
    and agrees with the restatement applied to the same mask."""
    import models
    from dram_amd import lesion_report
    from dram_amd.configs import SLIM
    from dram_amd.inference import LobeInference, synthetic_ct
    torch.manual_seed(3)
    model = models.DC3D(**SLIM)
    model.init(models.HeNorm(mode="fan_in"))
    scan, lobe, spacing = synthetic_ct((41, 57, 66), (2.5, 1.0, 1.0), seed=7, n_lesions=8)
    lesion = ((scan > -500) & (lobe > 0)).astype(np.uint8)
    res = LobeInference(model.cuda().eval(), resample_size=24).run(scan, lobe, spacing, lesion=lesion)
    rep = lesion_report(res["mask_post"], lobe, spacing, connectivity=2, min_volume_mm3=10.0, reference=lesion)
    ref = CR.report(res["mask_post"].cpu().numpy(), lobe, spacing, connectivity=2, min_volume_mm3=10.0, reference=lesion)
    _assert_reports_equal(rep, ref)
    assert sorted(rep["lobes"]) == [1, 2, 3, 4, 5] and rep["n_reference"] >= 1


def test_error_paths_launch_nothing():
    """D*H*W >= 2^31 (sizes only, nothing of that size is allocated), connectivity 4, a workspace that is too small: the error
    code comes back and the outputs keep their poison."""
    from dram_amd._lib import DramHipError, call, lib
    m = _dev(np.ones((4, 5, 6), dtype=np.uint8))
    labels = torch.full((4, 5, 6), -7, dtype=torch.int32, device="cuda")
    count = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    ws_bytes = lib.dram_cc_ws_bytes(4, 5, 6)
    ws = torch.full((max(ws_bytes // 4, 1),), -7, dtype=torch.int32, device="cuda")
    args = lambda c, D, H, W, nbytes: (m.data_ptr(), labels.data_ptr(), count.data_ptr(), c, D, H, W, ws.data_ptr(), nbytes, _st())
    assert lib.dram_cc_label(*args(1, 2048, 1024, 1024, 1 << 40)) == -1
    assert lib.dram_cc_label(*args(4, 4, 5, 6, ws_bytes)) == -1
    assert lib.dram_cc_label(*args(1, 4, 5, 6, ws_bytes - 1)) == -2
    assert lib.dram_cc_ws_bytes(2048, 1024, 1024) == 0
    with pytest.raises(DramHipError, match="connectivity"):
        call("dram_cc_label", *args(0, 4, 5, 6, ws_bytes))
    torch.cuda.synchronize()
    assert bool((labels == -7).all()) and int(count.item()) == -7 and bool((ws == -7).all())
    from dram_amd import label_components
    with pytest.raises(ValueError, match="connectivity"):
        label_components(m, 4)
