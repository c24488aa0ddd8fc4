"""CPU-side checks of the lesion-wise report: the numpy restatement (tests/components_restatement.py) against scipy.ndimage on
every named case, its report arithmetic on a hand-made case, and the C ABI surface of csrc/components.hip (no kernel runs)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import component_cases as CC
import component_large_cases as CL
import components_restatement as CR

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ENTRY_ARGS = {"dram_cc_ws_bytes": 3, "dram_cc_label": 10, "dram_cc_stats": 10, "dram_cc_relabel": 7, "dram_lobe_burden": 5}


@pytest.mark.parametrize("connectivity", CC.CONNECTIVITIES)
@pytest.mark.parametrize("name", list(CC.CASES))
def test_restatement_labels_like_scipy(name, connectivity):
    ndimage = pytest.importorskip("scipy.ndimage")
    mask = CC.mask_of(name)
    labels, n = CC.expected(name, connectivity)
    ref, n_ref = ndimage.label(mask, structure=ndimage.generate_binary_structure(3, connectivity))
    assert n == n_ref
    assert labels.dtype == np.int32 and np.array_equal(labels, ref)
    if name in CC.KNOWN_COUNTS:
        assert n == CC.KNOWN_COUNTS[name][connectivity]


@pytest.mark.parametrize("name", CC.STATS_CASES)
def test_restatement_stats_like_scipy(name):
    ndimage = pytest.importorskip("scipy.ndimage")
    labels, n = CC.expected(name, 1)
    other = CC.other_mask(name)
    voxels, bbox, hits = CR.stats(labels, n, other)
    index = np.arange(1, n + 1)
    assert np.array_equal(voxels, ndimage.sum(np.ones(labels.shape), labels, index).astype(np.int64))
    assert np.array_equal(hits, ndimage.sum(other != 0, labels, index).astype(np.int64))
    objects = ndimage.find_objects(labels, max_label=n)
    assert len(objects) == n
    for k, sl in enumerate(objects):
        assert [v for s in sl for v in (s.start, s.stop)] == bbox[k].tolist()
    assert CR.stats(labels, n)[2] is None
    # a label above n counts nowhere and leaves the others as they are
    if n >= 2:
        v2, b2, _ = CR.stats(labels, n - 1)
        assert np.array_equal(v2, voxels[:-1]) and np.array_equal(b2, bbox[:-1])


def test_restatement_burden_and_relabel():
    rng = np.random.default_rng(5)
    lobe = rng.choice(np.array([0, 1, 2, 3, 4, 5, 255], dtype=np.uint8), size=(3, 7, 11))
    mask = (rng.random(lobe.shape) < 0.3).astype(np.uint8) * 7             # non-zero means set
    counts = CR.burden(mask, lobe)
    for v in range(256):
        assert counts[v, 0] == np.count_nonzero(lobe == v) and counts[v, 1] == np.count_nonzero((lobe == v) & (mask != 0))
    labels, n = CR.label(mask, 1)
    keep = np.arange(n) % 2 == 0
    out, n_kept, kept_mask = CR.relabel(labels, n, keep)
    assert n_kept == keep.sum() and np.array_equal(kept_mask != 0, np.isin(labels, 1 + np.nonzero(keep)[0]))
    assert np.array_equal(np.unique(out), np.arange(n_kept + 1))
    firsts = [np.flatnonzero(out.ravel() == k)[0] for k in range(1, n_kept + 1)]
    assert firsts == sorted(firsts)                                          # the old order is kept


def test_report_arithmetic_on_a_hand_made_case():
    from dram_amd import inference
    spacing = (1.0, 0.5, 0.5)                                                # 0.25 mm^3 per voxel, exact in binary
    voxels = np.array([4, 3, 40], dtype=np.int64)                            # 1.0, 0.75 and 10.0 mm^3
    bbox = np.arange(18, dtype=np.int32).reshape(3, 6)
    hits = np.array([0, 0, 2], dtype=np.int64)
    counts = np.zeros((256, 2), dtype=np.int64)
    counts[0] = (5000, 1)                                                    # the background is no lobe
    counts[1] = (1000, 10)                                                   # 0.01: the lower edge of band 2, inclusive
    counts[2] = (100, 5)                                                     # 0.05: the upper edge of band 2, exclusive -> 3
    counts[3] = (1000, 49)                                                   # 0.049: still 2
    counts[5] = (8, 8)                                                       # 1.0 -> 5; lobe 4 is absent
    rep = CR.report_from_tables(voxels, bbox, hits, lambda keep: counts, spacing, 1.0, ref_found=lambda keep: [])
    assert rep["keep"].tolist() == [True, False, True]                       # kept at exactly the threshold volume
    assert rep["n_lesions"] == 2 and rep["volumes_ml"].tolist() == [0.001, 0.01]
    assert np.array_equal(rep["bboxes"], bbox[[0, 2]])
    assert sorted(rep["lobes"]) == [1, 2, 3, 5]
    assert [rep["lobes"][k]["ctss"] for k in (1, 2, 3, 5)] == [2, 3, 2, 5]
    assert rep["lobes"][2] == {"voxels": 100, "lesion_voxels": 5, "ratio": 0.05, "ctss": 3}
    assert rep["n_reference"] == 0 and rep["n_found"] == 0 and math.isnan(rep["sensitivity"])
    assert rep["n_false"] == 1                                               # component 1 is kept and touches nothing
    just_above = CR.report_from_tables(voxels, bbox, hits, lambda keep: counts, spacing, np.nextafter(1.0, 2.0))
    assert just_above["keep"].tolist() == [False, False, True] and "n_reference" not in just_above
    found = CR.report_from_tables(voxels, bbox, hits, lambda keep: counts, spacing, 0.0, ref_found=lambda keep: [True, False, True, True])
    assert (found["n_reference"], found["n_found"], found["sensitivity"], found["n_false"]) == (4, 3, 0.75, 2)
    # the restated score map is the product's own, at every band edge
    assert CR.CTSS_RATIO_MAP == inference.CTSS_RATIO_MAP
    for lo, hi in CR.CTSS_RATIO_MAP.values():
        for r in (lo, np.nextafter(hi, 0.0)):
            assert CR.ratio_to_label(r) == inference.ratio_to_label(r)


def test_report_restatement_end_to_end_small():
    mask = np.zeros((4, 6, 8), dtype=np.uint8)
    mask[0, 0, 0:3] = 1                      # 3 voxels, lobe 1
    mask[2:4, 2:4, 4:6] = 1                  # 8 voxels, lobe 2
    mask[3, 5, 7] = 1                        # 1 voxel: a speck, lobe 2
    lobe = np.zeros(mask.shape, dtype=np.uint8)
    lobe[:2] = 1
    lobe[2:] = 2
    reference = np.zeros(mask.shape, dtype=np.uint8)
    reference[2, 2, 4] = 1                   # found
    reference[0, 5, 5] = 1                   # missed
    rep = CR.report(mask, lobe, (2.0, 1.0, 1.0), min_volume_mm3=6.0, reference=reference)
    assert rep["n_lesions"] == 2 and rep["volumes_ml"].tolist() == [0.006, 0.016]
    assert rep["bboxes"].tolist() == [[0, 1, 0, 1, 0, 3], [2, 4, 2, 4, 4, 6]]
    assert rep["mask"].sum() == 11 and rep["mask"][3, 5, 7] == 0 and np.array_equal(np.unique(rep["labels"]), [0, 1, 2])
    assert rep["lobes"] == {1: {"voxels": 96, "lesion_voxels": 3, "ratio": 3 / 96, "ctss": 2},
                            2: {"voxels": 96, "lesion_voxels": 8, "ratio": 8 / 96, "ctss": 3}}
    assert (rep["n_reference"], rep["n_found"], rep["sensitivity"], rep["n_false"]) == (2, 1, 0.5, 1)


@pytest.mark.parametrize("connectivity", CL.CONNECTIVITIES)
@pytest.mark.parametrize("name", list(CL.GENERATORS))
def test_large_case_constructions_label_like_the_flood_fill(name, connectivity):
    """The expectations of the whole-scan masks are built, not computed: at SMALL every generator's (labels, n) is the flood
    fill's, at all three connectivities (lattice_gap also with a gap that lies inside SMALL)."""
    variants = [CL.GENERATORS[name](CL.SMALL, connectivity)]
    if name == "lattice_gap":
        variants.append(CL.lattice_gap(CL.SMALL, connectivity, gap=(CL.TILE, 2 * CL.TILE)))
        assert variants[1][0].sum() < variants[0][0].sum() and not variants[1][0].ravel()[CL.TILE:2 * CL.TILE].any()
    for mask, labels, n in variants:
        assert mask.shape == CL.SMALL and mask.dtype == np.uint8 and labels.dtype == np.int32 and mask.any()
        ref, n_ref = CR.label(mask, connectivity)
        assert n == n_ref and np.array_equal(labels, ref)
    if name == "tiled_random":
        assert n > 6 and np.bincount(labels.ravel())[1:].max() >= 8            # more than one per cell; shapes, not single voxels


def test_large_masks_reach_the_laps_they_are_built_for():
    """What the GPU tests rely on, asserted on the masks themselves: more than two laps of 1024 tiles, uneven and empty tile
    counts, a whole lap of zeros between populated ones, labels far above one lap's, components that cross tiles."""
    tiles = CL.tiles_of(CL.LARGE)
    assert tiles == 2095 and tiles > 2 * CL.TILE and CL.LARGE[2] % 64 != 0
    mask, labels, n = CL.large("lattice_thinned")
    counts = CL.tile_counts(mask, CL.LARGE)                                   # every set voxel is a root
    assert n == mask.sum() == labels.max() and n > 65536
    assert counts.size == tiles and len(set(counts.tolist())) > 1 and (counts == 0).any()
    assert counts[:1024].any() and counts[1024:2048].any() and counts[2048:].any()
    assert not mask[1::2].any() and not mask[:, 1::2].any() and not mask[:, :, 1::2].any()   # no two set voxels touch
    for c in (2, 3):
        assert CL.large("lattice_thinned", c)[2] == n and np.array_equal(CL.large("lattice_thinned", c)[1], labels)
    mask, labels, n = CL.large("lattice_gap")
    counts = CL.tile_counts(mask, CL.LARGE)
    assert counts[:1024].sum() > 0 and not counts[1024:2048].any() and counts[2048:].sum() > 0
    assert mask.ravel()[:CL.GAP[0]].any() and mask.ravel()[CL.GAP[1]:].any() and n == counts.sum() > 1024
    for c in CL.CONNECTIVITIES:
        mask, labels, n = CL.large("tiled_random", c)
        flat = labels.ravel()
        assert n == labels.max() > 5120 and np.array_equal(np.unique(flat), np.arange(n + 1))
        first = np.full(n + 1, flat.size, dtype=np.int64)
        last = np.zeros(n + 1, dtype=np.int64)
        np.minimum.at(first, flat, np.arange(flat.size))
        np.maximum.at(last, flat, np.arange(flat.size))
        assert np.all(np.diff(first[1:]) > 0)                                 # numbered in raster order of the first voxels
        crossing = (first[1:] // CL.TILE) != (last[1:] // CL.TILE)            # voxels in another tile than the root's
        other_lap = (first[1:] // (CL.TILE * CL.TILE)) != (last[1:] // (CL.TILE * CL.TILE))
        assert crossing.sum() > n // 4 and other_lap.any()
        roots = np.zeros(flat.size, dtype=bool)
        roots[first[1:]] = True
        counts = CL.tile_counts(roots, CL.LARGE)
        assert counts[:1024].any() and counts[1024:2048].any() and counts[2048:].any() and len(set(counts.tolist())) > 2
    assert CL.large("tiled_random", 1)[2] > CL.large("tiled_random", 2)[2] > CL.large("tiled_random", 3)[2]
    for name in ("comb_large", "comb_large_mirrored"):
        mask, labels, n = CL.large(name)
        assert n == 1 and np.array_equal(labels, mask) and mask[0, 0].all() and mask[1, 1].sum() == 1
        assert mask[:, :, 0 if name.endswith("mirrored") else -1].all()


@pytest.mark.parametrize("name", CL.STATS_CASES)
def test_vectorised_stats_equal_the_restatement(name):
    mask, labels, n = CL.GENERATORS[name](CL.SMALL, 1)
    other = CL.other_mask(CL.SMALL)
    for oth in (None, other):
        v, b, h = CL.stats(labels, n, oth)
        v_ref, b_ref, h_ref = CR.stats(labels, n, oth)
        assert v.dtype == np.int64 and b.dtype == np.int32 and np.array_equal(v, v_ref) and np.array_equal(b, b_ref)
        assert (h is None and h_ref is None) or (h.dtype == np.int64 and np.array_equal(h, h_ref))
    bad = labels.copy()
    bad[0, 0, 0], bad[4, 19, 38], bad[2, 3, 4] = n + 1, -3, n             # outside 1..n twice, and the last label itself
    for a, b in zip(CL.stats(bad, n, other), CR.stats(bad, n, other)):
        assert np.array_equal(a, b)
    # the large expectation: n above one block of cc_stats_init, rows that are no multiple of a wave
    labels, n = CL.large(name)[1:]
    v, b, h = CL.stats(labels, n, CL.other_mask(CL.LARGE))
    assert n > 256 and v.sum() == np.count_nonzero(labels) and 0 < h.sum() < v.sum() and v.min() >= 1
    assert np.all(b[:, 0::2] < b[:, 1::2]) and np.all(b[:, 1::2] <= np.array(CL.LARGE))


def test_relabel_case_is_what_it_claims():
    labels, lut, n, expected, mask = CL.relabel_case()
    cap = CL.RELABEL_CAP
    assert labels.size == CL.RELABEL_NVOX == cap + 300 and lut.size == n + 1 == 1001
    outside = np.flatnonzero((labels < 0) | (labels > n))
    assert outside.tolist() == sorted(CL.RELABEL_BAD)
    below, above = labels[outside] < 0, labels[outside] > n
    for lo, hi in ((0, 256), (cap - 256, cap), (cap, cap + 256), (CL.RELABEL_NVOX - 300, CL.RELABEL_NVOX)):
        here = (outside >= lo) & (outside < hi)
        assert (here & below).any() and (here & above).any(), (lo, hi)      # both kinds in every region
    assert not expected[outside].any() and not mask[outside].any()
    rng = np.random.default_rng(1)
    for i in np.concatenate([rng.integers(0, labels.size, 2000), np.arange(cap - 50, cap + 50), outside]):
        want = int(lut[labels[i]]) if 0 <= labels[i] <= n else 0
        assert expected[i] == want and mask[i] == (want != 0)
    assert (labels == n).sum() >= 2 and lut[n] != 0 and (expected[cap:] == lut[n]).any()
    assert 0 < (lut == 0).sum() < n and (lut < 0).any() and (lut > n).any()
    assert 0 < mask[cap:].sum() < 300 and 0 < mask[:cap].mean() < 1       # the second lap's outputs are not all one value


def _header_functions():
    src = open(os.path.join(ROOT, "include", "dram_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(?:int|size_t|const char\*)\s+(dram_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S):
        args = m.group(2).strip()
        out[m.group(1)] = 0 if args in ("", "void") else len(args.split(","))
    return out


def test_component_entry_points_are_exported_with_the_declared_argument_counts():
    from dram_amd import _lib
    decl = _header_functions()
    lib = ctypes.CDLL(os.path.join(ROOT, "bodyct-dram_amd", "libdram_hip.so"))
    for name, nargs in ENTRY_ARGS.items():
        assert hasattr(lib, name), f"libdram_hip.so does not export {name}"
        assert decl[name] == nargs and len(_lib.SIGNATURES[name][1]) == nargs, name
    assert _lib.SIGNATURES["dram_cc_ws_bytes"][0] is ctypes.c_size_t
    import dram_amd
    for name in ("label_components", "component_stats", "remove_small", "lesion_report"):
        assert callable(getattr(dram_amd, name)) and name in dram_amd.__all__


def test_component_argument_errors_are_reported_without_a_gpu():
    """Every check comes before the first launch, so the error paths answer on a machine without a GPU (dummy non-null
    pointers; nothing is allocated for the 2^31-voxel volume)."""
    from dram_amd import _lib
    q = 16
    ws = lambda *s: _lib.lib.dram_cc_ws_bytes(*s)
    assert ws(4, 5, 6) >= 4 and ws(300, 512, 512) >= 4 * (300 * 512 * 512 // 1024)
    assert ws(2048, 1024, 1024) == 0 and ws(0, 5, 6) == 0 and ws(4, -1, 6) == 0
    assert ws(2047, 1024, 1024) > 0                                          # 2^31 - 2^20 voxels is still in range
    label = lambda *a: _lib.lib.dram_cc_label(*a)
    assert label(q, q, q, 1, 2048, 1024, 1024, q, 1 << 30, None) == -1       # D*H*W = 2^31
    assert b"2^31" in _lib.lib.dram_last_error()
    assert label(q, q, q, 4, 4, 5, 6, q, 1 << 20, None) == -1 and b"connectivity" in _lib.lib.dram_last_error()
    assert label(q, q, q, 0, 4, 5, 6, q, 1 << 20, None) == -1
    assert label(q, q, q, 1, 4, 5, 6, q, ws(4, 5, 6) - 1, None) == -2 and b"workspace too small" in _lib.lib.dram_last_error()
    assert label(None, q, q, 1, 4, 5, 6, q, 1 << 20, None) == -1 and label(q, q, None, 1, 4, 5, 6, q, 1 << 20, None) == -1
    assert label(q, q, q, 1, 4, 0, 6, q, 1 << 20, None) == -1
    stats = lambda *a: _lib.lib.dram_cc_stats(*a)
    assert stats(q, None, 3, q, q, None, 2048, 1024, 1024, None) == -1
    assert stats(q, q, 3, q, q, None, 4, 5, 6, None) == -1 and b"together" in _lib.lib.dram_last_error()
    assert stats(None, None, 3, q, q, None, 4, 5, 6, None) == -1 and stats(q, None, 0, q, q, None, 4, 5, 6, None) == -1
    relabel = lambda *a: _lib.lib.dram_cc_relabel(*a)
    assert relabel(q, q, 3, None, None, 100, None) == -1 and relabel(q, q, 3, q, None, 1 << 31, None) == -1
    assert relabel(q, None, 3, q, None, 100, None) == -1 and relabel(q, q, -1, q, None, 100, None) == -1
    burden = lambda *a: _lib.lib.dram_lobe_burden(*a)
    assert burden(q, q, q, 0, None) == -1 and burden(q, q, q, 1 << 31, None) == -1 and burden(q, None, q, 10, None) == -1
