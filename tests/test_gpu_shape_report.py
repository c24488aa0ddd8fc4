"""dram_amd/shape.py on the device: `lesion_shape` against the same host arithmetic on the restatement's tables (equal integers in,
equal floats out), and the `shape=` keyword of `lesion_report`."""
import numpy as np
import pytest
import torch

import shape_cases as SC
import shape_restatement as SR

pytestmark = pytest.mark.gpu


def _assert_rows_equal(got, ref):
    assert len(got) == len(ref)
    for k, (a, b) in enumerate(zip(got, ref)):
        assert sorted(a) == sorted(b), k
        for key in b:
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key]), equal_nan=True), (k, key)


@pytest.mark.parametrize("name", ["random_u8", "random_i32_300", "blobs", "above_n_i32"])
def test_lesion_shape_matches_the_restatement(name):
    from dram_amd import label_shape, lesion_shape
    from dram_amd.shape import rows_from_tables
    c = SC.case(name)
    spacing = (2.5, 0.7, 0.8)
    got = label_shape(torch.from_numpy(c["labels"].copy()).cuda(), c["n"])
    for key, v in SC.expected(name).items():
        assert got[key].dtype == v.dtype and np.array_equal(got[key], v), key
    _assert_rows_equal(lesion_shape(c["labels"].copy(), c["n"], spacing), rows_from_tables(SC.expected(name), spacing))   # host arrays go in as they are
    assert lesion_shape(c["labels"].copy(), 0, spacing) == []
    with pytest.raises(ValueError, match="uint8 or int32"):
        label_shape(c["labels"].astype(np.int64), c["n"])


def _planted():
    """24 x 32 x 40: four blobs in one lobe, the smallest below the volume filter."""
    shape = (24, 32, 40)
    z, y, x = np.meshgrid(*(np.arange(s, dtype=np.float64) for s in shape), indexing="ij")
    mask = np.zeros(shape, dtype=np.uint8)
    for (cz, cy, cx), (rz, ry, rx) in (((6, 8, 9), (3, 5, 6)), ((16, 20, 28), (5, 4, 7)), ((8, 24, 30), (2, 3, 3)), ((20, 6, 6), (1, 1, 1))):
        mask[((z - cz) / rz) ** 2 + ((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 <= 1.0] = 1
    mask[16, 20, 28] = 0                                                               # a cavity in the second blob
    lobe = np.ones(shape, dtype=np.uint8)
    return mask, lobe, (2.0, 0.8, 0.8)


def test_lesion_report_with_shape():
    from dram_amd import lesion_report
    from dram_amd.shape import rows_from_tables
    mask, lobe, spacing = _planted()
    kw = dict(connectivity=1, min_volume_mm3=20.0)
    plain = lesion_report(mask, lobe, spacing, **kw)
    assert "shape" not in plain and plain["n_lesions"] == 3
    rep = lesion_report(mask, lobe, spacing, shape=True, **kw)
    assert sorted(rep) == sorted(list(plain) + ["shape"])
    for key in plain:                                                                  # every other key as without the keyword
        if isinstance(plain[key], torch.Tensor):
            assert torch.equal(rep[key], plain[key]), key
        elif isinstance(plain[key], np.ndarray):
            assert np.array_equal(rep[key], plain[key]), key
        else:
            assert rep[key] == plain[key], key
    rows = rep["shape"]
    labels = rep["labels"].cpu().numpy()
    assert len(rows) == 3
    for i, row in enumerate(rows):                                                     # the order of volumes_ml
        assert row["voxels"] == np.count_nonzero(labels == i + 1)
        assert abs(row["volume_mm3"] / 1000.0 - rep["volumes_ml"][i]) <= 1e-12 * rep["volumes_ml"][i]
    _assert_rows_equal(rows, rows_from_tables(SR.tables(labels, 3), spacing))
    assert sorted(r["euler"] for r in rows) == [1, 1, 2]                               # the cavity shows
    assert lesion_report(np.zeros_like(mask), lobe, spacing, shape=True)["shape"] == []
