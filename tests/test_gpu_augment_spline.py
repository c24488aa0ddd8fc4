"""RandomAffineTransform3D and RandomRotate on the device (dram_amd/augment.py over csrc/spline.hip) against what the
reference's own classes produced on the CPU (tests/golden/augment_spline.npz, scripts/make_golden_spline.py).

Bounds, as in tests/test_augment_spline_cpu.py: an image (order 3) within one fp32 step (np.spacing) of the fixture's value --
device and scipy both add the taps in fp64 and round once --, every order-0 entry (uint8 and fp32) exactly equal.  Left out are
only the knife-edge voxels: those whose fp64 source coordinate (tests/spline_restatement.py, from the matrices the package
builds) lies within 1e-9 of a bound 0 or n - 1 or, for the order-0 entries, of a .5 tie, without being that number exactly.
The fixture script asserts that they are at most 0.1 % of a case (with the committed seeds there are none).  A coordinate that
IS the bound or the tie is kept: the same IEEE operations in the same order give the same number, and the identity and the
90 degree sample consist of such voxels.

Cases, each for something that can go wrong:
  affine    3 x (13, 18, 70), the middle sample None: x lines longer than a 64-lane wave and than the 16-column LDS step, odd
            sizes, a skipped sample; fp32 image (order 3), uint8 and fp32 references (order 0)
  identity  scales 1, angles 0: prefilter and taps give the input back
  rotate    4 x (12, 20, 67): each of the three planes (17, -20 and 90 degrees: integer coordinates) and 0 degrees
  rotate1   3 x (1, 9, 11): a plane axis of one element (mirror with n == 1, lines that are not filtered)
"""
import os

import numpy as np
import pytest
import torch

from dram_amd import augment as A

import spline_restatement as SR

pytestmark = pytest.mark.gpu
KNIFE = 1e-9
ENTRIES = (("image", "#image", 3), ("lobe", "#lobe_reference", 0), ("lesion", "#lesion_reference", 0))


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "augment_spline.npz"))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def knife_edges(m, off, shape, ties):
    coords = SR.source_coordinates(m, off, shape)
    edge = np.zeros(shape, dtype=bool)
    for h, n in enumerate(shape):
        for bound in (0.0, float(n - 1)):
            edge |= (np.abs(coords[h] - bound) < KNIFE) & (coords[h] != bound)
        if ties:
            frac = coords[h] - np.floor(coords[h])
            edge |= (np.abs(frac - 0.5) < KNIFE) & (frac != 0.5)
    return edge


def check(got, want, order, record, what):
    """`record`: (matrix, offset) of the sample, or None for a sample that was left alone."""
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if record is None:
        assert np.array_equal(got, want), what
        return
    keep = ~knife_edges(record[0], record[1], want.shape, order == 0)
    assert keep.mean() >= 0.999, what
    if order == 3:
        err = np.abs(got.astype(np.float64) - want.astype(np.float64))
        step = np.spacing(np.abs(want)).astype(np.float64)
        worst = float((err / step)[keep].max())
        print(f"{what}: worst error {worst:.2f} fp32 steps, {int((~keep).sum())} knife-edge voxels left out")
        assert worst <= 1.0, f"{what}: {int(((err > step) & keep).sum())} voxels off by more than one fp32 step (worst {worst:.1f})"
    else:
        bad = (got != want) & keep
        assert not bad.any(), f"{what}: {int(bad.sum())} voxels differ"


def sample_of(gold, case, rows=slice(None)):
    return {key: dev(gold[f"{case}/x_{name}"][rows]) for name, key, _ in ENTRIES} | {"other": 1}


def affine_params(gold):
    return [None if s < 0 else {"scales": [float(v) for v in gold["affine/scales"][i]],
                                "rotate_angles": [float(v) for v in gold["affine/angles"][i]]}
            for i, s in enumerate(gold["affine/seeds"])]


def rotate_params(gold, case):
    return [{"rotate_axis": tuple(int(v) for v in ax), "rotate_angle": int(a)}
            for ax, a in zip(gold[f"{case}/axes"], gold[f"{case}/angles"])]


def test_affine_batch_with_a_skipped_sample(gold):
    shape = tuple(gold["affine/x_image"].shape[1:])
    params = affine_params(gold)
    assert [p is None for p in params] == [False, True, False]
    sample = sample_of(gold, "affine")
    out = A.RandomAffineTransform3D(3).apply(sample, params)
    assert out["other"] == 1 and set(out) == set(sample)
    for name, key, order in ENTRIES:
        got = out[key].cpu().numpy()
        for i, p in enumerate(params):
            rec = None if p is None else A.affine_matrix(p["scales"], p["rotate_angles"], shape)
            check(got[i], gold[f"affine/out_{name}"][i], order, rec, f"affine sample {i} {name}")


def test_identity_gives_the_fixtures_result(gold):
    sample = sample_of(gold, "affine", slice(0, 1))
    out = A.RandomAffineTransform3D(3).apply(sample, [{"scales": [1.0] * 3, "rotate_angles": [0.0] * 3}])
    for name, key, order in ENTRIES:
        check(out[key].cpu().numpy()[0], gold[f"identity/out_{name}"][0], order, (np.eye(3), np.zeros(3)), f"identity {name}")
    x = gold["affine/x_image"][0]
    assert np.abs(out["#image"].cpu().numpy()[0] - x).max() <= 4 * np.spacing(np.abs(x).max())


@pytest.mark.parametrize("case", ["rotate", "rotate1"])
def test_rotate_every_plane(gold, case):
    shape = tuple(gold[f"{case}/x_image"].shape[1:])
    params = rotate_params(gold, case)
    out = A.RandomRotate(3, tuple(int(v) for v in gold["rotate_range"])).apply(sample_of(gold, case), params)
    for name, key, order in ENTRIES:
        got = out[key].cpu().numpy()
        for i, p in enumerate(params):
            rec = A.rotate_matrix(p["rotate_angle"], p["rotate_axis"], shape)[:2]
            check(got[i], gold[f"{case}/out_{name}"][i], order, rec, f"{case} sample {i} {name}")


def test_prefilter_coefficients(gold):
    """The workspace against the restatement's fp64 coefficients: all three axes, and the two plane axes of each plane.  Bound:
    a pass rounds each element a handful of times and the three passes amplify by at most the gain 6 each, so 1e-13 of the
    largest coefficient is two hundred times the fp64 step."""
    x = dev(gold["rotate/x_image"]).unsqueeze(1)
    flags = A._dev([A.TRANSFORM, A.TRANSFORM, A.PASS, A.TRANSFORM], torch.int32, x.device)
    masks = [7, 6, 3, 5]
    ws, nbytes = A.spline_prefilter(x, A._dev(masks, torch.int32, x.device), flags)
    assert nbytes == x.numel() * 8
    coef = ws[:nbytes].view(torch.float64).view(x.shape).cpu().numpy()[:, 0]
    for i, mask in enumerate(masks):
        if i == 2:
            continue            # not flagged: its part of the workspace is not written
        want = SR.prefilter(gold["rotate/x_image"][i], [a for a in range(3) if mask >> a & 1])
        assert np.abs(coef[i] - want).max() <= 1e-13 * np.abs(want).max(), (i, mask)


def test_strided_input_uint8_alone_and_five_dims(gold):
    params = rotate_params(gold, "rotate")
    t = A.RandomRotate(3, (0, 0))
    base = sample_of(gold, "rotate")
    want = t.apply(base, params)
    wide = torch.zeros((4, 12, 20, 2 * 67), dtype=torch.float32, device="cuda")
    wide[..., ::2] = base["#image"]
    strided = wide[..., ::2]
    assert not strided.is_contiguous()
    assert torch.equal(t.apply({"#image": strided}, params)["#image"], want["#image"])
    alone = t.apply({"#lobe_reference": base["#lobe_reference"]}, params)
    assert alone["#lobe_reference"].dtype == torch.uint8 and torch.equal(alone["#lobe_reference"], want["#lobe_reference"])
    five = t.apply({"#image": base["#image"].unsqueeze(1)}, params)["#image"]
    assert five.shape == (4, 1, 12, 20, 67) and torch.equal(five[:, 0], want["#image"])
    with pytest.raises(NotImplementedError, match="order 3 is built for float32"):
        t.apply({"#image": base["#lobe_reference"]}, params)
    with pytest.raises(ValueError, match="parameter sets"):
        t.apply(base, params[:2])


def test_repeat_is_bit_identical_and_input_untouched(gold):
    params = affine_params(gold)
    sample = sample_of(gold, "affine")
    before = {k: v.clone() for k, v in sample.items() if k != "other"}
    t = A.RandomAffineTransform3D(3)
    a, b = t.apply(sample, params), t.apply(sample, params)
    for _, key, _ in ENTRIES:
        assert torch.equal(a[key], b[key]) and torch.equal(sample[key], before[key])


def test_in_a_pool_of_the_users_own(gold):
    """Through the ensemble driver (SKIP flags, caller's output buffers): sample 1 is rotated, then flipped; sample 3 only
    rotated; the others left alone."""
    params = rotate_params(gold, "rotate")
    rot, flip = A.RandomRotate(3, (0, 0)), A.RandomFlip(3)
    chains = [[], [(rot, params[1]), (flip, {"flip_axis": -1})], [], [(rot, params[3])]]
    sample = sample_of(gold, "rotate")
    out = A.EnsembleScanAugmentation(1.0, pool=[rot, flip]).apply(sample, chains)
    for name, key, _ in ENTRIES:
        want = gold[f"rotate/out_{name}"]
        got = out[key].cpu().numpy()
        x = gold[f"rotate/x_{name}"]
        direct = rot.apply({key: sample[key]}, params)[key].cpu().numpy()
        assert np.array_equal(got[0], x[0]) and np.array_equal(got[2], x[2]), name
        assert np.array_equal(got[1], direct[1][..., ::-1]) and np.array_equal(got[3], direct[3]), name
        assert want.shape == got.shape
