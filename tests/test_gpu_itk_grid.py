"""The grid of sitk.ResampleImageFilter has one device definition (csrc/volume_math.h).  Two of its consumers, given the same
volume and the same steps, must return the same bits: the RandomCrop primitive (csrc/crop.hip) with a window that is the whole
chunk, and resample_volume (csrc/infer.hip).  Both against oracle.resample_itk as well."""
import numpy as np
import pytest
import torch

from dram_amd import augment as A
from dram_amd.inference import resample_volume
from oracle import dram_oracle as O

pytestmark = pytest.mark.gpu
SHAPE = (6, 7, 13)       # a second sample starts 546 bytes in: not 16-byte aligned for uint8


@pytest.mark.parametrize("steps", [(0.75, 1.3, 1.03), (1.6, 0.5, 0.6)])
def test_crop_resample_and_resample_volume_share_the_grid(steps):
    """(0.75, 1.3, 1.03): y leaves the buffer from o = 5 on (6.5 is not < 6.5), x ends on the clamped neighbour with t = 0
    (12.36 in [12, 12.5)).  (1.6, 0.5, 0.6): z leaves the buffer from o = 4 (6.4 >= 5.5).  Bit for bit between the two kernels;
    against the oracle bit for bit where the suites of either kernel claim it, fp32 linear of resample_volume to 1e-6."""
    rng = np.random.default_rng(3)
    img = (rng.random((2,) + SHAPE) + 0.5).astype(np.float32)
    lab = rng.integers(1, 250, (2,) + SHAPE).astype(np.uint8)
    table = np.zeros(2, dtype=A.CROP_DTYPE)
    table[:] = (0, 0, 0) + SHAPE + (A.PAD_MODES["constant"], 0) + tuple(steps)
    table = torch.from_numpy(table.view(np.uint8).copy()).cuda()
    flags = torch.full((2,), A.TRANSFORM, dtype=torch.int32, device="cuda")
    for src, how in ((img, "linear"), (img, "nearest"), (lab, "nearest")):
        x = torch.from_numpy(src).cuda()
        crop = A.crop_resample(x.unsqueeze(1), table, flags, how == "linear")[:, 0].cpu().numpy()
        for n in range(2):
            vol = resample_volume(x[n], (1, 1, 1), steps, SHAPE, how).cpu().numpy()
            ref = O.resample_itk(src[n], (1, 1, 1), steps, SHAPE, how)
            assert np.array_equal(crop[n], vol), (how, src.dtype, n, int((crop[n] != vol).sum()))
            assert np.array_equal(crop[n], ref), (how, src.dtype, n, int((crop[n] != ref).sum()))
            if how == "linear":
                assert np.abs(vol - ref).max() <= 1e-6
            else:
                assert np.array_equal(vol, ref)
            if steps[1] > 1:
                assert (vol[:, 5:] == 0).all() and (vol[:, :5] != 0).all()
            else:
                assert (vol[4:] == 0).all() and (vol[:4] != 0).all()
