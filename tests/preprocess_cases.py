"""Shared by test_preprocess_cpu.py and test_gpu_preprocess.py: the ragged batch of six chunks and the host composition of the
oracle's restatements (`oracle.windowing`, `oracle.binary_cam`, `oracle.resample_itk`) in the order the reference composes them
(dram/dataset.py:460-463, then Windowing and Resample('fixed_size'), dram/job_runner.py:586-597)."""
import numpy as np

from oracle import dram_oracle as O

# (9,14,23) / (17,8,11): plain odd sizes; (5,5,5) upsamples: the last outputs along each axis lie beyond size_in - 0.5 and are 0;
# (33,20,70): x rows longer than a wave; (1,7,3): a one-voxel axis (upper neighbour = base); (12,10,16): the first output size
SHAPES = [(9, 14, 23), (17, 8, 11), (5, 5, 5), (33, 20, 70), (1, 7, 3), (12, 10, 16)]
SPACINGS = [(0.7, 0.73, 0.7), (2.5, 0.68359375, 0.9), (0.8, 0.8, 0.8), (0.37, 1.1, 0.3), (5.0, 0.45, 1.3), (1.0, 0.6, 0.9)]
OUT_SIZES = [(12, 10, 16), (7, 9, 13)]          # Wo = 13: no multiple of 4; the chunk offsets are unaligned
WINDOW = (-1000, -300)
PSEUDO_WINDOW, PSEUDO_SCALER = (-1150, 350), 0.75


def make_chunks(seed=11, with_vessel=True):
    """HU uniform in [-2048, 1500]; lobes: random ellipsoids of values {0, 1}, sample 3's lobe holds the value 3."""
    rng = np.random.default_rng(seed)
    chunks = []
    for i, (shape, spacing) in enumerate(zip(SHAPES, SPACINGS)):
        scan = rng.integers(-2048, 1501, size=shape).astype(np.int16)
        grid = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij", sparse=True)
        centre = [(n - 1) / 2 + rng.uniform(-0.2, 0.2) * n for n in shape]
        radius = [rng.uniform(0.3, 0.48) * n + 0.6 for n in shape]
        lobe = (sum(((g - c) / r) ** 2 for g, c, r in zip(grid, centre, radius)) < 1.0).astype(np.uint8)
        if i == 3:
            lobe[lobe > 0] = 3
        assert lobe.any()
        c = {"#image": scan, "#lobe_reference": lobe, "meta": {"spacing": spacing}}
        vessel = (rng.random(shape) > 0.7).astype(np.uint8) * rng.integers(1, 4, size=shape).astype(np.uint8)
        if with_vessel:
            c["#vessel_reference"] = vessel
        chunks.append(c)
    return chunks


# Output sizes for the other `rows` regimes of chunk_prepare_kernel (rows = min(64, cdiv(2048, Wo)) output rows per block):
# (2,70,33): rows = 63, three blocks per sample whose spans are 2079 elements, so 16-byte output quads straddle the block seams;
# (3,5,300): the x table takes two strides of 256 threads, rows = 7; (1,3,2048): one row per block at the largest Wo accepted
ROW_REGIME_SIZES = [(2, 70, 33), (3, 5, 300), (1, 3, 2048)]
MAX_WO = 2048


def prepare_rows(out_size):
    """(rows per block, blocks per sample) as dram_chunk_prepare chooses them."""
    rows = min(64, -(-2048 // out_size[2]))
    return rows, -(-out_size[0] * out_size[1] // rows)


# dram_chunk_hist256 with N = 2 runs per = 512 blocks per sample; a block covers 256 groups of 8 elements per lap
HIST_LAP = 512 * 256 * 8
HIST_SHAPES = [(3, 5, 7), (9, 300, 391)]        # 105 elements: chunk 1 starts neither 8- nor 16-aligned, and is longer than a lap


def hist_second_lap_start():
    """Index inside chunk 1 of the first element of the second lap: laps count from the 8-aligned group that holds the chunk's
    first element."""
    off = int(np.prod(HIST_SHAPES[0]))
    return (off // 8) * 8 + HIST_LAP - off


def make_hist_chunks(seed=12):
    """Two chunks for the histogram alone: HU uniform in [-2048, 1500], chunk 1's lobe a seeded ellipsoid (values {0, 2}) that
    reaches into the last rows of the last slice, i.e. into the second lap."""
    rng = np.random.default_rng(seed)
    chunks = []
    for shape in HIST_SHAPES:
        scan = rng.integers(-2048, 1501, size=shape).astype(np.int16)
        grid = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij", sparse=True)
        centre = [(n - 1) * f + rng.uniform(-0.02, 0.02) * n for n, f in zip(shape, (0.62, 0.62, 0.5))]
        radius = [f * n for n, f in zip(shape, (0.7, 0.5, 0.55))]
        lobe = (sum(((g - c) / r) ** 2 for g, c, r in zip(grid, centre, radius)) < 1.0).astype(np.uint8) * np.uint8(2)
        chunks.append({"#image": scan, "#lobe_reference": lobe, "meta": {"spacing": (1.0, 0.7, 0.7)}})
    return chunks


def hist_expected(chunk):
    """The 256-bin histogram of binary_cam's 8-bit view inside the lobe."""
    w = O.windowing(chunk["#image"], from_span=PSEUDO_WINDOW, to_span=(0, 1))[chunk["#lobe_reference"] > 0]
    view = O.windowing(w, from_span=(0, 1), to_span=(0, 255)).astype(np.uint8)
    return np.bincount(view, minlength=256)


def oracle_prepare(chunk, out_size, plan):
    """One chunk the reference's way on the host.  plan(spacing, size) -> (required_spacing, new_size).  Returns the dict of
    [D,H,W] float32 arrays and the threshold."""
    scan, lobe, spacing = chunk["#image"], chunk["#lobe_reference"], chunk["meta"]["spacing"]
    w_scan = O.windowing(scan, from_span=PSEUDO_WINDOW, to_span=(0, 1))            # dataset.py:461
    assert w_scan.dtype == np.float64
    _, th = O.binary_cam(w_scan[lobe > 0], PSEUDO_SCALER)                           # dataset.py:462
    sample = {"#pseudo_lesion_reference": ((w_scan > th) & (lobe > 0)).astype(np.uint8), "#lobe_reference": lobe}
    if "#vessel_reference" in chunk:
        sample["#vessel_reference"] = np.logical_and(chunk["#vessel_reference"] > 0, lobe > 0).astype(np.uint8)
    image = O.windowing(scan.astype(np.float32), from_span=WINDOW, to_span=(0, 1))  # Windowing, data_transforms.py:46-54
    assert image.dtype == np.float32
    req, new_size = plan(np.asarray(spacing), scan.shape)
    assert tuple(new_size) == tuple(out_size)
    out = {"#image": O.resample_itk(image, spacing, req, new_size, "linear")}
    for k, v in sample.items():
        out[k] = O.resample_itk(v, spacing, req, new_size, "nearest").astype(np.float32)
    assert out["#image"].dtype == np.float32
    return out, float(th)
