"""numpy restatement of the library's counter-based generator and of the dropout mask built on it (include/dram_hip.h,
dram_dropout): written from the definition, not from the kernel.  tests/test_dropout_cpu.py holds it to the Random123 known
answers; tests/test_gpu_dropout.py holds the device to it bit for bit."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57        # Philox4x32 multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85        # Weyl key increments
MASK32 = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """ctr: four uint32 words (arrays broadcast against each other), key: two.  Returns the four output words (uint32)."""
    c = [np.asarray(v, dtype=np.uint64) & MASK32 for v in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]          # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK32, p1 >> np.uint64(32), p1 & MASK32
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return [v.astype(np.uint32) for v in c]


def threshold24(p):
    return int(round(p * 2 ** 24))


def dropout_scale(p):
    return np.float32(0.0) if p == 1 else np.float32(1.0 / (1.0 - p))


def dropout_mask(n, p, seed, offset):
    """keep[i] of element i of an n-element contiguous tensor: group g = i // 4, word e = i % 4 of
    philox4x32_10({g lo, g hi, offset lo, offset hi}, {seed lo, seed hi}); kept iff (word >> 8) >= round(p * 2^24)."""
    g = np.arange((n + 3) // 4, dtype=np.uint64)
    r = philox4x32_10((g & MASK32, g >> np.uint64(32), offset & MASK32, (offset >> 32) & MASK32),
                      (seed & MASK32, (seed >> 32) & MASK32))
    words = np.stack(r, axis=1).reshape(-1)[:n]
    return (words >> np.uint32(8)) >= np.uint32(threshold24(p))
