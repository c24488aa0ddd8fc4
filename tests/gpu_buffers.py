"""Guard-banded, poisoned device buffers and the lazy-operand helpers of the C-ABI kernel tests (tests/test_gpu_onload.py,
tests/test_gpu_k1_kernels.py).  A plain module: importing it needs no GPU, using it does."""
import numpy as np
import torch

from onload_reference import coef_table

DEV = "cuda:0"
NAN = float("nan")
GUARD = 8                 # floats (or bytes, for uint8) kept around every placed tensor


def g(seed):
    return torch.Generator().manual_seed(seed)


def p(t):
    return None if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


class Placed:
    """A device tensor of `shape` whose base pointer is `shift` bytes off a 16-byte boundary (the place() idiom of
    test_conv3d_k3_wgrad_wzy_fused), with GUARD elements on either side that .intact() expects unchanged."""

    def __init__(self, shape, shift=0, fill=NAN, dtype=torch.float32, src=None):
        n = int(np.prod(shape))
        size = torch.empty((), dtype=dtype).element_size()
        assert shift % size == 0
        self.sentinel = 77 if dtype == torch.uint8 else -12345.0
        self.store = torch.full((n + 2 * GUARD + 16,), self.sentinel, dtype=dtype, device=DEV)
        lo = GUARD + ((-(self.store.data_ptr() + GUARD * size)) % 16 + shift) // size
        self.lo, self.hi = lo, lo + n
        self.t = self.store[lo:lo + n].view(*shape)
        assert self.t.data_ptr() % 16 == shift
        if src is not None:
            self.t.copy_(src)
        else:
            self.t.fill_(255 if dtype == torch.uint8 else fill)

    def intact(self):
        return bool((self.store[:self.lo] == self.sentinel).all()) and bool((self.store[self.hi:] == self.sentinel).all())


def call(name, *args):
    from dram_amd import _lib
    _lib.call(name, *args, stream())


def materialise(raw, coef, relu, shift=0):
    """xa = dram_row_affine_act(raw, coef, relu): the operand the lazy tensor stands for (pinned by test_row_affine_act)."""
    rows = coef.shape[0]
    xa = Placed(tuple(raw.shape), shift)
    call("dram_row_affine_act", p(raw), p(coef), p(xa.t), relu, rows, raw.numel() // rows)
    torch.cuda.synchronize()
    assert xa.intact() and not bool(torch.isnan(xa.t).any())
    return xa.t


def lazy_operand(shape, seed, shift=0):
    """raw ~ N(0, 1) of `shape` = (N, C, ...) on the device, its coefficient table (one row per (n, c)) and the special rows."""
    rows = shape[0] * shape[1]
    raw = Placed(shape, shift, src=torch.randn(*shape, generator=g(seed))).t
    coef, special = coef_table(rows, g(seed + 1))
    return raw, coef.to(DEV), special
