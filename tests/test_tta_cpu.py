"""Host-side checks of test-time augmentation: the view tables of dram_amd.inference.tta_views, the fp64 restatement of
tests/tta_cases.py against numpy / torch and against the oracle's evaluate_scan, the refusals, and that each planted mistake
moves the restatement by at least ten of the tolerances the GPU tests use, on their inputs.  No GPU."""
import numpy as np
import pytest
import torch

import tta_cases as T
from oracle import dram_oracle as O


def test_view_tables():
    import dram_amd
    from dram_amd.inference import tta_views
    assert dram_amd.tta_views is tta_views
    flip, full = tta_views("flip"), tta_views("full")
    assert flip == T.FLIP_VIEWS and full == T.FULL_VIEWS
    assert len(flip) == 8 and flip[0] == T.IDENTITY and all(p == (0, 1, 2) for p, _ in flip)
    assert [4 * f[0] + 2 * f[1] + f[2] for _, f in flip] == list(range(8))            # z is the high bit
    assert len(full) == 48 and len(set(full)) == 48 and full[0] == T.IDENTITY
    assert [p for p, _ in full[::8]] == sorted({p for p, _ in full})                    # lexicographic, flips fastest
    assert all(full[8 * k + n][1] == flip[n][1] for k in range(6) for n in range(8))
    group = set(full)
    for a in full:
        assert T.inverse_view(a) in group
        for b in full:
            assert T.compose_views(a, b) in group
    assert tta_views([T.CYCLE_VIEW, T.CYCLE_VIEW]) == (T.CYCLE_VIEW, T.CYCLE_VIEW)      # a repeated view is kept
    assert tta_views([([1, 2, 0], [True, 0, np.int64(0)])]) == (T.CYCLE_VIEW,)


def test_apply_view_is_transpose_and_flip():
    R = 5
    x = np.arange(R ** 3, dtype=np.float64).reshape(R, R, R)
    xt = torch.from_numpy(x)
    for view in T.FULL_VIEWS:
        perm, flip = view
        ref = np.flip(np.transpose(x, perm), axis=[k for k in range(3) if flip[k]])
        got = T.apply_view(x, view)
        assert np.array_equal(got, ref)
        assert np.array_equal(T.apply_view(got, T.inverse_view(view)), x)
        assert np.array_equal(T.apply_view(T.apply_view(x, T.inverse_view(view)), view), x)
        for other in (T.CYCLE_VIEW, T.FULL_VIEWS[29]):
            assert np.array_equal(T.apply_view(got, other), T.apply_view(x, T.compose_views(view, other)))
    for dims in ((0,), (2,), (0, 1), (0, 1, 2)):
        view = ((0, 1, 2), tuple(int(k in dims) for k in range(3)))
        assert np.array_equal(T.apply_view(x, view), torch.flip(xt, dims=dims).numpy())
    # torch.rot90 by one quarter turn in the (a, b) plane: out[.., i, .., j, ..] = in[.., j, .., n-1-i, ..]
    for a, b in ((1, 2), (0, 2), (0, 1), (2, 1)):
        perm, flip = [0, 1, 2], [0, 0, 0]
        perm[a], perm[b], flip[a] = b, a, 1
        assert np.array_equal(T.apply_view(x, (tuple(perm), tuple(flip))), torch.rot90(xt, 1, dims=(a, b)).numpy())
    # a leading batch axis rides along, and a non-cube works too
    y = np.arange(2 * 3 * 4 * 5, dtype=np.float64).reshape(2, 3, 4, 5)
    assert np.array_equal(T.apply_view(y, T.CYCLE_VIEW), np.flip(np.transpose(y, (0, 2, 3, 1)), axis=1))


def test_reference_with_the_identity_is_evaluate_scan():
    from dram_amd.configs import SLIM
    scan, lobe, spacing = T.scan_inputs()
    params, buffers = O.split_state_dict({k: v.clone() for k, v in T.slim_model().state_dict().items()})
    ref = T.run_tta_ref(SLIM, params, buffers, scan, lobe, spacing, (T.IDENTITY,), T.SCAN_R)
    htp, mask, th, ratio = O.evaluate_scan(SLIM, params, buffers, scan, lobe, spacing, resample=T.SCAN_R)
    assert np.array_equal(ref["htp"], htp) and np.array_equal(ref["mask"], mask)
    assert ref["threshold"] == th and ref["ratio"] == ratio
    assert not ref["spread"].any()
    assert float(htp.max() - htp[lobe > 0].min()) > 1e-3


def test_tolerances_are_what_the_docstring_derives():
    U = T.U
    assert T.mean_tol(1) == 5 * U and T.mean_tol(48) == 52 * U
    assert T.SIGMOID_TOL + T.RESIZE_TOL == 15 * U <= T.PASTE_TOL == 16 * U
    d = (4 + 52 + 1) * U
    assert T.var_tol(48) == 2 * d + d * d + U + 47 * U / 4 + U / 4
    assert T.spread_tol(8, T.S_MIN) == T.var_tol(8) * 256 + U
    # the additions of the mean: U ceil(log2 V) over the tree, U (2 + ... + V) / V left to right, both <= (V - 1) U
    for V in range(1, 49):
        assert (V - 1).bit_length() <= V - 1 and sum(range(2, V + 1)) / V <= V - 1


def test_tree_sum_of_equal_values():
    """The header's order of the sums, in fp32 on the host: 2, 4, 8 equal values are exact, 3 and 48 within 2 ulp -- and left to
    right they are not (the reason the definition is a tree)."""
    p = T.sigmoid32(T.base_logits(12, 3))
    for V in (1, 2, 4, 8, 16, 32):
        assert np.array_equal(T.tree_sum32([p] * V) / np.float32(V), p)
    for V in (3, 11, 48):
        m = T.tree_sum32([p] * V) / np.float32(V)
        assert (np.abs(m.astype(np.float64) - p) / np.spacing(p)).max() <= 2
    acc = p.copy()
    for _ in range(47):
        acc = acc + p
    assert (np.abs((acc / np.float32(48)).astype(np.float64) - p) / np.spacing(p)).max() > 2
    # the tree is a sum: against fp64 on distinct terms, and in the stated shape for V = 3 and V = 6
    g = np.random.default_rng(1)
    t = [g.random(50, dtype=np.float32) for _ in range(48)]
    for V in range(1, 49):
        assert np.abs(T.tree_sum32(t[:V]) - np.sum(np.float64(t[:V]), axis=0)).max() <= V * (V - 1).bit_length() * T.U + 1e-30
    assert np.array_equal(T.tree_sum32(t[:3]), (t[0] + t[1]) + t[2])
    assert np.array_equal(T.tree_sum32(t[:6]), ((t[0] + t[1]) + (t[2] + t[3])) + (t[4] + t[5]))
    assert np.array_equal(T.tree_sum32(t[:7]), ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + t[6]))


@pytest.mark.parametrize("R,L", T.SHAPES)
def test_planted_mistakes_move_the_reference(R, L):
    """On the inputs of tests/test_gpu_tta_kernels.py."""
    def moved(name, mutate):
        views = T.RANDOM_CASES[name]
        m0, v0, _ = T.random_reference(R, L, name)
        m1, v1, _ = T.combine_ref(T.random_dense(R, L, name), views, mutate)
        return np.abs(m1 - m0).max() / T.mean_tol(len(views)), np.abs(v1 - v0).max() / T.var_tol(len(views))
    assert moved("cycle_3", "forward")[0] >= 10          # the forward move in place of the inverse, a 3-cycle
    assert moved("flip8", "noflip")[0] >= 10 and moved("full48", "noflip")[0] >= 10
    assert moved("flip8", "logits")[0] >= 10 and moved("full48", "logits")[0] >= 10
    assert moved("flip8", "sample")[1] >= 10 and moved("full48", "sample")[1] >= 10
    assert moved("flip8", "sample")[0] == 0


def test_spread_pasted_without_the_lobe_test_moves_the_reference():
    prob, prob2, lobe = T.paste_prob_inputs()
    htp0 = np.full(T.VOLUME, -1.0)
    good, written = T.paste_prob_ref(prob2, lobe, T.PASTE_CHUNKS, T.PASTE_R, htp0)
    bad, written_bad = T.paste_prob_ref(prob2, lobe, T.PASTE_CHUNKS, T.PASTE_R, htp0, mutate="nolobe")
    assert written_bad.sum() > 2 * written.sum() and (written_bad | ~written).all()
    assert np.abs(bad - good).max() >= 10 * T.RESIZE_TOL
    assert np.array_equal(good[~written], htp0[~written])
    # and against the restatement with the sigmoid of tests/infer_kernel_cases.py: pasting sigmoid(dense) is lobe_paste
    dense, lobe_k, sentinel = T.K.paste_inputs()
    p64 = 1.0 / (1.0 + np.exp(-dense.astype(np.float64)))
    a, wa = T.K.lobe_paste_ref(dense, lobe_k, T.PASTE_CHUNKS, T.PASTE_R, sentinel)
    b, wb = T.paste_prob_ref(p64, lobe_k, T.PASTE_CHUNKS, T.PASTE_R, sentinel)
    assert np.array_equal(a, b) and np.array_equal(wa, wb)


def test_refusals():
    from dram_amd.inference import LobeInference, tta_views
    bad = [[],                                                  # V = 0
           list(T.FULL_VIEWS) + [T.IDENTITY],                   # V = 49
           [((0, 1, 1), (0, 0, 0))], [((0, 1, 3), (0, 0, 0))], [((0, 1), (0, 0, 0))], [((0.0, 1.0, 2.0), (0, 0, 0))],
           [((0, 1, 2), (0, 2, 0))], [((0, 1, 2), (0, 0))], [((0, 1, 2), (0, -1, 0))],
           [(0, 1, 2)], 5, "rot"]
    for views in bad:
        with pytest.raises(ValueError):
            tta_views(views)
        with pytest.raises(ValueError):
            LobeInference(object(), tta=views)
    for batch in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            LobeInference(object(), tta="flip", tta_batch=batch)
    with pytest.raises(NotImplementedError, match="cam"):
        LobeInference(object(), head="cam", tta="flip")
    inf = LobeInference(object(), tta="full", tta_batch=5)
    assert inf.views == T.FULL_VIEWS and inf.tta_batch == 5
    assert LobeInference(object()).views is None and LobeInference(object(), head="cam").views is None
