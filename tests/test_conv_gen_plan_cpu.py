"""CPU checks behind tests/test_gpu_conv_gen_tiles.py: the restated plans of csrc/conv3d_gen.hip (tests/conv_gen_cases.py)
agree with the library where the library can be asked without a GPU, the restated backward-data phases are the transposed
convolution, and the case table reaches every branch it was written for."""
import pytest

from dram_amd import _lib

import conv_gen_cases as G

IDS = [c.name for c in G.CASES]


@pytest.mark.parametrize("case", G.CASES, ids=IDS)
def test_workspace_bytes_pin_the_split_plan(case):
    """ws_bytes = nsplit * Cout * Cin * T * 4: the library's nsplit (hence boxes_per_split) is the restated one."""
    w = G.plan(case)["wgrad"]
    got = int(_lib.lib.dram_conv3d_wgrad_ws_bytes(*G.geom_args(case)))
    assert got > 0, "the library rejects the geometry"
    assert got == w["nsplit"] * case.Cout * case.Cin * w["T"] * 4, (got, w)
    assert got == w["ws_bytes"]
    # the split plan is self-consistent: every box in exactly one split, no empty split
    assert (w["nsplit"] - 1) * w["boxes_per_split"] < w["nboxes"] <= w["nsplit"] * w["boxes_per_split"]
    assert w["last_split"] == w["nboxes"] - (w["nsplit"] - 1) * w["boxes_per_split"]
    assert w["CIB"] * w["HV"] <= G.WG_HALO_MAX and w["CIB"] * w["T"] <= 4 * G.WG_NT * 32


def test_unsplit_and_split_workspace_sizes():
    """Two geometries worked out by hand from wgrad_plan, so that the restatement is not only compared with itself."""
    # 1 x 4 -> 8, 9^3, 3^3 valid: output 7^3, boxes 1 x 2 x 4 = 8 < 1024 splits -> one box per split
    assert int(_lib.lib.dram_conv3d_wgrad_ws_bytes(1, 4, 8, 9, 9, 9, 3, 3, 3, 1, 1, 1, 0, 0, 0)) == 8 * 8 * 4 * 27 * 4
    # 3 x 64 -> 64, (10, 10, 40), 5^3 pad 2: HV = 36 * 8 * 6 = 1728, CIB = min(512 / 125, 12288 / 1728, 64) = 4, 16 groups x 2
    # tiles -> 32 splits for 3 * 2 * 3 * 5 = 90 boxes -> 3 boxes per split, 30 splits
    assert int(_lib.lib.dram_conv3d_wgrad_ws_bytes(3, 64, 64, 10, 10, 40, 5, 5, 5, 1, 1, 1, 2, 2, 2)) == 30 * 64 * 64 * 125 * 4


def _phase_geometries():
    for size in range(1, 13):
        for k in range(1, 8):
            for s in (1, 2):
                for p in range(0, max(k - 1, 1) + 1):
                    if size + 2 * p >= k:
                        yield size, k, s, p


def test_phases_partition_the_input_and_match_the_transposed_convolution():
    n = 0
    for size, k, s, p in _phase_geometries():
        out = (size + 2 * p - k) // s + 1
        assert out >= 1
        phases = [G.make_phase(size, k, s, p, r) for r in range(s)]
        pos = sorted(i for ph in phases for i in G.phase_positions(ph))
        assert pos == list(range(size)), (size, k, s, p, pos)
        for ph in phases:
            assert ph["T"] == len(range(ph["r"], k, s))
            for q, i in enumerate(G.phase_positions(ph)):
                assert G.phase_pairs(ph, q, out) == G.transposed_pairs(i, out, k, s, p), (size, k, s, p, ph, q)
                n += 1
    assert n == 4364          # dx positions visited: none of the loops above was empty


@pytest.mark.parametrize("case", G.CASES, ids=IDS)
def test_case_meets_its_conditions(case):
    pl = G.plan(case)
    assert case.conds, "a case without a purpose"
    for name in case.conds:
        assert G.CONDITIONS[name](case, pl), (name, pl)
    # the limits of check_geom and launch_fwd
    for a in range(3):
        assert 1 <= case.k[a] <= 7 and case.s[a] in (1, 2) and 0 <= case.p[a] <= max(case.k[a] - 1, 1)
    assert case.shift % 4 == 0 and 0 <= case.shift < 16
    # backward-data writes every dx element exactly once (or zero-fills it)
    for a in range(3):
        pos = sorted(i for ph in pl["dx"]["axes"][a] for i in G.phase_positions(ph))
        assert pos == list(range(case.size[a]))


def test_every_condition_has_a_case():
    met = {name for c in G.CASES for name in c.conds}
    assert met == set(G.CONDITIONS), set(G.CONDITIONS) ^ met


def test_table_reaches_each_instantiation_and_plan_branch():
    plans = [(c, G.plan(c)) for c in G.CASES]
    # forward kernel: BX = 32 with each WQ, in the forward launch and among the backward-data phases
    assert {pl["fwd"]["WQ"] for _, pl in plans if pl["fwd"]["BX"] == 32 and pl["fwd"]["nbx"] >= 2} == {5, 13, 25}
    assert any(la["nbx"] >= 2 and la["phase"][2]["os"] == 2 for _, pl in plans for la in pl["dx"]["launches"])
    # forward launch with and without dynamic LDS
    assert {pl["fwd"]["lds"] > G.LDS_STATIC_LIMIT for _, pl in plans} == {True, False}
    # backward-weights: one, two and three boxes per split; nsplit != nboxes for the slab reduction
    assert {min(pl["wgrad"]["boxes_per_split"], 3) for _, pl in plans} == {1, 2, 3}
    assert any(pl["wgrad"]["nsplit"] != pl["wgrad"]["nboxes"] for _, pl in plans)
    # the float64 reference stays small: below 40 GFLOP for the forward and both gradients of the largest case
    for c, pl in plans:
        vox = c.N * pl["out"][0] * pl["out"][1] * pl["out"][2]
        assert 3 * 2 * vox * c.Cin * c.Cout * c.k[0] * c.k[1] * c.k[2] < 40e9, c.name
