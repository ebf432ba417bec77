"""The index tables of the rank-local Schwarz passes (local_maps_build, csrc/halo.hpp, through ddm_local_maps_host) against a numpy
replay of the kernels they stand in for, on the plans and the extension map a single rank hands the library:
  src_of            k_extend, then k_pack + k_unpack<false> of the copy plan (the last source of a destination's list wins)
  own_of, cp_*      k_pack + k_unpack<true> of the add plan (the sources added in list order), then k_restrict<false, false>
The replay carries row numbers (defect) and lists of rows (sum) instead of values, so the comparison is of indices, exact.  No device."""
import numpy as np
import pytest


CASES = ["9x8x7-overlap1", "9x8x7-overlap2", "islands-2x1x2", "one-subdomain"]


def decomposition(name):
    """(the package is importable once the ddm fixture has run)"""
    from dune_ddm_amd import synth
    from dune_ddm_amd.problem import build_structured
    if name == "islands-2x1x2":
        grid, overlap = synth.StructuredPoisson((9, 8, 7), (2, 1, 2), synth.islands_kappa((8, 7, 6), 1e4, 4, 2)), 2
    elif name == "one-subdomain":
        grid, overlap = synth.StructuredPoisson((9, 8, 7), (1, 1, 1)), 2
    else:
        grid, overlap = synth.StructuredPoisson((9, 8, 7), (2, 2, 2)), int(name[-1])
    return build_structured(grid, overlap=overlap, pou_type="distance", shrink=0)


def replay_defect(n, ext_map, plan):
    """row of the non-overlapping defect each overlapping row holds after k_extend and the copy exchange, -1 for 0.0"""
    v = np.asarray(ext_map, dtype=np.int64).copy()                      # k_extend
    buf = v[np.asarray(plan["send_idx"], dtype=np.int64)]               # k_pack (reads before any row is written)
    for t, i in enumerate(plan["dst_idx"]):                             # k_unpack<false>
        s = -1                                                          # (an empty list leaves 0.0)
        for k in range(plan["dst_ptr"][t], plan["dst_ptr"][t + 1]):
            s = buf[plan["src_pos"][k]]
        v[i] = s
    return v


def replay_sum(n, n_novlp, ext_map, plan):
    """per non-overlapping row: the overlapping rows whose values k_unpack<true> + k_restrict add up, in order (first: the row itself)"""
    terms = [[i] for i in range(n)]
    buf = [[int(i)] for i in plan["send_idx"]]                          # k_pack
    for t, i in enumerate(plan["dst_idx"]):                             # k_unpack<true>: s = v[i]; s = s + buf[...] in list order
        for k in range(plan["dst_ptr"][t], plan["dst_ptr"][t + 1]):
            terms[i] = terms[i] + buf[plan["src_pos"][k]]
    out = [None] * n_novlp
    for i in range(n):                                                  # k_restrict<false, false>
        if ext_map[i] >= 0:
            assert out[ext_map[i]] is None
            out[ext_map[i]] = terms[i]
    return out


@pytest.mark.parametrize("name", CASES)
def test_tables_match_the_replayed_kernels(ddm, name):
    from dune_ddm_amd.problem import RankLocal
    rl = RankLocal(decomposition(name), 0, 1)
    maps = ddm.local_maps_host(rl.n, rl.n_o, rl.ext_map, rl.plan_ovlp_copy, rl.plan_ovlp_add)
    assert maps is not None, "a single rank's plans are rank-local: the tables exist"
    assert np.array_equal(maps["src_of"], replay_defect(rl.n, rl.ext_map, rl.plan_ovlp_copy))
    want = replay_sum(rl.n, rl.n_o, rl.ext_map, rl.plan_ovlp_add)
    assert all(w is not None for w in want)
    assert np.array_equal(maps["own_of"], [w[0] for w in want])
    assert np.array_equal(maps["cp_ptr"], np.concatenate([[0], np.cumsum([len(w) - 1 for w in want])]))
    assert np.array_equal(maps["cp_idx"], [i for w in want for i in w[1:]])
    if name == "one-subdomain":
        assert len(maps["cp_idx"]) == 0 and len(rl.plan_ovlp_add["dst_idx"]) == 0            # no halo, empty lists
        assert np.array_equal(maps["src_of"], rl.ext_map)
    else:
        assert len(maps["cp_idx"]) > 0 and (maps["src_of"] != np.asarray(rl.ext_map)).any()   # (the exchanges do something here)
        assert max(len(w) for w in want) > 2                                                 # rows with several copies: order matters


def test_tables_are_refused_where_the_general_path_is_needed(ddm):
    """a non-overlapping row with two images, or with none, has no own_of: the library keeps its general kernels"""
    none = dict(send_idx=[], dst_idx=[], dst_ptr=[0], src_pos=[])
    assert ddm.local_maps_host(3, 2, [0, 1, 1], none, none) is None
    assert ddm.local_maps_host(3, 3, [0, 1, -1], none, none) is None
    ok = ddm.local_maps_host(3, 2, [0, -1, 1], none, None)
    assert ok is not None and list(ok["own_of"]) == [0, 2] and list(ok["cp_ptr"]) == [0, 0, 0] and list(ok["src_of"]) == [0, -1, 1]
