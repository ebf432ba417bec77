"""The coded blocks of the diagonal-row-block layout (dia_build in dune-ddm_amd/csrc/csr.hpp) through the host entries: a block
of a staged segment whose rows read at most 16 distinct bit patterns keeps them in a dictionary and a 4-bit code per (row,
diagonal).  The host apply decodes as k_spmv_dia does -- window position and dictionary -- and multiplies the same doubles in the
same order as the CSR row sum => bit-exact; which blocks are coded, with how many entries, is what the values give.  No GPU needed."""
import numpy as np
import pytest

from tests.dia_cases import reference_mv, vector
from tests.dia_code_cases import WG, code_cases

CASES = code_cases()
_REF = {}


def _x(name):
    M, x, _ = CASES[name]
    return vector(M.shape[0], 11) if x is None else x


def _reference(name):
    if name not in _REF:
        with np.errstate(invalid="ignore"):
            _REF[name] = reference_mv(CASES[name][0], _x(name))
    return _REF[name]


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


def _assert_product(y, ref):
    assert np.array_equal(y, ref, equal_nan=True)
    finite = np.isfinite(ref)
    assert _same_bits(y[finite], ref[finite])                                   # the sign of a zero counts
    assert np.array_equal(np.isnan(y), np.isnan(ref))


def _env(monkeypatch, stage="default", code="default"):
    for name, value in (("DDM_SPMV_STAGE_X", stage), ("DDM_SPMV_CODE", code)):
        if value == "default":
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)


def _check_codes(M, kinds, info):
    """every coded block: the dictionary holds the block's distinct values in order of first appearance, padded with +0.0, and
    nibble k of a row's word selects the row's entry on diagonal k"""
    offsets_of = {}
    for b, (r0, r1, nd, _) in enumerate(kinds.tolist()):
        if not info["coded"][b]:
            assert info["entries"][b] == 0 and not info["codes"][r0:r1].any()
            continue
        d = info["dictionaries"][int(np.count_nonzero(info["coded"][:b]))]
        seen = []
        for r in range(r0, r1):
            for z in range(M.indptr[r], M.indptr[r + 1]):
                bits = M.data[z:z + 1].view(np.int64)[0]
                if bits not in seen:
                    seen.append(bits)
        assert len(seen) == info["entries"][b] <= 16
        assert d.view(np.int64).tolist() == seen + [0] * (16 - len(seen))
        # the segment's table: the offsets of all blocks with as many diagonals (they form one segment in all cases but one)
        offs = offsets_of.setdefault(nd, sorted({int(M.indices[z]) - r for rr0, rr1, nnd, _ in kinds.tolist() if nnd == nd
                                                 for r in range(rr0, rr1) for z in range(M.indptr[r], M.indptr[r + 1])}))
        if len(offs) != nd:
            continue                                                            # (several segments with nd diagonals: the product checks them)
        for r in range(r0, r1):
            word = info["codes"][r]
            used = np.zeros(32, dtype=bool)
            for z in range(M.indptr[r], M.indptr[r + 1]):
                k = offs.index(int(M.indices[z]) - r)
                used[k] = True
                assert d.view(np.int64)[(int(word[k // 8]) >> (4 * (k % 8))) & 15] == M.data[z:z + 1].view(np.int64)[0]
            for k in np.flatnonzero(~used):                                     # absent entries and slots from nd on: code 0
                assert (int(word[k // 8]) >> (4 * (k % 8))) & 15 == 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_coded_blocks_and_host_apply(ddm, monkeypatch, name):
    _env(monkeypatch)
    M, _, expected = CASES[name]
    y, kinds, counts = ddm.dia_build_and_apply_host(M, _x(name))
    _assert_product(y, _reference(name))
    info = ddm.dia_codes_host(M)
    assert len(info["coded"]) == counts["blocks"] == len(kinds)
    assert np.array_equal(info["coded"], info["entries"] > 0) and (info["entries"] <= 16).all()
    assert len(info["dictionaries"]) == int(info["coded"].sum())
    if expected is not None:
        assert [(r0, r1, int(e)) for (r0, r1, _, _), e in zip(kinds.tolist(), info["entries"])] == expected
    _check_codes(M, kinds, info)
    # a segment has slabs exactly when one of its blocks is not coded (the cases have one segment, or none with an uncoded block)
    mixed = bool((~info["coded"] & (kinds[:, 2] > 0)).any())
    assert (info["slabs"][kinds[:, 2] > 0] == mixed).all()
    assert info["slots_built"] == (counts["slots"] if mixed else 0)


def test_constant_boxes_are_coded_throughout(ddm, monkeypatch):
    _env(monkeypatch)
    M = CASES["constant_box"][0]
    _, kinds, counts = ddm.dia_build_and_apply_host(M, np.ones(1320))
    assert [tuple(k[:3]) for k in kinds.tolist()] == [(a, min(a + WG, 1320), 27) for a in range(0, 1320, WG)]      # the last block: 40 rows
    info = ddm.dia_codes_host(M)
    assert info["coded"].all() and info["slots_built"] == 0 and counts["slots"] > 0
    assert 2 <= info["entries"].min() and info["entries"].max() <= 5            # of {32, 0, -2, -1, 1}
    M = CASES["two_constant_boxes"][0]
    _, kinds, counts = ddm.dia_build_and_apply_host(M, np.ones(270))
    assert [tuple(k[:2]) for k in kinds.tolist()] == [(0, 60), (60, 270)] and counts["segments"] == 2
    info = ddm.dia_codes_host(M)
    assert info["coded"].all() and not info["slabs"].any() and info["slots_built"] == 0


def test_sixteen_values_are_coded_seventeen_are_not(ddm, monkeypatch):
    name = "16_and_17_values"
    M = CASES[name][0]
    _env(monkeypatch)
    y, kinds, counts = ddm.dia_build_and_apply_host(M, _x(name))
    info = ddm.dia_codes_host(M)
    assert info["entries"].tolist() == [16, 0, 3, 3, 3, 3] and counts["segments"] == 1
    assert info["slabs"].all() and info["slots_built"] == counts["slots"]        # one uncoded block: the segment keeps its slabs
    assert (info["dictionaries"][0] != 0.0).all()                               # no padding in a full dictionary
    _env(monkeypatch, code="0")
    y0, kinds0, counts0 = ddm.dia_build_and_apply_host(M, _x(name))
    info0 = ddm.dia_codes_host(M)
    assert not info0["coded"].any() and info0["slots_built"] == counts0["slots"] == counts["slots"]
    assert _same_bits(y, y0) and np.array_equal(kinds, kinds0)


def test_both_zeros_are_dictionary_entries(ddm, monkeypatch):
    _env(monkeypatch)
    name = "zeros_and_signs"
    M = CASES[name][0]
    info = ddm.dia_codes_host(M)
    bits = info["dictionaries"][0].view(np.int64)[:4].tolist()
    assert info["entries"].tolist() == [4]
    assert np.float64(0.0).view(np.int64) in bits and np.float64(-0.0).view(np.int64) in bits
    y, _, _ = ddm.dia_build_and_apply_host(M, _x(name))
    ref = _reference(name)
    assert _same_bits(y, ref)                                                   # signs included


def test_stored_zero_multiplies_absent_entry_does_not(ddm, monkeypatch):
    _env(monkeypatch)
    name = "stored_zero_and_absent_entry"
    M, x, _ = CASES[name]
    c = int(np.flatnonzero(np.isnan(x))[0])
    assert M[c - 1, c] == 0.0 and c in M.indices[M.indptr[c - 1]:M.indptr[c]] and c not in M.indices[M.indptr[c + 1]:M.indptr[c + 2]]
    assert ddm.dia_codes_host(M)["coded"].all()
    y, _, _ = ddm.dia_build_and_apply_host(M, x)
    assert np.isnan(y[c - 1]) and np.isnan(y[c]) and np.isfinite(np.delete(y, [c - 1, c])).all()


def test_full_table_uses_every_nibble(ddm, monkeypatch):
    _env(monkeypatch)
    M = CASES["full_table"][0]
    _, kinds, _ = ddm.dia_build_and_apply_host(M, np.ones(600))
    assert (kinds[:, 2] == 32).all()
    codes = ddm.dia_codes_host(M)["codes"]
    nibbles = (codes[:, :, None] >> (4 * np.arange(8, dtype=np.uint32))[None, None, :]) & 15
    assert (nibbles.reshape(600, 32).max(axis=0) == 15).all()                   # the highest code on every diagonal, the last included


def test_layout_does_not_depend_on_the_host_threads(ddm, monkeypatch):
    _env(monkeypatch)
    for name in ("constant_box", "16_and_17_values", "two_constant_boxes"):
        M = CASES[name][0]
        one, five = ddm.dia_codes_host(M, threads=1), ddm.dia_codes_host(M, threads=5)
        assert one["coded"].any()
        for key in ("coded", "entries", "slabs", "codes"):
            assert np.array_equal(one[key], five[key]), (name, key)
        assert _same_bits(one["dictionaries"], five["dictionaries"]) and one["slots_built"] == five["slots_built"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_switches_give_the_same_bits(ddm, monkeypatch, name):
    M = CASES[name][0]
    _env(monkeypatch)
    y, kinds, _ = ddm.dia_build_and_apply_host(M, _x(name))
    for stage, code in (("0", "default"), ("default", "0"), ("0", "0")):
        _env(monkeypatch, stage=stage, code=code)
        info = ddm.dia_codes_host(M, arrays=False)
        assert not info["coded"].any()                                          # only staged segments are coded
        y1, kinds1, counts1 = ddm.dia_build_and_apply_host(M, _x(name))
        assert _same_bits(y, y1) and np.array_equal(kinds, kinds1)
        assert info["slots_built"] == counts1["slots"]
