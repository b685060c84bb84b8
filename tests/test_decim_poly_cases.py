"""The restated polyphase-decimator rule (tests/decim_poly_cases.py) on the CPU: how many kernels it
reaches, that the GPU cases of tests/test_gpu_decim_poly.py reach every one of them, and that the
inputs those cases use are fair to f32 arithmetic in the kernel's summation order."""
import collections

import pytest

import decim_poly_cases as D


def test_rule_yields_120_instantiations_and_24_geometries():
    inst = D.instantiations()
    assert len(inst) == len(set(inst)) == 120
    per_pair = collections.Counter(p for p, _, _, _ in inst)
    assert per_pair == {"RR32": 32, "RC32": 24, "CC32": 24, "RR64": 24, "RC64": 8, "CC64": 8}
    # shapes (pair, M, K): the 32-bit and real f64 ones have two lane widths each, c64 one
    assert len(D.SHAPES) == 16 + 12 + 12 + 12 + 8 + 8 == 68
    geo = {D.geometry(*i) for i in inst}
    assert len(geo) == 24
    assert len(D.geometry_shapes()) == 24 and {D.geometry(*i) for i in D.geometry_shapes()} == geo
    # both reduction branches, 1 .. 8 K-row steps per chunk, 1 .. 32 groups per wave
    assert {g[2] >= g[0] for g in geo} == {True, False}
    assert {g[3] for g in geo if g[2] < g[0]} == {2, 4}
    assert max(g[4] for g in geo) == 8
    assert {g[5] for g in geo} == {1, 2, 4, 8}
    assert {g[1] for g in geo} == {1, 2, 4, 8, 16, 32}
    for MV, G, CH, P, RPL, SPC in geo:
        assert MV * G == 64 and CH % SPC == 0 and (P == 1 or RPL == 1) and D.SEG % CH == 0


def test_rule_edges():
    assert D.on_rule("RC32", 256, 32) and not D.on_rule("RC32", 256, 32, fma=False)
    assert not D.on_rule("RC32", 512, 64) and D.on_rule("RR32", 512, 64)   # a 512-byte row
    assert not D.on_rule("RC64", 128, 32) and D.on_rule("RR64", 128, 32)
    for L, M in D.OFF_RULE[:6]:
        assert not any(D.on_rule(p, L, M) for p in D.PAIRS), (L, M)
    assert len(D.off_rule_cases()) == 6 * 6 + 5 + 2
    assert [D.j0_of(8, ci) for ci in (0, 1, 4, 7)] == [7, 6, 3, 0]
    assert D.lane_width("RR32", 7, 100, 1, True) == 4 and D.lane_width("RR32", 7, 100, 1, False) == 1
    assert D.lane_width("RR32", 6, 100, 1, True) == 1
    assert D.lane_width("RC32", 3, 101, 3, True) == 1 and D.lane_width("RC32", 3, 102, 3, True) == 2
    assert D.lane_width("CC64", 7, 100, 1, True) == 1
    assert D.poly_seg(20, 5000, 8) == 24 and D.poly_seg(0, 5000, 8) == 8 and D.poly_seg(0, 1 << 24, 4) == 256


def test_gpu_stream_cases_cover_every_instantiation():
    """the three calls of test_every_instantiation run (VW, VW, 1) lanes on an aligned input and
    (1, 1, 1) one sample past it; together they reach all 120 kernels, every call has more waves
    than a workgroup holds (interior waves and edge waves at both ends) and the second has a short
    last group"""
    cases = D.stream_cases()
    assert len(cases) == 2 * len(D.SHAPES)
    reached = set()
    for pair, M, K, offset, widths in cases:
        vw = D.vector_width(pair)
        assert widths == ((vw, vw, 1) if offset == 0 else (1, 1, 1)), (pair, M, K, offset, widths)
        plan = D.call_plan(pair, M, offset)
        assert [c[1] for c in plan] == [0, 4, (4 + D.CALLS[1]) % M] and plan[2][1] % 2 == 1
        for n, ci, j0, nout, V in plan:
            reached.add((pair, M, K, V))
            seg, groups, waves = D.waves_of(pair, M, K, V, nout, D.SEG)
            assert seg == D.SEG and waves > D.K_POLY_WAVES, (pair, M, K, V, nout, waves)
        assert any(c[3] % D.SEG for c in plan)
    assert reached == set(D.instantiations())
    assert len({D.case_id(*c) for c in cases}) == len(cases)


# the largest L of each 32-bit pair at both lane widths, and real f32 at M = 8 with four samples per
# lane (two lanes per group, every lane sums 64 products and 8 whole rows)
MODEL_CASES = [("RR32", 64, 16, 1), ("RR32", 64, 16, 4), ("RR32", 8, 16, 4), ("RC32", 32, 16, 1), ("RC32", 32, 16, 2),
               ("CC32", 32, 16, 1), ("CC32", 32, 16, 2)]


@pytest.mark.parametrize("pair,M,K,V", MODEL_CASES)
def test_f32_in_the_kernels_order_meets_8d_on_these_inputs(pair, M, K, V):
    """unfused f32 in decim_poly_kernel's summation order against f64, on the GPU cases' own taps,
    scale and stream: rel-RMS 1.2e-7 .. 1.7e-7 and a max error of at most 2.0 % of the bound
    (profiles/r16/LAB.md P1), so a GPU case that misses section 8d on these inputs is the kernel's fault"""
    L = M * K
    h, s, x = D.inputs(pair, L, sum(D.CALLS))
    y = D.model_f32(pair, M, K, V, h, s, x)
    ref = D.ref_f64(h, s, x, M)
    D.check_8d(pair, y, ref, h, s, x, f"model {pair} M={M} K={K} V={V}")
    # the model is a model of this filter: exact in f64 up to f64 rounding
    if V == 1:
        h64, x64 = h.astype(D.wide(h.dtype)), x.astype(D.wide(x.dtype))
        pairs64 = {"RR32": "RR64", "RC32": "RC64", "CC32": "CC64"}
        y64 = D.model_f32(pairs64[pair], M, K, 1, h64, D.wide(h.dtype)(s), x64)
        assert D.measure_8d(y64, ref)[0] <= 1e-14
