"""The restated polyphase-bank rule (tests/pfb_cases.py) on the CPU: that the case tables of
tests/test_gpu_pfb_paths.py reach all 72 identity-hook instantiations of the three kernels, that
every case runs on the kernel its id names, which kernels the shapes of an older test really reach,
and that the white inputs of the fused cases are fair to the handle's own precision."""
import collections

import numpy as np
import pytest

import oracle_lib as O
import pfb_cases as P


def test_sub_filter_lengths():
    # sdsp_interp_create: whole quotients as they are, others rounded up, in f32
    assert [P.interp_k(L, M) for L, M in ((64, 8), (60, 16), (9, 3), (5, 1), (10, 4), (1, 7))] == [8, 4, 3, 5, 3, 1]
    assert P.interp_k((1 << 24) + 1, 1) == 1 << 24  # the f32 quotient drops the odd tap
    # pfb_create_common: surplus taps ignored
    assert [P.pfb_k(L, M) for L, M in ((64, 8), (60, 16), (9, 3), (10, 4), (18, 4))] == [8, 3, 3, 2, 4]
    h = np.arange(1, 11, dtype=np.float32)
    assert P.handle_taps("interp", h, 4).tolist() == list(range(1, 11)) + [0, 0]
    assert P.handle_taps("pfb", h, 4).tolist() == list(range(1, 9))


def test_rule_edges():
    for pair in P.PAIRS:
        assert P.interp_tile_applies(pair, 8, 4, 4, 0) and P.interp_tile_applies(pair, 512, 16, 16, 2)
        assert not P.interp_tile_applies(pair, 8, 4, 4, 1)     # output not aligned to a pair of samples
        assert not P.interp_tile_applies(pair, 8, 4, 3, 0)     # execute(idx): H = K - 1
        assert not P.interp_tile_applies(pair, 4, 4, 4, 0) and not P.interp_tile_applies(pair, 1024, 4, 4, 0)
        assert not P.interp_tile_applies(pair, 24, 8, 8, 0) and not P.interp_tile_applies(pair, 32, 5, 5, 0)
    assert [P.tile_geometry(M) for M in (8, 32, 512)] == [(4, 64, 1024), (16, 16, 256), (256, 1, 16)]
    # the staged kernel's last shape and the per-output kernel's first, per sample size
    assert P.pfb_route("RC64", 2, 1025)[:2] == (2048, 48 * 1024) and P.kernel_of_k("RC64", 2, 1025) == "staged_global"
    assert P.kernel_of_k("RC64", 2, 1026) == "per_output"
    assert P.kernel_of_k("CC64", 1, 1) == "per_output"  # M = 1: T = 4096 16-byte samples never fit
    assert P.kernel_of_k("RC32", 1, 2049) == "staged_global" and P.kernel_of_k("RC32", 1, 2050) == "per_output"
    assert P.kernel_of_k("RR32", 1, 8193) == "staged_global" and P.kernel_of_k("RR32", 1, 8194) == "per_output"
    assert P.kernel_of_k("RR32", 2, 10241) == "staged_global" and P.kernel_of_k("RR32", 2, 10242) == "per_output"
    # branch taps leave LDS when they no longer fit beside the samples
    assert P.kernel_of_k("RR32", 128, 95) == "staged_lds" and P.kernel_of_k("RR32", 128, 96) == "staged_global"
    assert P.kernel_of("RC64", "interp", 2, 1) == "per_output"  # the grid-stride case
    assert P.GRID_STRIDE_N > 65536 * 256


def test_tables_reach_all_72_instantiations():
    inst = P.instantiations()
    assert len(inst) == len(set(inst)) == 72
    for table in (P.EXACT_CASES + P.FMA_CASES, P.IMPULSE_CASES + P.cases("exact")):
        reached = collections.Counter((c.pair, c.kernel, c.order) for c in table)
        assert set(reached) == set(inst), set(inst) - set(reached)
    print(f"{len(set(inst))} of 72 instantiations reached by {len(P.EXACT_CASES)} exact, "
          f"{len(P.FMA_CASES)} fused and {len(P.IMPULSE_CASES)} impulse cases")
    # the impulse test runs every fused instantiation and the long-branch kernels in reference order
    imp = {(c.pair, c.kernel, c.order) for c in P.IMPULSE_CASES}
    assert {i for i in inst if i[2] == "fma" or i[1] in ("staged_global", "per_output")} == imp
    ids = [P.case_id(c) for c in P.EXACT_CASES + P.FMA_CASES]
    assert len(set(ids)) == len(ids)
    # the corners the issue names
    shapes = {(c.L, c.M, c.kernel) for c in P.FMA_CASES}
    assert {(128, 8, "tile16"), (2048, 512, "tile4"), (8192, 512, "tile16")} <= shapes
    for pair in P.PAIRS:
        tiles = {(c.M, c.kernel) for c in P.FMA_CASES if c.pair == pair and c.kernel.startswith("tile")}
        assert tiles >= {(M, f"tile{K}") for M in (8, 32, 512) for K in (4, 8, 16)}
    # M = 8 with K = 16 fills the tile kernel's sample array to its last entry but one
    assert P.tile_geometry(8)[2] + 16 - 1 == 1039


@pytest.mark.parametrize("c", P.EXACT_CASES + P.IMPULSE_CASES, ids=P.case_id)
def test_every_case_runs_on_the_kernel_its_id_names(c):
    for ctor in c.ctors:
        assert P.kernel_of(c.pair, ctor, c.L, c.M) == c.kernel, (ctor, P.k_of(ctor, c.L, c.M))
    assert c.kernel in P.case_id(c) and c.order in P.case_id(c)


def test_three_kernel_and_channel_cases():
    for pair in P.PAIRS:
        for L, M in P.THREE_KERNEL_SHAPES:
            K = L // M
            assert P.kernel_of(pair, "pfb", L, M) == f"tile{K}"
            assert P.kernel_of(pair, "pfb", L, M, offset=1) == "staged_lds"
            assert P.kernel_of(pair, "pfb", L, M, H=K - 1) == "staged_lds"
    assert {L // M for L, M in P.THREE_KERNEL_SHAPES} == {4, 8, 16}
    for c in P.CHANNEL_CASES:
        assert P.kernel_of(c.pair, "interp", c.L, c.M) == c.kernel, c
    assert {(P.sample_bytes(c.pair), c.kernel, c.order) for c in P.CHANNEL_CASES} == \
        {(sb, k, o) for sb in (4, 8, 16) for k in P.CHANNEL_KERNELS for o in P.ORDERS}


def test_kernels_of_the_older_staged_parity_shapes():
    """test_pfb_staged_kernel_bit_parity (tests/test_gpu_fir.py) by the same rule: only pairs with
    8- and 16-byte samples leave the staged kernel at (12000, 2), and only 16-byte ones at
    (6000, 2); real f32 stays on it throughout, so no shape there runs pfb_kernel<float, float, *>"""
    got = {(L, M): {pair: P.kernel_of(pair, "pfb", L, M) for pair in P.PAIRS} for L, M in P.STAGED_PARITY_SHAPES}
    for L, M in ((21, 3), (240, 24), (3000, 1000)):
        assert set(got[L, M].values()) == {"staged_lds"}
    assert got[6000, 2] == {"RR32": "staged_lds", "RC32": "staged_global", "CC32": "staged_global",
                            "RR64": "staged_global", "RC64": "per_output", "CC64": "per_output"}
    assert got[12000, 2] == {"RR32": "staged_global", "RC32": "per_output", "CC32": "per_output",
                             "RR64": "per_output", "RC64": "per_output", "CC64": "per_output"}
    assert "per_output" not in {got[s]["RR32"] for s in got}


def test_streams():
    assert P.calls_of(16) == P.RAGGED and sum(P.RAGGED) == 3778
    for K in (1025, 2050, 10242):
        calls = P.calls_of(K)
        assert 1 not in calls and max(calls) <= 300 and sum(calls[:-1]) >= K + 300  # the history is full before the last call
    for c in P.IMPULSE_CASES:
        K = P.k_of(c.ctors[0], c.L, c.M)
        h, calls, x, pos = P.impulse_case(c)
        assert pos[0] == 0 and pos[1] == calls[0] - 1 and len(x) == sum(calls)
        assert np.count_nonzero(x) == len(pos) and min(np.diff(pos)) > K and pos[-1] + K <= len(x)
        in2 = [p - calls[0] for p in pos[2:]]
        if c.kernel.startswith("tile"):
            T = P.tile_geometry(c.M)[2]
            assert (in2[0] + 1) % T == 0 and (in2[1] + 1) % 16 == 0 and (T == 16 or (in2[1] + 1) % T)
        elif c.kernel.startswith("staged"):
            assert (in2[0] + 1) % P.pfb_route(c.pair, c.M, K)[0] == 0 and calls[1] > in2[0] + 1
        else:
            assert not in2
        assert len(x) * c.M * K <= 5e8  # a few seconds at the most on one core


def oracle(code, ctor, h, M):
    return O.interp(code, h, M) if ctor == "interp" else O.pfb(code, h, M, 1.0)


WORST = {}


@pytest.mark.parametrize("c", P.FMA_CASES, ids=P.case_id)
def test_own_precision_in_reference_order_keeps_to_0p6_tol(c):
    """the condition that keeps section 8d meaningful for a fused kernel: on every white-input case
    the reference-order restatement at the handle's own precision is within 0.6 tol of the 64-bit
    restatement on the widened input, on both criteria, per call and over the stream"""
    h, calls, x = P.white_case(c)
    ctor = c.ctors[0]
    K = P.k_of(ctor, c.L, c.M)
    if P.is_32bit(c.pair) and K >= P.LONG_K:
        assert np.count_nonzero(h.reshape(K, c.M)[:, 0]) == 192
    own = oracle(P.code_of(c.pair), ctor, h, c.M).execute_block(x)
    ref = oracle(P.wide_code(c.pair), ctor, h.astype(P.wide(h.dtype)), c.M).execute_block(x.astype(P.wide(x.dtype)))
    assert len(own) == len(x) * c.M
    rr, share = P.check_stream_8d(c.pair, own, ref, P.handle_taps(ctor, h, c.M), x, c.M, calls, P.case_id(c), share=0.6)
    key = (c.kernel, c.pair)
    WORST[key] = max(WORST.get(key, 0.0), rr)
    print(f"worst own-precision rel-RMS on {key} so far {WORST[key]:.3e}")
