"""The receive-chain case tables reach every kernel path (no GPU).

tests/rx_cases.py restates the launch rules of kern_rx.hip; tests/test_gpu_rx_paths.py runs the
tables.  Here: every sum branch, chunk shape, boundary value, pointer form and chunk form is hit by
some case (deleting the only case on a branch fails a test below), the f32 NCO model the GPU test
compares against is the restatement's formula, and the AGC inputs drive the restatement through
every squelch mode, the gain clamp and the energy freeze.
"""
import numpy as np
import pytest

import oracle_lib as O
import rx_cases as R

C64, C128 = R.C64, R.C128


# ---------------------------------------------------------------- AutoCorrelator
def test_pipe_sum_shapes_by_hand():
    """the walk of acorr_pipe_kernel's sum at K followed by hand against kern_rx.hip, and the two limits"""
    assert R.pipe_sum_shape(1)[0] == R.pipe_sum_shape(7)[0] == "K<8"
    assert R.pipe_sum_shape(8) == ("head-only", 0, 0, False)
    assert R.pipe_sum_shape(9) == ("m7-only", 0, 0, True)
    assert R.pipe_sum_shape(10) == ("scalar", 1, 0, True)
    assert R.pipe_sum_shape(16) == ("scalar", 7, 0, True)
    assert R.pipe_sum_shape(17) == ("block", 0, 1, True)
    assert R.pipe_sum_shape(18) == ("both", 1, 1, True)
    assert R.pipe_sum_shape(128) == ("both", 7, 14, True)
    for K in range(1, R.K_PIPE_K + 1):  # the walk's own assertion: every term once
        assert R.pipe_sum_shape(K)[0] in R.PIPE_BRANCHES


def _pipe_calls(cases):
    return [p for c in cases for p in R.case_plans(c) if p["pipe"]]


def test_acorr_branch_cases_reach_every_pipelined_branch():
    """both sample types run the same table, so one count serves both"""
    plans = _pipe_calls(R.ACORR_BRANCH)
    assert {p["pipe"]["branch"] for p in plans} == set(R.PIPE_BRANCHES)
    # every residue of K mod 8 in the scalar body's length (0..7 scalar terms before the blocks)
    assert {R.pipe_sum_shape(p["K"])[1] for p in plans if p["K"] >= 8} == set(range(8))
    # the first call: leading edge tile, three interior tiles, ragged trailing tile; the second:
    # whole tiles exactly, no trailing launch
    for case in R.ACORR_BRANCH:
        first, second = R.case_plans(case)
        assert first["launches"] == [("pipe", 1, 4), ("oneshot-stage", 0, 1), ("oneshot-stage", 4, 5)], case
        assert second["launches"] == [("pipe", 1, 3), ("oneshot-stage", 0, 1)], case
        assert second["n"] % R.K_OUT == 0 and second["pipe"]["trailing"] == 0


def test_acorr_delay_cases_cross_both_limits():
    by_d = {c[1]: R.case_plans(c)[0] for c in R.ACORR_DELAY if c[0] - c[1] == 16}
    assert set(by_d) == set(R.D_BOUNDARIES)
    for d, p in by_d.items():
        assert (p["pipe"] is not None) == (d <= 128), d       # 129 leaves the pipelined kernel
        assert p["stage"] == (d <= 256), d                    # 257 leaves STAGE
        assert p["launches"][0][0] == ("pipe" if d <= 128 else "oneshot-stage" if d <= 256 else "oneshot-2load")
    # the pipelined kernel's largest footprint: K = 128 with d = 128
    big = [R.case_plans(c)[0] for c in R.ACORR_DELAY if (c[0] - c[1], c[1]) == (128, 128)]
    assert len(big) == 1 and big[0]["pipe"] and big[0]["pipe"]["branch"] == "both"


def test_acorr_no_interior_tile_case():
    (case,) = R.ACORR_NO_INTERIOR
    (p,) = R.case_plans(case)
    assert p["pipe_eligible"] and p["t_hi"] == p["t_lo"] and p["pipe"] is None
    assert p["launches"] == [("oneshot-stage", 0, 2)]


def test_acorr_oneshot_cases_reach_every_chunk_shape():
    plans = [(c, p) for c in R.ACORR_ONESHOT for p in R.case_plans(c)]
    assert all(p["pipe"] is None and not p["pipe_eligible"] for _, p in plans)  # K > 128 on the default knob
    assert {p["launches"][0][0] for _, p in plans} == {"oneshot-stage", "oneshot-2load"}
    for kern in ("oneshot-stage", "oneshot-2load"):
        chunks = [p["chunks"] for _, p in plans if p["launches"][0][0] == kern]
        assert {len(c) for c in chunks} == {1, 2, 3}, kern
        later = {c[-1] for c in chunks if len(c) > 1}
        # a later chunk of 1, 3 and 7 terms (edge()) and of 8 (the cj >= kR switch), a full last chunk
        assert {(1, "edge"), (3, "edge"), (7, "edge"), (8, "cj>=8"), (256, "cj>=8")} <= later, kern
    # the knob cases: a single chunk on either side of cj >= 8, on both one-shot forms
    knob = {(c[3], p["chunks"][0][1]) for c in R.ACORR_KNOB for p in R.case_plans(c)}
    assert knob == {(1, "edge"), (1, "cj>=8"), (2, "edge"), (2, "cj>=8")}
    assert {p["launches"][0][0] for c in R.ACORR_KNOB for p in R.case_plans(c)} == {"oneshot-stage", "oneshot-2load"}
    assert any(len(p["chunks"]) == 2 for c in R.ACORR_KNOB if c[3] == 2 for p in R.case_plans(c))


def test_acorr_cases_hit_every_boundary_value():
    ks = {c[0] - c[1] for c in R.ACORR_ALL}
    ds = {c[1] for c in R.ACORR_ALL}
    assert set(R.K_BOUNDARIES) <= ks, sorted(set(R.K_BOUNDARIES) - ks)
    assert set(R.D_BOUNDARIES) <= ds, sorted(set(R.D_BOUNDARIES) - ds)


def test_acorr_slots_cases_walk_several_tiles():
    """slots knob at its smallest value: one wave per XCD eighth"""
    branches = set()
    for case in R.ACORR_SLOTS:
        (p,) = R.case_plans(case)
        assert case[4] == 1 and case[5] == 2 and p["pipe"] and p["pipe"]["G"] == 8, case
        walks, eighths = p["pipe"]["walks"], p["pipe"]["eighths"]
        branches.add(p["pipe"]["branch"])
        if case[2][0] == 30 * R.K_OUT + 77:
            assert walks == [4] * 7 + [1] and p["pipe"]["leading"] == 1 and p["pipe"]["trailing"] == 1
        else:
            assert p["pipe"]["Q"] == 2 and eighths == [2, 2, 2, 2, 2, 1, 0, 0], case
    assert branches == {"K<8", "m7-only", "block", "both"}
    long_ = [R.case_plans(c)[0]["pipe"] for c in R.ACORR_SLOTS if c[2][0] == R.N_SLOTS[0]]
    short = [R.case_plans(c)[0]["pipe"] for c in R.ACORR_SLOTS if c[2][0] == R.N_SLOTS[1]]
    assert long_ and all(max(p["walks"]) >= 3 for p in long_)                       # the loop-carried part
    assert all(len(set(p["eighths"])) > 1 for p in long_ + short)                    # unequal eighths
    assert short and all(0 in p["eighths"] for p in short)                           # an empty eighth
    # without the knob the same calls give every tile a wave of its own: nothing walks
    for case in R.ACORR_SLOTS:
        p = R.acorr_plan(case[0], case[1], case[2][0])
        assert max(p["pipe"]["walks"]) == 1


def test_acorr_channel_cases_mix_history_and_input():
    for W, d, calls, knob, slots, ch in R.ACORR_CHANNELS:
        assert ch == 3 and calls[0] < W and sum(calls[:2]) < W      # short blocks: n < W twice over
        assert any(n > W for n in calls)
    kinds = {R.case_plans(c)[-1]["launches"][0][0] for c in R.ACORR_CHANNELS}
    assert kinds == {"pipe", "oneshot-stage"}


def test_acorr_case_ids_are_unique():
    ids = [R.acorr_id(c) for c in R.ACORR_ALL]
    assert len(ids) == len(set(ids))


# ---------------------------------------------------------------- NCO
def test_nco_cases_reach_every_form():
    forms = {R.nco_form(n, 0, i == 0, o == 0) for n in R.NCO_N for i, o in R.NCO_SHAPES}
    v2 = {f[1:] for f in forms if f[0] == "v2"}
    # two samples per lane: no vector (n = 1), one vector (n = 2), one vector and the tail lane
    # (n = 3), and the lengths round a workgroup's 2048 vectors
    assert R.nco_plan(1, 0) == {"V": 2, "nv": 0, "blocks": 1, "tail": 1, "last_block_vecs": 0, "bounded_store": True}
    assert R.nco_plan(2, 0)["nv"] == 1 and R.nco_plan(2, 0)["tail"] == 0
    assert R.nco_plan(3, 0)["nv"] == 1 and R.nco_plan(3, 0)["tail"] == 1
    assert {(1, "empty", 1), (1, "part", 0), (1, "part", 1), (1, "full", 0), (1, "full", 1),
            (2, "one-over", 1), (2, "full", 1)} <= v2
    assert [R.nco_plan(n, 0)["nv"] for n in (4095, 4096, 4097, 4099)] == [2047, 2048, 2048, 2049]
    for why in ("in-off", "out-off", "both-off"):  # one sample per lane, each cause on its own
        got = {f[1:] for f in forms if f[0] == why}
        assert {(1, "part", 0), (1, "full", 0), (2, "one-over", 0), (2, "full", 0), (3, "one-over", 0)} <= got, why
        assert all(f[3] == 0 for f in forms if f[0] == why)
    c64 = {R.nco_form(n, 1) for n in R.NCO_N}
    assert {f[0] for f in c64} == {"c64"} and {f[2] for f in c64} == {"part", "full", "one-over"}
    assert not R.nco_plan(5, 0, False, True)["bounded_store"] and not R.nco_plan(5, 1)["bounded_store"]


def test_nco_phase_cases_wrap_and_round_up():
    n = 4099
    th0, dth = R.NCO_PHASES[0]
    wraps = (th0 + (n - 1) * dth) >> 32
    assert wraps > 100                                             # wraps hundreds of times
    assert R.nco_index([0xFFE00000])[0] == 0 and R.nco_index([0xFFDFFFFF])[0] == 1023
    th = R.nco_thetas(*R.NCO_PHASES[2], 3)
    assert list(R.nco_index(th)) == [1023, 0, 0]                   # crosses the rounding point inside the call
    assert set(R.nco_index(R.nco_thetas(*R.NCO_PHASES[1], 5))) == {0}
    assert R.nco_end_state(0xFFFFFFF0, 0x20, 1) == 0x10


def test_nco_table_equals_the_restatement():
    tab = R.nco_table()
    o = O.Nco()
    for i in range(1024):
        o.set_state(i << 22, 0)
        s, c = o.sincos()
        assert s == tab[i] and c == tab[(i + 256) & 1023], i


@pytest.mark.parametrize("down", [False, True])
def test_nco_model_at_f64_is_the_restatement(down):
    """the model the c32 kernel is held to, run at f64, is O.Nco.mix_block bit for bit"""
    x = R.crand(61, 5000, C128)
    for th0, dth in R.NCO_PHASES + ((0x12345678, 0x01F7A3C5),):
        o = O.Nco()
        o.set_state(th0, dth)
        ref = o.mix_block(x, down)
        got = R.nco_model(x, th0, dth, down, np.float64)
        assert got.tobytes() == ref.tobytes(), (hex(th0), hex(dth))
        assert o.state() == (R.nco_end_state(th0, dth, len(x)), dth)
    # and the f32 run differs from it only by f32 rounding (a model that ignored its type would not)
    y32 = R.nco_model(x.astype(C64), 0x12345678, 0x01F7A3C5, down, np.float32)
    assert y32.dtype == C64
    rel = np.linalg.norm(y32 - got) / np.linalg.norm(got)
    assert 1e-9 < rel < 1e-6, rel


# ---------------------------------------------------------------- AGC
def test_agc_cases_reach_every_form():
    forms = {R.agc_form(n, R.AGC_EDGE_CHANNELS, knob, cplx)
             for n in R.AGC_EDGE_CALLS for knob in (0, 1) for cplx in (True, False)}
    want = {(k, t, l) for k in ("pipe", "plain") for t in ("complex", "real")
            for l in ("nfull=0", "exact", "whole+ragged")}
    assert forms == want
    p = R.agc_plan(16, R.AGC_EDGE_CHANNELS)
    assert p["workgroups"] == 2 and p["idle_lanes"] == 63
    idle = {c: R.agc_plan(16, c)["idle_lanes"] for c in R.AGC_EDGE_EXTRA_CHANNELS}
    assert idle == {1: 63, 63: 1, 64: 0, 130: 62} and R.agc_plan(16, 130)["workgroups"] == 3
    assert R.agc_plan(1 << 22, 2)["kernel"] == "plain" and R.agc_plan((1 << 22) - 1, 2)["kernel"] == "pipe"
    # the heterogeneous bank's three calls: whole chunks and a ragged one on either kernel
    for n in R.AGC_HET_CALLS:
        assert R.agc_form(n, R.AGC_HET_CHANNELS, 0, True)[2] == "whole+ragged"
        assert R.agc_form(n, R.AGC_HET_CHANNELS, 1, True)[2] == "whole+ragged"
    assert R.agc_plan(57, R.AGC_HET_CHANNELS)["idle_lanes"] == 58


def test_agc_het_params_are_in_range_and_differ():
    ps = R.agc_het_params()
    assert len(ps) == 70
    assert all(0.01 - 1e-12 <= p["bandwidth"] <= 0.3 + 1e-12 for p in ps)
    assert min(p["bandwidth"] for p in ps) < 0.0101 and max(p["bandwidth"] for p in ps) > 0.299
    assert all(-40.0 <= p["threshold"] <= -10.0 for p in ps)
    assert {p["scale"] for p in ps} == {0.5, 1.0, 3.0} and {p["timeout"] for p in ps} == {1, 5, 37}
    assert {p["squelch"] for p in ps} == {True, False}
    assert [c for c, p in enumerate(ps) if p["lock"]] == list(range(6, 70, 7))
    # one wave holds lanes that differ in every parameter
    first = ps[:64]
    assert len({p["bandwidth"] for p in first}) == 64 and len({p["threshold"] for p in first}) == 64
    assert {(p["squelch"], p["lock"]) for p in first} == {(True, False), (True, True), (False, False), (False, True)}


@pytest.mark.parametrize("cplx", [True, False])
def test_agc_het_inputs_are_fair(cplx):
    """on the restatement alone, sample by sample: the bank's inputs visit every squelch mode,
    reach the 1e6 gain clamp and the energy freeze, and leave no channel's output all zero"""
    x = R.agc_het_input(cplx)
    ps = R.agc_het_params()
    amps = np.sqrt(np.mean(np.abs(x[:, :R.AGC_HET_PARTS[0]]) ** 2, axis=1))
    assert amps.min() < 3e-4 and amps.max() > 5.0               # bursts over 1e-4 .. 10
    modes, clamp, freeze = set(), [], []
    for c, p in enumerate(ps):
        o = R.agc_oracle(O, p)
        y = np.empty_like(x[c])
        seen = set()
        for i in range(x.shape[1]):
            y[i] = o.execute_block(x[c, i:i + 1])[0]
            seen.add(o.get_mode())
            if o.get_gain() == 1000000.0:
                clamp.append(c)
            if o.get_energy() <= 0.000001:
                freeze.append(c)
        assert np.any(y != 0), c
        if p["lock"]:
            assert o.get_gain() == 1.0                            # locked: the gain never moves
        if not p["squelch"]:
            assert seen == {R.SQ_DISABLED}, c
        modes |= seen
    assert {R.SQ_ENABLED, R.SQ_RISE, R.SQ_SIGNALHI, R.SQ_FALL, R.SQ_SIGNALLO, R.SQ_TIMEOUT} <= modes, modes
    assert clamp and freeze, (len(set(clamp)), len(set(freeze)))
    unlocked_frozen = [c for c in set(freeze) if not ps[c]["lock"]]
    assert unlocked_frozen                                        # the freeze holds a gain that was moving


@pytest.mark.parametrize("cplx", [True, False])
def test_agc_edge_inputs_move_the_squelch(cplx):
    """the chunk-edge stream (squelch on at -30 dB, bandwidth 0.05): some channel leaves SIGNALHI"""
    x = R.agc_edge_input(R.AGC_EDGE_CHANNELS, cplx)
    assert x.shape == (65, 269)
    modes = set()
    for c in range(0, 65, 8):
        o = O.Agc()
        o.squelch(1)
        o.squelch_set_threshold(-30.0)
        o.squelch_set_timeout(5)
        assert o.set_bandwidth(0.05) == 0
        for i in range(x.shape[1]):
            o.execute_block(x[c, i:i + 1])
            modes.add(o.get_mode())
    assert {R.SQ_SIGNALHI, R.SQ_FALL, R.SQ_SIGNALLO} <= modes, modes
