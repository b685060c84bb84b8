"""The decimator's polyphase kernel (decim_poly_kernel, csrc/kern_decim.hip; the walk in
csrc/sdsp_decim_walk.hpp) at every instantiation and lane width, on MI355X.

The dispatch instantiates the kernel 120 times: 6 type pairs x M in {8, 16, 32, 64} with an M-sample
row of 32..256 bytes x K = L / M in {2, 4, 8, 16} x lane width V in {1, 16 / sizeof(sample)}, with 24
distinct lane geometries (tests/test_decim_poly_cases.py counts them on the CPU).  Which one a call
gets is decided by the shape, the decimation phase, the input pointer and the channel count; the
handle cannot report it, so the case ids take the lane width from the restated rule in
tests/decim_poly_cases.py, which a reader has to compare with poly_by_m / poly_by_k / poly_by_v.

Every call is device work on device buffers.  The reference is the f64 restatement O.decim(<64-bit
pair>) on the widened taps, scale and stream; the tolerances are the section-8d pair, rel-RMS <= tol
and max-abs <= tol * sum|h| * |scale| * max|x| with tol = 1e-6 for 32-bit samples and 1e-13 for
64-bit, over the whole stream and over every call.  Taps are white (variance 1 / L), the scale real
or complex with the taps, the stream white at the handle's sample type.

Every case prints its rel-RMS and max-abs error against its bound.  Measured on MI355X
(profiles/r16/LAB.md P2, beside the CPU model's figures in P1): the polyphase kernel at most 1.7e-7
rel-RMS and 3.6 % of the max bound on 32-bit samples (the model: 1.7e-7, 2.0 %), 8.0e-16 on 64-bit; the
reference-order kernel with fused multiply-adds at most 6.1e-7 (L = 512) and 1.4e-15."""
import functools

import numpy as np
import pytest

import decim_poly_cases as D
import oracle_lib as O
from gpu_util import bits_equal, to_dev, empty_dev, to_host

pytestmark = pytest.mark.gpu

sd = pytest.importorskip("solid_dsp_amd")
L_ = sd._lib


def stream():
    import torch
    return torch.cuda.current_stream()


def make(pair, h, s, M, channels=1, seg=None):
    d = sd.DecimatingFIRFilter(h, s, M, sample_dtype=D.PAIRS[pair][2], channels=channels, host_step=False,
                               algo=sd.ALGO_FMA)
    if seg is not None:
        d.set_tuning(L_.TUNE_DECIM_SEG, seg)
    return d


def run(d, x, offset=0):
    """one device call; offset = samples the input sits past a 16-byte aligned allocation"""
    n = x.shape[-1]
    flat = np.ascontiguousarray(x).reshape(-1)
    buf = to_dev(np.concatenate([np.zeros(offset, flat.dtype), flat, np.zeros(1, flat.dtype)]))
    assert buf.data_ptr() % 16 == 0
    nout = d.output_count(n)
    out = empty_dev(max(d.channels * nout, 1), d.sample_dtype)
    got = d.execute_block_device(buf[offset:], n, out, stream())
    assert got == nout
    y = to_host(out)[:d.channels * nout]
    return y.reshape(d.channels, nout) if d.channels > 1 else y


def oracle(pair, h, s, M):
    w = D.wide(h.dtype)
    return O.decim(D.PAIRS[pair][3], h.astype(w), w(s), M)


@functools.lru_cache(maxsize=None)
def stream_case(pair, L, M):
    """taps, scale, the three calls' stream and its f64 restatement, computed once per shape"""
    h, s, x = D.inputs(pair, L, sum(D.CALLS))
    ref = oracle(pair, h, s, M).execute_block(x.astype(D.wide(x.dtype)))
    ref.setflags(write=False)
    return h, s, x, ref


def run_stream(d, pair, L, M, offset, what, widths=None):
    """the three ragged calls of D.CALLS on handle d under the 8d pair, per call and whole, with the
    output count, the phase and the delay line after every call"""
    h, s, x, ref = stream_case(pair, L, M)
    plan = D.call_plan(pair, M, offset)
    ys, at, mo = [], 0, 0
    for k, (n, ci, j0, nout, V) in enumerate(plan):
        assert d.get_state()[1] == ci
        y = run(d, x[at:at + n], offset)
        at += n
        assert len(y) == nout
        hist, phase = d.get_state()
        assert phase == at % M
        assert bits_equal(hist, x[at - (L - 1):at]), (what, k)
        D.check_8d(pair, y, ref[mo:mo + nout], h, s, x, f"{what} call {k + 1}" + (f" V={V}" if widths else ""))
        mo += nout
        ys.append(y)
    assert mo == len(ref)
    D.check_8d(pair, np.concatenate(ys), ref, h, s, x, f"{what} whole stream")


# ---------------------------------------------------------------- every instantiation
@pytest.mark.parametrize("pair,M,K,offset,widths", [pytest.param(*c, id=D.case_id(*c)) for c in D.stream_cases()])
def test_every_instantiation(pair, M, K, offset, widths):
    """every shape on the rule with an aligned input (lane widths VW, VW, 1 over the three calls:
    the second starts at phase 4, still vector-aligned, the third at an odd phase) and with one a
    sample past it (1, 1, 1): all 120 kernels.  SDSP_TUNE_DECIM_SEG = 32 gives every call more waves
    than a workgroup holds, so interior waves and edge waves at both ends, and the second call a
    last group shorter than seg.

    Largest rel-RMS / share of the max bound per pair (profiles/r16/LAB.md P2; the CPU model of the same
    order in P1 gives 1.2e-7 .. 1.7e-7 and at most 2.0 %): RR32 1.68e-7 / 2.7 %, RC32 1.32e-7 / 2.2 %,
    CC32 1.70e-7 / 3.6 %, RR64 8.0e-16, RC64 5.8e-16, CC64 6.1e-16."""
    plan = D.call_plan(pair, M, offset)
    assert tuple(c[4] for c in plan) == widths
    assert any(c[3] % D.SEG for c in plan)  # a short last group
    for n, ci, j0, nout, V in plan:
        assert D.waves_of(pair, M, K, V, nout, D.SEG)[2] > D.K_POLY_WAVES
    h, s, _, _ = stream_case(pair, M * K, M)
    d = make(pair, h, s, M, seg=D.SEG)
    run_stream(d, pair, M * K, M, offset, D.case_id(pair, M, K, offset, widths), widths)


@pytest.mark.parametrize("pair,M,K", [pytest.param(*c, id="{}-M{}-K{}".format(*c)) for c in D.SHAPES
                                      if D.vector_width(c[0]) > 1])
def test_lane_width_shows_in_the_bits(pair, M, K):
    """what can be observed of the restated lane-width rule: V samples per lane sum an output's
    products in another order than one per lane, so the same stream through an aligned pointer and
    through one a sample past it differs in bits in the calls where the rule gives the two different
    widths (the first two) and is bit-identical where it gives both one sample per lane (the third)"""
    L = M * K
    h, s, x, _ = stream_case(pair, L, M)
    plans = [D.call_plan(pair, M, offset) for offset in (0, 1)]
    ds = [make(pair, h, s, M, seg=D.SEG) for _ in plans]
    at = 0
    for k, n in enumerate(D.CALLS):
        ya, yb = (run(d, x[at:at + n], offset) for offset, d in enumerate(ds))
        at += n
        assert bits_equal(ya, yb) == (plans[0][k][4] == plans[1][k][4]), (pair, M, K, k)
    assert [p[4] for p in plans[0]] != [p[4] for p in plans[1]]


# ---------------------------------------------------------------- group length does not change bits
SEGS = (0, 32, 20, 4096)  # automatic, the stream cases', one rounded up where CH is 8 or 16, one group for the call


@pytest.mark.parametrize("pair,M,K,V", [pytest.param(*g, id="{}-M{}-K{}-v{}".format(*g)) for g in D.geometry_shapes()])
def test_group_length_does_not_change_bits(pair, M, K, V):
    """one shape per distinct lane geometry: an output's arithmetic is its own K rows whatever group
    walks them, so every SDSP_TUNE_DECIM_SEG gives the same bits for the same input and pointer
    (a call of 4096 inputs, then one of 20003 that reads its history, both at phase 0)"""
    L = M * K
    h, s, x = D.inputs(pair, L, 4096 + 20003)
    offset = 0 if V > 1 or D.vector_width(pair) == 1 else 1
    for n in (4096, 20003):
        assert D.lane_width(pair, D.j0_of(M, 0), n, 1, offset == 0) == V
    nout = D.output_count(M, 0, 20003)
    assert D.waves_of(pair, M, K, V, nout, 4096)[1] == 1
    outs = []
    for seg in SEGS:
        d = make(pair, h, s, M, seg=seg)
        outs.append(np.concatenate([run(d, x[:4096], offset), run(d, x[4096:], offset)]))
    for seg, y in zip(SEGS[1:], outs[1:]):
        assert bits_equal(y, outs[0]), (pair, M, K, V, seg)
    ref = oracle(pair, h, s, M).execute_block(x.astype(D.wide(x.dtype)))
    D.check_8d(pair, outs[0], ref, h, s, x, f"{pair} M={M} K={K} V={V} every seg")


# ---------------------------------------------------------------- every tap, every phase
def impulse_cases():
    out = []
    for pair in ("RR32", "RC32", "CC32", "RR64"):
        ms = [M for M in D.MS if D.on_rule(pair, 2 * M, M)]
        for M in (ms[0], ms[-1]):
            for K in (2, 16):
                for V in (1, D.vector_width(pair)):
                    out.append(pytest.param(pair, M, K, V, id=f"{pair}-M{M}-K{K}-v{V}"))
    return out


@pytest.mark.parametrize("pair,M,K,V", impulse_cases())
def test_impulse_at_every_decimation_phase(pair, M, K, V):
    """one impulse a per decimation phase, each whole response inside the call, seg = 16: output m
    after an impulse at p is scale * cr[i] * a with i = j0 + m M - p and cr[i] = h[L - 1 - i] (the
    reference walks its reversed taps forward), so a dropped or swapped tap or column shows as an
    error of the size of a tap, far above the bound"""
    L = M * K
    _, cdt, sdt, _ = D.PAIRS[pair]
    h, s = D.white_taps(L, cdt, 31 + M + K), D.scale_of(cdt)
    n = 1000 + M * (L + 3 * M + 1) + 2 * L
    pos = [1000 + k * (L + 3 * M) + k for k in range(M)]
    assert sorted(p % M for p in pos) == list(range(M)) and pos[-1] + L < n
    a = sdt(1.0 + 0.5j) if np.dtype(sdt).kind == "c" else sdt(1.25)
    x = np.zeros(n, dtype=sdt)
    x[pos] = a
    offset = 0 if V > 1 else 1
    j0 = D.j0_of(M, 0)
    assert D.lane_width(pair, j0, n, 1, offset == 0) == V
    w = D.wide(cdt)
    want = np.zeros(D.output_count(M, 0, n), dtype=D.wide(sdt))
    for p in pos:
        m = np.arange(-(-(p - j0) // M), (p + L - 1 - j0) // M + 1)
        want[m] = w(s) * h.astype(w)[L - 1 - (j0 + m * M - p)] * D.wide(sdt)(a)
    ref = oracle(pair, h, s, M).execute_block(x.astype(D.wide(sdt)))
    assert np.max(np.abs(ref - want)) <= 1e-15 * np.max(np.abs(want))  # the formula is the reference's
    assert np.count_nonzero(ref) >= L - M  # the responses do cover the taps
    y = run(make(pair, h, s, M, seg=16), x, offset)
    ma = float(np.max(np.abs(y.astype(np.complex128) - ref)))
    bound = D.bound_8d(pair, h, s, x)
    print(f"{pair} M={M} K={K} V={V} impulses: max-abs {ma:.3e} (bound {bound:.3e})")
    assert ma <= bound, (ma, bound)


# ---------------------------------------------------------------- channels
@pytest.mark.parametrize("pair,M,K", [("RR32", 8, 4), ("RC32", 32, 8), ("RR64", 16, 2)])
@pytest.mark.parametrize("n1,n2", [(20004, 10004), (20003, 10001)], ids=["n_multiple_of_VW", "n_odd"])
def test_three_channels(pair, M, K, n1, n2):
    """three channels, two calls.  n a multiple of VW keeps the channel bases 16-byte aligned and the
    vector lanes run (the second call starts at phase 4); n odd drops to one sample per lane.  Every
    channel against the f64 restatement, bit-identical to a one-channel handle fed that channel
    wherever the rule gives both the same lane width, and the state per channel"""
    L = M * K
    h, s, x = D.inputs(pair, L, 3 * (n1 + n2))
    x = x.reshape(3, n1 + n2)
    vw = D.vector_width(pair)
    v3 = [c[4] for c in D.call_plan(pair, M, 0, (n1, n2), channels=3)]
    v1 = [c[4] for c in D.call_plan(pair, M, 0, (n1, n2))]
    assert v3 == ([vw, vw] if n1 % vw == 0 else [1, 1]), v3
    d3 = make(pair, h, s, M, channels=3, seg=D.SEG)
    ones = [make(pair, h, s, M, seg=D.SEG) for _ in range(3)]
    ys, at = [], 0
    for k, n in enumerate((n1, n2)):
        y = run(d3, x[:, at:at + n])
        for c in range(3):
            yc = run(ones[c], x[c, at:at + n])
            if v3[k] == v1[k]:
                assert bits_equal(y[c], yc), (pair, k, c)
        at += n
        ys.append(y)
        hist, phase = d3.get_state()
        assert phase == at % M
        for c in range(3):
            assert bits_equal(hist[c * (L - 1):(c + 1) * (L - 1)], x[c, at - (L - 1):at]), (pair, k, c)
            assert bits_equal(ones[c].get_state()[0], x[c, at - (L - 1):at]) and ones[c].get_state()[1] == phase
    assert any(a == b for a, b in zip(v3, v1))  # the bit comparison did run
    y = np.concatenate(ys, axis=1)
    for c in range(3):
        ref = oracle(pair, h, s, M).execute_block(x[c].astype(D.wide(x.dtype)))
        D.check_8d(pair, y[c], ref, h, s, x[c], f"{pair} M={M} K={K} 3 channels v{v3} channel {c}")


# ---------------------------------------------------------------- just off the rule
@pytest.mark.parametrize("pair,L,M", [pytest.param(*c, id="{}-L{}-M{}".format(*c)) for c in D.off_rule_cases()])
def test_just_off_the_rule(pair, L, M):
    """shapes the dispatch turns away (K = 3, 1, 32; L % M != 0; M < 8; M off the list; rows of more
    than 256 bytes): ALGO_FMA runs the reference-order kernel with fused multiply-adds
    (decim_direct_kernel<..., false>), held to the same tolerances over the same three calls"""
    assert not D.on_rule(pair, L, M)
    h, s, _, _ = stream_case(pair, L, M)
    run_stream(make(pair, h, s, M, seg=D.SEG), pair, L, M, 0, f"{pair} L={L} M={M} off the rule")
