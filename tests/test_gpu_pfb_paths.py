"""Every kernel behind PolyPhaseFilterBank and InterpolatingFIRFilter, in both summation orders, on MI355X.

The three kernel templates of csrc/sdsp_pfb_walk.hpp have 72 instantiations with the identity
store hook (6 type pairs x {tile K = 4, 8, 16; staged with branch taps in LDS or in global memory;
per output} x {reference order, fused}).  Which one a shape runs on is pfb_route's rule, restated
in tests/pfb_cases.py and checked on the CPU in tests/test_pfb_cases.py; every case id names its
kernel and order.

 a. reference order: bit-identical to the CPU restatement (oracle/) at the handle's precision;
 b. fused, white input: both section-8d criteria against the 64-bit restatement on the widened
    input, per call and over the stream (1e-6 for 32-bit pairs, 1e-13 for 64-bit);
 c. impulses: every tap of every branch comes out exactly, in both orders, zeros elsewhere;
 d. one order, three kernels: the tile kernel, the staged kernel (output one sample past
    alignment) and execute(idx) on the last window agree bit for bit;
 e. three channels equal three one-channel handles, clone() mid-stream included;
 f. the per-output kernel's grid-stride loop takes its second turn.

Measured figures: profiles/r20/LAB.md."""
import numpy as np
import pytest

import oracle_lib as O
import pfb_cases as P
from gpu_util import bits_equal, to_dev, to_host

pytestmark = pytest.mark.gpu

sd = pytest.importorskip("solid_dsp_amd")
from solid_dsp_amd import InterpolatingFIRFilter, PolyPhaseFilterBank  # noqa: E402


def algo_of(order):
    return sd.ALGO_EXACT if order == "exact" else sd.ALGO_FMA


def handle(pair, ctor, h, M, order, channels=1):
    kw = dict(sample_dtype=P.sample_dt(pair), algo=algo_of(order), channels=channels)
    if ctor == "interp":
        f = InterpolatingFIRFilter(h, M, **kw)
    else:
        f = PolyPhaseFilterBank(h, M, P.coef_dt(pair)(1.0), **kw)
    assert len(f) == M and f.subfilter_len() == P.k_of(ctor, len(h), M)
    return f


def restatement(code, ctor, h, M):
    return O.interp(code, h, M) if ctor == "interp" else O.pfb(code, h, M, 1.0)


def stream():
    import torch
    return torch.cuda.current_stream()


def sentinel(sdt):
    sdt = np.dtype(sdt).type
    return sdt(-7.25 + 3.5j) if np.dtype(sdt).kind == "c" else sdt(-7.25)


def device_run(f, x, offset=0, guard=5):
    """one device call on [channels][n] inputs, the output `offset` samples past its allocation;
    the samples before and after the output must come back untouched"""
    n = x.shape[-1]
    total = f.channels * n * len(f)
    sdt = f.sample_dtype
    d_in = to_dev(np.array(x, dtype=sdt).reshape(-1))
    d_out = to_dev(np.full(offset + total + guard, sentinel(sdt), sdt))
    assert f.execute_block_device(d_in, n, d_out[offset:offset + total], stream()) == n * len(f)
    got = to_host(d_out)
    assert np.all(got[:offset] == sentinel(sdt)) and np.all(got[offset + total:] == sentinel(sdt))
    y = got[offset:offset + total]
    return y.reshape(f.channels, -1) if f.channels > 1 else y


FIGURES = {}  # (test, kernel, pair) -> [cases, worst rel-RMS, worst share of the max-abs bound]


def record(test, c, rr, share):
    f = FIGURES.setdefault((test, c.kernel, c.pair), [0, 0.0, 0.0])
    f[0], f[1], f[2] = f[0] + 1, max(f[1], rr), max(f[2], share)
    print(f"figure {test} {c.kernel} {c.pair}: {f[0]} cases, worst rel-RMS {f[1]:.3e}, worst share of the "
          f"max-abs bound {f[2]:.4f}")


# ---------------------------------------------------------------- a. reference order
@pytest.mark.parametrize("c", P.EXACT_CASES, ids=P.case_id)
def test_exact_is_the_restatement_bit_for_bit(c):
    h, calls, x = P.white_case(c)
    for ctor in c.ctors:
        assert P.kernel_of(c.pair, ctor, c.L, c.M) == c.kernel
        f = handle(c.pair, ctor, h, c.M, "exact")
        o = restatement(P.code_of(c.pair), ctor, h, c.M)
        for a, b in P.spans(calls):
            assert bits_equal(f.execute_block(x[a:b]), o.execute_block(x[a:b])), (ctor, a, b)


# ---------------------------------------------------------------- b. fused, white input
@pytest.mark.parametrize("c", P.FMA_CASES, ids=P.case_id)
def test_fma_meets_section_8d_on_white_input(c):
    """tests/test_pfb_cases.py holds the reference order at the handle's own precision to 0.6 of
    either criterion on these very inputs, so a fused kernel that misses them is wrong, not unlucky"""
    h, calls, x = P.white_case(c)
    ctor = c.ctors[0]
    assert P.kernel_of(c.pair, ctor, c.L, c.M) == c.kernel
    f = handle(c.pair, ctor, h, c.M, "fma")
    y = np.concatenate([f.execute_block(x[a:b]) for a, b in P.spans(calls)])
    ref = restatement(P.wide_code(c.pair), ctor, h.astype(P.wide(h.dtype)), c.M).execute_block(x.astype(P.wide(x.dtype)))
    rr, share = P.check_stream_8d(c.pair, y, ref, P.handle_taps(ctor, h, c.M), x, c.M, calls, P.case_id(c))
    record("white", c, rr, share)


# ---------------------------------------------------------------- c. impulses
@pytest.mark.parametrize("c", P.IMPULSE_CASES, ids=P.case_id)
def test_impulses_bring_out_every_tap_exactly(c):
    """amplitudes with power-of-two components: every product is exact and an output holds at most
    one rounded sum, so both orders must give the restatement's values (the two zeros count as one)"""
    h, calls, x, pos = P.impulse_case(c)
    ctor = c.ctors[0]
    K = P.k_of(ctor, c.L, c.M)
    assert P.kernel_of(c.pair, ctor, c.L, c.M) == c.kernel
    f = handle(c.pair, ctor, h, c.M, c.order)
    o = restatement(P.code_of(c.pair), ctor, h, c.M)
    y = np.concatenate([f.execute_block(x[a:b]) for a, b in P.spans(calls)])
    ref = np.concatenate([o.execute_block(x[a:b]) for a, b in P.spans(calls)])
    inside = P.response_mask(len(x), c.M, K, pos)
    assert np.count_nonzero(ref[inside]) == len(pos) * np.count_nonzero(P.handle_taps(ctor, h, c.M))
    assert not np.any(ref[~inside])
    assert y.dtype == ref.dtype and np.array_equal(y, ref), np.flatnonzero(y != ref)[:8]
    assert not np.any(y[~inside])


# ---------------------------------------------------------------- d. one order, three kernels
DEVICE_CALLS = (1028, 1, 1970, 777)


@pytest.mark.parametrize("order", P.ORDERS)
@pytest.mark.parametrize("L,M", P.THREE_KERNEL_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("pair", P.PAIRS)
def test_three_kernels_one_order(pair, L, M, order):
    """every kernel runs the same sequence of mac<EXACT> per output: the tile kernel on a
    pair-aligned output, the staged kernel on the same stream one sample past alignment and
    execute(idx) on the last window (H = K - 1, the staged kernel again) agree bit for bit"""
    K = L // M
    assert P.kernel_of(pair, "pfb", L, M) == f"tile{K}"
    assert P.kernel_of(pair, "pfb", L, M, offset=1) == P.kernel_of(pair, "pfb", L, M, H=K - 1) == "staged_lds"
    h = P.taps_of(pair, L, M, dense=True)
    x = P.white_input(sum(DEVICE_CALLS), P.sample_dt(pair), 6000 + L)
    fa, fb, fc = (handle(pair, "pfb", h, M, order) for _ in range(3))
    ya = np.concatenate([device_run(fa, x[a:b], 0) for a, b in P.spans(DEVICE_CALLS)])
    yb = np.concatenate([device_run(fb, x[a:b], 1) for a, b in P.spans(DEVICE_CALLS)])
    assert bits_equal(ya, yb), np.flatnonzero(ya != yb)[:8]
    fc.execute_block(x[:-1])
    fc.push(x[-1])
    last = np.array([fc.execute(idx) for idx in range(M)], dtype=P.sample_dt(pair))
    assert bits_equal(last, ya[-M:])


# ---------------------------------------------------------------- e. channels
@pytest.mark.parametrize("c", P.CHANNEL_CASES, ids=P.case_id)
def test_three_channels_are_three_handles(c):
    """blockIdx.y of every kernel: the same kernel in the same order, so bit-identical in both"""
    K = P.k_of("interp", c.L, c.M)
    assert P.kernel_of(c.pair, "interp", c.L, c.M) == c.kernel
    n1, n2 = (150, 131) if K >= P.LONG_K else (1028, 777)
    h = P.taps_of(c.pair, c.L, c.M, dense=True)
    x = P.white_input(3 * (n1 + n2), P.sample_dt(c.pair), 7000 + c.M).reshape(3, n1 + n2)
    f3 = handle(c.pair, "interp", h, c.M, c.order, channels=3)
    ones = [handle(c.pair, "interp", h, c.M, c.order) for _ in range(3)]
    y1 = device_run(f3, x[:, :n1])
    twin = f3.clone() if c.kernel == "per_output" else None
    y2 = device_run(f3, x[:, n1:])
    for ch in range(3):
        assert bits_equal(y1[ch], device_run(ones[ch], x[ch, :n1])), ch
        assert bits_equal(y2[ch], device_run(ones[ch], x[ch, n1:])), ch
    if twin is not None:  # the clone took the three windows, the order and the channels mid-stream
        assert twin.channels == 3
        assert bits_equal(device_run(twin, x[:, n1:]), y2)
    if c.order == "exact":
        o = restatement(P.code_of(c.pair), "interp", h, c.M)
        assert bits_equal(np.concatenate([y1[0], y2[0]]), o.execute_block(x[0]))


# ---------------------------------------------------------------- f. the grid-stride loop
def test_per_output_kernel_grid_stride_second_turn():
    """complex128 samples, two real taps, M = 1: one call of 65536 * 256 + 777 outputs, the last 777
    by lanes on their second turn.  (0 + cb[0] x[j]) + cb[1] x[j - 1] in numpy on the real view:
    plain elementwise roundings"""
    n = P.GRID_STRIDE_N
    assert P.kernel_of("RC64", "interp", 2, 1) == "per_output"
    h = np.array([0.8125, -0.3], dtype=np.float64)  # cb[0] = (h[1], h[0]): the branch is stored reversed
    r = np.random.default_rng(65536)
    xv = r.standard_normal(2 * n)
    f = InterpolatingFIRFilter(h, 1, sample_dtype=np.complex128, algo=sd.ALGO_EXACT)
    y = f.execute_block(xv.view(np.complex128))
    ref = 0.0 + h[1] * xv
    ref[2:] += h[0] * xv[:-2]
    head = O.interp(O.RC64, h, 1).execute_block(xv[:2000].view(np.complex128))  # the formula is the restatement's
    assert bits_equal(head.view(np.float64), ref[:2000])
    assert bits_equal(y.view(np.float64), ref), np.flatnonzero(y.view(np.float64) != ref)[:8]
