"""The arbitrary-rate resampler (sd.ArbResampler, kern_arb.hip) on MI355X.

An ArbResampler(taps, P, step=s) is by definition a linear interpolation a + mu (c - a) between two
neighbouring samples of the interpolating FIR's stream, chosen by a Q32.32 time accumulator
(include/sdsp.h).  On ALGO_EXACT it must equal that bit for bit: the yardstick is existing code, an
ALGO_EXACT InterpolatingFIRFilter on the same device that produces z (its last sample kept across
calls as z(-1)), with the formula applied on the host in the sample's dtype on real views
(tests/arb_cases.py), so every operation is rounded once.  On ALGO_FMA it is held to the
interpolator family's own pair of bounds against the formula in f64 on the widened input.

Taps and input are white throughout (tests/test_arb_capi.py test_what_the_inputs_see).  Which
kernel a shape runs on is arb_plan's rule (csrc/kern_arb.hip), restated in plans() below, asserted
against info() and named in the case ids; no case is skipped."""
import functools

import numpy as np
import pytest

import arb_cases as A
import oracle_lib as O
from gpu_util import bits_equal, rel_rms, to_dev, empty_dev, to_host

pytestmark = pytest.mark.gpu

sd = pytest.importorskip("solid_dsp_amd")

C64, C128, F32, F64 = np.complex64, np.complex128, np.float32, np.float64
# name -> (coef dtype, sample dtype, oracle dtype of the f64 restatement)
PAIRS = {
    "RR32": (F32, F32, O.RR64),
    "RC32": (F32, C64, O.RC64),
    "CC32": (C64, C64, O.CC64),
    "RR64": (F64, F64, O.RR64),
    "RC64": (F64, C128, O.RC64),
    "CC64": (C128, C128, O.CC64),
}
ALL = list(PAIRS)
STAGED, PER_OUTPUT = 1, 2
NAMES = {0: "auto", STAGED: "staged", PER_OUTPUT: "per_output"}
LDS = 48 * 1024
TUNE = 29  # SDSP_TUNE_ARB_KERNEL
NMAX = 8192  # inputs per call, at most
ONE = A.ONE


def white_taps(L, coef_dt, seed):
    r = np.random.default_rng(seed)
    h = r.standard_normal(L)
    if np.dtype(coef_dt).kind == "c":
        h = h + 1j * r.standard_normal(L)
    return (h / np.sqrt(L)).astype(coef_dt)


def white_input(n, sample_dt, seed):
    r = np.random.default_rng(seed)
    x = r.standard_normal(n)
    if np.dtype(sample_dt).kind == "c":
        x = x + 1j * r.standard_normal(n)
    return x.astype(sample_dt)


def stream():
    import torch
    return torch.cuda.current_stream()


def sub_len(L, P):
    """K as sdsp_interp_create computes it, in f32 (interp.rs:35-40)"""
    q = np.float32(L) / np.float32(P)
    return int(q) if q == np.floor(q) else int(np.ceil(q))


def plans(pair, L, P, step):
    """arb_plan restated: {kernel: outputs per workgroup} of every kernel that applies to the shape
    and step, and the automatic choice"""
    sb = np.dtype(PAIRS[pair][1]).itemsize
    K = sub_len(L, P)
    out = {PER_OUTPUT: 256}
    if (step >> 32) < K:  # else most of a staged span is samples no output reads
        tile = 4096
        while tile >= 256 and ((((A.MASK + (tile - 1) * step) >> 32) + K + 1) * sb + 15) // 16 * 16 > LDS:
            tile //= 2
        if tile >= 256:
            out[STAGED] = tile
    return out, (STAGED if STAGED in out else PER_OUTPUT)


def kernel_of(pair, L, P, step, forced=0):
    """(kernel, tile) of the next call of a handle with SDSP_TUNE_ARB_KERNEL = forced"""
    applies, auto = plans(pair, L, P, step)
    k = forced if forced in applies else auto
    return k, applies[k]


def cb_in_lds(pair, L, P, step):
    """the staged kernel's CB_LDS: span and branch table (row stride K | 1) within 48 KiB"""
    cdt, sdt = PAIRS[pair][:2]
    K = sub_len(L, P)
    tile = plans(pair, L, P, step)[0][STAGED]
    xb = ((((A.MASK + (tile - 1) * step) >> 32) + K + 1) * np.dtype(sdt).itemsize + 15) // 16 * 16
    return xb + P * (K | 1) * np.dtype(cdt).itemsize <= LDS


def make(pair, L, P, step, algo=sd.ALGO_EXACT, seed=1, channels=1, forced=0):
    cdt, sdt = PAIRS[pair][:2]
    h = white_taps(L, cdt, seed)
    r = sd.ArbResampler(h, P, step=step, sample_dtype=sdt, algo=algo, channels=channels)
    if forced:
        r.set_tuning(TUNE, forced)
    return r, h


def run(r, x, offset=0, in_offset=0, st=None):
    """one device call; offset / in_offset = samples the output / input sits past a 16-byte
    aligned allocation.  The samples before the output block and the one after its end must stay
    as they were."""
    n = x.shape[-1]
    no = r.output_count(n)
    flat = np.ascontiguousarray(x).reshape(-1)
    buf = to_dev(np.concatenate([np.zeros(in_offset, x.dtype), flat, np.zeros(1, x.dtype)]))
    out = to_dev(np.full(offset + r.channels * no + 1, 7.0, dtype=r.sample_dtype))
    got = r.execute_block_device(buf[in_offset:], n, out[offset:], st if st is not None else stream())
    assert got == no
    full = to_host(out)
    assert np.all(full[:offset] == 7.0) and full[-1] == 7.0  # nothing written outside the block
    y = full[offset:offset + r.channels * no]
    return y.reshape(r.channels, no) if r.channels > 1 else y


class Lerped:
    """The yardstick: an EXACT interpolator on the same device produces z; its last sample is kept
    across calls as z(-1); the definition's formula is applied on the host (one channel)."""

    def __init__(self, pair, taps, P, step):
        self.sdt = PAIRS[pair][1]
        self.itp = sd.InterpolatingFIRFilter(taps, P, sample_dtype=self.sdt, algo=sd.ALGO_EXACT)
        self.P, self.step, self.t = P, step, 0
        self.z_prev = self.sdt(0)

    def run(self, x):
        n = len(x)
        if n == 0:
            return np.zeros(0, self.sdt)
        d_in = to_dev(np.concatenate([x, np.zeros(1, x.dtype)]))
        d_mid = empty_dev(n * self.P + 1, self.sdt)
        self.itp.execute_block_device(d_in, n, d_mid, stream())
        z = to_host(d_mid)[:n * self.P]
        y, self.t = A.model(z, self.z_prev, self.step, self.t, n, self.P)
        self.z_prev = z[-1]
        return y.astype(self.sdt, copy=False)


# ---------------------------------------------------------------- EXACT is the formula on the interpolator
def ragged(tile, step, K):
    """call lengths: 0, 1, 2, K - 1, K, K + 1, enough inputs for two tiles and three outputs more
    (within NMAX), 0, 1 and a tail"""
    per_tile = -(-tile * step // ONE)
    big = min(NMAX, 2 * per_tile + -(-3 * step // ONE) + 2)
    return [0, 1, 2, K - 1, K, K + 1, big, 0, 1, min(NMAX, per_tile // 2 + 3)]


STEPS = [A.step_of(rate) for rate in A.RATES]
# (L, P, pairs): P in {1, 7, 32, 64}, K in {1, 4, 8, 16}; 250 taps on 32 branches are zero-padded to K = 8
SHAPES = [
    (256, 32, ALL),    # K = 8; 0.1234567 steps by 8.1 inputs: the per-output path under automatic choice
    (1024, 64, ALL),   # K = 16; the branch table of CC64 does not fit LDS beside the span
    (28, 7, ALL),      # K = 4; 0.1234567 again steps over whole windows
    (250, 32, ALL),    # a tap length that is no multiple of P
    (1, 1, ALL),       # P = 1, K = 1: b = 0 always, a is always the window one sample earlier
    (7, 7, ["RC32", "CC64"]),   # K = 1 with more than one branch
    (64, 64, ["RR32", "RC64"]),  # K = 1 at P = 64
]


def exact_cases():
    out = []
    for L, P, pairs in SHAPES:
        for pair in pairs:
            for rate, step in zip(A.RATES, STEPS):
                applies, _ = plans(pair, L, P, step)
                for forced in [0] + sorted(applies):
                    k, _ = kernel_of(pair, L, P, step, forced)
                    out.append(pytest.param(pair, L, P, step, forced,
                                            id=f"{pair}-L{L}-P{P}-r{rate}-{NAMES[forced]}-{NAMES[k]}"))
    return out


def check_stream(pair, L, P, step, forced, lens=None, offset=0, in_offset=0):
    r, h = make(pair, L, P, step, forced=forced)
    kern, tile = kernel_of(pair, L, P, step, forced)
    assert r.info() == (kern, tile), (r.info(), kern, tile)
    if forced:
        assert kern == forced  # a forced kernel applies to its shape: nothing here runs a fallback
    K = sub_len(L, P)
    assert (r.filters(), r.subfilter_len(), r.step(), r.time()) == (P, K, step, 0)
    ref = Lerped(pair, h, P, step)
    sdt = PAIRS[pair][1]
    lens = lens if lens is not None else ragged(tile, step, K)
    x = white_input(sum(lens), sdt, 11)
    at, ys, t = 0, [], 0
    for n in lens:
        blk = x[at:at + n]
        at += n
        want = ref.run(blk)
        assert r.output_count(n) == len(want)
        ys.append(run(r, blk, offset, in_offset))
        assert bits_equal(ys[-1], want), (pair, L, P, step, n)
        t = sd.arb.count(step, t, n)[1]
        assert r.time() == ref.t == t, (pair, L, P, step, n)
    return r, h, x, ys


@pytest.mark.parametrize("pair,L,P,step,forced", exact_cases())
def test_exact_is_the_formula_on_the_interpolator(pair, L, P, step, forced):
    check_stream(pair, L, P, step, forced)


def test_the_shapes_reach_what_they_are_for():
    """the restated rule against info() on every shape, step and forced value, then what the rule
    says about the shapes that are there for one path"""
    for L, P, pairs in SHAPES:
        for pair in pairs:
            for step in STEPS:
                for forced in range(3):
                    assert make(pair, L, P, step, forced=forced)[0].info() == kernel_of(pair, L, P, step, forced)
    slow = STEPS[3]  # 0.1234567: 8.1 inputs per output
    assert slow >> 32 == 8
    for L, P in ((256, 32), (28, 7), (1, 1)):  # step >= K 2^32: per output, forced staged falls back
        assert plans("RC32", L, P, slow) == ({PER_OUTPUT: 256}, PER_OUTPUT)
        assert kernel_of("RC32", L, P, slow, STAGED) == (PER_OUTPUT, 256)
    assert plans("RC32", 1024, 64, slow)[0][STAGED] == 512 and plans("RR32", 1024, 64, slow)[0][STAGED] == 1024
    assert plans("CC64", 1024, 64, slow)[0][STAGED] == 256  # the smallest tile there is
    assert plans("RC32", 256, 32, STEPS[0])[0][STAGED] == 4096 and plans("CC64", 256, 32, STEPS[0])[0][STAGED] == 2048
    assert cb_in_lds("RC32", 256, 32, STEPS[0]) and not cb_in_lds("CC64", 1024, 64, STEPS[0])
    assert STAGED not in plans("RC32", 1, 1, ONE)[0] and STAGED in plans("RC32", 1, 1, ONE - 1)[0]


# (pair, L, P, step index, forced): at least one call emits 2 tile + 3 outputs or more within NMAX inputs
RAGGED = [("RC32", 256, 32, 2, STAGED), ("RR32", 1024, 64, 2, STAGED), ("CC64", 256, 32, 0, STAGED),
          ("RC64", 28, 7, 1, STAGED), ("CC32", 250, 32, 2, 0), ("RC32", 256, 32, 3, 0), ("RR64", 28, 7, 0, PER_OUTPUT),
          ("CC32", 1, 1, 1, PER_OUTPUT), ("RC32", 7, 7, 2, STAGED)]


@pytest.mark.parametrize("pair,L,P,si,forced", RAGGED)
def test_ragged_streaming_is_one_long_call(pair, L, P, si, forced):
    """call lengths from {0, 1, 2, K - 1, K, K + 1, large}: every call equals the yardstick bit for
    bit (check_stream), the chain equals one long call of a fresh handle bit for bit, and time()
    follows sdsp_arb_count's chain"""
    step = STEPS[si]
    tile = kernel_of(pair, L, P, step, forced)[1]
    K = sub_len(L, P)
    lens = ragged(tile, step, K)
    assert set(lens) >= {0, 1, 2, K - 1, K, K + 1} and max(lens) <= NMAX
    r, h, x, ys = check_stream(pair, L, P, step, forced, lens=lens)
    assert max(len(y) for y in ys) >= 2 * tile + 3
    whole = sd.ArbResampler(h, P, step=step, sample_dtype=PAIRS[pair][1], algo=sd.ALGO_EXACT)
    whole.set_tuning(TUNE, forced)
    cut = len(x) // 2  # (two calls: one call of the whole chain would be more than NMAX inputs)
    y = np.concatenate([run(whole, x[:cut]), run(whole, x[cut:])])
    assert bits_equal(y, np.concatenate(ys))
    assert whole.time() == r.time() == sd.arb.count(step, 0, len(x))[1]


@pytest.mark.parametrize("pair", ["RC32", "RR64"])
def test_calls_that_emit_nothing_move_the_window_and_the_time(pair):
    """step = 40.25 inputs: calls of 7 inputs emit one output in five or six; the others still move
    the window (the next output reads their inputs through it) and t"""
    L, P, step = 28, 7, 40 * ONE + ONE // 4
    r, h = make(pair, L, P, step)
    ref = Lerped(pair, h, P, step)
    x = white_input(7 * 40, PAIRS[pair][1], 4)
    t, counts = 0, []
    for k in range(40):
        blk = x[7 * k:7 * (k + 1)]
        y = run(r, blk)
        assert bits_equal(y, ref.run(blk)), k
        no, t = sd.arb.count(step, t, 7)
        assert len(y) == no and r.time() == t == ref.t
        counts.append(no)
    assert counts.count(0) >= 30 and counts.count(1) == 40 - counts.count(0) == 7


# ---------------------------------------------------------------- special steps and times
@pytest.mark.parametrize("forced", [STAGED, PER_OUTPUT])
@pytest.mark.parametrize("pair,L,P,D", [("RC32", 256, 32, 1), ("CC32", 256, 32, 3), ("RR64", 28, 7, 2),
                                        ("CC64", 1024, 64, 5), ("RR32", 7, 7, 1)])
def test_integer_step_takes_the_sample_before_every_dth_input(pair, L, P, D, forced):
    """step = D 2^32: mu = 0 and b = 0 always, so the output is z(j P - 1), the interpolator's
    stream at [D P k - 1]: branch P - 1 on the window shifted by one, at every output"""
    K = sub_len(L, P)
    if forced == STAGED and D >= K:
        forced = PER_OUTPUT  # (K = 1: the staged kernel does not apply to an integer step)
    step = D * ONE
    r, h = make(pair, L, P, step, forced=forced)
    assert r.info()[0] == forced
    sdt = PAIRS[pair][1]
    n1, n2 = 3001, 1500
    x = white_input(n1 + n2, sdt, 5)
    itp = sd.InterpolatingFIRFilter(h, P, sample_dtype=sdt, algo=sd.ALGO_EXACT)
    z = np.concatenate([np.zeros(1, sdt), itp.execute_block(x)])  # z[i + 1] = z(i), z(-1) = 0
    y = np.concatenate([run(r, x[:n1]), run(r, x[n1:])])
    assert len(y) == -(-(n1 + n2) // D)
    assert bits_equal(y, z[0::D * P][:len(y)])
    assert r.time() == (-(n1 + n2)) % D * ONE


@pytest.mark.parametrize("forced", [STAGED, PER_OUTPUT])
@pytest.mark.parametrize("pair,L,P", [("RC32", 1024, 64), ("RR32", 28, 7), ("CC64", 256, 32)])
def test_a_step_with_a_tiny_fraction(pair, L, P, forced):
    """step = 2^32 + 1: the fraction grows by 2^-32 per output, so from t = 0 the branch would
    change after 2^32 / P outputs.  set_time places the fraction 100 outputs before the first
    branch boundary (b goes 0 -> 1, mu from just under 1 to just over 0), 100 before a middle one
    and 50 before it wraps (b goes P - 1 -> 0 and one input is stepped over)."""
    step = ONE + 1
    n = 700
    sdt = PAIRS[pair][1]
    x = white_input(2 * n, sdt, 6)
    for bnd in (1, P // 2 + 1, P):
        f0 = -(-bnd * ONE // P) - (100 if bnd < P else 50)  # the first f with f P >= bnd 2^32, less 100
        r, h = make(pair, L, P, step, forced=forced)
        assert r.info()[0] == forced
        ref = Lerped(pair, h, P, step)
        r.set_time(2 * ONE + f0)
        ref.t = 2 * ONE + f0
        assert r.time() == ref.t
        u, m = A.select(step, ref.t, r.output_count(n), P)
        b = u % P
        assert b[0] == bnd - 1 and b[-1] == bnd % P and len(set(b.tolist())) == 2  # the branch changes once
        assert m[0] > ONE - 101 * P and m[-1] < 1000 * P
        for blk in (x[:n], x[n:]):
            assert bits_equal(run(r, blk), ref.run(blk)), bnd
            assert r.time() == ref.t


@pytest.mark.parametrize("forced", [STAGED, PER_OUTPUT])
@pytest.mark.parametrize("pair", ["RR32", "RC32", "CC32", "RC64"])
def test_f32_mu_rounds_up_to_one(pair, forced):
    """t with f = 2^27 - 1 at P = 32: v = f P = 2^32 - 32, so b = 0 and m = 2^32 - 32 >= 2^32 - 64.
    (float)m rounds to 2^32 and mu = 1.0f (a conversion that truncates gives 1 - 2^-24, a signed one a
    negative mu); in f64 mu = 1 - 2^-27 exactly.  With mu = 1 the output is a + (c - a): c up to
    the two roundings, |out - c| <= 2^-24 (|c - a| + |c|) (1 + 2^-24), and c itself wherever c - a is
    exact."""
    L, P, n = 256, 32, 2000
    step = ONE + ONE // 2  # f alternates between 2^27 - 1 and 2^27 - 1 + 2^31: m = 2^32 - 32 both times
    t0 = 3 * ONE + (1 << 27) - 1
    cdt, sdt = PAIRS[pair][:2]
    r, h = make(pair, L, P, step, forced=forced)
    assert r.info()[0] == forced
    r.set_time(t0)
    x = white_input(n, sdt, 7)
    y = run(r, x)
    u, m = A.select(step, t0, len(y), P)
    assert np.all(m == ONE - 32) and set((u % P).tolist()) == {0, 16}
    itp = sd.InterpolatingFIRFilter(h, P, sample_dtype=sdt, algo=sd.ALGO_EXACT)
    z = itp.execute_block(x)
    assert bits_equal(y, A.lerp(z, sdt(0), u, m))
    rdt = np.dtype(sdt).type(0).real.dtype.type
    mu = m.astype(rdt) * rdt(2.0 ** -32)
    a, c = z[u - 1], z[u]
    if rdt is F32:
        assert np.all(mu == 1.0)
        assert bits_equal(y, (a + (c - a)).astype(sdt))
        # out = (c + (c - a) d1)(1 + d2), |d1|, |d2| <= 2^-24, per component; the moduli bound both
        eps = 2.0 ** -24
        a, c = a.astype(C128), c.astype(C128)
        assert np.all(np.abs(y.astype(C128) - c) <= eps * (1 + eps) * (np.abs(c - a) + np.abs(c)))
    else:
        assert np.all(mu == 1.0 - 2.0 ** -27) and not bits_equal(y, c)


# ---------------------------------------------------------------- state calls
@pytest.mark.parametrize("forced", [STAGED, PER_OUTPUT])
def test_set_step_takes_effect_at_the_next_output(forced):
    pair, L, P = "CC32", 256, 32
    r, h = make(pair, L, P, STEPS[0], forced=forced)
    ref = Lerped(pair, h, P, STEPS[0])
    x = white_input(4 * 1500, C64, 8).reshape(4, 1500)
    for k, step in enumerate((STEPS[0], STEPS[2], ONE + 1, STEPS[1])):
        t = r.time()
        r.set_step(step)
        ref.step = step
        assert r.step() == step and r.time() == t == ref.t  # t stays
        assert r.info() == kernel_of(pair, L, P, step, forced) and r.info()[0] == forced
        assert bits_equal(run(r, x[k]), ref.run(x[k])), k
    r.set_rate(0.75)
    assert r.step() == sd.arb.step_from_rate(0.75) and r.rate() == 2.0 ** 32 / r.step()
    for bad in (0, (1 << 16) - 1, (1 << 48) + 1):
        with pytest.raises(sd.SdspError) as e:
            r.set_step(bad)
        assert e.value.code == 90 and "step" in str(e.value)
    t = r.time()
    with pytest.raises(sd.SdspError) as e:
        r.set_time(1 << 63)
    assert e.value.code == 90 and r.time() == t  # a refused call moves nothing
    r.set_time((1 << 63) - 1)
    assert r.time() == (1 << 63) - 1 and r.output_count(5) == 0


def test_clone_continues_identically():
    pair, L, P, n = "RC32", 256, 32, 1101
    r, h = make(pair, L, P, STEPS[0], algo=sd.ALGO_FMA, forced=PER_OUTPUT)
    x = white_input(3 * n, C64, 9)
    run(r, x[:n])
    c = r.clone()
    assert c.time() == r.time() == sd.arb.count(STEPS[0], 0, n)[1] and c.step() == STEPS[0]
    assert c.get_algo() == sd.ALGO_FMA and c.info() == r.info() == (PER_OUTPUT, 256)
    assert (c.filters(), c.subfilter_len()) == (P, 8)
    assert bits_equal(run(c, x[n:2 * n]), run(r, x[n:2 * n]))  # window, step, time, algorithm, tuning
    assert c.time() == r.time()
    t = r.time()
    run(c, x[2 * n:])
    c.set_step(ONE)
    assert r.time() == t and r.step() == STEPS[0]  # the clone is its own object


def test_reset_and_set_channels_zero_window_and_time():
    pair, L, P, n = "RR32", 28, 7, 1001
    step = STEPS[0]
    r, h = make(pair, L, P, step)
    x = white_input(2 * n, F32, 10)
    first = run(r, x[:n])
    assert r.time() == sd.arb.count(step, 0, n)[1] != 0
    assert not bits_equal(run(r, x[:n])[:len(first) - 1], first[:len(first) - 1])  # another window, another time
    r.reset()
    assert r.time() == 0 and r.step() == step
    assert bits_equal(run(r, x[:n]), first)
    r.set_channels(1)
    assert r.time() == 0
    assert bits_equal(run(r, x[:n]), first)
    r.set_channels(2)
    assert r.time() == 0
    y = run(r, np.stack([x[:n], x[:n]]))
    assert bits_equal(y[0], first) and bits_equal(y[1], first)


@pytest.mark.parametrize("L,P,si,forced", [(256, 32, 0, STAGED), (256, 32, 2, PER_OUTPUT), (28, 7, 3, 0)])
def test_three_channels_share_the_time(L, P, si, forced):
    n, step = 4001, STEPS[si]
    r3, h = make("CC32", L, P, step, channels=3, forced=forced)
    ones = [Lerped("CC32", h, P, step) for _ in range(3)]
    singles = [make("CC32", L, P, step, forced=forced)[0] for _ in range(3)]
    x = white_input(2 * 3 * n, C64, 8).reshape(2, 3, n)
    for call in range(2):
        y = run(r3, x[call])
        for c in range(3):
            assert bits_equal(y[c], run(singles[c], x[call, c])), (call, c)
            assert bits_equal(y[c], ones[c].run(x[call, c])), (call, c)
            assert r3.time() == singles[c].time() == ones[c].t
        assert not bits_equal(y[0], y[1]) and not bits_equal(y[1], y[2])  # three different streams


# ---------------------------------------------------------------- buffer placement
@pytest.mark.parametrize("forced", [STAGED, PER_OUTPUT])
@pytest.mark.parametrize("pair", ["RR32", "RC32", "CC64"])
def test_blocks_one_sample_past_a_16_byte_boundary(pair, forced):
    """input and output each one sample past a 16-byte boundary, sentinels before the output block
    and just past its end (run): no kernel here assumes more than a sample's alignment"""
    check_stream(pair, 256, 32, STEPS[0], forced, lens=[1, 1500, 3, 900], offset=1, in_offset=1)


def test_host_block_equals_device_block():
    L, P, n, step = 256, 32, 1103, STEPS[0]
    x = white_input(2 * 2 * n, C64, 12).reshape(2, 2, n)
    a, _ = make("CC32", L, P, step, channels=2)
    b, _ = make("CC32", L, P, step, channels=2)
    for k in range(2):
        y = a.execute_block(x[k])
        assert y.shape == (2, b.output_count(n))
        assert bits_equal(y, run(b, x[k]))
        assert a.time() == b.time()
    big = 1000 * ONE
    a1, _ = make("RR64", 28, 7, big)  # a host block that emits nothing still moves the time
    a1.set_time(500 * ONE)
    assert a1.execute_block(white_input(7, F64, 1)).shape == (0,) and a1.time() == 493 * ONE
    assert len(a1.execute_block(np.zeros(0))) == 0 and a1.time() == 493 * ONE


def test_refusals():
    r, h = make("RC32", 256, 32, ONE)
    buf = empty_dev(8 * 512, C64)
    with pytest.raises(sd.SdspError) as e:  # in place
        r.execute_block_device(buf, 512, buf, stream())
    assert e.value.code == 90 and "overlap" in str(e.value)
    with pytest.raises(sd.SdspError) as e:  # the input inside the output
        r.execute_block_device(buf[200:], 300, buf, stream())
    assert e.value.code == 90
    assert r.time() == 0  # a refused call moves nothing
    for algo in (sd.ALGO_AUTO, sd.ALGO_FFT):
        with pytest.raises(sd.SdspError) as e:
            r.set_algo(algo)
        assert e.value.code == 90
    assert r.get_algo() == sd.ALGO_EXACT
    for key, value in ((TUNE, 3), (TUNE, -1), (24, 1)):
        with pytest.raises(sd.SdspError) as e:
            r.set_tuning(key, value)
        assert e.value.code == 90
    with pytest.raises(sd.SdspError) as e:
        sd.ArbResampler(h, 0, step=ONE, sample_dtype=C64)
    assert e.value.code == 3
    with pytest.raises(sd.SdspError) as e:
        sd.ArbResampler(h, 32, step=1, sample_dtype=C64)
    assert e.value.code == 90 and "step" in str(e.value)


# ---------------------------------------------------------------- FMA path
N1, N2, CH = 3001, 2222, 2  # two calls, two channels
FMA_SHAPES = ([(pair, K * P, P, si) for pair in ("RC32", "CC32") for P, K in ((32, 8), (64, 16), (7, 4))
               for si in range(4)] +
              [("RR32", 256, 32, 0), ("RC64", 256, 32, 0), ("CC64", 28, 7, 2), ("RR64", 1024, 64, 3)])
WORST = {}  # (kernel, precision) -> worst rel-RMS seen so far in this run


def fma_cases():
    out = []
    for pair, L, P, si in FMA_SHAPES:
        for k in sorted(plans(pair, L, P, STEPS[si])[0]):
            out.append(pytest.param(pair, L, P, si, k, id=f"{pair}-L{L}-P{P}-r{A.RATES[si]}-{NAMES[k]}"))
    return out


@functools.lru_cache(maxsize=None)
def fma_case(pair, L, P, si):
    """taps, input and the formula in f64 on the widened input per channel, computed once per shape"""
    cdt, sdt, odt = PAIRS[pair]
    h = white_taps(L, cdt, 100 + L + P)
    x = white_input(CH * (N1 + N2), sdt, 200 + P).reshape(CH, N1 + N2)
    wide_c = C128 if np.dtype(cdt).kind == "c" else F64
    wide_s = C128 if np.dtype(sdt).kind == "c" else F64
    ref = np.stack([A.model(O.interp(odt, h.astype(wide_c), P).execute_block(x[c].astype(wide_s)), wide_s(0),
                            STEPS[si], 0, N1 + N2, P)[0] for c in range(CH)])
    for a in (h, x, ref):
        a.setflags(write=False)
    return h, x, ref


@pytest.mark.parametrize("pair,L,P,si,forced", fma_cases())
def test_fma_path_meets_the_interpolators_bounds(pair, L, P, si, forced):
    """ALGO_FMA against the definition's formula in f64 on O.interp(<64-bit pair>) of the widened
    input, per channel, over two calls: rel-RMS <= 1e-6 (32-bit) / 1e-13 (64-bit) and max-abs <=
    tol sum|h| max|x|, the bounds of tests/test_gpu_resamp.py."""
    h, x, ref = fma_case(pair, L, P, si)
    sdt = PAIRS[pair][1]
    r = sd.ArbResampler(h, P, step=STEPS[si], sample_dtype=sdt, algo=sd.ALGO_FMA, channels=CH)
    r.set_tuning(TUNE, forced)
    assert r.info()[0] == forced
    y = np.concatenate([run(r, x[:, :N1]), run(r, x[:, N1:])], axis=1)
    assert y.shape == ref.shape
    narrow = np.dtype(sdt).itemsize // (2 if np.dtype(sdt).kind == "c" else 1) == 4
    tol = 1e-6 if narrow else 1e-13
    bound = tol * float(np.sum(np.abs(h.astype(C128)))) * float(np.max(np.abs(x.astype(C128))))
    key = (NAMES[forced], "32" if narrow else "64")
    for c in range(CH):
        rr = rel_rms(y[c], ref[c])
        ma = float(np.max(np.abs(y[c].astype(C128) - ref[c])))
        WORST[key] = max(WORST.get(key, 0.0), rr)
        print(f"{pair} L={L} P={P} rate={A.RATES[si]} {key[0]} channel {c}: rel-RMS {rr:.3e} max-abs {ma:.3e} "
              f"(bound {bound:.3e}); worst on {key[0]} {key[1]}-bit so far {WORST[key]:.3e}")
        assert rr <= tol, (pair, L, P, si, c, rr)
        assert ma <= bound, (pair, L, P, si, c, ma, bound)
