"""The fused digital down-converter (sd.DDC, kern_ddc.hip) on MI355X.

A DDC handle is by definition NCO mix-down followed by the decimating FIR.  On ALGO_EXACT it
must equal that composition bit for bit: the yardstick is existing code, NCO.mix_block_device
into a scratch buffer and then an ALGO_EXACT DecimatingFIRFilter on it (and, for complex128, the
CPU restatement O.Nco().mix_block into O.decim).  On ALGO_FMA it is held to the decimators'
section-8d pair against the f64 restatement of the same composition on the widened input:
rel-RMS <= 1e-6 and max-abs <= 1e-6 * sum|h| * |scale| * max|x| for 32-bit samples, rel-RMS <=
1e-13 for 64-bit.

Taps are white (Kaiser taps hide dropped end taps, tests/test_gpu_fir_ols_white.py), real and
complex, with a complex scale on the complex-tap pairs."""
import functools

import numpy as np
import pytest

import oracle_lib as O
from gpu_util import bits_equal, rel_rms, to_dev, empty_dev, to_host

pytestmark = pytest.mark.gpu

sd = pytest.importorskip("solid_dsp_amd")
L_ = sd._lib

C64, C128, F32, F64 = np.complex64, np.complex128, np.float32, np.float64
# name -> (sdsp dtype, coef dtype, sample dtype, oracle dtype of the f64 restatement, NCO precision)
PAIRS = {
    "RC32": (sd.RC32, F32, C64, O.RC64, 0),
    "CC32": (sd.CC32, C64, C64, O.CC64, 0),
    "RC64": (sd.RC64, F64, C128, O.RC64, 1),
    "CC64": (sd.CC64, C128, C128, O.CC64, 1),
}
THETA0, DTHETA = 0x9E3779B9, 0x0A3D70A3  # an odd-ish phase and a frequency near 0.04 cycles / sample


def white_taps(L, coef_dt, seed):
    r = np.random.default_rng(seed)
    h = r.standard_normal(L)
    if np.dtype(coef_dt).kind == "c":
        h = h + 1j * r.standard_normal(L)
    return (h / np.sqrt(L)).astype(coef_dt)


def scale_of(coef_dt):
    return coef_dt(0.75 - 0.5j) if np.dtype(coef_dt).kind == "c" else coef_dt(0.75)


def white_input(n, sample_dt, seed):
    r = np.random.default_rng(seed)
    return (r.standard_normal(n) + 1j * r.standard_normal(n)).astype(sample_dt)


def stream():
    import torch
    return torch.cuda.current_stream()


def ddc_run(d, x, offset=0, st=None):
    """one device call; offset = samples the input sits past a 16-byte aligned allocation"""
    n = x.shape[-1]
    flat = np.ascontiguousarray(x).reshape(-1)
    buf = to_dev(np.concatenate([np.zeros(offset, flat.dtype), flat, np.zeros(1, flat.dtype)]))
    nout = d.output_count(n)
    out = empty_dev(max(d.channels * nout, 1), d.sample_dtype)
    got = d.execute_block_device(buf[offset:], n, out, st if st is not None else stream())
    assert got == nout
    y = to_host(out)[:d.channels * nout]
    return y.reshape(d.channels, nout) if d.channels > 1 else y


class Pair:
    """The two-handle composition as the parent commit has it."""

    def __init__(self, pair, taps, scale, M, algo=None):
        _, _, sdt, _, self.prec = PAIRS[pair]
        self.nco = sd.NCO()
        self.dec = sd.DecimatingFIRFilter(taps, scale, M, sample_dtype=sdt, host_step=False,
                                          algo=sd.ALGO_EXACT if algo is None else algo)
        self.sdt = sdt

    def run(self, x, down=True):
        n = len(x)
        d_in = to_dev(np.concatenate([x, np.zeros(1, x.dtype)]))
        d_mix = empty_dev(n + 1, self.sdt)
        nout = self.dec.output_count(n)
        d_out = empty_dev(max(nout, 1), self.sdt)
        self.nco.mix_block_device(d_in, n, d_mix, down=down, precision=self.prec, stream=stream())
        got = self.dec.execute_block_device(d_mix, n, d_out, stream())
        assert got == nout
        return to_host(d_out)[:nout]


def make(pair, L, M, algo=sd.ALGO_EXACT, seed=1, channels=1):
    dt, cdt, sdt, _, _ = PAIRS[pair]
    h, s = white_taps(L, cdt, seed), scale_of(cdt)
    return sd.DDC(h, s, M, sample_dtype=sdt, algo=algo, channels=channels), h, s


def same_state(d, p):
    hd, cd = d.get_state()
    hp, cp = p.dec.get_state()
    return bits_equal(hd, hp) and cd == cp and d.nco_state() == p.nco.state()


# ---------------------------------------------------------------- EXACT is the composition
EXACT_SHAPES = [(2, 7), (5, 33), (32, 256), (1, 16)]


@pytest.mark.parametrize("M,L", EXACT_SHAPES)
@pytest.mark.parametrize("pair", list(PAIRS))
def test_exact_is_the_two_handle_composition(pair, M, L):
    d, h, s = make(pair, L, M)
    p = Pair(pair, h, s, M)
    d.set_nco_state(THETA0, DTHETA)
    p.nco.set_state(THETA0, DTHETA)
    _, _, sdt, odt, _ = PAIRS[pair]
    lens = [0, 1, M - 1, M, L - 2, L - 1, L, 3001, 0, 2 * M + 1, 4097, 777]
    x = white_input(sum(lens), sdt, 11)
    at = 0
    for n in lens:
        blk = x[at:at + n]
        at += n
        assert d.output_count(n) == p.dec.output_count(n)
        y = ddc_run(d, blk)
        assert bits_equal(y, p.run(blk)), (pair, M, L, n)
        assert same_state(d, p), (pair, M, L, n)
    if sdt is C128:  # and the CPU restatement, over the whole stream
        nco = O.Nco()
        d2, _, _ = make(pair, L, M)
        for obj in (nco, d2):
            obj.set_phase(1.25)
            obj.set_frequency(0.3)
        assert nco.state() == d2.nco_state()
        ref = O.decim(odt, h, s, M).execute_block(nco.mix_block(x, down=True))
        assert bits_equal(np.concatenate([ddc_run(d2, x[:5000]), ddc_run(d2, x[5000:])]), ref)
        assert nco.state() == d2.nco_state()


# ---------------------------------------------------------------- oscillator wrap, direction
@pytest.mark.parametrize("pair", ["RC32", "CC64"])
def test_oscillator_wraps_inside_and_between_calls(pair):
    """theta near 2^32 and a delta_theta for which (u32) j * dtheta wraps thousands of times in a
    call and n * delta_theta wraps between calls; delta_theta = 0 is a constant phase"""
    M, L = 5, 33
    sdt = PAIRS[pair][2]
    x = white_input(3 * 6001, sdt, 5)
    for theta, dtheta in ((0xFFFFFF00, 0xC0000001), (0xFFFFFFFF, 0x7FFFFFFF), (0x40000000, 0)):
        d, h, s = make(pair, L, M)
        p = Pair(pair, h, s, M)
        d.set_nco_state(theta, dtheta)
        p.nco.set_state(theta, dtheta)
        for k in range(3):
            blk = x[6001 * k:6001 * (k + 1)]
            assert bits_equal(ddc_run(d, blk), p.run(blk)), (theta, dtheta, k)
            assert same_state(d, p)
        assert d.nco_state() == ((theta + 3 * 6001 * dtheta) & 0xFFFFFFFF, dtheta)
    # a constant phase is one complex factor in front of the plain decimator
    d, h, s = make(pair, L, M)
    d.set_nco_state(0x40000000, 0)  # a quarter turn: the phasor is (0, 1), mix_down multiplies by -j
    dec = sd.DecimatingFIRFilter(h, s, M, sample_dtype=sdt, host_step=False, algo=sd.ALGO_EXACT)
    y = ddc_run(d, x[:6001])
    ref = dec.execute_block((x[:6001] * -1j).astype(sdt))
    assert rel_rms(y, ref) <= (1e-6 if sdt is C64 else 1e-13)


@pytest.mark.parametrize("pair", ["CC32", "RC64"])
def test_direction_up_is_mix_up(pair):
    M, L = 2, 7
    d, h, s = make(pair, L, M)
    p = Pair(pair, h, s, M)
    d.set_direction(True)
    d.set_nco_state(THETA0, DTHETA)
    p.nco.set_state(THETA0, DTHETA)
    x = white_input(4001, PAIRS[pair][2], 6)
    up = ddc_run(d, x)
    assert bits_equal(up, p.run(x, down=False))
    d.set_direction(False)
    d.reset()
    d.set_nco_state(THETA0, DTHETA)
    assert not bits_equal(ddc_run(d, x), up)


# ---------------------------------------------------------------- FMA path
N1, N2 = 98306, 40001  # N1 = 2 mod every M: the second call starts at decimator phase 2
FMA_SEG = 32           # outputs per lane group: every call has dozens of waves and a short last group


@functools.lru_cache(maxsize=None)
def fma_case(pair, M, K):
    """taps, scale, input and the f64 restatement of the composition, computed once per shape"""
    _, cdt, sdt, odt, _ = PAIRS[pair]
    L = M * K
    h, s = white_taps(L, cdt, 100 + M + K), scale_of(cdt)
    x = white_input(N1 + N2, sdt, 200 + M)
    nco = O.Nco()
    nco.set_phase(2.0)
    nco.set_frequency(0.7)
    wide = np.complex128 if np.dtype(cdt).kind == "c" else np.float64
    ref = O.decim(odt, h.astype(wide), wide(s), M).execute_block(nco.mix_block(x.astype(C128), down=True))
    for a in (h, x, ref):
        a.setflags(write=False)
    return h, s, x, ref


def check_8d(y, ref, h, s, x, sdt, what):
    rr = rel_rms(y, ref)
    ma = float(np.max(np.abs(y.astype(C128) - ref)))
    bound = 1e-6 * float(np.sum(np.abs(h))) * abs(s) * float(np.max(np.abs(x)))
    print(f"{what}: rel-RMS {rr:.3e} max-abs {ma:.3e} (bound {bound:.3e})")
    if sdt is C64:
        assert rr <= 1e-6, (what, rr)
        assert ma <= bound, (what, ma, bound)
    else:
        assert rr <= 1e-13, (what, rr)


# (pair, M, K).  The polyphase kernel takes L = K M with K in {2, 4, 8, 16} and an M-sample row of
# 32..256 bytes: M in {8, 16, 32} for c32 samples, {8, 16} for c64.  Its corners are therefore
# (8 | 32, 2 | 16) on c32; a 64-sample c32 row is 512 bytes and runs the reference-order kernel with
# fused multiply-adds (ddc_direct_kernel<FMA>), which has one lane shape.  Besides the corners:
# (32, 8) is cfg4's shape, (32, 2), (32, 4) and c64 (16, 2) walk several K-row steps per reduction
# chunk (SPC = 2 or 4), (16, 16) is the middle M at the largest K.
FMA_SHAPES = [("RC32", 8, 2), ("RC32", 8, 16), ("RC32", 32, 2), ("RC32", 32, 16), ("RC32", 32, 8), ("RC32", 32, 4),
              ("RC32", 16, 16), ("RC32", 64, 2), ("RC32", 64, 16),
              ("CC32", 8, 2), ("CC32", 8, 16), ("CC32", 32, 2), ("CC32", 32, 16), ("CC32", 32, 8),
              ("CC32", 64, 2), ("CC32", 64, 16),
              ("RC64", 16, 4), ("RC64", 16, 2), ("CC64", 8, 4)]


def fma_kernel(pair, M, K, offset):
    """the kernel a shape runs on, as kern_ddc.hip dispatches it (the case ids name it)"""
    c32 = PAIRS[pair][2] is C64
    if M * (8 if c32 else 16) > 256:
        return "direct_fma"
    # two samples per lane: c32, aligned input and j0, and not complex taps at K = 16
    two = c32 and offset == 0 and not (pair == "CC32" and K == 16)
    return "poly_v2" if two else "poly_v1"


def fma_cases():
    """every shape with an aligned input and with one a sample past it (on the reference-order
    kernel and on c64 that changes the addresses only, not the kernel)"""
    return [pytest.param(pair, M, K, offset,
                         id=f"{pair}-M{M}-K{K}-{fma_kernel(pair, M, K, offset)}-{'offset1' if offset else 'aligned'}")
            for pair, M, K in FMA_SHAPES for offset in (0, 1)]


@pytest.mark.parametrize("pair,M,K,offset", fma_cases())
def test_fma_path_meets_the_8d_pair(pair, M, K, offset):
    """both lane shapes of the polyphase kernel where a shape has two (a 16-byte aligned c32 input
    with j0 aligned takes 16-byte vectors, an input one sample past it one sample per lane; c64
    and complex taps at K = 16 always take one sample per lane, and run with both alignments);
    each call has interior waves, edge waves at both ends and a last group shorter than seg; the
    second call starts at decimator phase 2.

    Measured on MI355X (profiles/r12/LAB.md): every c32 case stays inside 1e-6 without the
    oscillator's allowance."""
    h, s, x, ref = fma_case(pair, M, K)
    sdt = PAIRS[pair][2]
    d = sd.DDC(h, s, M, sample_dtype=sdt, algo=sd.ALGO_FMA)
    d.set_tuning(L_.TUNE_DECIM_SEG, FMA_SEG)
    d.set_phase(2.0)
    d.set_frequency(0.7)
    y1 = ddc_run(d, x[:N1], offset)
    assert d.get_state()[1] == 2
    y = np.concatenate([y1, ddc_run(d, x[N1:], offset)])
    assert len(y) == len(ref)
    what = f"{pair} M={M} K={K} {fma_kernel(pair, M, K, offset)} offset={offset}"
    check_8d(y, ref, h, s, x, sdt, what)
    check_8d(y[len(y1):], ref[len(y1):], h, s, x, sdt, what + " second call")


# ---------------------------------------------------------------- tiles beyond LDS
@pytest.mark.parametrize("pair", ["RC32", "CC64"])
def test_large_decimation_takes_the_kernel_without_a_tile(pair):
    """M = 256, L = 513: 66 rows of 256 samples do not fit the LDS tile (64 KB less the sine
    table), so ddc_global_kernel runs, EXACT, against the two handles bit for bit"""
    M, L = 256, 513
    d, h, s = make(pair, L, M)
    p = Pair(pair, h, s, M)
    d.set_nco_state(THETA0, DTHETA)
    p.nco.set_state(THETA0, DTHETA)
    lens = [0, 1, M - 1, M, L - 2, L - 1, L, 3001, 777]
    x = white_input(sum(lens), PAIRS[pair][2], 15)
    at = 0
    for n in lens:
        blk = x[at:at + n]
        at += n
        assert bits_equal(ddc_run(d, blk), p.run(blk)), (pair, n)
        assert same_state(d, p), (pair, n)


def test_large_decimation_fma():
    """the same kernel with fused multiply-adds (M = 256 is outside the polyphase rule), two calls"""
    M, L = 256, 512
    h, s = white_taps(L, F32, 61), F32(0.75)
    x = white_input(20011 + 5003, C64, 16)
    nco = O.Nco()
    nco.set_phase(2.0)
    nco.set_frequency(0.7)
    ref = O.decim(O.RC64, h.astype(F64), F64(s), M).execute_block(nco.mix_block(x.astype(C128), down=True))
    d = sd.DDC(h, s, M, sample_dtype=C64, algo=sd.ALGO_FMA)
    d.set_phase(2.0)
    d.set_frequency(0.7)
    y = np.concatenate([ddc_run(d, x[:20011]), ddc_run(d, x[20011:])])
    assert len(y) == len(ref)
    check_8d(y, ref, h, s, x, C64, "RC32 M=256 L=512 global fma")


# ---------------------------------------------------------------- every tap, every phase
@pytest.mark.parametrize("pair", ["RC32", "CC32"])
@pytest.mark.parametrize("algo", [sd.ALGO_EXACT, sd.ALGO_FMA], ids=["exact", "fma"])
def test_impulse_at_every_decimation_phase(pair, algo):
    """one impulse per decimation phase, each whole response inside the call: output m after an
    impulse at p is scale * h[j0 + m M - p] * conj(phasor(p)), so a dropped tap or a phase off by
    one shows as an error of the size of a tap, far above the bound"""
    M, K = 8, 16
    L = M * K
    _, cdt, sdt, odt, _ = PAIRS[pair]
    h, s = white_taps(L, cdt, 31), scale_of(cdt)
    n = 1000 + M * (L + 3 * M + 1) + 2 * L
    x = np.zeros(n, dtype=sdt)
    pos = [1000 + k * (L + 3 * M) + k for k in range(M)]
    assert sorted(p % M for p in pos) == list(range(M)) and pos[-1] + L < n
    x[pos] = 1.0 + 0.5j
    d = sd.DDC(h, s, M, sample_dtype=sdt, algo=algo)
    d.set_tuning(L_.TUNE_DECIM_SEG, 16)
    d.set_phase(0.5)
    d.set_frequency(1.1)
    nco = O.Nco()
    nco.set_phase(0.5)
    nco.set_frequency(1.1)
    wide = np.complex128 if np.dtype(cdt).kind == "c" else np.float64
    ref = O.decim(odt, h.astype(wide), wide(s), M).execute_block(nco.mix_block(x.astype(C128), down=True))
    y = ddc_run(d, x)
    ma = float(np.max(np.abs(y.astype(C128) - ref)))
    assert ma <= 1e-6 * float(np.sum(np.abs(h))) * abs(s) * float(np.max(np.abs(x))), ma
    assert np.count_nonzero(ref) >= L - M  # the responses do cover the taps


@pytest.mark.parametrize("pair,algo,tol", [("RC64", sd.ALGO_EXACT, 1e-13), ("RC32", sd.ALGO_FMA, 1e-6),
                                           ("CC32", sd.ALGO_EXACT, 1e-6)])
def test_tone_at_the_oscillator_frequency_becomes_dc(pair, algo, tol):
    """x[i] = the oscillator's own phasor at sample i: mixed down it is |phasor|^2 = 1, so once the
    delay line is full every output is scale * sum(h)"""
    M, K = 16, 4
    L = M * K
    _, cdt, sdt, _, _ = PAIRS[pair]
    h, s = white_taps(L, cdt, 41), scale_of(cdt)
    n = 20011
    table = np.sin(2.0 * np.pi * np.arange(1024) / 1024.0)
    theta = (np.uint64(THETA0) + np.arange(n, dtype=np.uint64) * np.uint64(DTHETA)) & np.uint64(0xFFFFFFFF)
    idx = (((theta + np.uint64(1 << 21)) >> np.uint64(22)) & np.uint64(1023)).astype(np.int64)
    x = (table[(idx + 256) & 1023] + 1j * table[idx]).astype(sdt)
    d = sd.DDC(h, s, M, sample_dtype=sdt, algo=algo)
    d.set_nco_state(THETA0, DTHETA)
    y = ddc_run(d, x)[K:]
    want = complex(s) * complex(np.sum(h.astype(np.complex128)))
    err = float(np.max(np.abs(y - want)))
    assert err <= tol * float(np.sum(np.abs(h))) * abs(s), err


# ---------------------------------------------------------------- channels
def test_three_channels_share_the_oscillator():
    M, L, n = 5, 33, 4099
    d3, h, s = make("CC32", L, M, channels=3)
    ones = [make("CC32", L, M)[0] for _ in range(3)]
    for d in [d3] + ones:
        d.set_nco_state(THETA0, DTHETA)
    x = white_input(3 * 2 * n, C64, 8).reshape(2, 3, n)
    for call in range(2):
        y = ddc_run(d3, x[call])
        for c in range(3):
            assert bits_equal(y[c], ddc_run(ones[c], x[call, c])), (call, c)
            assert d3.nco_state() == ones[c].nco_state()
    hist3, ci3 = d3.get_state()
    for c in range(3):
        hc, cc = ones[c].get_state()
        assert bits_equal(hist3[c * (L - 1):(c + 1) * (L - 1)], hc) and cc == ci3


# ---------------------------------------------------------------- life cycle
def test_clone_reset_and_state_round_trip():
    M, L = 5, 33
    d, h, s = make("RC32", L, M)
    d.set_nco_state(THETA0, DTHETA)
    x = white_input(3 * 3001, C64, 9)
    first = ddc_run(d, x[:3001])
    c = d.clone()
    assert c.nco_state() == d.nco_state() and c.get_algo() == d.get_algo()
    assert bits_equal(ddc_run(c, x[3001:6002]), ddc_run(d, x[3001:6002]))
    hist, ci = d.get_state()
    th, dt = d.nco_state()
    after = ddc_run(d, x[6002:])
    e, _, _ = make("RC32", L, M)  # a fresh handle given the saved state continues identically
    e.set_state(hist, ci)
    e.set_nco_state(th, dt)
    assert bits_equal(e.get_state()[0], hist) and e.get_state()[1] == ci
    assert bits_equal(ddc_run(e, x[6002:]), after)
    d.reset()  # as NCO.reset: phase and frequency return to zero with the delay line
    assert d.nco_state() == (0, 0) and d.get_state()[1] == 0 and not d.get_state()[0].any()
    d.set_nco_state(THETA0, DTHETA)
    assert bits_equal(ddc_run(d, x[:3001]), first)


def test_set_frequency_takes_effect_at_the_next_call():
    M, L = 2, 7
    d, h, s = make("RC64", L, M)
    p = Pair("RC64", h, s, M)
    x = white_input(2 * 2001, C128, 10)
    for k, f in enumerate((0.3, -1.7)):
        d.set_frequency(f)
        p.nco.set_frequency(f)
        d.adjust_phase(0.01)
        p.nco.adjust_phase(0.01)
        blk = x[2001 * k:2001 * (k + 1)]
        assert bits_equal(ddc_run(d, blk), p.run(blk)), k
        assert same_state(d, p)
    d.adjust_frequency(0.2)
    p.nco.adjust_frequency(0.2)
    d.set_phase(3.0)
    p.nco.set_phase(3.0)
    assert d.nco_state() == p.nco.state()


def test_host_block_equals_device_block():
    M, L = 5, 33
    x = white_input(2 * 5003, C64, 12)
    a, _, _ = make("CC32", L, M)
    b, _, _ = make("CC32", L, M)
    for d in (a, b):
        d.set_nco_state(THETA0, DTHETA)
    for k in range(2):
        blk = x[5003 * k:5003 * (k + 1)]
        assert bits_equal(a.execute_block(blk), ddc_run(b, blk))
    assert a.nco_state() == b.nco_state() and a.get_state()[1] == b.get_state()[1]
    assert len(a.execute_block(x[:0])) == 0


def test_refusals():
    d, h, s = make("RC32", 16, 4)
    buf = empty_dev(4096, C64)
    with pytest.raises(sd.SdspError) as e:  # in place
        d.execute_block_device(buf, 4096, buf, stream())
    assert e.value.code == 90 and "overlap" in str(e.value)
    with pytest.raises(sd.SdspError) as e:  # the output inside the input
        d.execute_block_device(buf, 4096, buf[1000:], stream())
    assert e.value.code == 90
    assert d.nco_state() == (0, 0) and d.get_state()[1] == 0  # a refused call moves nothing
    with pytest.raises(sd.SdspError) as e:
        d.set_algo(sd.ALGO_FFT)
    assert e.value.code == 91
    for taps, sdt in ((np.ones(8, F32), F32), (np.ones(8, F64), F64)):  # real samples: not in scope
        with pytest.raises(sd.SdspError) as e:
            sd.DDC(taps, 1.0, 2, sample_dtype=sdt)
        assert e.value.code == 90


def test_auto_switches_to_fma_at_65536_inputs():
    M, L = 8, 32
    h, s = white_taps(L, F32, 51), F32(0.75)
    x = white_input(65536, C64, 13)
    outs = {}
    for algo in (sd.ALGO_AUTO, sd.ALGO_EXACT, sd.ALGO_FMA):
        for n in (65535, 65536):
            d = sd.DDC(h, s, M, sample_dtype=C64, algo=algo)
            d.set_nco_state(THETA0, DTHETA)
            outs[algo, n] = ddc_run(d, x[:n])
    for n in (65535, 65536):
        assert not bits_equal(outs[sd.ALGO_EXACT, n], outs[sd.ALGO_FMA, n])  # the two paths do differ
    assert bits_equal(outs[sd.ALGO_AUTO, 65535], outs[sd.ALGO_EXACT, 65535])
    assert bits_equal(outs[sd.ALGO_AUTO, 65536], outs[sd.ALGO_FMA, 65536])
    d64 = sd.DDC(h.astype(F64), 0.75, M, sample_dtype=C128, algo=sd.ALGO_AUTO)  # 64-bit: always EXACT
    e64 = sd.DDC(h.astype(F64), 0.75, M, sample_dtype=C128, algo=sd.ALGO_EXACT)
    assert bits_equal(ddc_run(d64, x.astype(C128)), ddc_run(e64, x.astype(C128)))


def test_blocks_alternating_on_two_streams_run_in_call_order():
    """as tests/test_gpu_streams.py for FIR handles: a long block on s1, then short ones on the
    handle's stream, s1 and s2, queued with no host sync; each reads the delay line the one before
    wrote, so an unordered launch shows in the bits"""
    import torch
    M, L = 4, 64
    n0, n1 = 1 << 18, 4096
    x = white_input(n0 + 3 * n1, C64, 14)
    cuts = [0, n0, n0 + n1, n0 + 2 * n1, n0 + 3 * n1]
    blocks = [x[cuts[k]:cuts[k + 1]] for k in range(4)]
    ref_h, h, s = make("RC32", L, M)
    ref_h.set_nco_state(THETA0, DTHETA)
    ref = [ddc_run(ref_h, b) for b in blocks]  # one at a time, synchronised
    d, _, _ = make("RC32", L, M)
    d.set_nco_state(THETA0, DTHETA)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ins = [to_dev(b) for b in blocks]
    outs = [empty_dev(len(b) // M, C64) for b in blocks]
    torch.cuda.synchronize()
    for i, o, b, st in zip(ins, outs, blocks, [s1, None, s1, s2]):
        assert d.execute_block_device(i, len(b), o, st) == len(b) // M
    d.synchronize()
    torch.cuda.synchronize()
    for k in range(4):
        assert bits_equal(to_host(outs[k]), ref[k]), k
    assert d.nco_state() == ref_h.nco_state()
