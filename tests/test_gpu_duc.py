"""The fused digital up-converter (sd.DUC, kern_duc.hip) on MI355X.

A DUC handle is by definition the interpolating FIR followed by NCO mix-up.  On ALGO_EXACT it
must equal that composition bit for bit: the yardstick is existing code, an ALGO_EXACT
InterpolatingFIRFilter into a scratch buffer and then NCO.mix_block_device(down=False) on it, per
channel, from the same (theta, delta_theta) (and, for complex128, the CPU restatement O.interp
into O.Nco().mix_block).  On ALGO_FMA it is held to the interpolator's own bound
(tests/test_gpu_fir.py) against the f64 restatement of the same composition on the widened
input: rel-RMS <= 1e-6 for 32-bit samples, <= 1e-13 for 64-bit.

Taps are white (Kaiser taps hide dropped end taps, tests/test_gpu_fir_ols_white.py), real and
complex; the input is white.  Which kernel a shape runs on is launch_pfb's rule
(csrc/sdsp_pfb_walk.hpp pfb_route), restated in kernel_of below and named in the case ids."""
import functools

import numpy as np
import pytest

import oracle_lib as O
from gpu_util import bits_equal, rel_rms, to_dev, empty_dev, to_host

pytestmark = pytest.mark.gpu

sd = pytest.importorskip("solid_dsp_amd")

C64, C128, F32, F64 = np.complex64, np.complex128, np.float32, np.float64
# name -> (coef dtype, sample dtype, oracle dtype, oracle dtype of the f64 restatement, NCO precision)
PAIRS = {
    "RC32": (F32, C64, O.RC32, O.RC64, 0),
    "CC32": (C64, C64, O.CC32, O.CC64, 0),
    "RC64": (F64, C128, O.RC64, O.RC64, 1),
    "CC64": (C128, C128, O.CC64, O.CC64, 1),
}
THETA0, DTHETA = 0x9E3779B9, 0x0A3D70A3  # an odd-ish phase and a frequency near 0.04 cycles / sample


def white_taps(L, coef_dt, seed):
    r = np.random.default_rng(seed)
    h = r.standard_normal(L)
    if np.dtype(coef_dt).kind == "c":
        h = h + 1j * r.standard_normal(L)
    return (h / np.sqrt(L)).astype(coef_dt)


def white_input(n, sample_dt, seed):
    r = np.random.default_rng(seed)
    return (r.standard_normal(n) + 1j * r.standard_normal(n)).astype(sample_dt)


def stream():
    import torch
    return torch.cuda.current_stream()


def sub_len(L, M):
    """K as sdsp_interp_create computes it, in f32 (interp.rs:35-40)"""
    q = np.float32(L) / np.float32(M)
    return int(q) if q == np.floor(q) else int(np.ceil(q))


def kernel_of(pair, L, M, offset=0):
    """the kernel pfb_route picks for an interpolator of L taps (offset: samples the output sits
    past a 16-byte aligned allocation)"""
    sb = 8 if PAIRS[pair][1] is C64 else 16
    cb = sb if PAIRS[pair][0] in (C64, C128) else sb // 2
    K = sub_len(L, M)
    if 8 <= M <= 512 and M & (M - 1) == 0 and K in (4, 8, 16) and (offset * sb) % (2 * sb) == 0:
        return "tile"
    T = 1 if M >= 4096 else 4096 // M
    xb = ((T + K - 1) * sb + 15) // 16 * 16
    if xb <= 48 * 1024:
        return "staged_lds" if xb + M * K * cb <= 48 * 1024 else "staged_global"
    return "per_output"


def duc_run(d, x, offset=0, st=None):
    """one device call; offset = samples the output sits past a 16-byte aligned allocation"""
    n = x.shape[-1]
    M = d.interpolation()
    buf = to_dev(np.concatenate([np.ascontiguousarray(x).reshape(-1), np.zeros(1, x.dtype)]))
    out = empty_dev(offset + d.channels * n * M + 1, d.sample_dtype)
    got = d.execute_block_device(buf, n, out[offset:], st if st is not None else stream())
    assert got == n * M
    y = to_host(out)[offset:offset + d.channels * n * M]
    return y.reshape(d.channels, n * M) if d.channels > 1 else y


class Pair:
    """The two-handle composition as the parent commit has it (one channel)."""

    def __init__(self, pair, taps, M, algo=sd.ALGO_EXACT):
        _, self.sdt, _, _, self.prec = PAIRS[pair]
        self.nco = sd.NCO()
        self.itp = sd.InterpolatingFIRFilter(taps, M, sample_dtype=self.sdt, algo=algo)
        self.M = M

    def run(self, x, down=False):
        n = len(x)
        d_in = to_dev(np.concatenate([x, np.zeros(1, x.dtype)]))
        d_mid = empty_dev(n * self.M + 1, self.sdt)
        d_out = empty_dev(n * self.M + 1, self.sdt)
        self.itp.execute_block_device(d_in, n, d_mid, stream())
        self.nco.mix_block_device(d_mid, n * self.M, d_out, down=down, precision=self.prec, stream=stream())
        return to_host(d_out)[:n * self.M]


def make(pair, L, M, algo=sd.ALGO_EXACT, seed=1, channels=1):
    cdt, sdt = PAIRS[pair][:2]
    h = white_taps(L, cdt, seed)
    return sd.DUC(h, M, sample_dtype=sdt, algo=algo, channels=channels), h


# ---------------------------------------------------------------- EXACT is the composition
LENS = [0, 1, 1, 1028, 1, 1970, 0, 777]  # ragged calls that straddle tile boundaries
ALL = list(PAIRS)
# (L, M, pairs, kernel): the smallest shapes that reach every kernel
EXACT_SHAPES = [
    (32, 8, ALL, "tile"),            # T = 1024 inputs, K = 4
    (256, 32, ALL, "tile"),          # the benchmark's shape, K = 8
    (4096, 512, ALL, "tile"),        # T = 16, K = 8
    (256, 16, ALL, "tile"),          # K = 16
    (60, 16, ALL, "tile"),           # zero-padded taps, K = 4
    (10, 4, ALL, "staged_lds"),
    (9, 3, ALL, "staged_lds"),
    (5, 1, ["RC32", "CC32"], "staged_lds"),
    (6400, 64, ["CC32"], "staged_global"),
    (5, 1, ["RC64", "CC64"], "per_output"),
    (2050, 1, ["RC32", "CC32"], "per_output"),
]
EXACT_CASES = [pytest.param(pair, L, M, kern, id=f"{pair}-L{L}-M{M}-{kern}")
               for L, M, pairs, kern in EXACT_SHAPES for pair in pairs]


def check_composition(pair, L, M, offset, kern):
    assert kernel_of(pair, L, M, offset) == kern
    d, h = make(pair, L, M)
    assert d.interpolation() == M and d.subfilter_len() == sub_len(L, M)
    p = Pair(pair, h, M)
    d.set_nco_state(THETA0, DTHETA)
    p.nco.set_state(THETA0, DTHETA)
    _, sdt, odt, _, _ = PAIRS[pair]
    x = white_input(sum(LENS), sdt, 11)
    at, ys = 0, []
    for n in LENS:
        blk = x[at:at + n]
        at += n
        ys.append(duc_run(d, blk, offset))
        assert bits_equal(ys[-1], p.run(blk)), (pair, L, M, n)
        assert d.nco_state() == p.nco.state(), (pair, L, M, n)
    if sdt is C128:  # and the CPU restatement, over the whole stream
        nco = O.Nco()
        d2, _ = make(pair, L, M)
        for obj in (nco, d2):
            obj.set_phase(1.25)
            obj.set_frequency(0.3)
        assert nco.state() == d2.nco_state()
        ref = nco.mix_block(O.interp(odt, h, M).execute_block(x), down=False)
        assert bits_equal(np.concatenate([duc_run(d2, x[:1500], offset), duc_run(d2, x[1500:], offset)]), ref)
        assert nco.state() == d2.nco_state()


@pytest.mark.parametrize("pair,L,M,kern", EXACT_CASES)
def test_exact_is_the_two_handle_composition(pair, L, M, kern):
    check_composition(pair, L, M, 0, kern)


@pytest.mark.parametrize("pair", ALL)
def test_misaligned_output_takes_the_staged_kernel(pair):
    """a tile shape whose output starts one sample past a 16-byte boundary (for 64-bit samples:
    past a 32-byte one) cannot take the tile kernel's paired stores"""
    check_composition(pair, 256, 32, 1, "staged_lds")


# ---------------------------------------------------------------- oscillator wrap, direction
@pytest.mark.parametrize("M", [8, 3])
@pytest.mark.parametrize("pair", ["RC32", "CC64"])
def test_oscillator_wraps_inside_and_between_calls(pair, M):
    """theta near 2^32 and a delta_theta for which (u32) o * dtheta wraps thousands of times in a
    call and n * M * delta_theta wraps between calls; delta_theta = 0 is a constant phase"""
    L, n = 4 * M, 601
    sdt = PAIRS[pair][1]
    x = white_input(3 * n, sdt, 5)
    for theta, dtheta in ((0xFFFFFF00, 0xC0000001), (0xFFFFFFFF, 0x7FFFFFFF), (0x40000000, 0)):
        d, h = make(pair, L, M)
        p = Pair(pair, h, M)
        d.set_nco_state(theta, dtheta)
        p.nco.set_state(theta, dtheta)
        for k in range(3):
            blk = x[n * k:n * (k + 1)]
            assert bits_equal(duc_run(d, blk), p.run(blk)), (theta, dtheta, k)
            assert d.nco_state() == p.nco.state()
        assert d.nco_state() == ((theta + 3 * n * M * dtheta) & 0xFFFFFFFF, dtheta)
    # a constant phase is one complex factor behind the plain interpolator
    d, h = make(pair, L, M)
    d.set_nco_state(0x40000000, 0)  # a quarter turn: the phasor is (0, 1), mix_up multiplies by j
    itp = sd.InterpolatingFIRFilter(h, M, sample_dtype=sdt, algo=sd.ALGO_EXACT)
    y = duc_run(d, x[:n])
    ref = itp.execute_block(x[:n]).astype(C128) * 1j
    assert rel_rms(y, ref) <= (1e-6 if sdt is C64 else 1e-13)


@pytest.mark.parametrize("pair", ["CC32", "RC64"])
def test_direction_down_is_mix_down(pair):
    L, M = 32, 8
    d, h = make(pair, L, M)
    p = Pair(pair, h, M)
    d.set_direction(True)
    d.set_nco_state(THETA0, DTHETA)
    p.nco.set_state(THETA0, DTHETA)
    x = white_input(1501, PAIRS[pair][1], 6)
    down = duc_run(d, x)
    assert bits_equal(down, p.run(x, down=True))
    d.set_direction(False)
    d.reset()
    d.set_nco_state(THETA0, DTHETA)
    assert not bits_equal(duc_run(d, x), down)


def test_oscillator_setters_are_the_ncos():
    L, M = 9, 3
    d, h = make("RC64", L, M)
    p = Pair("RC64", h, M)
    x = white_input(2 * 701, C128, 10)
    for k, f in enumerate((0.3, -1.7)):
        d.set_frequency(f)
        p.nco.set_frequency(f)
        d.adjust_phase(0.01)
        p.nco.adjust_phase(0.01)
        assert d.nco_state() == p.nco.state()
        blk = x[701 * k:701 * (k + 1)]
        assert bits_equal(duc_run(d, blk), p.run(blk)), k  # the setter acts at the next call's first output
        assert d.nco_state() == p.nco.state()
    d.adjust_frequency(0.2)
    p.nco.adjust_frequency(0.2)
    d.set_phase(3.0)
    p.nco.set_phase(3.0)
    assert d.nco_state() == p.nco.state()


# ---------------------------------------------------------------- channels and state
@pytest.mark.parametrize("L,M", [(32, 8), (9, 3)])
def test_three_channels_share_the_oscillator(L, M):
    n = 1100
    d3, h = make("CC32", L, M, channels=3)
    pairs = [Pair("CC32", h, M) for _ in range(3)]
    d3.set_nco_state(THETA0, DTHETA)
    for p in pairs:
        p.nco.set_state(THETA0, DTHETA)
    x = white_input(2 * 3 * n, C64, 8).reshape(2, 3, n)
    for call in range(2):
        y = duc_run(d3, x[call])
        for c in range(3):
            assert bits_equal(y[c], pairs[c].run(x[call, c])), (call, c)
            assert d3.nco_state() == pairs[c].nco.state()


def test_clone_reset_and_set_channels():
    L, M, n = 32, 8, 1101
    d, h = make("RC32", L, M)
    d.set_direction(True)
    d.set_nco_state(THETA0, DTHETA)
    x = white_input(3 * n, C64, 9)
    first = duc_run(d, x[:n])
    c = d.clone()
    assert c.nco_state() == d.nco_state() and c.get_algo() == d.get_algo()
    assert c.interpolation() == M and c.subfilter_len() == 4
    assert bits_equal(duc_run(c, x[n:2 * n]), duc_run(d, x[n:2 * n]))  # window, direction, oscillator
    d.reset()  # as NCO.reset: phase and frequency return to zero with the window
    assert d.nco_state() == (0, 0)
    d.set_nco_state(THETA0, DTHETA)
    assert bits_equal(duc_run(d, x[:n]), first)
    d.set_channels(1)  # zeroes the windows, leaves the oscillator
    th = d.nco_state()
    f, _ = make("RC32", L, M)
    f.set_direction(True)
    f.set_nco_state(*th)
    assert bits_equal(duc_run(d, x[2 * n:]), duc_run(f, x[2 * n:]))


def test_host_block_equals_device_block():
    L, M, n = 256, 32, 1103
    x = white_input(2 * n, C64, 12)
    a, _ = make("CC32", L, M)
    b, _ = make("CC32", L, M)
    for d in (a, b):
        d.set_nco_state(THETA0, DTHETA)
    for k in range(2):
        blk = x[n * k:n * (k + 1)]
        assert bits_equal(a.execute_block(blk), duc_run(b, blk))
    assert a.nco_state() == b.nco_state()
    assert len(a.execute_block(x[:0])) == 0 and a.nco_state() == b.nco_state()


def test_refusals():
    d, h = make("RC32", 32, 8)
    buf = empty_dev(8 * 512, C64)
    with pytest.raises(sd.SdspError) as e:  # in place
        d.execute_block_device(buf, 512, buf, stream())
    assert e.value.code == 90 and "overlap" in str(e.value)
    with pytest.raises(sd.SdspError) as e:  # the input inside the output
        d.execute_block_device(buf[1000:], 300, buf, stream())
    assert e.value.code == 90
    assert d.nco_state() == (0, 0)  # a refused call moves nothing
    for algo in (sd.ALGO_AUTO, sd.ALGO_FFT):
        with pytest.raises(sd.SdspError) as e:
            d.set_algo(algo)
        assert e.value.code == 90
    assert d.get_algo() == sd.ALGO_EXACT
    for taps, sdt in ((np.ones(8, F32), F32), (np.ones(8, F64), F64)):  # real samples
        with pytest.raises(sd.SdspError) as e:
            sd.DUC(taps, 2, sample_dtype=sdt)
        assert e.value.code == 90


def test_blocks_alternating_on_two_streams_run_in_call_order():
    """as tests/test_gpu_ddc.py: a long block on s1, then short ones on the handle's stream, s1
    and s2, queued with no host sync; each reads the window the one before wrote, so an
    unordered launch shows in the bits"""
    import torch
    L, M = 64, 4
    n0, n1 = 1 << 17, 1024
    x = white_input(n0 + 3 * n1, C64, 14)
    cuts = [0, n0, n0 + n1, n0 + 2 * n1, n0 + 3 * n1]
    blocks = [x[cuts[k]:cuts[k + 1]] for k in range(4)]
    ref_h, h = make("RC32", L, M)
    ref_h.set_nco_state(THETA0, DTHETA)
    ref = [duc_run(ref_h, b) for b in blocks]  # one at a time, synchronised
    d, _ = make("RC32", L, M)
    d.set_nco_state(THETA0, DTHETA)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ins = [to_dev(b) for b in blocks]
    outs = [empty_dev(len(b) * M, C64) for b in blocks]
    torch.cuda.synchronize()
    for i, o, b, st in zip(ins, outs, blocks, [s1, None, s1, s2]):
        assert d.execute_block_device(i, len(b), o, st) == len(b) * M
    d.synchronize()
    torch.cuda.synchronize()
    for k in range(4):
        assert bits_equal(to_host(outs[k]), ref[k]), k
    assert d.nco_state() == ref_h.nco_state()


# ---------------------------------------------------------------- FMA path
N1, N2, CH = 1028, 777, 2  # two calls, the first ends inside a tile; two channels
# (pair, L, M): both tile lane cases (real and complex taps) at K = 4, 8, 16 and M = 8, 32, the
# largest 64-bit tile instance, one staged and one per-output shape per precision
FMA_SHAPES = ([(pair, K * M, M) for pair in ("RC32", "CC32") for M in (8, 32) for K in (4, 8, 16)] +
              [("RC64", 32, 8), ("RC64", 256, 32), ("CC64", 128, 8), ("CC64", 512, 32),
               ("RC32", 10, 4), ("CC32", 9, 3), ("CC64", 10, 4), ("CC32", 2050, 1), ("RC64", 5, 1)])
WORST = {}  # kernel -> worst rel-RMS seen so far in this run, per precision


@functools.lru_cache(maxsize=None)
def fma_case(pair, L, M):
    """taps, input and the f64 restatement of the composition per channel, computed once per shape"""
    cdt, sdt, _, odt, _ = PAIRS[pair]
    h = white_taps(L, cdt, 100 + L + M)
    x = white_input(CH * (N1 + N2), sdt, 200 + M).reshape(CH, N1 + N2)
    wide = C128 if np.dtype(cdt).kind == "c" else F64
    refs = []
    for c in range(CH):
        nco = O.Nco()
        nco.set_phase(2.0)
        nco.set_frequency(0.7)
        refs.append(nco.mix_block(O.interp(odt, h.astype(wide), M).execute_block(x[c].astype(C128)), down=False))
    ref = np.stack(refs)
    for a in (h, x, ref):
        a.setflags(write=False)
    return h, x, ref


@pytest.mark.parametrize("pair,L,M", [pytest.param(p, L, M, id=f"{p}-L{L}-M{M}-{kernel_of(p, L, M)}")
                                      for p, L, M in FMA_SHAPES])
def test_fma_path_meets_the_interpolators_bound(pair, L, M):
    """ALGO_FMA against the f64 restatement, per channel: rel-RMS <= 1e-6 (c32) / 1e-13 (c64).
    Should a c32 case exceed 1e-6 the f32 sine table may be the cause and not the kernel: the
    unfused FMA pair is then measured against the same restatement and 1.5 times its figure is
    allowed for that case.

    Measured on MI355X (profiles/r13/LAB.md): no case needed the allowance."""
    h, x, ref = fma_case(pair, L, M)
    sdt = PAIRS[pair][1]
    d = sd.DUC(h, M, sample_dtype=sdt, algo=sd.ALGO_FMA, channels=CH)
    d.set_phase(2.0)
    d.set_frequency(0.7)
    y = np.concatenate([duc_run(d, x[:, :N1]), duc_run(d, x[:, N1:])], axis=1)
    assert y.shape == ref.shape
    kern = kernel_of(pair, L, M)
    same = True
    for c in range(CH):
        p = Pair(pair, h, M, algo=sd.ALGO_FMA)
        p.nco.set_phase(2.0)
        p.nco.set_frequency(0.7)
        yp = np.concatenate([p.run(x[c, :N1]), p.run(x[c, N1:])])
        same = same and bits_equal(y[c], yp)
        rr, rp = rel_rms(y[c], ref[c]), rel_rms(yp, ref[c])
        key = (kern, "c32" if sdt is C64 else "c64")
        WORST[key] = max(WORST.get(key, 0.0), rr)
        print(f"{pair} L={L} M={M} {kern} channel {c}: fused rel-RMS {rr:.3e}, unfused FMA pair {rp:.3e}; "
              f"worst on {key[0]} {key[1]} so far {WORST[key]:.3e}")
        if sdt is C64:
            assert rr <= 1e-6 or rr <= 1.5 * rp, (pair, L, M, c, rr, rp)
        else:
            assert rr <= 1e-13, (pair, L, M, c, rr)
    print(f"{pair} L={L} M={M} {kern}: fused FMA output bit-identical to the unfused FMA pair: {same}")
