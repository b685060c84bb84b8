"""Every overlap-save kernel against its reference on inputs that weigh every tap and every bin:
white taps, single-bin streams and impulses.

The other overlap-save files filter noise with firdes_kaiser(L, 0.1, 80, 0) taps.  That design has
no weight at either end of the tap vector (deleting the oldest or the newest tap of 3842 moves
the output by 3e-7), it is symmetric (the reversed taps give the same output) and 80 % of its
bins sit 80 dB down.  test_what_the_inputs_see shows this on the CPU, and that white taps see all
three.  Here:

- white taps: default_rng(seed).standard_normal(L) as f32 (CC32: an independent imaginary part,
  as complex64), scale 0.2 on RR32 / RC32 and 0.2 - 0.15j on CC32;
- white streams from O.synth;
- single-bin streams exp(2 pi i ((k n) mod N) / N) as complex64 (RR32: cos(...), N = 4096) on a
  fresh handle.  The rounding error of a transform is relative to its whole spectrum and the
  output of a single bin to |G[k]|, G = fft(scale h[::-1], N): the tap seed is the first, counting
  up from BIN_SEED, whose taps have |G[k]| >= 0.5 rms|G| at every named bin (asserted and printed);
- impulse streams: one sample of 1 at p, zeros elsewhere, p + L <= n (asserted): the whole
  response lies inside the call.  (With the impulse on the last sample the error of a whole
  segment would be set against one output: 3.7e-6 for exact float32 arithmetic.)

References: the complex128 FFT convolution fft_conv of test_gpu_fir_ols_long.py on the long path
(pinned here once more to O.fir(O.CC64, ...) with complex white taps and the complex scale), the
f64 restatement O.fir(O.RR64 / O.CC64, ...) on the 4096-point paths.
Tolerance: the section 8d pair everywhere,
    rel_RMS <= 1e-6   and   max|err| <= 1e-6 * sum|h| * |scale| * max|x|.
"""
import functools

import numpy as np
import pytest

import oracle_lib as O
from gpu_util import bits_equal, rel_rms

gpu = pytest.mark.gpu

sd = pytest.importorskip("solid_dsp_amd")
from solid_dsp_amd import FIRFilter as _FIRFilter  # noqa: E402

F32, F64, C64, C128 = np.float32, np.float64, np.complex64, np.complex128
SCALE, SCALE_C = 0.2, 0.2 - 0.15j
SEED = 20251117      # streams
TAP_SEED = 20251118  # white taps of the white-stream and impulse cases
BIN_SEED = 20251119  # single-bin cases: the search for a tap seed starts here
TUNE_OLS_KERNEL, TUNE_LOG2N, TUNE_SEGS = 14, 22, 23
L0 = 3842            # the shortest filter of the long path
TAIL = 1234


def FIRFilter(*a, **k):
    k.setdefault("host_step", False)
    return _FIRFilter(*a, **k)


@functools.lru_cache(maxsize=None)
def white_taps(L, cplx=False, seed=TAP_SEED):
    rng = np.random.default_rng(seed)
    h = rng.standard_normal(L).astype(F32)
    if cplx:
        h = (h + 1j * rng.standard_normal(L).astype(F32)).astype(C64)
    h.setflags(write=False)
    return h


@functools.lru_cache(maxsize=8)
def stream(ch, n, cplx=True):
    x = O.synth(SEED, ch, 0, n, complex_=cplx)
    x.setflags(write=False)
    return x


def scale_of(cplx):
    return SCALE_C if cplx else SCALE


def fft_conv(h, scale, x):
    """y[j] = scale * sum_i h[L-1-i] x[j-i] (the stored taps are the reversed ones), x[<0] = 0,
    by a complex128 FFT convolution"""
    n, L = len(x), len(h)
    M = 1 << int(n + L - 1).bit_length()
    g = np.asarray(h)[::-1].astype(C128) * complex(scale)
    return np.fft.ifft(np.fft.fft(np.asarray(x).astype(C128), M) * np.fft.fft(g, M))[:n]


def check_8d(y, ref, h, scale, x, what):
    rel = rel_rms(y, ref)
    err = float(np.abs(np.asarray(y).astype(C128) - ref).max())
    bound = 1e-6 * float(np.abs(np.asarray(h).astype(C128)).sum()) * abs(scale) * float(np.abs(x).max())
    print(f"{what}: rel-RMS {rel:.3e}, max|err| {err:.3e} (bound {bound:.3e}, {err / bound:.1e} of it)")
    assert rel <= 1e-6, f"{what}: rel-RMS {rel:.3e} > 1e-6"
    assert err <= bound, f"{what}: max|err| {err:.3e} > {bound:.3e} (rel-RMS {rel:.3e})"
    return rel


def history_after(x, b, L):
    """the last L - 1 inputs before position b of every channel, zeros before the stream"""
    x2 = np.asarray(x).reshape(-1, np.asarray(x).shape[-1])
    want = np.zeros((x2.shape[0], L - 1), dtype=x2.dtype)
    k = min(b, L - 1)
    if k:
        want[:, L - 1 - k:] = x2[:, b - k:b]
    return want.reshape(-1)


# ---------------------------------------------------------------- the two conditions
def bin_gains(h, scale, N, bins):
    """(|G[k]| for k in bins, rms|G|) of G = fft(scale * h[::-1], N); the rms by Parseval"""
    g = np.asarray(h)[::-1].astype(C128) * complex(scale)
    i = np.arange(len(g))
    gains = np.array([abs(np.sum(g * np.exp(-2j * np.pi * ((k * i) % N) / N))) for k in bins])
    return gains, float(np.sqrt(np.sum(np.abs(g) ** 2)))


def bins_carry_weight(h, scale, N, bins):
    gains, rms = bin_gains(h, scale, N, bins)
    return bool(np.all(gains >= 0.5 * rms))


@functools.lru_cache(maxsize=None)
def bin_seed(L, cplx, N, bins):
    """the first seed from BIN_SEED whose white taps carry weight at every bin of `bins`"""
    for seed in range(BIN_SEED, BIN_SEED + 4096):
        if bins_carry_weight(white_taps(L, cplx, seed), scale_of(cplx), N, bins):
            return seed
    raise AssertionError("no tap seed found")


def tone(k, N, n, real=False):
    ph = 2.0 * np.pi * ((k * np.arange(n, dtype=np.int64)) % N) / N
    x = np.cos(ph).astype(F32) if real else np.exp(1j * ph).astype(C64)
    x.setflags(write=False)
    return x


def impulse(p, n, L, dtype=C64):
    assert 0 <= p and p + L <= n, f"impulse at {p}: its response leaves the call of {n} samples"
    x = np.zeros(n, dtype=dtype)
    x[p] = 1
    return x


# ---------------------------------------------------------------- 1. what the new inputs see (CPU)
def rejected(y, ref, h, scale, x, what):
    try:
        check_8d(y, ref, h, scale, x, what)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("L", [L0, 257])
def test_what_the_inputs_see(L):
    """three wrong filters in complex128 (the oldest tap zeroed, the newest tap zeroed, the taps
    reversed) against the right one, under the section 8d pair: white taps reject all three;
    Kaiser taps accept the reversal, and at L = 3842 both deletions (at L = 257 a deleted end tap
    of the Kaiser design is near the bound, and nothing is asserted about it)"""
    x = stream(9, 20000)
    kaiser = O.firdes_kaiser(L, 0.1, 80.0, 0.0).astype(F32)

    def mutations(h):
        old, new = h.copy(), h.copy()
        old[0] = 0    # the stored taps are reversed: h[0] multiplies x[j - (L-1)]
        new[-1] = 0
        return {"oldest tap zeroed": old, "newest tap zeroed": new, "taps reversed": h[::-1].copy()}

    for kind, h, scale in (("kaiser", kaiser, SCALE), ("white", white_taps(L), SCALE),
                           ("white complex", white_taps(L, True), SCALE_C)):
        ref = fft_conv(h, scale, x)
        for name, hm in mutations(h).items():
            bad = rejected(fft_conv(hm, scale, x), ref, h, scale, x, f"L={L} {kind} taps, {name}")
            if kind != "kaiser":
                assert bad, f"L={L}: {kind} taps accept '{name}'"
            elif name == "taps reversed" or L == L0:
                assert not bad, f"L={L}: kaiser taps reject '{name}'"


def test_fft_reference_matches_restatement_white():
    """fft_conv against O.fir(O.CC64, ...) with complex white taps and the complex scale, and
    against O.fir(O.RC64, ...) with real ones: n = 3000, L = 300"""
    x = stream(0, 3000)
    for cplx, dt, cdt in ((True, O.CC64, C128), (False, O.RC64, F64)):
        h, s = white_taps(300, cplx), scale_of(cplx)
        ref = O.fir(dt, h.astype(cdt), s).execute_block(x.astype(C128))
        rel = rel_rms(fft_conv(h, s, x), ref)
        print(f"{'CC64' if cplx else 'RC64'} L=300 white taps: rel-RMS {rel:.3e}")
        assert rel <= 1e-12


# ================================================================ 2. the long path
def long_geom(lg):
    """(N1, N2, C, R) of launch_fir_ols_long: N = N1 N2, C columns per P1 / P3 workgroup, R rows
    per P2 workgroup"""
    N1 = 1 << (lg // 2)
    N2 = (1 << lg) // N1
    C = 16 if N1 <= 256 else 8 if N1 <= 1024 else 4
    R = max(1, min(2048 // N2, 8))
    return N1, N2, C, R


def ols_long(h, cplx, lg=0, **k):
    f = FIRFilter(h, (C64 if cplx else F32)(scale_of(cplx)), sample_dtype=C64, algo=sd.ALGO_FFT, **k)
    if lg:
        f.set_tuning(TUNE_LOG2N, lg)
    return f


def test_long_geometry_of_the_untested_shapes():
    """what the issue names: N1 = 512 at log2 N = 18, 19 (8 columns per workgroup), N2 = 512 at 17, 18
    (4 rows per workgroup), 1024 x 2048 at 21"""
    assert [long_geom(lg)[0] for lg in (18, 19)] == [512, 512] and long_geom(18)[2] == long_geom(19)[2] == 8
    assert [long_geom(lg)[1] for lg in (17, 18)] == [512, 512] and long_geom(17)[3] == long_geom(18)[3] == 4
    assert long_geom(21)[:2] == (1024, 2048)
    assert long_geom(13) == (64, 128, 16, 8) and long_geom(22) == (2048, 2048, 4, 1)


@gpu
@pytest.mark.parametrize("lg,cplx", [(lg, False) for lg in range(13, 23)] + [(lg, True) for lg in (13, 14, 17, 18, 19, 21)])
def test_ols_long_every_factor_shape(lg, cplx):
    """white taps (L = 3842) and a white stream on one call of 2 V + V / 2 samples at every
    N = 2^13 .. 2^22 (RC32; CC32 with the complex scale at six of them): every output against
    fft_conv, and the history"""
    h, s = white_taps(L0, cplx), scale_of(cplx)
    f = ols_long(h, cplx, lg)
    N, V = f.ols_info()
    assert (N, V) == (1 << lg, (1 << lg) - (L0 - 1))
    n = 2 * V + V // 2
    x = stream(1, n)
    y = f.execute_block(x)
    hist, _ = f.get_state()
    assert bits_equal(hist, x[n - (L0 - 1):])
    check_8d(y, fft_conv(h, s, x), h, s, x, f"long {'CC32' if cplx else 'RC32'} N=2^{lg} white")


def named_bins(lg):
    N1, N2, C, R = long_geom(lg)
    N = N1 * N2
    return tuple(dict.fromkeys([0, 1, N1 - 1, N1, N // 2, N // 2 + N1 - 1, N - N1, N - 1, R - 1, R, N1 * (N2 - 1) + R]))


@gpu
@pytest.mark.parametrize("lg", [13, 17, 19])
def test_ols_long_named_bins(lg):
    """single-bin streams on RC32 handles (real white taps): with k = k1 + N1 k2 the corners of the
    [k1][k2] spectrum, Nyquist, the last row of one P2 workgroup and the first of the next
    (k = R - 1, R) and a bin of the last column; a call of 2 V + 1234 samples each"""
    bins = named_bins(lg)
    N = 1 << lg
    seed = bin_seed(L0, False, N, bins)
    h = white_taps(L0, False, seed)
    gains, rms = bin_gains(h, SCALE, N, bins)
    print(f"N=2^{lg}: tap seed {seed} (BIN_SEED + {seed - BIN_SEED}), min |G[k]| / rms|G| = {gains.min() / rms:.3f}")
    assert np.all(gains >= 0.5 * rms)
    V = N - (L0 - 1)
    n = 2 * V + TAIL
    for k in bins:
        x = tone(k, N, n)
        y = ols_long(h, False, lg).execute_block(x)
        check_8d(y, fft_conv(h, SCALE, x), h, SCALE, x, f"long RC32 N=2^{lg} bin {k}")


def named_positions(lg):
    """impulse positions by what they hit in the window w[i] = x[V - (L-1) + i], i = n2 + N2 n1, of
    segment 1"""
    N1, N2, C, R = long_geom(lg)
    N = N1 * N2
    V = N - (L0 - 1)
    at = lambda i: V - (L0 - 1) + i  # noqa: E731
    return {"n2 = C - 1 (n1 = N1 / 2)": at(C - 1 + N2 * (N1 // 2)), "n2 = C (n1 = N1 / 2)": at(C + N2 * (N1 // 2)),
            "window index 0": at(0), "window index N - 1": at(N - 1), "p = 0": 0, "p = V - 1": V - 1, "p = V": V}


@gpu
@pytest.mark.parametrize("lg", [13, 17, 19])
def test_ols_long_named_positions(lg):
    """impulses on CC32 handles (complex white taps, the complex scale): the output is the taps
    themselves, in order, at the impulse.  A call of 3 V + 1234 samples (2 V + 1234 would cut the
    response of the window's newest sample, p = 2 V - 1)"""
    h = white_taps(L0, True)
    V = (1 << lg) - (L0 - 1)
    n = 3 * V + TAIL
    pos = named_positions(lg)
    assert pos["window index 0"] == V - (L0 - 1) and pos["window index N - 1"] == 2 * V - 1
    for name, p in pos.items():
        x = impulse(p, n, L0)
        y = ols_long(h, True, lg).execute_block(x)
        check_8d(y, fft_conv(h, SCALE_C, x), h, SCALE_C, x, f"long CC32 N=2^{lg} impulse at {p} ({name})")


@gpu
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("L", [4097, 5000])
def test_ols_long_far_end_history(L, cplx):
    """L = 4097 (4 (L-1) = 2^14 exactly) and 5000, white taps: calls of 1, L - 2, L - 1, L, V and
    V + 1 samples; the history after every call (short calls keep older samples), the
    concatenated output against fft_conv: every call's first outputs read the oldest history
    sample through the oldest tap"""
    h, s = white_taps(L, cplx), scale_of(cplx)
    f = ols_long(h, cplx)
    _, V = f.ols_info()
    cuts = np.cumsum([0, 1, L - 2, L - 1, L, V, V + 1]).tolist()
    n = cuts[-1]
    x = stream(2, n)
    y = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        y.append(f.execute_block(x[a:b]))
        hist, _ = f.get_state()
        assert bits_equal(hist, history_after(x, b, L)), (a, b)
    check_8d(np.concatenate(y), fft_conv(h, s, x), h, s, x, f"long {'CC32' if cplx else 'RC32'} L={L} six calls")


@gpu
def test_ols_long_rounds_across_channels():
    """N = 2^13, three channels of 2 V + 17 samples (three segments each, nine in all): rounds of
    2 and of 4 segments straddle the channel boundaries at segments 3 and 6.  The bits of a handle
    with automatic rounds and of three one-channel handles; section 8d per channel"""
    h = white_taps(L0)
    V = (1 << 13) - (L0 - 1)
    n = 2 * V + 17
    assert -(-n // V) == 3
    x = np.stack([stream(3 + c, n) for c in range(3)])
    auto = ols_long(h, False, 13, channels=3).execute_block(x)
    for segs in (2, 4):
        f = ols_long(h, False, 13, channels=3)
        f.set_tuning(TUNE_SEGS, segs)
        y = f.execute_block(x)
        assert bits_equal(y, auto), f"rounds of {segs} differ from automatic rounds"
        hist, _ = f.get_state()
        assert bits_equal(hist, history_after(x, n, L0))
    for c in range(3):
        y1 = ols_long(h, False, 13).execute_block(x[c])
        assert bits_equal(auto[c], y1), f"channel {c} of 3 differs from a one-channel handle"
        check_8d(auto[c], fft_conv(h, SCALE, x[c]), h, SCALE, x[c], f"long RC32 N=2^13 channel {c} of 3")


# ================================================================ 3. the real pair kernel
LANES = [0, 3]  # SDSP_TUNE_OLS_KERNEL on an RR32 handle: 4-byte lanes, 8-byte lanes


def advance(L):
    return 4096 - 256 * (-(-(L - 1) // 256))


def real_pairs(n, L):
    """(segments, first interior pair, end of the interior pairs) of one RR32 call, restated: pair p
    holds segments 2p and 2p + 1, it is interior when both windows lie inside the call, and the
    call's last pair never is"""
    V = advance(L)
    H = 4096 - V
    nseg = -(-n // V)
    npair = (nseg + 1) // 2
    inside = [p for p in range(npair - 1) if 2 * p * V - H >= 0 and (2 * p + 1) * V - H + 4096 <= n]
    return nseg, (inside[0] if inside else 0), (inside[-1] + 1 if inside else 0)


def real_cuts(L):
    """an odd block (2 plo + 5 segments), an even one (2 plo + 6) and a ragged tail; every call length
    is odd"""
    V = advance(L)
    plo = -(-(4096 - V) // (2 * V))
    t1, t2 = (1235, 777) if V > 1235 else (V // 2 + 1, V // 4 + 1)
    lens = [(2 * plo + 4) * V + t1, (2 * plo + 5) * V + t2, 1235]
    for m, nseg in zip(lens[:2], (2 * plo + 5, 2 * plo + 6)):
        got, lo, hi = real_pairs(m, L)
        assert got == nseg and lo == plo and hi - lo >= 2, (L, m, got, lo, hi)
    assert all(m % 2 for m in lens)
    return np.cumsum([0] + lens).tolist()


def ols_real(h, kern, **k):
    f = FIRFilter(h, F32(SCALE), sample_dtype=F32, algo=sd.ALGO_FFT, **k)
    f.set_tuning(TUNE_OLS_KERNEL, kern)
    return f


def restate_real(h, x):
    return O.fir(O.RR64, np.asarray(h).astype(F64), SCALE).execute_block(np.asarray(x).astype(F64))


@functools.lru_cache(maxsize=None)
def real_white_case(L, ch):
    n = real_cuts(L)[-1]
    x = np.stack([stream(10 + c, n, False) for c in range(ch)])
    ref = np.stack([restate_real(white_taps(L), x[c]) for c in range(ch)])
    x.setflags(write=False)
    ref.setflags(write=False)
    return x, ref


@gpu
@pytest.mark.parametrize("kern", LANES)
@pytest.mark.parametrize("L,ch", [(2, 1), (256, 1), (257, 1), (700, 1), (3841, 1), (700, 3)])
def test_ols_real_white(L, ch, kern):
    """white real taps and streams, h2 = 1, 1, 2, 3, 15: a call with an odd and one with an even
    segment count (two interior pairs each; in the odd one the last pair has no B) and a ragged
    tail; the history after every call.  With three channels the odd call lengths put the
    channel bases at odd float offsets"""
    h = white_taps(L)
    cuts = real_cuts(L)
    x, ref = real_white_case(L, ch)
    xs = x if ch > 1 else x[0]
    f = ols_real(h, kern, channels=ch)
    y = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        y.append(f.execute_block(xs[..., a:b]))
        hist, _ = f.get_state()
        assert bits_equal(hist, history_after(xs, b, L)), (a, b)
    y = np.concatenate(y, axis=-1).reshape(ch, -1)
    for c in range(ch):
        check_8d(y[c], ref[c], h, SCALE, x[c], f"real L={L} kern={kern} ch={c}/{ch} white")


REAL_BINS = (0, 1, 16, 128, 273, 2047, 2048)


@functools.lru_cache(maxsize=None)
def real_tone_case(L, k):
    n = real_cuts(L)[1]
    x = tone(k, 4096, n, real=True)
    ref = restate_real(white_taps(L, False, bin_seed(L, False, 4096, REAL_BINS)), x)
    ref.setflags(write=False)
    return x, ref


@gpu
@pytest.mark.parametrize("kern", LANES)
@pytest.mark.parametrize("L", [256, 700])
def test_ols_real_tones(L, kern):
    """real tones cos(2 pi k n / 4096) at DC, 1, 16, 128, 273, 2047 and Nyquist on one call with two
    interior pairs"""
    seed = bin_seed(L, False, 4096, REAL_BINS)
    h = white_taps(L, False, seed)
    gains, rms = bin_gains(h, SCALE, 4096, REAL_BINS)
    print(f"real L={L}: tap seed {seed} (BIN_SEED + {seed - BIN_SEED}), min |G[k]| / rms|G| = {gains.min() / rms:.3f}")
    assert np.all(gains >= 0.5 * rms)
    for k in REAL_BINS:
        x, ref = real_tone_case(L, k)
        y = ols_real(h, kern).execute_block(x)
        check_8d(y, ref, h, SCALE, x, f"real L={L} kern={kern} bin {k}")


@functools.lru_cache(maxsize=None)
def real_gated_case(L, loud):
    """white noise on the output spans [s V, (s + 1) V) of the segments with s % 2 == loud, exact
    zeros on the others"""
    V = advance(L)
    n = real_cuts(L)[1]
    x = stream(14, n, False).copy()
    x[(np.arange(n) // V) % 2 != loud] = 0
    ref = restate_real(white_taps(L), x)
    x.setflags(write=False)
    ref.setflags(write=False)
    return x, ref


@gpu
@pytest.mark.parametrize("kern", LANES)
@pytest.mark.parametrize("loud", [0, 1])
@pytest.mark.parametrize("L", [256, 700])
def test_ols_real_silent_segment_beside_a_loud_one(L, loud, kern):
    """A = 2p and B = 2p + 1 share one transform as A + i B.  One of them carries white noise, the
    other exact zeros (then the complement).  Section 8d over the call; and where the reference is
    exactly zero (the silent segment past the loud one's reach), |y| is within the max-error
    bound: the silent segment's error is relative to its pair (kern_fir_ols_real.hip), and
    nothing of the loud segment lands in it"""
    h = white_taps(L)
    x, ref = real_gated_case(L, loud)
    y = ols_real(h, kern).execute_block(x)
    what = f"real L={L} kern={kern} loud {'even' if loud == 0 else 'odd'} segments"
    check_8d(y, ref, h, SCALE, x, what)
    zero = ref == 0
    assert zero.sum() > len(x) // 4
    bound = 1e-6 * float(np.abs(h.astype(F64)).sum()) * SCALE * float(np.abs(x).max())
    worst = float(np.abs(y[zero]).max())
    print(f"{what}: max|y| over {int(zero.sum())} outputs whose reference is 0: {worst:.3e} ({worst / bound:.1e} of the bound)")
    assert worst <= bound


# ================================================================ 4. the 4096-point c32 kernels
KERNELS = [0, 1, 2, 3]  # one-shot, persistent packed (h2 <= 4; else scalar) + edge, scalar, one-shot wide


def c32_interior(n, L):
    """interior segments of one c32 call (ols_interior_range, restated): window and outputs inside"""
    V = advance(L)
    H = 4096 - V
    return sum(1 for s in range(-(-n // V)) if s * V - H >= 0 and s * V - H + 4096 <= n)


@functools.lru_cache(maxsize=None)
def c32_case(L):
    n = 37 * advance(L) + TAIL + 3001
    x = stream(15, n)
    ref = O.fir(O.CC64, white_taps(L, True).astype(C128), SCALE_C).execute_block(x.astype(C128))
    ref.setflags(write=False)
    return x, ref


@gpu
@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("L", [256, 257, 1025, 3841])
def test_ols_c32_complex_white(L, kern):
    """complex white taps and the complex scale on every setting of SDSP_TUNE_OLS_KERNEL, h2 = 1, 2,
    5, 15 (at h2 = 5 and 15 setting 1 runs the scalar kernel): one call of 37 V + 1234 samples from
    a host array (the staged device rows are 16-byte aligned), then 3001 samples on the same
    handle.  The first call holds 36 interior segments (26 at h2 = 15, whose first 15 windows
    reach into the history); the packed kernel's eight workgroups take 16, 16, 4 and none"""
    h = white_taps(L, True)
    n1 = 37 * advance(L) + TAIL
    assert c32_interior(n1, L) == (26 if L == 3841 else 36)
    x, ref = c32_case(L)
    f = FIRFilter(h, C64(SCALE_C), sample_dtype=C64, algo=sd.ALGO_FFT)
    f.set_tuning(TUNE_OLS_KERNEL, kern)
    y = []
    for a, b in ((0, n1), (n1, len(x))):
        y.append(f.execute_block(x[a:b]))
        hist, _ = f.get_state()
        assert bits_equal(hist, history_after(x, b, L)), (a, b)
    check_8d(np.concatenate(y), ref, h, SCALE_C, x, f"c32 L={L} kern={kern} complex white")
