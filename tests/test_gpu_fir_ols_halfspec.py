"""The one-shot overlap-save kernel on a real circular kernel g (real f32 taps, real scale, c32
samples): its interior instances read half the spectrum (bins k2 < 8 of every lane) and take the
other half as the conjugates of the mirror lane's, through a DPP operand; the 16 lanes of row 0
load their mirror's entries themselves.  A wrong, unconjugated or misplaced bin shows here:

1. white taps and a white input give every one of the 4096 bins the same weight, so one bad bin
   costs about 1/64 of the output's RMS against a bound of 1e-6;
2. single-bin inputs exp(2 pi i k n / 4096) name the special places: bin 0 and bin 128 (the two
   lanes of row 0 that mirror themselves: k1 = 0 and k1 = 8), 2048 (Nyquist) and 2176, 16 and 4080
   (row 0, a mirror pair), 1 and 4095 (rows 1 and 15), 273 and 3823 (rows 1 and 15, k1 = 1 and 14),
   8 and 4088 (row 8, which mirrors within itself);
3. the boundary instance reads the full table: the same stream cut into calls whose segments all
   run in the boundary launch gives the same bits as one call whose segments 1..5 are interior
   (the few inputs a cut call cannot see, older than its history, are zero in the stream);
4. a 3-channel call is three 1-channel calls, bit for bit.

Blocks of (k + 1) V + 1234 samples with k = 2 interior segments (V = 4096 - 256 h2): every interior
segment uses every lane of the workgroup, so small blocks check as much as long ones.  L = 256 is
the instance with one halo row compiled in, L = 700 the generic one; kernels 0 and 3 are the
8-byte-lane and 16-byte-lane forms."""
import functools

import numpy as np
import pytest

import oracle_lib as O
from gpu_util import bits_equal, rel_rms

pytestmark = pytest.mark.gpu

sd = pytest.importorskip("solid_dsp_amd")
from solid_dsp_amd import FIRFilter  # noqa: E402

C64, C128, F32, F64 = np.complex64, np.complex128, np.float32, np.float64
TUNE_OLS_KERNEL = 14
KERNELS = [0, 3]  # one-shot, one-shot with 16-byte lanes
LENGTHS = [256, 700]
SCALE = 0.2
TAIL = 1234
BINS = [0, 128, 2048, 2176, 16, 4080, 1, 4095, 273, 3823, 8, 4088]


def advance(L):
    return 4096 - 256 * (-(-(L - 1) // 256))


def block_length(L, k=2):
    """a block with k interior segments: k + 1 whole advances and a ragged tail"""
    return (k + 1) * advance(L) + TAIL


def interior_segments(n, L):
    V = advance(L)
    H, nseg = 4096 - V, -(-n // V)
    return [s for s in range(nseg) if s * V - H >= 0 and s * V - H + 4096 <= n and s != nseg - 1]


@functools.lru_cache(maxsize=None)
def taps(L, kind):
    if kind == "white":
        h = np.random.default_rng(20250308 + L).standard_normal(L).astype(F32)
    else:  # L = 256: the taps of bench.py's config 2
        h = O.firdes_kaiser(L, 0.1, 80.0, 0.0).astype(F32)
    h.setflags(write=False)
    return h


def restate(h, x):
    return O.fir(O.RC64, h.astype(F64), SCALE).execute_block(x.astype(C128))


@functools.lru_cache(maxsize=None)
def white_case(L, kind, channels=3, k=2):
    """(inputs [channels][n], f64 restatement per channel), shared by the kernels"""
    n = block_length(L, k)
    x = O.synth(20250232, 5, 0, channels * n, complex_=True).reshape(channels, n)
    ref = np.stack([restate(taps(L, kind), x[c]) for c in range(channels)])
    x.setflags(write=False)
    ref.setflags(write=False)
    return x, ref


@functools.lru_cache(maxsize=None)
def tone_case(L, k):
    n = block_length(L)
    x = np.exp(2j * np.pi * ((k * np.arange(n)) % 4096) / 4096.0).astype(C64)
    ref = restate(taps(L, "white"), x)
    x.setflags(write=False)
    ref.setflags(write=False)
    return x, ref


def make(L, kind, kern, channels=1):
    f = FIRFilter(taps(L, kind), F32(SCALE), sample_dtype=C64, channels=channels, algo=sd.ALGO_FFT, host_step=False)
    assert sd.lib().sdsp_fir_set_tuning(f._h, TUNE_OLS_KERNEL, kern) == 0
    return f


def check(y, ref, h, x, what):
    r, worst = rel_rms(y, ref), float(np.abs(y - ref).max())
    bound = 1e-6 * float(np.abs(h).sum()) * SCALE * float(np.abs(x).max())
    print(f"{what}: rel_rms {r:.3e} (bound 1e-6) max|err| {worst:.3e} (bound {bound:.3e})")
    assert r <= 1e-6, what
    assert worst <= bound, what


@pytest.mark.parametrize("kind", ["white", "kaiser"])
@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("L", LENGTHS)
def test_every_bin_carries_weight(L, kern, kind):
    n = block_length(L)
    assert n < 20000 and interior_segments(n, L) == [1, 2]
    x, ref = white_case(L, kind)
    y = make(L, kind, kern).execute_block(x[0])
    check(y, ref[0], taps(L, kind), x[0], f"L={L} kern={kern} {kind} taps")


@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("L", LENGTHS)
def test_named_bins(L, kern):
    for k in BINS:
        x, ref = tone_case(L, k)
        y = make(L, "white", kern).execute_block(x)
        check(y, ref, taps(L, "white"), x, f"L={L} kern={kern} bin {k}")


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("L", LENGTHS)
def test_boundary_and_interior_agree_bit_for_bit(L, kern, channels):
    V = advance(L)
    n = 6 * V + TAIL
    assert interior_segments(n, L) == [1, 2, 3, 4, 5]
    assert interior_segments(2 * V, L) == [] and interior_segments(TAIL, L) == []
    x = O.synth(20250233, 7, 0, channels * n, complex_=True).reshape(channels, n).copy()
    # A call's first window starts 256 h2 inputs before the call, and the history holds only the last
    # L - 1: the 256 h2 - (L - 1) inputs before those read as 0.  They reach no output that is kept,
    # but they are part of the transform's input, so its rounding depends on them.  Zero in the
    # stream itself, they make the windows of the two runs the same numbers.
    for cut in (2 * V, 4 * V, 6 * V):
        x[:, cut - (4096 - V): cut - (L - 1)] = 0
    xs = x if channels > 1 else x[0]
    f = make(L, "white", kern, channels)
    y_one = f.execute_block(xs)
    hist_one, _ = f.get_state()
    g = make(L, "white", kern, channels)
    cuts = [0, 2 * V, 4 * V, 6 * V, n]  # the same segment grid, every segment in the boundary launch
    y_cut = np.concatenate([g.execute_block(xs[..., a:b]) for a, b in zip(cuts, cuts[1:])], axis=-1)
    hist_cut, _ = g.get_state()
    diff = int(np.count_nonzero(np.ascontiguousarray(y_one).view(np.uint32) != np.ascontiguousarray(y_cut).view(np.uint32)))
    print(f"L={L} kern={kern} channels={channels}: {diff} differing 32-bit patterns of {2 * y_one.size}")
    assert bits_equal(y_one, y_cut)
    assert bits_equal(hist_one, hist_cut)
    assert bits_equal(hist_one, x[:, -(L - 1):].reshape(-1))


@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("L", LENGTHS)
def test_three_channels_are_three_single_channels(L, kern):
    x, ref = white_case(L, "white")
    y3 = make(L, "white", kern, 3).execute_block(x)
    for c in range(3):
        y1 = make(L, "white", kern).execute_block(x[c])
        assert bits_equal(y3[c], y1), (L, kern, c)
        check(y3[c], ref[c], taps(L, "white"), x[c], f"L={L} kern={kern} channel {c} of 3")
