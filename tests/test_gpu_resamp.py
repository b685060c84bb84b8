"""The rational resampler (sd.Resampler, kern_resamp.hip) on MI355X.

A Resampler(taps, M, D) is by definition the interpolating FIR's stream taken at
u_k = (k + 1) D - 1 - c.  On ALGO_EXACT it must equal that bit for bit: the yardstick is existing
code, an ALGO_EXACT InterpolatingFIRFilter on the same device whose output is taken at
[D - 1 - c :: D] (and, for the 64-bit pairs, the CPU restatement O.interp).  On ALGO_FMA it is held
to the interpolator's own pair of bounds against the f64 restatement on the widened input.

Taps are white (tests/test_resamp_capi.py test_what_the_inputs_see), real and complex per pair;
the input is white.  Which kernel a shape runs on is resamp_plan's rule (csrc/kern_resamp.hip),
restated in kernel_of below, asserted against info() and named in the case ids."""
import functools
import math

import numpy as np
import pytest

import oracle_lib as O
from gpu_util import bits_equal, rel_rms, to_dev, empty_dev, to_host

pytestmark = pytest.mark.gpu

sd = pytest.importorskip("solid_dsp_amd")

C64, C128, F32, F64 = np.complex64, np.complex128, np.float32, np.float64
# name -> (coef dtype, sample dtype, oracle dtype, oracle dtype of the f64 restatement)
PAIRS = {
    "RR32": (F32, F32, O.RR32, O.RR64),
    "RC32": (F32, C64, O.RC32, O.RC64),
    "CC32": (C64, C64, O.CC32, O.CC64),
    "RR64": (F64, F64, O.RR64, O.RR64),
    "RC64": (F64, C128, O.RC64, O.RC64),
    "CC64": (C128, C128, O.CC64, O.CC64),
}
ALL = list(PAIRS)
STAGED, PER_OUTPUT, BRANCH = 1, 2, 3
NAMES = {0: "auto", STAGED: "staged", PER_OUTPUT: "per_output", BRANCH: "branch"}
LDS = 48 * 1024
TUNE = 24  # SDSP_TUNE_RESAMP_KERNEL


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


def sub_len(L, M):
    """K as sdsp_interp_create computes it, in f32 (interp.rs:35-40)"""
    q = np.float32(L) / np.float32(M)
    return int(q) if q == np.floor(q) else int(np.ceil(q))


def plans(pair, L, M, D):
    """resamp_plan restated: {kernel: outputs per workgroup} of every kernel that applies to the
    shape, and the automatic choice"""
    sb = np.dtype(PAIRS[pair][1]).itemsize
    K = sub_len(L, M)
    out = {PER_OUTPUT: 256}
    dense = D <= M * K  # else most of a staged span is samples no output reads
    if dense:
        T = 4096
        while T >= 256 and (((T * D + M - 1) // M + K) * sb + 15) // 16 * 16 > LDS:
            T //= 2
        if T >= 256 and M + T * D < 1 << 31:
            out[STAGED] = T
    g = math.gcd(M, D)
    Pd = M // g
    if dense and K in (4, 8, 16) and Pd <= 256 and M + 256 * D < 1 << 31:
        A = Pd * (256 // Pd)
        step = (A // Pd) * (D // g)
        R = 16
        while R >= 1 and ((M - 1 + (A - 1) * D) // M + (R - 1) * step + K) * sb > LDS:
            R //= 2
        if R >= 1:
            out[BRANCH] = A * R
    return out, (STAGED if STAGED in out else PER_OUTPUT)


def kernel_of(pair, L, M, D, forced=0):
    """(kernel, tile) of the next call of a handle with SDSP_TUNE_RESAMP_KERNEL = forced"""
    applies, auto = plans(pair, L, M, D)
    k = forced if forced in applies else auto
    return k, applies[k]


def cb_in_lds(pair, L, M, D):
    """the staged kernel's CB_LDS: span and branch table (row stride K | 1) within 48 KiB"""
    cdt, sdt = PAIRS[pair][:2]
    K = sub_len(L, M)
    T = plans(pair, L, M, D)[0][STAGED]
    xb = (((T * D + M - 1) // M + K) * np.dtype(sdt).itemsize + 15) // 16 * 16
    return xb + M * (K | 1) * np.dtype(cdt).itemsize <= LDS


def make(pair, L, M, D, algo=sd.ALGO_EXACT, seed=1, channels=1, forced=0):
    cdt, sdt = PAIRS[pair][:2]
    h = white_taps(L, cdt, seed)
    r = sd.Resampler(h, M, D, sample_dtype=sdt, algo=algo, channels=channels)
    if forced:
        r.set_tuning(TUNE, forced)
    return r, h


def run(r, x, offset=0, in_offset=0, st=None):
    """one device call; offset / in_offset = samples the output / input sits past a 16-byte
    aligned allocation.  The sample after the output's end must stay as it was."""
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


class Strided:
    """The yardstick: an EXACT (or FMA) interpolator on the same device, its output taken at
    [D - 1 - c :: D], with the phase counter kept on the host (one channel)."""

    def __init__(self, pair, taps, M, D, algo=sd.ALGO_EXACT):
        self.sdt = PAIRS[pair][1]
        self.itp = sd.InterpolatingFIRFilter(taps, M, sample_dtype=self.sdt, algo=algo)
        self.M, self.D, self.c = M, D, 0

    def run(self, x):
        n = len(x)
        if n == 0:
            return np.zeros(0, self.sdt)
        d_in = to_dev(np.concatenate([x, np.zeros(1, x.dtype)]))
        d_mid = empty_dev(n * self.M + 1, self.sdt)
        self.itp.execute_block_device(d_in, n, d_mid, stream())
        # (the slice is taken on the device, by torch: the kept samples alone come back)
        y = to_host(d_mid[:n * self.M][self.D - 1 - self.c::self.D].contiguous())
        self.c = (self.c + n * self.M) % self.D
        return y


# ---------------------------------------------------------------- EXACT is the strided interpolator
def ragged(tile, M, D):
    """call lengths: 0, 1, 1, enough inputs for three tiles and a ragged fourth, 1, a long one, 0
    and a tail"""
    per_tile = -(-tile * D // M)
    return [0, 1, 1, 3 * per_tile + per_tile // 3 + 5, 1, 2 * per_tile + 7, 0, per_tile // 2 + 3]


# (L, M, D, pairs)
SHAPES = [
    (12, 3, 2, ALL), (8, 2, 3, ALL),   # coprime, up and down; K = 4
    (40, 5, 7, ALL),                   # K = 8
    (16, 4, 6, ALL),                   # g = 2, Pd = 2
    (64, 8, 2, ALL),                   # D divides M
    (32, 2, 8, ALL),                   # M divides D; inputs skipped within a window
    (16, 1, 4, ALL),                   # M = 1, Pd = 1
    (588, 147, 160, ALL),              # Pd = 147: the branch kernel launches 147 lanes
    (60, 16, 3, ALL),                  # zero-padded taps, K = 4
    (10, 4, 3, ALL),                   # K = 3: no branch instance
    (6400, 64, 5, ["CC32"]),           # table too large for LDS
    (32, 2, 7, ["CC64"]),              # T shrinks below 4096 to fit the span
    (4, 1, 5000, ALL), (12, 3, 10007, ALL),  # D > M K: per-output kernel; most calls emit nothing
]


def exact_cases():
    out = []
    for L, M, D, pairs in SHAPES:
        for pair in pairs:
            applies, _ = plans(pair, L, M, D)
            for forced in [0] + sorted(applies):
                k, _ = kernel_of(pair, L, M, D, forced)
                out.append(pytest.param(pair, L, M, D, forced,
                                        id=f"{pair}-L{L}-M{M}-D{D}-{NAMES[forced]}-{NAMES[k]}"))
    return out


def check_stream(pair, L, M, D, forced, lens=None, offset=0, in_offset=0):
    r, h = make(pair, L, M, D, forced=forced)
    kern, tile = kernel_of(pair, L, M, D, forced)
    assert r.info() == (kern, tile), (r.info(), kern, tile)
    assert (r.interpolation(), r.decimation(), r.subfilter_len()) == (M, D, sub_len(L, M))
    assert r.phase() == 0
    ref = Strided(pair, h, M, D)
    _, sdt, odt, _ = PAIRS[pair]
    lens = lens if lens is not None else ragged(tile, M, D)
    x = white_input(sum(lens), sdt, 11)
    at, ys = 0, []
    for n in lens:
        blk = x[at:at + n]
        at += n
        want = ref.run(blk)
        assert r.output_count(n) == len(want)
        ys.append(run(r, blk, offset, in_offset))
        assert bits_equal(ys[-1], want), (pair, L, M, D, n)
        assert r.phase() == ref.c, (pair, L, M, D, n)
    if odt in (O.RR64, O.RC64, O.CC64):  # and the CPU restatement, over the whole stream
        z = O.interp(odt, h, M).execute_block(x)
        assert bits_equal(np.concatenate(ys), z[D - 1::D])
    return sum(len(y) for y in ys)


@pytest.mark.parametrize("pair,L,M,D,forced", exact_cases())
def test_exact_is_the_strided_interpolator(pair, L, M, D, forced):
    check_stream(pair, L, M, D, forced)


def test_the_shapes_reach_what_they_are_for():
    """the table's right-hand column: the restated rule against info() on every shape and forced
    value, then what the rule says about the shapes that are there for one path"""
    for L, M, D, pairs in SHAPES:
        for pair in pairs:
            for forced in range(4):
                assert make(pair, L, M, D, forced=forced)[0].info() == kernel_of(pair, L, M, D, forced)
    assert kernel_of("CC32", 10, 4, 3, BRANCH)[0] == STAGED and BRANCH not in plans("CC32", 10, 4, 3)[0]
    assert not cb_in_lds("CC32", 6400, 64, 5) and cb_in_lds("CC32", 40, 5, 7)
    assert plans("CC64", 32, 2, 7)[0][STAGED] == 512
    for L, M, D in ((4, 1, 5000), (12, 3, 10007)):
        assert plans("RC32", L, M, D)[0] == {PER_OUTPUT: 256}
    assert plans("RC32", 588, 147, 160)[0][BRANCH] == 147 * 16  # 147 lanes: a partial last wave
    assert plans("RC32", 16, 4, 6)[0][BRANCH] % 256 == 0 and plans("RC32", 16, 1, 4)[0][BRANCH] % 256 == 0


@pytest.mark.parametrize("pair", ["RR32", "CC64"])
@pytest.mark.parametrize("forced", [0, PER_OUTPUT, BRANCH])
def test_decimation_one_is_the_whole_interpolator(pair, forced):
    L, M, D = 32, 8, 1
    total = check_stream(pair, L, M, D, forced)
    assert total == M * sum(ragged(kernel_of(pair, L, M, D, forced)[1], M, D))


@pytest.mark.parametrize("pair", ["RC32", "RR64"])
def test_calls_that_emit_nothing(pair):
    """ten calls of 7 inputs at M = 3, D = 1000: n_out is 0 until the counter crosses D (the
    48th input), the phase accumulates, and the first output reads inputs of earlier calls
    through the window"""
    L, M, D = 12, 3, 1000
    r, h = make(pair, L, M, D)
    ref = Strided(pair, h, M, D)
    sdt = PAIRS[pair][1]
    x = white_input(70 + 400, sdt, 4)
    for k in range(10):
        blk = x[7 * k:7 * (k + 1)]
        y = run(r, blk)
        assert len(y) == 0 and bits_equal(y, ref.run(blk))
        assert r.phase() == 21 * (k + 1) == ref.c
    y = run(r, x[70:])
    assert len(y) == (210 + 1200) // 1000 == 1  # the stream's sample 999, input 263 of this call
    assert bits_equal(y, ref.run(x[70:])) and r.phase() == ref.c == 410
    # D = 40: the first output is the stream's sample 39, on input 13, alone in its call; the three
    # inputs before it came in calls that emitted nothing and are read through the window
    r, h = make(pair, L, M, 40)
    ref = Strided(pair, h, M, 40)
    at = 0
    for n, emits in ((5, 0), (5, 0), (3, 0), (1, 1), (9, 0)):
        blk = x[at:at + n]
        at += n
        y = run(r, blk)
        assert len(y) == emits and bits_equal(y, ref.run(blk)), at
        assert r.phase() == ref.c == at * M % 40


def test_set_phase_selects_the_stride_offset():
    L, M, D, n = 12, 3, 4, 1501
    x = white_input(n, C64, 6)
    for p in range(D):
        r, h = make("RC32", L, M, D)
        r.set_phase(p)
        assert r.phase() == p and r.output_count(n) == (p + n * M) // D
        itp = sd.InterpolatingFIRFilter(h, M, sample_dtype=C64, algo=sd.ALGO_EXACT)
        assert bits_equal(run(r, x), itp.execute_block(x)[D - 1 - p::D])
        assert r.phase() == (p + n * M) % D
    with pytest.raises(sd.SdspError) as e:
        r.set_phase(D)
    assert e.value.code == 90 and "phase" in str(e.value)
    assert r.phase() == (D - 1 + n * M) % D  # a refused call moves nothing


@pytest.mark.parametrize("forced", [STAGED, PER_OUTPUT, BRANCH])
@pytest.mark.parametrize("pair", ["RC32", "CC64"])
def test_blocks_one_sample_past_a_16_byte_boundary(pair, forced):
    """input and output each one sample past a 16-byte boundary: no kernel here assumes more
    than a sample's alignment, so the selection does not move"""
    check_stream(pair, 40, 5, 7, forced, lens=[1, 1500, 3, 900], offset=1, in_offset=1)


@pytest.mark.parametrize("L,M,D,forced", [(12, 3, 2, 0), (40, 5, 7, BRANCH), (12, 3, 10007, 0)])
def test_three_channels_share_the_phase(L, M, D, forced):
    n = 4001
    r3, h = make("CC32", L, M, D, channels=3, forced=forced)
    ones = [Strided("CC32", h, M, D) for _ in range(3)]
    singles = [make("CC32", L, M, D, forced=forced)[0] for _ in range(3)]
    x = white_input(2 * 3 * n, C64, 8).reshape(2, 3, n)
    for call in range(2):
        y = run(r3, x[call])
        for c in range(3):
            assert bits_equal(y[c], run(singles[c], x[call, c])), (call, c)
            assert bits_equal(y[c], ones[c].run(x[call, c])), (call, c)
            assert r3.phase() == singles[c].phase() == ones[c].c


def test_clone_continues_identically():
    L, M, D, n = 40, 5, 7, 1101
    r, h = make("RC32", L, M, D, algo=sd.ALGO_FMA, forced=BRANCH)
    x = white_input(3 * n, C64, 9)
    run(r, x[:n])
    c = r.clone()
    assert c.phase() == r.phase() == n * M % D and c.get_algo() == sd.ALGO_FMA
    assert c.info() == r.info() == kernel_of("RC32", L, M, D, BRANCH)
    assert (c.interpolation(), c.decimation(), c.subfilter_len()) == (M, D, 8)
    assert bits_equal(run(c, x[n:2 * n]), run(r, x[n:2 * n]))  # window, phase, algorithm, tuning
    assert c.phase() == r.phase()
    run(c, x[2 * n:])
    assert r.phase() == 2 * n * M % D  # the clone is its own object


def test_reset_and_set_channels_zero_window_and_phase():
    L, M, D, n = 12, 3, 2, 1001
    r, h = make("RR32", L, M, D)
    x = white_input(2 * n, F32, 10)
    first = run(r, x[:n])
    assert r.phase() == n * M % D == 1
    assert not bits_equal(run(r, x[:n]), first)  # another window and another phase
    r.reset()
    assert r.phase() == 0
    assert bits_equal(run(r, x[:n]), first)
    r.set_channels(1)
    assert r.phase() == 0
    assert bits_equal(run(r, x[:n]), first)
    r.set_channels(2)
    assert r.phase() == 0
    y = run(r, np.stack([x[:n], x[:n]]))
    assert bits_equal(y[0], first) and bits_equal(y[1], first)


def test_host_block_equals_device_block():
    L, M, D, n = 40, 5, 7, 1103
    x = white_input(2 * 2 * n, C64, 12).reshape(2, 2, n)
    a, _ = make("CC32", L, M, D, channels=2)
    b, _ = make("CC32", L, M, D, channels=2)
    for k in range(2):
        y = a.execute_block(x[k])
        assert y.shape == (2, b.output_count(n))
        assert bits_equal(y, run(b, x[k]))
        assert a.phase() == b.phase()
    a1, _ = make("RR64", 12, 3, 1000)  # a host block that emits nothing still moves the phase
    assert a1.execute_block(white_input(7, F64, 1)).shape == (0,) and a1.phase() == 21
    assert len(a1.execute_block(np.zeros(0))) == 0 and a1.phase() == 21


def test_refusals():
    r, h = make("RC32", 12, 3, 2)
    buf = empty_dev(8 * 512, C64)
    with pytest.raises(sd.SdspError) as e:  # in place
        r.execute_block_device(buf, 512, buf, stream())
    assert e.value.code == 90 and "overlap" in str(e.value)
    with pytest.raises(sd.SdspError) as e:  # the input inside the output
        r.execute_block_device(buf[400:], 300, buf, stream())
    assert e.value.code == 90
    assert r.phase() == 0  # a refused call moves nothing
    for algo in (sd.ALGO_AUTO, sd.ALGO_FFT):
        with pytest.raises(sd.SdspError) as e:
            r.set_algo(algo)
        assert e.value.code == 90
    assert r.get_algo() == sd.ALGO_EXACT
    for key, value in ((TUNE, 4), (TUNE, -1), (6, 1)):
        with pytest.raises(sd.SdspError) as e:
            r.set_tuning(key, value)
        assert e.value.code == 90
    with pytest.raises(sd.SdspError) as e:
        sd.Resampler(h, 3, 0, sample_dtype=C64)
    assert e.value.code == 2


def test_blocks_alternating_on_two_streams_run_in_call_order():
    """as tests/test_gpu_duc.py: a long block on s1, then short ones on the handle's stream, s1
    and s2, queued with no host sync; each reads the window and the phase the one before left,
    so an unordered launch shows in the bits"""
    import torch
    L, M, D = 40, 5, 7
    n0, n1 = 1 << 17, 1024
    x = white_input(n0 + 3 * n1, C64, 14)
    cuts = [0, n0, n0 + n1, n0 + 2 * n1, n0 + 3 * n1]
    blocks = [x[cuts[k]:cuts[k + 1]] for k in range(4)]
    ref_h, h = make("RC32", L, M, D)
    ref = [run(ref_h, b) for b in blocks]  # one at a time, synchronised
    r, _ = make("RC32", L, M, D)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ins = [to_dev(b) for b in blocks]
    outs = [empty_dev(len(y), C64) for y in ref]
    torch.cuda.synchronize()
    for i, o, b, y, st in zip(ins, outs, blocks, ref, [s1, None, s1, s2]):
        assert r.execute_block_device(i, len(b), o, st) == len(y)
    r.synchronize()
    torch.cuda.synchronize()
    for k in range(4):
        assert bits_equal(to_host(outs[k]), ref[k]), k
    assert r.phase() == ref_h.phase()


# ---------------------------------------------------------------- impulses
@pytest.mark.parametrize("forced", [STAGED, PER_OUTPUT, BRANCH])
@pytest.mark.parametrize("L,M,D", [(12, 3, 2), (40, 5, 7)])
def test_impulses_land_on_the_padded_taps(L, M, D, forced):
    """an impulse a at input j0 appears in the interpolated stream at offset v = u - j0 M,
    0 <= v < K M, as a hpad[(K - 1 - v // M) M + v % M], hpad the taps zero-padded to K M: every
    output inside the response equals that product exactly, every one outside is exactly zero.
    Impulses at input 0, at the last input of a call and at the input before a tile boundary."""
    pair = "RC64"
    r, h = make(pair, L, M, D, forced=forced)
    K = sub_len(L, M)
    tile = kernel_of(pair, L, M, D, forced)[1]
    assert r.info()[1] == tile
    hpad = np.concatenate([h, np.zeros(K * M - L)])
    n1 = (tile * D) // M + 50                # the first call ends inside the second tile
    edge = ((tile + 1) * D - 1) // M - 1     # the input before the one tile 1's first output sits on
    at = {0: 1.5 - 0.5j, edge: -0.75 + 2j, n1 - 1: 0.25 + 1j}
    assert len(at) == 3 and 0 < edge < n1 - 1
    n = n1 + 2 * K + 40
    x = np.zeros(n, C128)
    for j, a in at.items():
        x[j] = a
    want = np.zeros(n * M, C128)
    for j, a in at.items():
        for v in range(K * M):
            # responses further apart than K M samples: one product per output, nothing to add
            want[j * M + v] = a * hpad[(K - 1 - v // M) * M + v % M]
    assert min(abs(a - b) for a in at for b in at if a != b) >= K
    y = np.concatenate([run(r, x[:n1]), run(r, x[n1:])])
    assert y.shape == want[D - 1::D].shape and np.array_equal(y, want[D - 1::D])
    inside = np.zeros(n * M, bool)
    for j in at:
        inside[j * M:(j + K) * M] = True
    assert np.all(y[~inside[D - 1::D]] == 0)


# ---------------------------------------------------------------- FMA path
N1, N2, CH = 3001, 2222, 2  # two calls, two channels
FMA_MD = [(3, 2), (5, 7), (147, 160), (1, 4)]
FMA_SHAPES = ([(pair, K * M, M, D) for pair in ("RC32", "CC32") for M, D in FMA_MD for K in (4, 8, 16)] +
              [("RC64", 40, 5, 7), ("CC64", 16, 1, 4)])
WORST = {}  # (kernel, precision) -> worst rel-RMS seen so far in this run


def fma_cases():
    out = []
    for pair, L, M, D in FMA_SHAPES:
        for k in sorted(plans(pair, L, M, D)[0]):
            out.append(pytest.param(pair, L, M, D, k, id=f"{pair}-L{L}-M{M}-D{D}-{NAMES[k]}"))
    return out


@functools.lru_cache(maxsize=None)
def fma_case(pair, L, M, D):
    """taps, input and the f64 restatement per channel, computed once per shape"""
    cdt, sdt, _, odt = PAIRS[pair]
    h = white_taps(L, cdt, 100 + L + M)
    x = white_input(CH * (N1 + N2), sdt, 200 + M).reshape(CH, N1 + N2)
    wide = C128 if np.dtype(cdt).kind == "c" else F64
    ref = np.stack([O.interp(odt, h.astype(wide), M).execute_block(x[c].astype(C128))[D - 1::D] for c in range(CH)])
    for a in (h, x, ref):
        a.setflags(write=False)
    return h, x, ref


@pytest.mark.parametrize("pair,L,M,D,forced", fma_cases())
def test_fma_path_meets_the_interpolators_bounds(pair, L, M, D, forced):
    """ALGO_FMA against the f64 restatement O.interp(<64-bit pair>)[D - 1 - c :: D] on the widened
    input, per channel: rel-RMS <= 1e-6 (32-bit) / 1e-13 (64-bit) and max-abs <= tol sum|h| max|x|."""
    h, x, ref = fma_case(pair, L, M, D)
    sdt = PAIRS[pair][1]
    r = sd.Resampler(h, M, D, sample_dtype=sdt, algo=sd.ALGO_FMA, channels=CH)
    r.set_tuning(TUNE, forced)
    assert r.info()[0] == forced
    y = np.concatenate([run(r, x[:, :N1]), run(r, x[:, N1:])], axis=1)
    assert y.shape == ref.shape
    tol = 1e-6 if sdt is C64 else 1e-13
    bound = tol * float(np.sum(np.abs(h.astype(C128)))) * float(np.max(np.abs(x.astype(C128))))
    key = (NAMES[forced], "32" if sdt is C64 else "64")
    for c in range(CH):
        rr = rel_rms(y[c], ref[c])
        ma = float(np.max(np.abs(y[c].astype(C128) - ref[c])))
        WORST[key] = max(WORST.get(key, 0.0), rr)
        print(f"{pair} L={L} M={M} D={D} {key[0]} channel {c}: rel-RMS {rr:.3e} max-abs {ma:.3e} "
              f"(bound {bound:.3e}); worst on {key[0]} {key[1]}-bit so far {WORST[key]:.3e}")
        assert rr <= tol, (pair, L, M, D, c, rr)
        assert ma <= bound, (pair, L, M, D, c, ma, bound)
